"""Selectable reconstruction term (BCE / MSE) - host side, no kernel launch: the C ABI exports, the model option and the
numpy MSE reference the GPU tests (tests/test_recon_loss_gpu.py) use as their yardstick."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def mse_reference(xhat, t):
    """F.mse_loss(xhat, t) (reduction 'mean') with xhat = sigmoid(logit), and its gradient w.r.t. the logit, in float64:
    ((xhat - t) * 2/N) * (1 - xhat) * xhat - ATen's mse_loss_backward followed by sigmoid_backward."""
    xh = np.asarray(xhat, np.float64)
    t = np.asarray(t, np.float64)
    n = xh.size
    d = xh - t
    return float((d * d).sum() / n), d * (2.0 / n) * (1.0 - xh) * xh


def test_library_exports_recon_symbols():
    from torch_vae_amd import _lib
    L = _lib.lib()
    for name in ("vae_set_recon_loss", "vae_elbo_generic_ex"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert (_lib.RECON_BCE, _lib.RECON_MSE) == (0, 1)
    assert L.vae_set_recon_loss(None, _lib.RECON_MSE) != 0          # null context: refused, not dereferenced
    assert b"vae_set_recon_loss" in L.vae_last_error()


def test_model_recon_loss_option():
    from torch_vae_amd.models import VanillaVAE
    m = VanillaVAE(1, 16, 32)
    assert m.recon_loss == "bce"
    assert VanillaVAE(1, 16, 32, recon_loss="mse").recon_loss == "mse"
    with pytest.raises(ValueError):
        VanillaVAE(1, 16, 32, recon_loss="xyz")
    m.recon_loss = "mse"               # a writable attribute, read at every forward
    assert m.recon_loss == "mse"


@pytest.mark.parametrize("shape", [(3, 1, 8, 8), (2, 1, 32, 32)])
def test_mse_reference_matches_torch_autograd(shape):
    rng = np.random.default_rng(sum(shape))
    logit = rng.normal(0.0, 3.0, shape)
    t = rng.uniform(0.0, 1.0, shape) * (rng.uniform(size=shape) < 0.7)
    t.flat[:5] = 1.0
    lt = torch.tensor(logit, dtype=torch.float64, requires_grad=True)
    loss = F.mse_loss(torch.sigmoid(lt), torch.tensor(t))
    loss.backward()
    ref_loss, ref_dlogit = mse_reference(1.0 / (1.0 + np.exp(-logit)), t)
    np.testing.assert_allclose(ref_loss, loss.item(), rtol=1e-12)
    np.testing.assert_allclose(ref_dlogit, lt.grad.numpy(), rtol=1e-10, atol=1e-300)
