"""Positive-class weight of the BCE term (VanillaVAE(pos_weight=w), VAE_RECON_WBCE) - host side, no kernel launch: the C ABI
declarations and refusals, the model option, evaluation.balanced_pos_weight, and the numpy f64 reference the layer-local GPU
tests (tests/test_pos_weight_gpu.py) use, itself checked here against torch autograd of
    F.binary_cross_entropy(xhat, t, weight = 1 + (w - 1) t)."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_kl_control_host import declared_params
from torch_vae_amd import _lib

NEW = ("vae_set_recon_loss_ex", "vae_elbo_generic_w")


def wbce_reference(xhat, t, w):
    """mean over all cells of W * bce(xhat, t), W = 1 + (w - 1) t, with the logs clamped at -100, and its gradient w.r.t. the
    logit of xhat = sigmoid(logit), in float64: W * (xhat - t) / max(xhat (1 - xhat), 1e-12) * xhat (1 - xhat) / N - ATen's
    binary_cross_entropy_backward followed by sigmoid_backward."""
    xh = np.asarray(xhat, np.float64)
    t = np.asarray(t, np.float64)
    n = xh.size
    W = 1.0 + (w - 1.0) * t
    with np.errstate(divide="ignore"):
        l1, l0 = np.maximum(np.log(xh), -100.0), np.maximum(np.log(1.0 - xh), -100.0)
    loss = float((-(t * l1 + (1.0 - t) * l0) * W).sum() / n)
    om = xh * (1.0 - xh)
    return loss, (xh - t) / np.maximum(om, 1e-12) * om / n * W


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_bound():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == len(declared_params(name)), name
    assert _lib.RECON_WBCE == 2
    hdr = open(declared_params.__globals__["HEADER"]).read()
    assert re.search(r"#define VAE_RECON_WBCE (\d+)", hdr).group(1) == "2"
    assert declared_params("vae_set_recon_loss_ex") == ["vae_ctx*", "int", "double"]
    kl, w = declared_params("vae_elbo_generic_kl"), declared_params("vae_elbo_generic_w")
    i = kl.index("int", 8) + 1                              # behind `recon`
    assert w[:i] == kl[:i] and w[i] == "double" and w[i + 1:] == kl[i:]
    assert L.vae_abi_version() == 1


def test_null_context_and_the_old_setter_refuse():
    L = _lib.lib()
    assert L.vae_set_recon_loss_ex(None, _lib.RECON_WBCE, 8.0) == -1 and b"vae_set_recon_loss_ex" in L.vae_last_error()
    assert L.vae_set_recon_loss_ex(None, _lib.RECON_BCE, 0.0) == -1
    assert L.vae_set_recon_loss(None, _lib.RECON_WBCE) != 0 and b"vae_set_recon_loss" in L.vae_last_error()


@pytest.mark.parametrize("kind,w", [(7, 1.0), (-1, 0.0), (_lib.RECON_WBCE, 0.0), (_lib.RECON_WBCE, -2.0), (_lib.RECON_WBCE, float("nan")),
                                    (_lib.RECON_WBCE, float("inf")), (_lib.RECON_WBCE, 2000.0), (_lib.RECON_BCE, 8.0), (_lib.RECON_MSE, 1.0)])
def test_generic_entry_point_refuses_before_launching(kind, w):
    """fake, never dereferenced device addresses and a null stream: refused before anything is enqueued"""
    L = _lib.lib()
    rc = L.vae_elbo_generic_w(4096, 4096, 4096, 4096, 64, 4, 16, 1.0, kind, w, _lib.KL_PLAIN, 0.0, 4096, 4096, 4096, 4096, None)
    assert rc == -1 and L.vae_last_error().decode().startswith("vae_elbo_generic_w: "), (kind, w)


def test_older_generic_entry_points_keep_refusing_the_new_kind():
    L = _lib.lib()
    assert L.vae_elbo_generic_ex(4096, 4096, 4096, 4096, 64, 4, 16, 1.0, _lib.RECON_WBCE, 4096, 4096, 4096, 4096, None) == -1
    assert L.vae_elbo_generic_kl(4096, 4096, 4096, 4096, 64, 4, 16, 1.0, _lib.RECON_WBCE, _lib.KL_PLAIN, 0.0, 4096, 4096, 4096, 4096, None) == -1


# ---- the model option -------------------------------------------------------------------------------------------------------
def test_model_pos_weight_option():
    from torch_vae_amd.models import VanillaVAE, _recon_setting
    m = VanillaVAE(1, 16, 32)
    assert m.pos_weight is None and _recon_setting(m.recon_loss, m.pos_weight) == (_lib.RECON_BCE, 0.0)
    for w in (8, 8.0, 0.5, 1, 1024, 1e-3):
        m = VanillaVAE(1, 16, 32, pos_weight=w)
        assert m.pos_weight == w and _recon_setting(m.recon_loss, m.pos_weight) == (_lib.RECON_WBCE, float(w))
    assert _recon_setting("mse", None) == (_lib.RECON_MSE, 0.0)
    for kw in (dict(pos_weight=True), dict(pos_weight="8"), dict(pos_weight=float("nan")), dict(pos_weight=float("inf")),
               dict(pos_weight=0), dict(pos_weight=-1.0), dict(pos_weight=1024.5), dict(pos_weight=2000),
               dict(pos_weight=8.0, recon_loss="mse")):
        with pytest.raises(ValueError):
            VanillaVAE(1, 16, 32, **kw)
    with pytest.raises(TypeError):
        VanillaVAE(1, 16, 32, None, 1.0, False, None, "bf16", "bce", None, 0.0, None, None, 8.0)   # keyword-only
    m = VanillaVAE(1, 16, 32)
    m.pos_weight = 4.0                 # a writable attribute, read at every forward; a bad value is refused when it is read
    assert _recon_setting(m.recon_loss, m.pos_weight) == (_lib.RECON_WBCE, 4.0)
    m.recon_loss = "mse"
    with pytest.raises(ValueError):
        _recon_setting(m.recon_loss, m.pos_weight)


def test_balanced_pos_weight():
    from torch_vae_amd.evaluation import balanced_pos_weight
    assert balanced_pos_weight(0.5) == 1.0
    assert balanced_pos_weight(0.04) == pytest.approx(24.0)
    assert balanced_pos_weight(0.2) == pytest.approx(4.0)
    assert balanced_pos_weight(0.001) == 64.0                    # (1 - d) / d = 999: capped
    assert balanced_pos_weight(0.001, max_weight=2000.0) == pytest.approx(999.0)
    assert balanced_pos_weight(0.0) == 64.0 and balanced_pos_weight(0, max_weight=16.0) == 16.0
    assert balanced_pos_weight(1.0) == 0.0
    for d in (-0.01, 1.01, float("nan"), 4.0):                   # (4.0: a percentage where a fraction is meant)
        with pytest.raises(ValueError):
            balanced_pos_weight(d)


# ---- the yardstick itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8.0, 0.5, 1.0])
def test_wbce_reference_matches_torch_autograd_on_a_binary_roll(w):
    rng = np.random.default_rng(int(w * 10))
    shape = (3, 1, 8, 8)
    logit = rng.normal(0.0, 3.0, shape)
    t = (rng.uniform(size=shape) < 0.1).astype(np.float64)
    lt = torch.tensor(logit, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t)
    loss = F.binary_cross_entropy(torch.sigmoid(lt), tt, weight=1 + (w - 1) * tt)
    loss.backward()
    ref_loss, ref_dlogit = wbce_reference(1.0 / (1.0 + np.exp(-logit)), t, w)
    np.testing.assert_allclose(ref_loss, loss.item(), rtol=1e-12)
    np.testing.assert_allclose(ref_dlogit, lt.grad.numpy(), rtol=1e-10, atol=1e-300)
    # 0/1 targets: exactly BCEWithLogitsLoss(pos_weight = w) on the logits
    l2 = torch.tensor(logit, dtype=torch.float64, requires_grad=True)
    loss2 = F.binary_cross_entropy_with_logits(l2, tt, pos_weight=torch.tensor(w, dtype=torch.float64))
    loss2.backward()
    np.testing.assert_allclose(ref_loss, loss2.item(), rtol=1e-12)
    np.testing.assert_allclose(ref_dlogit, l2.grad.numpy(), rtol=1e-9, atol=1e-18)


@pytest.mark.parametrize("w", [8.0, 0.5])
def test_wbce_reference_matches_torch_autograd_on_a_velocity_roll(w):
    rng = np.random.default_rng(7)
    shape = (2, 1, 32, 32)
    logit = rng.normal(0.0, 3.0, shape)
    t = rng.uniform(0.2, 1.0, shape) * (rng.uniform(size=shape) < 0.1)
    t.flat[:5] = 1.0
    lt = torch.tensor(logit, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t)
    loss = F.binary_cross_entropy(torch.sigmoid(lt), tt, weight=1 + (w - 1) * tt)
    loss.backward()
    ref_loss, ref_dlogit = wbce_reference(1.0 / (1.0 + np.exp(-logit)), t, w)
    np.testing.assert_allclose(ref_loss, loss.item(), rtol=1e-12)
    np.testing.assert_allclose(ref_dlogit, lt.grad.numpy(), rtol=1e-10, atol=1e-300)
    # the per-cell optimum stays xhat = t: the gradient vanishes there whatever the weight
    _, g = wbce_reference(t.clip(1e-3, 1 - 1e-3), t.clip(1e-3, 1 - 1e-3), w)
    assert np.abs(g).max() == 0.0
