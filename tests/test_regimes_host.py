"""The regimes of tests/regimes.py on the host (no GPU): the numpy oracle against torch f64 autograd on every regime (it had been
pinned to the reference on binary data and fresh weights only), the conditions under which the regimes are a fair test of the
16-bit kernels, and three wrong kernels restated on the oracle that the default data cannot see and the regimes can."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from oracle.torch_cpu_step import TorchCpuStep
from tests.regimes import REGIMES, SHAPES, regime_eps, regime_inputs
from tests.util import PRE_BN_BIAS, rel_l2

GATE = 5e-4                  # the layer-local gate of the 16-bit modes (tests/test_parity_gpu.py)
BLOCKS = [f"encoder.{i}" for i in range(4)] + [f"decoder.{i}" for i in range(3)] + ["final_layer"]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 6, False), (64, 16, 5, True), (32, 3, 9, False)])
def test_oracle_matches_torch_f64_on_every_regime(regime, H, L, B, gen):
    """ELBO scalars, x_hat and every gradient of the numpy oracle against torch f64 autograd over the same ATen operators the
    reference dispatches, BCE with fractional targets and kld_weight 2: within 1e-9 (tests/test_oracle.py's f64 tolerance)."""
    kw = 2.0
    x, p = regime_inputs(regime, H, L, B, gen)
    eps = regime_eps(L, B)
    c = vo.forward(p, x, eps, None, train=True)
    lo = vo.loss(c, kw)
    g = vo.backward(p, c, kw)
    st = TorchCpuStep(p, kld_weight=kw, dtype=torch.float64)
    xt = torch.from_numpy(x)
    xhat, mu, lv, _ = st.forward(xt, torch.from_numpy(eps))
    rec = F.binary_cross_entropy(xhat, xt)
    kld = -0.5 * torch.mean(torch.sum(1 + lv - mu ** 2 - torch.exp(lv), dim=-1))
    (rec + kw * kld).backward()
    want = [float((rec + kw * kld).detach()), float(rec.detach()), float(-kld.detach())]
    np.testing.assert_allclose([float(lo["loss"]), float(lo["reconstruction_loss"]), float(lo["kld_loss"])], want, rtol=1e-9)
    gaps = {"xhat": rel_l2(c["output"], xhat.detach().numpy())}
    for n, v in st.p.items():
        if n not in PRE_BN_BIAS:
            gaps[n] = rel_l2(g[n], v.grad.numpy())
    bad = {k: v for k, v in gaps.items() if not v < 1e-9}
    assert not bad, bad


@pytest.mark.parametrize("storage", [None, "bf16", "f16"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,L,B,gen", SHAPES)
def test_regime_conditions(regime, H, L, B, gen, storage):
    """What makes a regime a fair test at the shapes the GPU tests use, with the storage-emulating oracle: everything finite, no
    BatchNorm channel near zero variance (where the reference itself is ill-conditioned), f16-scaled stored gradients 16x below
    the f16 maximum, x_hat away from the BCE clamps."""
    x, p = regime_inputs(regime, H, L, B, gen)
    c = vo.forward(p, x, regime_eps(L, B), None, train=True, storage=storage)
    g = vo.backward(p, c)
    lo = vo.loss(c)
    assert all(np.isfinite(v).all() for v in g.values()) and all(np.isfinite(float(v)) for v in lo.values())
    assert all(np.isfinite(c[n + ".y"]).all() for n in BLOCKS) and np.isfinite(c["output"]).all()
    min_var = min(float(c[n + ".bn"][3].min()) for n in BLOCKS)
    assert min_var > 2 * vo.BN_EPS, min_var
    gs = vo.f16_grad_scale(B, H) if storage == "f16" else 1.0
    max_dz = max(float(np.abs(g[n + ".dz"]).max()) for n in BLOCKS) * gs
    assert max_dz < 65504 / 16, max_dz
    assert 1e-6 < c["output"].min() and c["output"].max() < 1 - 1e-6, (c["output"].min(), c["output"].max())


def _step(regime, storage, H=32, L=16, B=6, gen=False):
    x, p = regime_inputs(regime, H, L, B, gen)
    c = vo.forward(p, x, regime_eps(L, B), None, train=True, storage=storage)
    return x, p, c, vo.backward(p, c)


def _bf16(v):
    return vo.round_storage(v, "bf16")


@pytest.mark.parametrize("storage", [None, "bf16"])
def test_mutant_x_staged_in_bf16(storage):
    """conv1_fwd / conv1_wgrad reading x rounded to bf16: bit-identical on {0, 1} cells, far above the gate on velocities."""
    for regime, seen in (("default", False), ("velocity", True), ("velocity+trained", True)):
        x, p, c, g = _step(regime, storage)
        w, b = p["encoder.0.0.weight"], p["encoder.0.0.bias"]
        dy, _, _ = vo.bn_train_bwd(g["encoder.0.dz"], p["encoder.0.1.weight"], c["encoder.0.bn"])
        assert np.array_equal(vo.conv_wgrad(x, dy, 2)[0], g["encoder.0.0.weight"])       # (the oracle's own route)
        moved = {"y0": rel_l2(vo.round_storage(vo.conv_fwd(_bf16(x), w, b, 2), storage), c["encoder.0.y"]),
                 "encoder.0.0.weight": rel_l2(vo.conv_wgrad(_bf16(x), dy, 2)[0], g["encoder.0.0.weight"])}
        for k, v in moved.items():
            assert (v > GATE) if seen else (v == 0.0), (regime, k, v)


@pytest.mark.parametrize("storage", [None, "bf16", "f16"])
def test_mutant_bce_as_a_select_on_the_target(storage):
    """BCE and its gradient with t replaced by t > 0.5 (a select instead of the two-term form): identical on binary targets; on
    fractional ones the reconstruction term, the output conv's gradients and dz7 all move by more than the gate."""
    for regime, seen in (("default", False), ("trained", False), ("velocity", True), ("velocity+trained", True)):
        x, p, c, g = _step(regime, storage)
        gs = vo.f16_grad_scale(*x.shape[:3:2]) if storage == "f16" else 1.0
        xh, a = c["output"], c["final_conv.in"]
        t = (x > 0.5).astype(np.float64)
        rec = float(np.mean(-(t * np.log(xh) + (1 - t) * np.log1p(-xh))))
        dlogit = (xh - t) / np.maximum(xh * (1 - xh), 1e-12) / xh.size * xh * (1 - xh)      # (the oracle's own expression)
        dl = vo.round_storage(dlogit, storage, gs)
        da = vo.conv_dgrad(dl, vo.round_storage(p["final_layer.3.weight"], storage), 1, a.shape[2:])
        ref = float(vo.loss(c)["reconstruction_loss"])
        moved = {"recon": abs(rec / ref - 1),
                 "final_layer.3.weight": rel_l2(vo.conv_wgrad(a, dl, 1)[0], g["final_layer.3.weight"]),
                 "final_layer.3.bias": rel_l2(dlogit.sum(axis=(0, 2, 3)), g["final_layer.3.bias"]),
                 "dz7": rel_l2(vo.round_storage(vo.lrelu_bwd(c["final_layer.z"], da), storage, gs), g["final_layer.dz"])}
        for k, v in moved.items():
            assert (v > GATE) if seen else (v < 1e-12), (regime, k, v)


@pytest.mark.parametrize("storage", [None, "bf16", "f16"])
def test_mutant_bn_backward_loses_gammas_sign(storage):
    """bn_train_bwd with |gamma|: nothing moves while every gamma is positive (perturbed_params: 1 +- 0.2); with trained-like
    gammas every block's conv weight gradient and the gradient it hands upstream move by more than the gate."""
    for regime, seen in (("default", False), ("velocity", False), ("trained", True), ("velocity+trained", True)):
        x, p, c, g = _step(regime, storage)
        gs = vo.f16_grad_scale(*x.shape[:3:2]) if storage == "f16" else 1.0
        rg = lambda v: vo.round_storage(v, storage, gs)          # noqa: E731
        for i, n in enumerate(BLOCKS):
            gamma = p[n + ".1.weight"]
            assert (gamma.min() > 0) != seen
            dy, _, _ = vo.bn_train_bwd(g[n + ".dz"], np.abs(gamma), c[n + ".bn"])
            first, xin = i == 0, c[n + ".in"]
            dyr = dy if first else rg(dy)
            w = p[n + ".0.weight"] if first else vo.round_storage(p[n + ".0.weight"], storage)
            if i >= 4:
                dx, dw, _ = vo.convT_bwd(xin, w, dyr)
            else:
                dw, dx = vo.conv_wgrad(xin, dyr, 2)[0], vo.conv_dgrad(dyr, w, 2, xin.shape[2:])
            moved = {n + ".0.weight": rel_l2(dw, g[n + ".0.weight"])}
            if 0 < i != 4:      # the stored gradient of the block in front (encoder.0 has none; decoder.0 hands dd0 to the latent block)
                up = BLOCKS[i - 1]
                moved["dz of " + up] = rel_l2(rg(vo.lrelu_bwd(c[up + ".z"], dx)), g[up + ".dz"])
            if i == 4:
                moved["dd0"] = rel_l2(rg(dx).reshape(g["__dd0"].shape), g["__dd0"])
            for k, v in moved.items():
                assert (v > GATE) if seen else (v == 0.0), (regime, k, v)
