"""Selectable reconstruction term of the ELBO (VanillaVAE(recon_loss="mse"), vae_set_recon_loss, vae_elbo_generic_ex) on the
GPU.  Targets are velocity-valued rolls: a synthetic pianoroll scaled by U(0.2, 1) per cell, with exact 0s and 1s kept.
The yardstick is torch autograd of F.mse_loss(sigmoid(logit), t) (oracle.torch_cpu_step restates the forward; the numpy MSE
helper of tests/test_recon_loss_host.py is checked against it there)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from oracle.torch_cpu_step import TorchCpuStep
from tests.test_recon_loss_host import mse_reference
from tests.util import PRE_BN_BIAS, flat_grad_dict, load_params, make_model, perturbed_params, rel_l2

pytestmark = pytest.mark.gpu
GRAD_TOL_F32 = 5e-3          # tests/test_parity_gpu.py GRAD_TOL["f32"] (LeakyReLU kink ties)
LAYER_TOL = 5e-4             # the layer-local gate of tests/test_parity_gpu.py


def velocity_roll(B, H, seed):
    x = vo.synth_pianoroll(B, H, seed).astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    v = x * rng.uniform(0.2, 1.0, x.shape)
    v.reshape(-1)[:: 97] = 1.0                              # some exact 1s (and the synthetic roll's 0s)
    return v.astype(np.float32)


def inputs(B, H, L, seed):
    x = velocity_roll(B, H, seed)
    eps = vo.counter_normal(B * L, seed, 5).reshape(B, L).astype(np.float32)
    return x, eps


def mse_model(H, L, gen, dtype, p, kld_weight=1.0):
    m = make_model(H, L, gen, dtype, p, kld_weight=kld_weight)
    m.recon_loss = "mse"
    return m


class MseCpuStep(TorchCpuStep):
    """TorchCpuStep with F.mse_loss as the reconstruction term."""

    def step(self, x, eps):
        xhat, mu, lv, z = self.forward(x, eps)
        self.opt.zero_grad()
        recon = F.mse_loss(xhat, x)
        kld = -0.5 * torch.mean(torch.sum(1 + lv - mu ** 2 - torch.exp(lv), dim=-1))
        loss = recon + self.kld_weight * kld
        loss.backward()
        self.opt.step()
        self.sched.step()
        return float(loss.detach()), float(recon.detach()), float(-kld.detach())


def cpu_mse_grads(p, x, eps, kld_weight):
    st = TorchCpuStep(p, kld_weight=kld_weight, dtype=torch.float64)
    xt = torch.from_numpy(x.astype(np.float64))
    xhat, mu, lv, _ = st.forward(xt, torch.from_numpy(eps.astype(np.float64)))
    recon = F.mse_loss(xhat, xt)
    kld = -0.5 * torch.mean(torch.sum(1 + lv - mu ** 2 - torch.exp(lv), dim=-1))
    loss = recon + kld_weight * kld
    loss.backward()
    return [float(loss), float(recon), float(-kld)], xhat.detach().numpy(), {k: v.grad.numpy() for k, v in st.p.items()}


@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 32, False), (64, 16, 5, True), (128, 16, 3, True)])
def test_f32_mse_step_against_torch_autograd(H, L, B, gen):
    p = perturbed_params(L, H, 51, gen)
    x, eps = inputs(B, H, L, 52)
    want3, want_xhat, want_g = cpu_mse_grads(p, x, eps, 2.0)
    m = mse_model(H, L, gen, "f32", p, kld_weight=2.0)
    out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()
    np.testing.assert_allclose(out3.tolist(), want3, rtol=1e-4)
    assert rel_l2(xhat.cpu().numpy(), want_xhat) < 1e-4
    got = flat_grad_dict(m)
    bad = {n: rel_l2(got[n], want_g[n].reshape(-1)) for n in got if n not in PRE_BN_BIAS}
    assert max(bad.values()) < GRAD_TOL_F32, {n: v for n, v in bad.items() if v >= GRAD_TOL_F32}


def test_f32_mse_train_one_epoch_against_cpu_loop():
    """train_one_epoch (one library call per step) follows the model's recon_loss: 3 steps of AdamW + OneCycle against the
    same loop on torch CPU f64 autograd with an MSE loss."""
    from argparse import Namespace
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    H, L, B, steps, total, kw = 32, 16, 4, 3, 10, 1.0
    p = vo.init_params(L, H, 61, False)
    batches = [inputs(B, H, L, 70 + s) for s in range(steps)]
    cpu = MseCpuStep(p, kld_weight=kw, batch=B, total_steps=total, dtype=torch.float64)
    want = [cpu.step(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(e.astype(np.float64))) for x, e in batches]
    model = mse_model(H, L, False, "f32", p, kld_weight=kw)
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                    epochs=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=total)
    it = iter([torch.from_numpy(e).cuda() for _, e in batches])
    got = []
    orig = model.fused_train_step

    def step(o, x, **k):
        out3, xhat = orig(o, x, **{**k, "eps": next(it)})
        got.append(out3.tolist())
        return out3, xhat
    model.fused_train_step = step
    loader = [(torch.from_numpy(x), torch.zeros(B, dtype=torch.long)) for x, _ in batches]
    res, total_step, _ = train_one_epoch(cfg, model, opt, sched, model.loss, loader, device="cuda", epoch=1)
    assert total_step == steps and len(got) == steps
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-4)
    np.testing.assert_allclose(res["loss"], np.mean([w[0] for w in want]), rtol=2e-4)


def _dbg(m, which, n):
    from torch_vae_amd import _lib
    t = torch.empty(n, device="cuda")
    _lib.check(_lib.lib().vae_debug_tensor(m._ctx.handle, which, t.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "dbg")
    return t


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("H,B", [(128, 3), (64, 5), (256, 1)])       # 128: row-streaming kernel; 64 / 256: tiled kernel
def test_16bit_output_conv_mse_on_its_own_inputs(dtype, H, B):
    """The fused output-conv kernels in MSE mode against the storage-emulating oracle on the kernel's own input (the stored y7):
    xhat, dz7, final_layer.3's gradients and the reconstruction term."""
    L, gen = 16, True
    p = perturbed_params(L, H, 41, gen)
    x, eps = inputs(B, H, L, 43)
    m = mse_model(H, L, gen, dtype, p)
    out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()
    gs = vo.f16_grad_scale(B, H) if dtype == "f16" else 1.0
    y7 = _dbg(m, 7, B * 32 * H * H).cpu().numpy().reshape(B, 32, H, H).astype(np.float64)
    dz7 = _dbg(m, 15, B * 32 * H * H).cpu().numpy().reshape(B, 32, H, H).astype(np.float64) / gs
    grads = flat_grad_dict(m)
    P = lambda k: p[k].astype(np.float64)                  # noqa: E731
    rs = lambda v: vo.round_storage(v, dtype)              # noqa: E731
    rg = lambda v: vo.round_storage(v, dtype, gs)          # noqa: E731
    z7, _ = vo.bn_train_fwd_stored(y7, P("final_layer.1.weight"), P("final_layer.1.bias"), dtype)
    a7, w = rs(vo.lrelu(z7)), rs(P("final_layer.3.weight"))
    logit = vo.conv_fwd(a7, w, P("final_layer.3.bias"), 1)
    xt = x.astype(np.float64)
    gaps = {"xhat": rel_l2(vo.sigmoid(logit), xhat.cpu().numpy())}
    xh = xhat.double().cpu().numpy()                       # the backward from the GPU's own xhat
    recon, dlogit = mse_reference(xh, xt)
    gaps["reconstruction_loss"] = abs(out3[1].item() - recon) / recon
    dw, _ = vo.conv_wgrad(a7, rg(dlogit), 1)
    gaps["final_layer.3.weight"] = rel_l2(dw, grads["final_layer.3.weight"].reshape(dw.shape))
    gaps["final_layer.3.bias"] = rel_l2(dlogit.sum(axis=(0, 2, 3)), grads["final_layer.3.bias"])
    gaps["dz7"] = rel_l2(rg(vo.lrelu_bwd(z7, vo.conv_dgrad(rg(dlogit), w, 1, (H, H)))), dz7)
    assert max(gaps.values()) < LAYER_TOL, gaps


def test_f16_mse_dz7_finite_at_bench_size():
    """B = 256 at 128x128: the unchanged f16 gradient scale keeps every stored MSE dz7 finite (|dlogit| <= 0.5/N < 1/N)."""
    H, L, B = 128, 16, 256
    m = mse_model(H, L, True, "f16", perturbed_params(L, H, 44, True))
    x, eps = inputs(B, H, L, 45)
    out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
    dz7 = _dbg(m, 15, B * 32 * H * H)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dz7).all()) and float(dz7.abs().max()) > 0
    assert bool(torch.isfinite(m.flat_grads()).all()) and bool(torch.isfinite(out3).all())
    want = float(((xhat.double() - torch.from_numpy(x).cuda().double()) ** 2).mean())
    assert abs(out3[1].item() - want) <= 1e-5 * want


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B,bands", [(3, 0), (5, 4)])
def test_mse_streaming_and_tiled_output_conv_bit_identical(dtype, B, bands):
    from torch_vae_amd import _lib
    H, L = 128, 16
    p = perturbed_params(L, H, 13, True)
    x, eps = inputs(B, H, L, 46)
    res = []
    for stream in (0, 1):
        m = mse_model(H, L, True, dtype, p, kld_weight=1.5)
        h = m._context(B).handle
        _lib.check(_lib.lib().vae_set_option(h, b"use_convout_stream", stream), "set")
        _lib.check(_lib.lib().vae_set_option(h, b"knob_convout_bands", bands), "set")
        out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
        res.append((out3.clone(), xhat.clone(), _dbg(m, 15, B * 32 * H * H), m.flat_grads().clone()))
    torch.cuda.synchronize()
    (o0, x0, d0, g0), (o1, x1, d1, g1) = res
    assert torch.equal(x0, x1) and torch.equal(d0, d1)
    np.testing.assert_allclose(o1.cpu().numpy(), o0.cpu().numpy(), rtol=2e-6)
    assert rel_l2(g1.cpu().numpy(), g0.cpu().numpy()) < {"bf16": 3e-2, "f16": 5e-3}[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_mse_deferred_and_separate_output_conv_agree(dtype):
    """use_fused_convout 0 / 1 (one kernel for the layer's forward and backward, or convout_fwd_mfma + convout_bwd_mfma) in MSE
    mode: the same arithmetic element for element, so xhat, out3, dz7 and every gradient are bit-identical.  use_mfma_convout 0
    (the VALU kernels, f32 operands) agrees with the 16-bit-operand MFMA kernels within the bounds of the BCE test
    (test_mfma_and_valu_output_conv_backward_agree)."""
    from torch_vae_amd import _lib
    H, L, B = 64, 16, 6
    p = perturbed_params(L, H, 11, True)
    x, eps = inputs(B, H, L, 47)
    res = []
    for opt, val in (("use_fused_convout", 0), ("use_fused_convout", 1), ("use_mfma_convout", 0)):
        m = mse_model(H, L, True, dtype, p, kld_weight=2.0)
        _lib.check(_lib.lib().vae_set_option(m._context(B).handle, opt.encode(), val), "set")
        out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
        res.append((out3.clone(), xhat.clone(), _dbg(m, 15, B * 32 * H * H), flat_grad_dict(m)))
    torch.cuda.synchronize()
    (o0, x0, d0, g0), (o1, x1, d1, g1), (o2, x2, _, g2) = res
    assert torch.equal(o0, o1) and torch.equal(x0, x1) and torch.equal(d0, d1)
    assert all(np.array_equal(g0[n], g1[n]) for n in g0), [n for n in g0 if not np.array_equal(g0[n], g1[n])]
    np.testing.assert_allclose(o2.cpu().numpy(), o0.cpu().numpy(), rtol={"bf16": 1e-2, "f16": 2e-3}[dtype])
    for n in g0:
        if n in PRE_BN_BIAS:
            continue
        a, b = g2[n].astype(np.float64), g0[n].astype(np.float64)
        assert float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30)) > 0.995, n
    assert rel_l2(g2["final_layer.3.bias"], g0["final_layer.3.bias"]) < 2e-3


def test_generic_mse_elbo_against_torch():
    from torch_vae_amd import _lib
    rng = np.random.default_rng(3)
    B, L, n = 7, 16, 7 * 1000
    xh = torch.from_numpy(rng.uniform(0.0, 1.0, n)).float().cuda()
    tg = torch.from_numpy(rng.uniform(0.0, 1.0, n) * (rng.uniform(size=n) < 0.6)).float().cuda()
    mu = torch.from_numpy(rng.normal(size=(B, L))).float().cuda()
    lv = torch.from_numpy(0.5 * rng.normal(size=(B, L))).float().cuda()
    kw = 3.0
    out3 = torch.empty(3, device="cuda")
    gx, gm, gl = torch.empty_like(xh), torch.empty_like(mu), torch.empty_like(lv)
    st = torch.cuda.current_stream().cuda_stream
    args = (xh.data_ptr(), tg.data_ptr(), mu.data_ptr(), lv.data_ptr(), n, B, L, kw)
    outs = (out3.data_ptr(), gx.data_ptr(), gm.data_ptr(), gl.data_ptr(), st)
    assert _lib.lib().vae_elbo_generic_ex(*args, 7, *outs) != 0            # unknown term: an error, nothing launched
    _lib.check(_lib.lib().vae_elbo_generic_ex(*args, _lib.RECON_MSE, *outs), "vae_elbo_generic_ex")
    torch.cuda.synchronize()
    x64, m64, l64 = (t.cpu().double().requires_grad_() for t in (xh, mu, lv))
    recon = F.mse_loss(x64, tg.cpu().double())
    kld = -0.5 * torch.mean(torch.sum(1 + l64 - m64 ** 2 - torch.exp(l64), dim=-1))
    loss = recon + kw * kld
    loss.backward()
    np.testing.assert_allclose(out3.tolist(), [loss.item(), recon.item(), -kld.item()], rtol=1e-6)
    for got, want in ((gx, x64.grad), (gm, m64.grad), (gl, l64.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-6 * float(want.abs().max()))


def test_mse_loss_on_foreign_tensors_equals_own_forward():
    """the MSE mirror of test_generic_loss_and_extra_gradients"""
    H, L, B, gen = 32, 16, 8, False
    p = perturbed_params(L, H, 3, gen)
    x, eps = (torch.from_numpy(a).cuda() for a in inputs(B, H, L, 48))
    m = mse_model(H, L, gen, "f32", p)
    m.set_next_eps(eps)
    out = m.forward(x)
    foreign = {"output": out["output"] * 1.0, "input": x, "encoded": {"mu": out["encoded"]["mu"] * 1.0, "log_var": out["encoded"]["log_var"] * 1.0}}
    lg = m.loss(foreign)
    lf = m.loss(out)
    for k in ("loss", "reconstruction_loss", "kld_loss"):
        np.testing.assert_allclose(lg[k].item(), lf[k].item(), rtol=1e-6)
    np.testing.assert_allclose(lg["reconstruction_loss"].item(), float(((out["output"].double() - x.double()) ** 2).mean()), rtol=1e-6)
    lg["loss"].backward()
    g_generic = m.flat_grads().clone()
    m2 = mse_model(H, L, gen, "f32", p)
    m2.fused_forward_backward(x, eps=eps)
    assert rel_l2(g_generic.cpu().numpy(), m2.flat_grads().cpu().numpy()) < 1e-5


def test_mse_autograd_fused_and_one_call_paths_agree():
    """model(x) -> loss() -> backward(), fused_forward_backward and fused_train_step give the same MSE gradients; the term is
    the one recorded at the forward even when recon_loss changes before loss() / backward; an eval-mode forward's loss() is
    mean((xhat - x)^2) of the returned tensors."""
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen = 32, 16, 16, False
    p = perturbed_params(L, H, 2, gen)
    x, eps = (torch.from_numpy(a).cuda() for a in inputs(B, H, L, 49))
    m1 = mse_model(H, L, gen, "f32", p, kld_weight=4.0)
    out3, _ = m1.fused_forward_backward(x, eps=eps)
    g1 = m1.flat_grads().clone()
    m2 = mse_model(H, L, gen, "f32", p, kld_weight=4.0)
    m2.set_next_eps(eps)
    out = m2.forward(x)
    m2.recon_loss = "bce"                   # after the forward: loss() and backward keep the forward's MSE
    lo = m2.loss(out)
    lo["loss"].backward()
    np.testing.assert_allclose([lo["loss"].item(), lo["reconstruction_loss"].item(), lo["kld_loss"].item()], out3.tolist(), rtol=1e-6)
    np.testing.assert_allclose(m2.flat_grads().cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-8)
    m3 = mse_model(H, L, gen, "f32", p, kld_weight=4.0)
    opt = FusedAdamW([{"params": m3.encoder.parameters()}, {"params": m3.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
    o3, _ = m3.fused_train_step(opt, x, eps=eps)
    torch.cuda.synchronize()
    np.testing.assert_allclose(o3.tolist(), out3.tolist(), rtol=1e-6)
    np.testing.assert_allclose(m3.flat_grads().cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-8)
    # eval mode
    m1.eval()
    with torch.no_grad():
        ev = m1.forward(x)
        le = m1.loss(ev)
    want = float(((ev["output"].double() - x.double()) ** 2).mean())
    np.testing.assert_allclose(le["reconstruction_loss"].item(), want, rtol=1e-5)


def test_bce_default_unchanged_and_switching_back():
    """bf16 at 128x128: a model built without recon_loss, one built with recon_loss="bce" and one switched bce -> mse -> bce
    across steps give bit-identical out3, xhat and flat gradients for the same BCE step."""
    from torch_vae_amd.models import VanillaVAE
    H, L, B = 128, 16, 4
    p = perturbed_params(L, H, 71, True)
    xb = torch.from_numpy(vo.synth_pianoroll(B, H, 72)).cuda()
    xv, eps = (torch.from_numpy(a).cuda() for a in inputs(B, H, L, 73))
    res = []
    for kind in (None, "bce", "switch"):
        if kind == "bce":
            m = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", recon_loss="bce").cuda()
            load_params(m, p)
        else:
            m = make_model(H, L, True, "bf16", p)
        if kind == "switch":
            m.fused_forward_backward(xb, eps=eps)
            m.recon_loss = "mse"
            o_mse, _ = m.fused_forward_backward(xv, eps=eps)
            m.recon_loss = "bce"
        out3, xhat = m.fused_forward_backward(xb, eps=eps)
        torch.cuda.synchronize()
        res.append((out3.clone(), xhat.clone(), m.flat_grads().clone()))
    for o, xh, g in res[1:]:
        assert torch.equal(o, res[0][0]) and torch.equal(xh, res[0][1]) and torch.equal(g, res[0][2])
    assert not torch.equal(o_mse, res[0][0])
