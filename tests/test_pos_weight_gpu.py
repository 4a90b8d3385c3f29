"""Positive-class weight of the BCE term (VanillaVAE(pos_weight=w), vae_set_recon_loss_ex, vae_elbo_generic_w) on the GPU.
The yardstick is torch CPU f64 autograd of F.binary_cross_entropy(xhat, x, weight=1 + (w - 1) x) over
oracle.torch_cpu_step.TorchCpuStep.forward; the layer-local tests use the numpy f64 wbce_reference of
tests/test_pos_weight_host.py (checked against torch autograd there).  Targets: the synthetic 0/1 pianoroll and the velocity
roll of tests/test_recon_loss_gpu.py (cells scaled by U(0.2, 1), exact 0s and 1s kept)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from oracle.torch_cpu_step import TorchCpuStep
from tests.test_pos_weight_host import wbce_reference
from tests.test_recon_loss_gpu import _dbg, velocity_roll
from tests.util import PRE_BN_BIAS, flat_grad_dict, load_params, make_model, perturbed_params, rel_l2

pytestmark = pytest.mark.gpu
GRAD_TOL_F32 = 5e-3          # tests/test_parity_gpu.py GRAD_TOL["f32"] (LeakyReLU kink ties)
LAYER_TOL = 5e-4             # the layer-local gate of tests/test_parity_gpu.py


def inputs(B, H, L, seed, velocity):
    x = velocity_roll(B, H, seed) if velocity else vo.synth_pianoroll(B, H, seed).astype(np.float32)
    eps = vo.counter_normal(B * L, seed, 5).reshape(B, L).astype(np.float32)
    return x, eps


def w_model(H, L, gen, dtype, p, w, kld_weight=1.0):
    m = make_model(H, L, gen, dtype, p, kld_weight=kld_weight)
    m.pos_weight = w
    return m


def weighted_bce(xhat, x, w):
    return F.binary_cross_entropy(xhat, x, weight=1 + (w - 1) * x)


class WbceCpuStep(TorchCpuStep):
    """TorchCpuStep with the positive-class-weighted BCE as the reconstruction term."""
    pos_weight = 1.0

    def step(self, x, eps):
        xhat, mu, lv, z = self.forward(x, eps)
        self.opt.zero_grad()
        recon = weighted_bce(xhat, x, self.pos_weight)
        kld = -0.5 * torch.mean(torch.sum(1 + lv - mu ** 2 - torch.exp(lv), dim=-1))
        loss = recon + self.kld_weight * kld
        loss.backward()
        self.opt.step()
        self.sched.step()
        return float(loss.detach()), float(recon.detach()), float(-kld.detach())


def cpu_wbce_grads(p, x, eps, kld_weight, w):
    st = TorchCpuStep(p, kld_weight=kld_weight, dtype=torch.float64)
    xt = torch.from_numpy(x.astype(np.float64))
    xhat, mu, lv, _ = st.forward(xt, torch.from_numpy(eps.astype(np.float64)))
    recon = weighted_bce(xhat, xt, w)
    kld = -0.5 * torch.mean(torch.sum(1 + lv - mu ** 2 - torch.exp(lv), dim=-1))
    loss = recon + kld_weight * kld
    loss.backward()
    return [float(loss.detach()), float(recon.detach()), float(-kld.detach())], xhat.detach().numpy(), {k: v.grad.numpy() for k, v in st.p.items()}


def f16_scale(B, H, w):
    """the test's own restatement of the f16 rule (vae_ctx.h: set_grad_scale): the BCE scale lowered by 2^ceil(log2 w), floored at 1"""
    return max(1.0, vo.f16_grad_scale(B, H) / 2.0 ** max(0, math.ceil(math.log2(w))))


# ---- the context-free entry point ---------------------------------------------------------------------------------------------
def _generic_w(xh, tg, mu, lv, kw, w):
    from torch_vae_amd import _lib
    n, (B, L) = xh.numel(), mu.shape
    out3 = torch.empty(3, device="cuda")
    gx, gm, gl = torch.empty_like(xh), torch.empty_like(mu), torch.empty_like(lv)
    _lib.check(_lib.lib().vae_elbo_generic_w(xh.data_ptr(), tg.data_ptr(), mu.data_ptr(), lv.data_ptr(), n, B, L, kw, _lib.RECON_WBCE, w,
                                            _lib.KL_PLAIN, 0.0, out3.data_ptr(), gx.data_ptr(), gm.data_ptr(), gl.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "vae_elbo_generic_w")
    torch.cuda.synchronize()
    return out3, gx, gm, gl


def test_generic_wbce_elbo_against_torch():
    rng = np.random.default_rng(3)
    B, L, n, w, kw = 7, 16, 7 * 1000, 8.0, 3.0
    xh = torch.from_numpy(rng.uniform(0.0, 1.0, n)).float().cuda()
    tg = torch.from_numpy(rng.uniform(0.0, 1.0, n) * (rng.uniform(size=n) < 0.6)).float().cuda()
    mu = torch.from_numpy(rng.normal(size=(B, L))).float().cuda()
    lv = torch.from_numpy(0.5 * rng.normal(size=(B, L))).float().cuda()
    out3, gx, gm, gl = _generic_w(xh, tg, mu, lv, kw, w)
    x64, m64, l64 = (t.cpu().double().requires_grad_() for t in (xh, mu, lv))
    recon = weighted_bce(x64, tg.cpu().double(), w)
    kld = -0.5 * torch.mean(torch.sum(1 + l64 - m64 ** 2 - torch.exp(l64), dim=-1))
    loss = recon + kw * kld
    loss.backward()
    print("generic out3", out3.tolist(), [loss.item(), recon.item(), -kld.item()])
    np.testing.assert_allclose(out3.tolist(), [loss.item(), recon.item(), -kld.item()], rtol=1e-6)
    for got, want in ((gx, x64.grad), (gm, m64.grad), (gl, l64.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    # exact 0 and 1 in xhat against targets 0 and 1: the -100 clamp of the logs and the 1e-12 clamp of the denominator, each
    # times W - against torch's own f32 CPU arithmetic
    xh2, tg2 = xh.clone(), tg.clone()
    xh2[:8] = torch.tensor([0., 0., 1., 1., 0., 1., 0., 1.])
    tg2[:8] = torch.tensor([1., 0., 0., 1., 1., 0., 0.5, 0.5])
    out3, gx, _, _ = _generic_w(xh2, tg2, mu, lv, kw, w)
    x32 = xh2.cpu().requires_grad_()
    recon32 = weighted_bce(x32, tg2.cpu(), w)
    recon32.backward()
    print("generic clamps", out3[1].item(), recon32.item(), gx[:8].tolist(), x32.grad[:8].tolist())
    assert recon32.item() > 100.0 * w * 2 / n                                   # the clamped cells dominate
    np.testing.assert_allclose(out3[1].item(), recon32.item(), rtol=1e-6)
    np.testing.assert_allclose(gx.cpu().numpy(), x32.grad.numpy(), rtol=1e-6, atol=0.0)


# ---- f32 against torch f64 autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,L,B,gen,w,velocity", [(32, 16, 32, False, 8.0, False), (64, 16, 5, True, 8.0, False), (128, 16, 3, True, 8.0, False),
                                                  (32, 16, 32, False, 0.5, True)])
def test_f32_wbce_step_against_torch_autograd(H, L, B, gen, w, velocity):
    p = perturbed_params(L, H, 51, gen)
    x, eps = inputs(B, H, L, 52, velocity)
    want3, want_xhat, want_g = cpu_wbce_grads(p, x, eps, 2.0, w)
    m = w_model(H, L, gen, "f32", p, w, kld_weight=2.0)
    out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()
    got = flat_grad_dict(m)
    bad = {n: rel_l2(got[n], want_g[n].reshape(-1)) for n in got if n not in PRE_BN_BIAS}
    print("f32 step", out3.tolist(), want3, rel_l2(xhat.cpu().numpy(), want_xhat), max(bad.values()))
    np.testing.assert_allclose(out3.tolist(), want3, rtol=1e-4)
    assert rel_l2(xhat.cpu().numpy(), want_xhat) < 1e-4
    assert max(bad.values()) < GRAD_TOL_F32, {n: v for n, v in bad.items() if v >= GRAD_TOL_F32}


def test_f32_wbce_train_one_epoch_against_cpu_loop():
    """train_one_epoch (one library call per step) takes config.recon_pos_weight: 3 steps of AdamW + OneCycle against the same
    loop on torch CPU f64 autograd with the weighted BCE."""
    from argparse import Namespace
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    H, L, B, steps, total, kw, w = 32, 16, 4, 3, 10, 1.0, 8.0
    p = vo.init_params(L, H, 61, False)
    batches = [inputs(B, H, L, 70 + s, False) for s in range(steps)]
    cpu = WbceCpuStep(p, kld_weight=kw, batch=B, total_steps=total, dtype=torch.float64)
    cpu.pos_weight = w
    want = [cpu.step(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(e.astype(np.float64))) for x, e in batches]
    model = make_model(H, L, False, "f32", p, kld_weight=kw)
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                    epochs=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0,
                    recon_pos_weight=w)
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
    assert total_step == steps and len(got) == steps and model.pos_weight == w
    print("train_one_epoch", got, want)
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-4)
    np.testing.assert_allclose(res["loss"], np.mean([x[0] for x in want]), rtol=2e-4)


def test_f32_wbce_torch_optimiser_path_of_train_one_epoch():
    """the unfused loop (model.forward -> model.loss -> backward -> a torch optimiser) of train_one_epoch honours the weight too"""
    from argparse import Namespace
    from torch_vae_amd.train import train_one_epoch
    H, L, B, kw, w = 32, 16, 4, 1.0, 8.0
    p = vo.init_params(L, H, 61, False)
    x, eps = inputs(B, H, L, 70, False)
    want3, _, _ = cpu_wbce_grads(p, x, eps, kw, w)
    model = make_model(H, L, False, "f32", p, kld_weight=kw)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    cfg = Namespace(world_size=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0, recon_pos_weight=w)
    model.set_next_eps(torch.from_numpy(eps).cuda())
    res, _, _ = train_one_epoch(cfg, model, opt, torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0), model.loss,
                                [(torch.from_numpy(x), torch.zeros(B, dtype=torch.long))], device="cuda", epoch=2)
    np.testing.assert_allclose(res["loss"], want3[0], rtol=1e-4)


# ---- 16-bit: the output conv on its own inputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("H,B,w,velocity", [(128, 3, 8.0, True), (64, 5, 8.0, True), (256, 1, 8.0, True), (128, 3, 32.0, False)])
def test_16bit_output_conv_wbce_on_its_own_inputs(dtype, H, B, w, velocity):
    """The fused output-conv kernels (128: row-streaming; 64 / 256: tiled) with the weight against the storage-emulating oracle on
    the kernel's own input (the stored y7): xhat, dz7, final_layer.3's gradients and the reconstruction term."""
    L, gen = 16, True
    p = perturbed_params(L, H, 41, gen)
    x, eps = inputs(B, H, L, 43, velocity)
    m = w_model(H, L, gen, dtype, p, w)
    out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()
    gs = f16_scale(B, H, w) if dtype == "f16" else 1.0
    y7 = _dbg(m, 7, B * 32 * H * H).cpu().numpy().reshape(B, 32, H, H).astype(np.float64)
    dz7 = _dbg(m, 15, B * 32 * H * H).cpu().numpy().reshape(B, 32, H, H).astype(np.float64) / gs
    grads = flat_grad_dict(m)
    P = lambda k: p[k].astype(np.float64)                  # noqa: E731
    rs = lambda v: vo.round_storage(v, dtype)              # noqa: E731
    rg = lambda v: vo.round_storage(v, dtype, gs)          # noqa: E731
    z7, _ = vo.bn_train_fwd_stored(y7, P("final_layer.1.weight"), P("final_layer.1.bias"), dtype)
    a7, wt = rs(vo.lrelu(z7)), rs(P("final_layer.3.weight"))
    logit = vo.conv_fwd(a7, wt, P("final_layer.3.bias"), 1)
    xt = x.astype(np.float64)
    gaps = {"xhat": rel_l2(vo.sigmoid(logit), xhat.cpu().numpy())}
    xh = xhat.double().cpu().numpy()                       # the backward from the GPU's own xhat
    recon, dlogit = wbce_reference(xh, xt, w)
    gaps["reconstruction_loss"] = abs(out3[1].item() - recon) / recon
    dw, _ = vo.conv_wgrad(a7, rg(dlogit), 1)
    gaps["final_layer.3.weight"] = rel_l2(dw, grads["final_layer.3.weight"].reshape(dw.shape))
    gaps["final_layer.3.bias"] = rel_l2(dlogit.sum(axis=(0, 2, 3)), grads["final_layer.3.bias"])
    gaps["dz7"] = rel_l2(rg(vo.lrelu_bwd(z7, vo.conv_dgrad(rg(dlogit), wt, 1, (H, H)))), dz7)
    print("own inputs", dtype, H, B, w, gs, gaps)
    assert max(gaps.values()) < LAYER_TOL, gaps


def test_f16_wbce_range_at_a_large_weight():
    """H = 128, B = 64, w = 64 on a 0/1 roll: the lowered f16 gradient scale keeps every stored dz7 and every gradient finite, and
    dz7 is not flushed to zero."""
    H, L, B, w = 128, 16, 64, 64.0
    m = w_model(H, L, True, "f16", perturbed_params(L, H, 44, True), w)
    x, eps = inputs(B, H, L, 45, False)
    out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
    dz7 = _dbg(m, 15, B * 32 * H * H)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dz7).all()) and float(dz7.abs().max()) > 0
    assert bool(torch.isfinite(m.flat_grads()).all()) and bool(torch.isfinite(out3).all())
    want, _ = wbce_reference(xhat.double().cpu().numpy(), x.astype(np.float64), w)
    print("f16 range", out3.tolist(), want, float(dz7.abs().max()))
    assert abs(out3[1].item() - want) <= 1e-5 * want


# ---- the kernel families agree ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B,bands", [(3, 0), (5, 4)])
def test_wbce_streaming_and_tiled_output_conv_bit_identical(dtype, B, bands):
    from torch_vae_amd import _lib
    H, L, w = 128, 16, 8.0
    p = perturbed_params(L, H, 13, True)
    x, eps = inputs(B, H, L, 46, True)
    res = []
    for stream in (0, 1):
        m = w_model(H, L, True, dtype, p, w, kld_weight=1.5)
        h = m._context(B).handle
        _lib.check(_lib.lib().vae_set_option(h, b"use_convout_stream", stream), "set")
        _lib.check(_lib.lib().vae_set_option(h, b"knob_convout_bands", bands), "set")
        out3, xhat = m.fused_forward_backward(torch.from_numpy(x).cuda(), eps=torch.from_numpy(eps).cuda())
        res.append((out3.clone(), xhat.clone(), _dbg(m, 15, B * 32 * H * H)))
    torch.cuda.synchronize()
    (o0, x0, d0), (o1, x1, d1) = res
    assert torch.equal(x0, x1) and torch.equal(d0, d1)
    np.testing.assert_allclose(o1.cpu().numpy(), o0.cpu().numpy(), rtol=2e-6)      # (the term's sum is partitioned differently)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_wbce_deferred_and_separate_output_conv_agree(dtype):
    """use_fused_convout 0 / 1 with the weight: the same arithmetic element for element, so xhat, out3, dz7 and every gradient are
    bit-identical.  use_mfma_convout 0 (the VALU kernels, f32 operands) agrees with the 16-bit-operand MFMA kernels within the
    bounds of the MSE test (test_mse_deferred_and_separate_output_conv_agree)."""
    from torch_vae_amd import _lib
    H, L, B, w = 64, 16, 6, 8.0
    p = perturbed_params(L, H, 11, True)
    x, eps = inputs(B, H, L, 47, True)
    res = []
    for opt, val in (("use_fused_convout", 0), ("use_fused_convout", 1), ("use_mfma_convout", 0)):
        m = w_model(H, L, True, dtype, p, w, kld_weight=2.0)
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


def test_weight_one_is_bce_and_switching_back():
    """bf16 at 128x128: a model with pos_weight=1.0 (the weighted kernels), one with pos_weight=None and one switched
    None -> 8 -> None across steps give bit-identical out3, xhat and flat gradients for the same step."""
    from torch_vae_amd.models import VanillaVAE
    H, L, B = 128, 16, 4
    p = perturbed_params(L, H, 71, True)
    xb = torch.from_numpy(vo.synth_pianoroll(B, H, 72)).cuda()
    eps = torch.from_numpy(inputs(B, H, L, 73, False)[1]).cuda()
    res = []
    for kind in (None, "one", "switch"):
        if kind == "one":
            m = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", pos_weight=1.0).cuda()
            load_params(m, p)
        else:
            m = make_model(H, L, True, "bf16", p)
        if kind == "switch":
            m.fused_forward_backward(xb, eps=eps)
            m.pos_weight = 8.0
            o_w, _ = m.fused_forward_backward(xb, eps=eps)
            o_w = o_w.clone()
            m.pos_weight = None
        out3, xhat = m.fused_forward_backward(xb, eps=eps)
        torch.cuda.synchronize()
        res.append((out3.clone(), xhat.clone(), m.flat_grads().clone()))
    for o, xh, g in res[1:]:
        assert torch.equal(o, res[0][0]) and torch.equal(xh, res[0][1]) and torch.equal(g, res[0][2])
    assert not torch.equal(o_w, res[0][0])


# ---- the weight is the forward's -----------------------------------------------------------------------------------------------------
def test_weight_recorded_at_the_forward_and_every_loss_path():
    """model(x) -> loss() -> backward() uses the weight the forward ran with even when pos_weight changes before loss() /
    backward(); fused_forward_backward and fused_train_step give the same; loss() on foreign tensors equals the own forward's;
    an eval-mode forward's loss() is the f64 formula on the returned tensors."""
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen, w = 32, 16, 16, False, 8.0
    p = perturbed_params(L, H, 2, gen)
    x, eps = (torch.from_numpy(a).cuda() for a in inputs(B, H, L, 49, False))
    m1 = w_model(H, L, gen, "f32", p, w, kld_weight=4.0)
    out3, _ = m1.fused_forward_backward(x, eps=eps)
    g1 = m1.flat_grads().clone()
    m2 = w_model(H, L, gen, "f32", p, w, kld_weight=4.0)
    m2.set_next_eps(eps)
    out = m2.forward(x)
    m2.pos_weight = None                    # after the forward: loss() and backward keep the forward's weight
    lo = m2.loss(out)
    lo["loss"].backward()
    np.testing.assert_allclose([lo["loss"].item(), lo["reconstruction_loss"].item(), lo["kld_loss"].item()], out3.tolist(), rtol=1e-5)
    np.testing.assert_allclose(m2.flat_grads().cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-8)
    m3 = w_model(H, L, gen, "f32", p, w, kld_weight=4.0)
    opt = FusedAdamW([{"params": m3.encoder.parameters()}, {"params": m3.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
    o3, _ = m3.fused_train_step(opt, x, eps=eps)
    torch.cuda.synchronize()
    np.testing.assert_allclose(o3.tolist(), out3.tolist(), rtol=1e-5)
    np.testing.assert_allclose(m3.flat_grads().cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-8)
    # foreign tensors (the context-free kernel) against the own forward, values and gradients
    m4 = w_model(H, L, gen, "f32", p, w, kld_weight=4.0)
    m4.set_next_eps(eps)
    out = m4.forward(x)
    foreign = {"output": out["output"] * 1.0, "input": x, "encoded": {"mu": out["encoded"]["mu"] * 1.0, "log_var": out["encoded"]["log_var"] * 1.0}}
    lg, lf = m4.loss(foreign), m4.loss(out)
    for k in ("loss", "reconstruction_loss", "kld_loss"):
        np.testing.assert_allclose(lg[k].item(), lf[k].item(), rtol=1e-6)
    lg["loss"].backward()
    assert rel_l2(m4.flat_grads().cpu().numpy(), g1.cpu().numpy()) < 1e-5
    # eval mode
    m1.eval()
    with torch.no_grad():
        ev = m1.forward(x)
        le = m1.loss(ev)
    want = float(weighted_bce(ev["output"].double().cpu(), x.double().cpu(), w))
    np.testing.assert_allclose(le["reconstruction_loss"].item(), want, rtol=1e-5)


def test_log_likelihood_ignores_the_weight():
    H, L, B, K = 32, 16, 4, 4
    p = perturbed_params(L, H, 5, False)
    x = torch.from_numpy(vo.synth_pianoroll(B, H, 81)).cuda()
    eps = torch.from_numpy(vo.counter_normal(K * B * L, 82, 6).reshape(K, B, L).astype(np.float32)).cuda()
    res = []
    for w in (8.0, None):
        m = w_model(H, L, False, "f32", p, w)
        m.eval()
        ll = m.log_likelihood(x, num_samples=K, eps=eps)
        res.append((ll["log_likelihood"].clone(), ll["elbo"].clone(), ll["log_weights"].clone()))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(res[0][0]).all())
