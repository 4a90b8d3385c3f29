"""Total-correlation objective (beta-TCVAE) on the GPU: the kernels behind vae_total_correlation on given latents, and
VanillaVAE(tc_weight=...) / VAE_KL_TC on every step path.

The yardstick is torch f64 autograd on the CPU of the definition (tests/test_tc_host.py: tc_parts), at step level over
oracle.torch_cpu_step.TorchCpuStep.forward (cpu_tc_step) - never the code under test.  Kernel-level gates, on the f32 inputs the
kernels themselves read:
    value     |TC - ref| <= 1e-4 + 1e-5 |ref|          (1e-4 nats: the latent-statistics tolerance; the relative term covers the
                                                         f32 sum over d at large L)
    gradient  ||g - ref|| <= 1e-4 ||ref|| + 1e-5 (||g_joint|| + ||g_dims||)   (the layer-local gate, and the floor of a difference
                                                         of two f32 results: it decides the cases whose true gradient is 0)
Step-level tolerances are the project's existing ones for the same comparisons (tests/test_kl_control_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.test_kl_control_host import synth_inputs
from tests.test_tc_host import (GRAD_FLOOR, GRAD_REL, KERNEL_SHAPES, REGIMES, VALUE_ABS, VALUE_REL, TcCpuStep, assert_gate_not_vacuous,
                                cpu_tc_step, kernel_case, tc_autograd)
from tests.util import PRE_BN_BIAS, flat_grad_dict, make_model, perturbed_params, profile_sequence, rel_l2

pytestmark = pytest.mark.gpu
GRAD_TOL_F32 = 5e-3          # tests/test_parity_gpu.py GRAD_TOL["f32"] (LeakyReLU kink ties)
BETA = 2.0                   # kld_weight: a wrong factor cannot hide behind a weight of 1
TC_WEIGHTS = [4.0, 0.25]     # both signs of (tc_weight - 1)
SHAPES = [(32, 16, 32, False), (64, 16, 5, True), (128, 16, 3, True), (64, 128, 6, True), (32, 10, 8, False)]   # test_kl_control_gpu.SHAPES
SMALL = (32, 16, 32, False)


def gpu(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def run_kernels(mu, lv, eps, grad=True):
    """vae_total_correlation on numpy f32 inputs: (tc f64 device scalar, g [B, 2L] f32 device tensor or None)."""
    from torch_vae_amd import _lib
    B, L = mu.shape
    mg, lg, eg = gpu(mu, lv, eps)
    tc = torch.full((), float("nan"), device="cuda", dtype=torch.float64)
    gm = torch.full((B, L), float("nan"), device="cuda") if grad else None
    gl = torch.full((B, L), float("nan"), device="cuda") if grad else None
    _lib.check(_lib.lib().vae_total_correlation(mg.data_ptr(), lg.data_ptr(), eg.data_ptr(), B, L, tc.data_ptr(), _lib.ptr(gm), _lib.ptr(gl),
                                               torch.cuda.current_stream().cuda_stream), "vae_total_correlation")
    torch.cuda.synchronize()
    return tc, (torch.cat([gm, gl], dim=1) if grad else None)


# ---- 1. kernel level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,L", KERNEL_SHAPES)
def test_kernels_against_torch_autograd(regime, B, L):
    mu, lv, eps, ref = kernel_case(regime, B, L)
    assert_gate_not_vacuous(regime, B, L)            # on the yardstick alone
    tc, g = run_kernels(mu, lv, eps)
    tc_only, _ = run_kernels(mu, lv, eps, grad=False)
    got, g = tc.item(), g.cpu().numpy().astype(np.float64)
    err_v, gate_v = abs(got - ref["tc"]), VALUE_ABS + VALUE_REL * abs(ref["tc"])
    err_g = float(np.linalg.norm(g - ref["g"]))
    gate_g = GRAD_REL * float(np.linalg.norm(ref["g"])) + GRAD_FLOOR * (ref["nj"] + ref["nd"])
    print(f"{regime} B{B} L{L}: TC {got:.9g} ref {ref['tc']:.9g} err/gate {err_v / gate_v:.3g}; gradient err/gate {err_g / gate_g:.3g} "
          f"(ref norm {np.linalg.norm(ref['g']):.3g})")
    assert np.isfinite(got) and np.all(np.isfinite(g))
    assert err_v <= gate_v, (err_v, gate_v)
    assert err_g <= gate_g, (err_g, gate_g)
    assert tc_only.item() == got                     # the value does not depend on whether the gradient was asked for


@pytest.mark.parametrize("B,L", [(257, 16), (2, 4096), (256, 128)])
def test_kernels_repeat_bit_for_bit(B, L):
    mu, lv, eps, _ = kernel_case("mixed", B, L)
    a, b = run_kernels(mu, lv, eps), run_kernels(mu, lv, eps)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 2. step level, f32 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_case(H, L, B, gen, tcw):
    """Parameters, inputs and the yardstick step of one shape / tc_weight (computed once, shared, never written to)."""
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    return p, x, eps, cpu_tc_step(p, x, eps, BETA, tcw)


def tc_model(H, L, gen, dtype, p, tcw, kld_weight=BETA):
    m = make_model(H, L, gen, dtype, p, kld_weight=kld_weight)
    m.tc_weight = tcw
    return m


def assert_step_matches(m, out3, xhat, want, tag=""):
    torch.cuda.synchronize()
    print(tag, "out3", out3.tolist(), "want", want["out3"])
    np.testing.assert_allclose(out3.tolist(), want["out3"], rtol=1e-4)
    gap = rel_l2(xhat.cpu().numpy(), want["xhat"])
    assert gap < 1e-4, gap
    got = flat_grad_dict(m)
    bad = {n: rel_l2(got[n], want["grads"][n].reshape(-1)) for n in got if n not in PRE_BN_BIAS}
    print(tag, "worst gradient", max(bad, key=bad.get), max(bad.values()))
    assert max(bad.values()) < GRAD_TOL_F32, {n: v for n, v in bad.items() if v >= GRAD_TOL_F32}


def dbg(m, which, n):
    from torch_vae_amd import _lib
    t = torch.empty(n, device="cuda")
    _lib.check(_lib.lib().vae_debug_tensor(m._ctx.handle, which, t.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "dbg")
    return t


@pytest.mark.parametrize("tcw", TC_WEIGHTS)
@pytest.mark.parametrize("H,L,B,gen", SHAPES)
def test_f32_fused_step_against_torch_autograd(H, L, B, gen, tcw):
    p, x, eps, want = step_case(H, L, B, gen, tcw)
    m = tc_model(H, L, gen, "f32", p, tcw)
    out3, xhat = m.fused_forward_backward(*gpu(x, eps))
    assert_step_matches(m, out3, xhat, want, f"tc_weight {tcw} {H}x{H} L{L} B{B}")
    tc = m.total_correlation()
    assert tc.dtype == torch.float64 and tc.dim() == 0
    print("TC", tc.item(), "want", want["tc"])
    # (as kl_per_dim in tests/test_kl_control_gpu.py: the value is a function of the f32 encoder's mu / log_var, whose relative
    #  error the project bounds by 1e-4 on the ELBO scalars; the relative part leaves room for that)
    assert abs(tc.item() - want["tc"]) <= 1e-4 + 1e-3 * abs(want["tc"])


@pytest.mark.parametrize("tcw", TC_WEIGHTS)
def test_f32_autograd_path_and_recorded_objective(tcw):
    """forward -> loss -> backward through autograd; the objective is the one the forward recorded: switching it off on the model
    before loss() / backward changes neither."""
    H, L, B, gen = SMALL
    p, x, eps, want = step_case(H, L, B, gen, tcw)
    m = tc_model(H, L, gen, "f32", p, tcw)
    xg, eg = gpu(x, eps)
    m.set_next_eps(eg)
    out = m.forward(xg)
    m.tc_weight = None
    lo = m.loss(out)
    lo["loss"].backward()
    out3 = torch.stack([lo["loss"].detach(), lo["reconstruction_loss"], lo["kld_loss"]])
    assert_step_matches(m, out3, out["output"].detach(), want, f"autograd tc_weight {tcw}")


@pytest.mark.parametrize("tcw", TC_WEIGHTS)
@pytest.mark.parametrize("clip", [None, 0.05])
def test_f32_one_call_step_with_and_without_clipping(tcw, clip):
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen = SMALL
    p, x, eps, want = step_case(H, L, B, gen, tcw)
    m = tc_model(H, L, gen, "f32", p, tcw)
    opt = FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0, max_grad_norm=clip)
    out3, xhat = m.fused_train_step(opt, *gpu(x), eps=gpu(eps)[0])
    assert_step_matches(m, out3.clone(), xhat.clone(), want, f"one call clip={clip} tc_weight {tcw}")   # (the buffer keeps the unclipped gradient)


def test_f32_split_backward_is_the_whole_backward():
    """vae_backward_part 1 + 2 (the data-parallel callers' form) against part 0: the same bits."""
    H, L, B, gen = SMALL
    p, x, eps, want = step_case(H, L, B, gen, 4.0)
    xg, eg = gpu(x, eps)
    m = tc_model(H, L, gen, "f32", p, 4.0)
    out3, xhat = m.fused_forward_backward(xg, eg)
    whole = (out3.clone(), xhat.clone(), m.flat_grads().clone())
    out3, xhat = m.fused_forward_backward(xg, eg, on_decoder_grads=lambda: None)
    assert_step_matches(m, out3, xhat, want, "split backward")
    assert torch.equal(out3, whole[0]) and torch.equal(xhat, whole[1]) and torch.equal(m.flat_grads(), whole[2])


def test_f32_exchanges_single_rank_rccl():
    """The one-call step with the in-line (1) and the bucketed (2) gradient exchange on a one-rank RCCL communicator (the only size
    one GPU allows): the bits of the step without an exchange (0).  (A replica's TC is over its own batch; with one rank that is
    the batch.)"""
    import os
    import torch.distributed as dist
    from torch_vae_amd.optim import FusedAdamW
    from torch_vae_amd.train import enable_library_allreduce, fused_step
    H, L, B, gen = SMALL
    p, x, eps, want = step_case(H, L, B, gen, 4.0)
    xg, eg = gpu(x, eps)

    def fresh():
        m = tc_model(H, L, gen, "f32", p, 4.0)
        return m, FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
    m0, opt0 = fresh()
    out3, xhat = m0.fused_train_step(opt0, xg, eps=eg, exchange=0)
    assert_step_matches(m0, out3.clone(), xhat.clone(), want, "exchange 0")
    base = (out3.clone(), xhat.clone(), m0.flat_grads().clone(), m0.flat_parameters().clone())
    env = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY", "GPU_MAX_HW_QUEUES")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29592", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) >= 8:
        os.environ["GPU_MAX_HW_QUEUES"] = "6"    # (train.fused_step refuses the bucketed exchange with eight queues)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for overlap in (False, True):
            m, opt = fresh()
            assert enable_library_allreduce(m)
            out3, xhat = fused_step(m, opt, xg, eps=eg, overlap=overlap)
            torch.cuda.synchronize()
            assert m.library_comm_world() == 1
            got = (out3, xhat, m.flat_grads(), m.flat_parameters())
            assert all(torch.equal(a, b) for a, b in zip(got, base)), f"exchange {2 if overlap else 1}"
    finally:
        dist.destroy_process_group()
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_readback_after_a_plain_forward_and_against_latent_statistics():
    """total_correlation() of a plain forward on the same inputs (computed on demand) is the TC step's value bit for bit, after
    encode() too; both agree with latent_statistics(mu, lv, eps=eps[None]).tc, each estimator within its own 1e-4.  It is refused
    after decode()."""
    from torch_vae_amd.evaluation import latent_statistics
    H, L, B, gen = SMALL
    p, x, eps, want = step_case(H, L, B, gen, 4.0)
    xg, eg = gpu(x, eps)
    m = tc_model(H, L, gen, "f32", p, 4.0)
    m.fused_forward_backward(xg, eg)
    tc = m.total_correlation()
    g_step = dbg(m, 20, B * 2 * L)
    m0 = make_model(H, L, gen, "f32", p, kld_weight=BETA)
    m0.set_next_eps(eg)
    with torch.no_grad():
        out = m0.forward(xg)
    assert torch.equal(out["encoded"]["mu"], m._last["mu"]) and torch.equal(out["encoded"]["log_var"], m._last["lv"])
    kl_d = m0.kl_per_dim()                               # (the other on-demand reduction keeps working beside it)
    tc0 = m0.total_correlation()
    assert torch.equal(tc0, tc) and torch.equal(m0.total_correlation(), tc)
    assert torch.equal(dbg(m0, 20, B * 2 * L), g_step)
    assert torch.equal(m0.kl_per_dim(), kl_d) and torch.equal(kl_d, m.kl_per_dim())
    stats = latent_statistics(out["encoded"]["mu"], out["encoded"]["log_var"], eps=eg[None])
    ref = float(stats["tc"])
    assert abs(tc.item() - ref) <= 2e-4 + 1e-5 * abs(ref), (tc.item(), ref)
    kernel_tc, _ = run_kernels(out["encoded"]["mu"].cpu().numpy(), out["encoded"]["log_var"].cpu().numpy(), eps)
    assert torch.equal(kernel_tc, tc)                    # the context-free entry point runs the same kernels
    m0.eval()
    with torch.no_grad():
        m0.decode(torch.zeros(2, L, device="cuda"))
    with pytest.raises(RuntimeError):
        m0.total_correlation()


def test_f32_train_one_epoch_with_tc_weight_against_cpu_loop():
    """4 steps of train_one_epoch (one library call per step) with config.kl_tc_weight against the same loop on torch CPU f64
    autograd (the gates of the free-bits epoch test of tests/test_kl_control_gpu.py)."""
    from argparse import Namespace
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    H, L, B, steps, total, tcw = 32, 16, 8, 4, 10, 4.0
    p = vo.init_params(L, H, 61, False)
    batches = [synth_inputs(B, H, L, 70 + s) for s in range(steps)]
    cpu = TcCpuStep(p, batch=B, total_steps=total, kld_weight=BETA, dtype=torch.float64)
    want = [cpu.step(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(e.astype(np.float64)), BETA, tcw) for x, e in batches]
    model = make_model(H, L, False, "f32", p, kld_weight=BETA)
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                    epochs=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0,
                    kl_tc_weight=tcw)
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
    res, total_step, _ = train_one_epoch(cfg, model, opt, sched, model.loss, loader, device="cuda", epoch=1, total_step=0)
    assert total_step == steps and len(got) == steps and model.tc_weight == tcw
    print("train_one_epoch got", got, "want", want)
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-4)
    np.testing.assert_allclose(res["loss"], np.mean([w[0] for w in want]), rtol=2e-4)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_launch_sequence(dtype):
    """With the option off no launch is labelled tc_*; with it on, the sequence without the tc_* and kl_shape labels is the off one."""
    from torch_vae_amd import _lib
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen = 64, 16, 5, True
    p = perturbed_params(L, H, 51, gen)
    xg, eg = gpu(*synth_inputs(B, H, L, 52))
    m = make_model(H, L, gen, dtype, p, kld_weight=BETA)
    opt = FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
    step = lambda: m.fused_train_step(opt, xg, eps=eg)   # noqa: E731
    step()
    lib = _lib.lib()
    ws = lib.vae_workspace_bytes(m._ctx.handle)
    off = profile_sequence(m, step)
    assert not [n for n in off if n.startswith("tc_") or "kl_shape" in n]
    m.tc_weight = 4.0
    on = profile_sequence(m, step)
    extra = [n for n in on if n.startswith("tc_") or "kl_shape" in n]
    assert [n.split(" ")[0] for n in extra] == ["kl_shape", "tc_prep", "tc_pair", "tc_row", "tc_query", "tc_comp", "tc_final"], extra
    assert [n for n in on if not (n.startswith("tc_") or "kl_shape" in n)] == off
    assert lib.vae_workspace_bytes(m._ctx.handle) >= ws + 4 * B * B       # the work space is counted
    m.tc_weight = None
    assert profile_sequence(m, step) == off


# ---- 3. 16-bit storage: the latent gradient on the GPU's own mu / log_var ---------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("tcw", TC_WEIGHTS)
@pytest.mark.parametrize("H,L,B", [(64, 16, 5), (64, 128, 6)])
def test_16bit_latent_gradient_on_its_own_inputs(dtype, H, L, B, tcw):
    """A TC step and a plain step on the same inputs: the difference of their latent gradients ([B, 2L] dmu | dlv, debug tensor 18)
    must be kld_weight (tc_weight - 1) gs [g_mu | g_log_var] of TC, the yardstick evaluated on the GPU's own mu / log_var and the
    given eps; gs is the f16 gradient scale.  Gate: 5e-4 ||want|| (the layer-local gate of tests/test_kl_control_gpu.py, which
    leaves room for the decoder-side part of the two runs cancelling only to within the BatchNorm statistics' f64 atomics) plus the
    f32 floor of the kernels' gradient, scaled like the term."""
    gen = True
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    xg, eg = gpu(x, eps)
    m0 = make_model(H, L, gen, dtype, p, kld_weight=BETA)
    m0.fused_forward_backward(xg, eps=eg)
    d0 = dbg(m0, 18, B * 2 * L).cpu().numpy().astype(np.float64).reshape(B, 2 * L)
    m1 = tc_model(H, L, gen, dtype, p, tcw)
    out3, _ = m1.fused_forward_backward(xg, eps=eg)
    d1 = dbg(m1, 18, B * 2 * L).cpu().numpy().astype(np.float64).reshape(B, 2 * L)
    torch.cuda.synchronize()
    assert torch.equal(m1._last["mu"], m0._last["mu"]) and torch.equal(m1._last["lv"], m0._last["lv"])
    ref = tc_autograd(m0._last["mu"].cpu().numpy(), m0._last["lv"].cpu().numpy(), eps)
    gs = vo.f16_grad_scale(B, H) if dtype == "f16" else 1.0
    k = BETA * (tcw - 1.0) * gs
    want = k * ref["g"]
    err = float(np.linalg.norm((d1 - d0) - want))
    gate = 5e-4 * float(np.linalg.norm(want)) + 1e-5 * abs(k) * (ref["nj"] + ref["nd"])
    print(dtype, H, L, B, tcw, "latent gradient difference err/gate", err / gate, "largest |dlat|", np.abs(d1).max())
    assert err <= gate, (err, gate)
    assert np.all(np.isfinite(d1)) and bool(torch.isfinite(m1.flat_grads()).all())
    assert abs(m1.total_correlation().item() - ref["tc"]) <= 1e-4 + 1e-5 * abs(ref["tc"])
    kl = -out3[2].item()
    np.testing.assert_allclose((out3[0].item() - out3[1].item()) / BETA, kl + (tcw - 1.0) * ref["tc"], rtol=1e-4, atol=1e-4)
