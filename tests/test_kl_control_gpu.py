"""KL control on the GPU: free bits and the KL capacity target (VanillaVAE(kl_free_bits=..., kl_capacity=...),
vae_set_kl_objective, vae_elbo_generic_kl, vae_kl_per_dim) on every step path, and train_one_epoch's KLSchedule.

The yardstick is torch f64 autograd on the CPU of recon + beta * clamp(kl_d, min=lambda).sum() resp. recon + beta * |KL - C|
over oracle.torch_cpu_step.TorchCpuStep.forward (tests/test_kl_control_host.py: cpu_kl_step).  lambda always comes from the data
by the fixed rule there (choose_lambda), which also asserts that dimensions fall on both sides of it with a relative margin of at
least 1e-2; C is 0.5 / 1.5 times the yardstick's KL, so both signs run.  Tolerances are the project's existing ones for the same
comparisons (tests/test_recon_loss_gpu.py, tests/test_parity_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.test_kl_control_host import (KlCpuStep, check_lambda, choose_lambda, cpu_kl_step, kl_terms, shaped_term, synth_inputs)
from tests.util import PRE_BN_BIAS, flat_grad_dict, make_model, perturbed_params, profile_sequence, rel_l2

pytestmark = pytest.mark.gpu
GRAD_TOL_F32 = 5e-3          # tests/test_parity_gpu.py GRAD_TOL["f32"] (LeakyReLU kink ties)
LAYER_TOL = 5e-4             # the layer-local gate of tests/test_parity_gpu.py
BETA = 2.0                   # a wrong factor cannot hide behind a weight of 1

SHAPES = [(32, 16, 32, False), (64, 16, 5, True), (128, 16, 3, True), (64, 128, 6, True), (32, 10, 8, False)]
OBJECTIVES = [("free_bits", None), ("capacity", "lo"), ("capacity", "hi")]


def set_objective(m, objective, param):
    m.kl_free_bits, m.kl_capacity = (param, None) if objective == "free_bits" else (0.0, param if objective == "capacity" else None)


def kl_model(H, L, gen, dtype, p, objective, param, kld_weight=BETA):
    m = make_model(H, L, gen, dtype, p, kld_weight=kld_weight)
    set_objective(m, objective, param)
    return m


def gpu(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


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


# ---- 5. f32, one fused step against the yardstick ------------------------------------------------------------------------
@pytest.mark.parametrize("objective,rule", OBJECTIVES)
@pytest.mark.parametrize("H,L,B,gen", SHAPES)
def test_f32_fused_step_against_torch_autograd(H, L, B, gen, objective, rule):
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    want = cpu_kl_step(p, x, eps, BETA, objective, rule)
    m = kl_model(H, L, gen, "f32", p, objective, want["param"])
    out3, xhat = m.fused_forward_backward(*gpu(x, eps))
    assert_step_matches(m, out3, xhat, want, f"{objective}/{rule} {H}x{H} L{L} B{B}")
    # (kl_d is quadratic in mu / log_var around 0: it carries about twice the relative error of the f32 encoder, which the
    #  project bounds by 1e-4 on the ELBO scalars; 1e-3 leaves room for dimensions whose mu is small against its absolute error)
    np.testing.assert_allclose(m.kl_per_dim().cpu().numpy(), want["kl_d"], rtol=1e-3)
    if objective == "free_bits":       # the mask itself
        np.testing.assert_array_equal(dbg(m, 19, L).cpu().numpy(), (want["kl_d"] > want["param"]).astype(np.float32))
    else:
        np.testing.assert_array_equal(dbg(m, 19, L).cpu().numpy(), np.full(L, 1.0 if rule == "lo" else -1.0, np.float32))


# ---- 6. the other paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective,rule", OBJECTIVES)
def test_f32_autograd_path_and_recorded_objective(objective, rule):
    """forward -> loss -> backward through autograd; the objective is the one the forward recorded (9e): switching it off on the
    model before loss() / backward changes neither."""
    H, L, B, gen = 32, 16, 32, False
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    want = cpu_kl_step(p, x, eps, BETA, objective, rule)
    m = kl_model(H, L, gen, "f32", p, objective, want["param"])
    xg, eg = gpu(x, eps)
    m.set_next_eps(eg)
    out = m.forward(xg)
    set_objective(m, "plain", None)
    lo = m.loss(out)
    lo["loss"].backward()
    out3 = torch.stack([lo["loss"].detach(), lo["reconstruction_loss"], lo["kld_loss"]])
    assert_step_matches(m, out3, out["output"].detach(), want, f"autograd {objective}/{rule}")


@pytest.mark.parametrize("objective,rule", OBJECTIVES)
@pytest.mark.parametrize("clip", [None, 0.05])
def test_f32_one_call_step_with_and_without_clipping(objective, rule, clip):
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen = 64, 16, 5, True
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    want = cpu_kl_step(p, x, eps, BETA, objective, rule)
    m = kl_model(H, L, gen, "f32", p, objective, want["param"])
    opt = FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0, max_grad_norm=clip)
    out3, xhat = m.fused_train_step(opt, *gpu(x), eps=gpu(eps)[0])
    assert_step_matches(m, out3.clone(), xhat.clone(), want, f"one call clip={clip} {objective}/{rule}")   # (the gradient buffer keeps the unclipped gradient)


def test_f32_split_backward_matches_whole():
    """vae_backward_part 1 + 2 (the data-parallel callers' form) takes the same factors as part 0."""
    H, L, B, gen = 32, 16, 32, False
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    want = cpu_kl_step(p, x, eps, BETA, "free_bits")
    m = kl_model(H, L, gen, "f32", p, "free_bits", want["param"])
    out3, xhat = m.fused_forward_backward(*gpu(x, eps), on_decoder_grads=lambda: None)
    assert_step_matches(m, out3, xhat, want, "split backward")


def test_f32_exchanges_single_rank_rccl():
    """The one-call step with the in-line (1) and the bucketed (2) gradient exchange on a one-rank RCCL communicator (the only
    size one GPU allows), free bits and the capacity target on: the yardstick's scalars and gradients, as without an exchange.
    (A replica decides on its own batch means; with one rank those are the batch's.)"""
    import os
    import torch.distributed as dist
    from torch_vae_amd.optim import FusedAdamW
    from torch_vae_amd.train import enable_library_allreduce, fused_step
    H, L, B, gen = 64, 16, 5, True
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    xg, eg = gpu(x, eps)
    wants = {(o, r): cpu_kl_step(p, x, eps, BETA, o, r) for o, r in (("free_bits", None), ("capacity", "hi"))}
    env = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY", "GPU_MAX_HW_QUEUES")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29591", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) >= 8:
        os.environ["GPU_MAX_HW_QUEUES"] = "6"    # (train.fused_step refuses the bucketed exchange with eight queues)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for (objective, rule), want in wants.items():
            for overlap in (False, True):
                m = kl_model(H, L, gen, "f32", p, objective, want["param"])
                assert enable_library_allreduce(m)
                opt = FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
                out3, xhat = fused_step(m, opt, xg, eps=eg, overlap=overlap)
                assert m.library_comm_world() == 1
                assert_step_matches(m, out3.clone(), xhat.clone(), want, f"exchange {2 if overlap else 1} {objective}/{rule}")
    finally:
        dist.destroy_process_group()
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def generic_inputs(seed=3, B=7, L=16, n=7000):
    rng = np.random.default_rng(seed)
    xh = rng.uniform(0.0, 1.0, n).astype(np.float32)
    tg = (rng.uniform(size=n) < 0.3).astype(np.float32)
    mu = (rng.normal(size=(B, L)) * rng.uniform(0.05, 1.0, L)).astype(np.float32)
    lv = (0.5 * rng.normal(size=(B, L)) * rng.uniform(0.05, 1.0, L)).astype(np.float32)
    return xh, tg, mu, lv


@pytest.mark.parametrize("objective,rule", OBJECTIVES)
def test_generic_entry_against_torch(objective, rule):
    """vae_elbo_generic_kl on caller tensors: f32 element-wise arithmetic on given inputs, so g_mu / g_log_var are compared element
    for element (rtol 1e-6, as tests/test_recon_loss_gpu.py::test_generic_mse_elbo_against_torch)."""
    import torch.nn.functional as F
    from torch_vae_amd import _lib
    xh, tg, mu, lv = generic_inputs()
    B, L, n = mu.shape[0], mu.shape[1], xh.size
    x64, m64, l64 = (torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (xh, mu, lv))
    kl_d, kl = kl_terms(m64.detach(), l64.detach())
    param = choose_lambda(kl_d.numpy()) if objective == "free_bits" else {"lo": 0.5, "hi": 1.5}[rule] * float(kl)
    recon = F.binary_cross_entropy(x64, torch.from_numpy(tg.astype(np.float64)))
    T, _ = shaped_term(m64, l64, objective, param)
    loss = recon + BETA * T
    loss.backward()
    kind = _lib.KL_FREE_BITS if objective == "free_bits" else _lib.KL_CAPACITY
    xg, tgg, mg, lg = gpu(xh, tg, mu, lv)
    out3 = torch.empty(3, device="cuda")
    gx, gm, gl = torch.empty_like(xg), torch.empty_like(mg), torch.empty_like(lg)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().vae_elbo_generic_kl(xg.data_ptr(), tgg.data_ptr(), mg.data_ptr(), lg.data_ptr(), n, B, L, BETA, _lib.RECON_BCE, kind,
                                             param, out3.data_ptr(), gx.data_ptr(), gm.data_ptr(), gl.data_ptr(), st), "vae_elbo_generic_kl")
    torch.cuda.synchronize()
    np.testing.assert_allclose(out3.tolist(), [loss.item(), recon.item(), -float(kl)], rtol=1e-6)
    for got, want in ((gx, x64.grad), (gm, m64.grad), (gl, l64.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    if objective == "free_bits":
        below = kl_d.numpy() < param
        assert np.all(gm.cpu().numpy()[:, below] == 0) and np.all(gm.cpu().numpy()[:, ~below] != 0)


def test_loss_on_foreign_tensors_and_eval_forward():
    """model.loss() on tensors that are not the model's own forward goes through the generic entry with the model's objective and
    differentiates to the fused step's gradients; loss() of an eval-mode no_grad forward reports recon + beta T of its own mu / log_var."""
    H, L, B, gen = 32, 16, 32, False
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    want = cpu_kl_step(p, x, eps, BETA, "free_bits")
    xg, eg = gpu(x, eps)
    m = kl_model(H, L, gen, "f32", p, "free_bits", want["param"])
    m.set_next_eps(eg)
    out = m.forward(xg)
    foreign = {"output": out["output"] * 1.0, "input": xg, "encoded": {"mu": out["encoded"]["mu"] * 1.0, "log_var": out["encoded"]["log_var"] * 1.0}}
    lg = m.loss(foreign)
    lg["loss"].backward()
    out3 = torch.stack([lg["loss"].detach(), lg["reconstruction_loss"], lg["kld_loss"]])
    assert_step_matches(m, out3, out["output"].detach(), want, "foreign tensors")
    m.eval()                      # (running statistics: nothing is written, so a second eval forward repeats the first)
    with torch.no_grad():
        ev = m.forward(xg)
        lam = choose_lambda(m.kl_per_dim().cpu().numpy())          # the rule on the eval posterior itself
        m.kl_free_bits = lam
        ev = m.forward(xg)
        le = m.loss(ev)
    mu, lv = ev["encoded"]["mu"].double().cpu(), ev["encoded"]["log_var"].double().cpu()
    check_lambda(kl_terms(mu, lv)[0].numpy(), lam)
    T, kl = shaped_term(mu, lv, "free_bits", lam)
    assert float(T) > float(kl)
    np.testing.assert_allclose(le["loss"].item(), le["reconstruction_loss"].item() + BETA * float(T), rtol=1e-5)
    np.testing.assert_allclose(le["kld_loss"].item(), -float(kl), rtol=1e-5)


# ---- 7. train_one_epoch with a schedule ---------------------------------------------------------------------------------------
def test_f32_train_one_epoch_linear_warmup_and_free_bits_against_cpu_loop():
    """3 steps of train_one_epoch (one library call per step), linear KL warm-up towards beta = 2 over 4 steps, entered at
    total_step = 1 as a resumed run would, with free bits, against the same loop on torch CPU f64 autograd; the weight a step sees
    is KLSchedule.value(total_step before the step)."""
    from argparse import Namespace
    from torch_vae_amd.train import KLSchedule, build_optimizer, train_one_epoch
    H, L, B, steps, total, t0 = 32, 16, 4, 3, 10, 1
    p = vo.init_params(L, H, 61, False)
    batches = [synth_inputs(B, H, L, 70 + s) for s in range(steps)]
    sched_ref = KLSchedule("linear", beta=BETA, warmup_steps=4)
    betas = [sched_ref.value(t0 + s) for s in range(steps)]
    assert betas == [0.5, 1.0, 1.5]
    first = cpu_kl_step(p, *batches[0], betas[0], "free_bits")
    lam = first["param"]
    cpu = KlCpuStep(p, batch=B, total_steps=total, dtype=torch.float64)
    want = []
    for (x, e), b in zip(batches, betas):
        w, kl_d = cpu.step(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(e.astype(np.float64)), b, lam)
        check_lambda(kl_d, lam)                      # every step of the yardstick keeps clear of a tie
        want.append(w)
    model = make_model(H, L, False, "f32", p, kld_weight=BETA)
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                    epochs=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0,
                    kl_schedule="linear", kl_warmup_steps=4, kl_free_bits=lam)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=total)
    it = iter([torch.from_numpy(e).cuda() for _, e in batches])
    got, seen = [], []
    orig = model.fused_train_step

    def step(o, x, **k):
        seen.append(model.kld_weight)
        out3, xhat = orig(o, x, **{**k, "eps": next(it)})
        got.append(out3.tolist())
        return out3, xhat
    model.fused_train_step = step
    loader = [(torch.from_numpy(x), torch.zeros(B, dtype=torch.long)) for x, _ in batches]
    res, total_step, _ = train_one_epoch(cfg, model, opt, sched, model.loss, loader, device="cuda", epoch=1, total_step=t0)
    assert total_step == t0 + steps and len(got) == steps
    assert seen == betas and cfg.kl_beta == BETA and model.kl_free_bits == lam
    print("train_one_epoch got", got, "want", want)
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-4)
    np.testing.assert_allclose(res["loss"], np.mean([w[0] for w in want]), rtol=2e-4)


# ---- 8. 16-bit storage: the latent gradient on the GPU's own mu / log_var ------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("H,L,B", [(64, 16, 5), (64, 128, 6)])
def test_16bit_latent_gradient_on_its_own_inputs(dtype, H, L, B):
    """A free-bits step and a plain step on the same inputs: the difference of their latent gradients ([B, 2L] dmu | dlv, debug
    tensor 18) must be (factor_d - 1) * beta/B * (mu, 0.5 (e^lv - 1)) times the f16 gradient scale, from the GPU's own mu / log_var,
    with lambda chosen by the rule on those.  The factor is 0 / 1, so the power-of-two gradient scale of f16 storage is untouched.
    The decoder-side part of the two runs cancels to within the f64 atomics of the BatchNorm statistics (order-dependent in the
    last bits of a double, almost never visible after the rounding to f32); LAYER_TOL leaves room for that."""
    gen = True
    p = perturbed_params(L, H, 51, gen)
    xg, eg = gpu(*synth_inputs(B, H, L, 52))
    m0 = make_model(H, L, gen, dtype, p, kld_weight=BETA)
    m0.fused_forward_backward(xg, eps=eg)
    d0 = dbg(m0, 18, B * 2 * L).cpu().numpy().astype(np.float64).reshape(B, 2 * L)
    mu, lv = m0._last["mu"].double().cpu(), m0._last["lv"].double().cpu()
    kl_d, kl = kl_terms(mu, lv)
    lam = choose_lambda(kl_d.numpy())
    m1 = kl_model(H, L, gen, dtype, p, "free_bits", lam)
    out3, _ = m1.fused_forward_backward(xg, eps=eg)
    d1 = dbg(m1, 18, B * 2 * L).cpu().numpy().astype(np.float64).reshape(B, 2 * L)
    torch.cuda.synchronize()
    assert torch.equal(m1._last["mu"], m0._last["mu"]) and torch.equal(m1._last["lv"], m0._last["lv"])
    gs = vo.f16_grad_scale(B, H) if dtype == "f16" else 1.0
    fac = (kl_d.numpy() > lam).astype(np.float64)
    np.testing.assert_array_equal(dbg(m1, 19, L).cpu().numpy(), fac.astype(np.float32))
    k = BETA / B
    want = np.concatenate([(fac - 1.0) * k * mu.numpy(), (fac - 1.0) * k * 0.5 * (np.exp(lv.numpy()) - 1.0)], axis=1) * gs
    gap = rel_l2(d1 - d0, want)
    print(dtype, H, L, B, "latent gradient difference gap", gap, "below", int((fac == 0).sum()))
    assert gap < LAYER_TOL, gap
    assert np.all(np.isfinite(d1)) and bool(torch.isfinite(m1.flat_grads()).all())
    np.testing.assert_allclose(m1.kl_per_dim().cpu().numpy(), kl_d.numpy(), rtol=1e-12)
    T = float(torch.clamp(kl_d, min=lam).sum())
    np.testing.assert_allclose((out3[0].item() - out3[1].item()) / BETA, T, rtol=1e-4)
    np.testing.assert_allclose(out3[2].item(), -float(kl), rtol=1e-5)


# ---- 9. properties that need no yardstick -----------------------------------------------------------------------------------
def _run(H, L, B, gen, dtype, p, xg, eg, objective, param, beta=BETA):
    m = kl_model(H, L, gen, dtype, p, objective, param, kld_weight=beta)
    out3, xhat = m.fused_forward_backward(xg, eps=eg)
    torch.cuda.synchronize()
    return m, out3.clone(), xhat.clone(), m.flat_grads().clone()


def _run_to_run(runs):
    """Largest relative L2 distance between the gradients (and xhat) of runs that should agree: 0 when they are bit-identical."""
    worst = 0.0
    for i in range(len(runs)):
        for j in range(i + 1, len(runs)):
            for a, b in ((runs[i][2], runs[j][2]), (runs[i][3], runs[j][3])):
                if not torch.equal(a, b):
                    worst = max(worst, rel_l2(a.cpu().numpy(), b.cpu().numpy()))
    return worst


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_floor_below_and_above_every_dimension(dtype):
    """(a) a floor under every kl_d masks nothing: xhat and gradients as the plain run's, bit for bit where plain runs repeat bit
    for bit (else within what three plain runs show among themselves), out3 to rtol 1e-6 (T comes from the f64 reduction, the plain
    KL from the f32 terms of the latent kernel).  (b) a floor above every kl_d: the gradients of a plain run with kld_weight = 0,
    and loss = recon + beta * L * lambda."""
    H, L, B, gen = 64, 16, 5, True
    p = perturbed_params(L, H, 51, gen)
    xg, eg = gpu(*synth_inputs(B, H, L, 52))
    plain = [_run(H, L, B, gen, dtype, p, xg, eg, "plain", None) for _ in range(3)]
    tol = _run_to_run(plain)
    print(dtype, "run-to-run distance of three plain runs", tol)
    kl_d = plain[0][0].kl_per_dim().cpu().numpy()
    low = _run(H, L, B, gen, dtype, p, xg, eg, "free_bits", 1e-30)
    assert kl_d.min() > 1e-30
    assert _run_to_run([plain[0], low]) <= tol
    np.testing.assert_allclose(low[1].cpu().numpy(), plain[0][1].cpu().numpy(), rtol=1e-6)
    lam = 2.0 * float(kl_d.max())
    high = _run(H, L, B, gen, dtype, p, xg, eg, "free_bits", lam)
    zero = [_run(H, L, B, gen, dtype, p, xg, eg, "plain", None, beta=0.0) for _ in range(3)]
    tol0 = _run_to_run(zero)
    assert _run_to_run([zero[0], high]) <= max(tol, tol0)
    np.testing.assert_allclose(high[1][0].item(), high[1][1].item() + BETA * L * lam, rtol=1e-6)
    np.testing.assert_allclose(high[1][2].item(), plain[0][1][2].item(), rtol=1e-6)


@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 32, False), (32, 10, 8, False), (32, 1, 3, False), (32, 300, 7, False), (32, 4096, 2, False)])
def test_reduction_is_reproducible_and_matches_latent_statistics(H, L, B, gen):
    """(c) two free-bits runs on the same inputs give bit-identical kl_per_dim() and factors (no atomic accumulation: a fixed
    summation order, in both the 16-byte-load and the scalar form of the kernel); (d) kl_per_dim() equals
    latent_statistics(mu, log_var).kl_per_dim on the same tensors to 1e-12; every latent size takes the kernel."""
    from torch_vae_amd.evaluation import latent_statistics
    p = perturbed_params(L, H, 51, gen)
    xg, eg = gpu(*synth_inputs(B, H, L, 52))
    m = make_model(H, L, gen, "f32", p, kld_weight=BETA)
    m.fused_forward_backward(xg, eps=eg)
    lam = float(np.median(m.kl_per_dim().cpu().numpy())) if L > 1 else 1e-3
    res = []
    for _ in range(2):
        m = kl_model(H, L, gen, "f32", p, "free_bits", lam)
        m.fused_forward_backward(xg, eps=eg)
        res.append((m.kl_per_dim(), dbg(m, 19, L), m._last["mu"], m._last["lv"]))
    torch.cuda.synchronize()
    assert torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])      # the same inputs to the reduction
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][0].dtype == torch.float64 and tuple(res[0][0].shape) == (L,)
    stats = latent_statistics(res[0][2], res[0][3])
    np.testing.assert_allclose(res[0][0].cpu().numpy(), stats["kl_per_dim"].cpu().numpy(), rtol=1e-12)
    mu, lv = res[0][2].double().cpu(), res[0][3].double().cpu()
    np.testing.assert_allclose(res[0][0].cpu().numpy(), kl_terms(mu, lv)[0].numpy(), rtol=1e-12)
    np.testing.assert_array_equal(res[0][1].cpu().numpy(), (res[0][0].cpu().numpy() > lam).astype(np.float32))
    # the reduction on demand after a plain forward, and after encode()
    m0 = make_model(H, L, gen, "f32", p)
    m0.set_next_eps(eg)
    with torch.no_grad():
        out = m0.forward(xg)
    assert torch.equal(out["encoded"]["mu"], res[0][2])
    assert torch.equal(m0.kl_per_dim(), res[0][0])
    with torch.no_grad():
        m0.encode(xg)
    assert torch.equal(m0.kl_per_dim(), res[0][0])


# ---- 10. the default path launches what it did -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_default_step_launches_nothing_new(dtype):
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen = 64, 16, 5, True
    p = perturbed_params(L, H, 51, gen)
    xg, eg = gpu(*synth_inputs(B, H, L, 52))
    m = make_model(H, L, gen, dtype, p, kld_weight=BETA)
    opt = FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
    step = lambda: m.fused_train_step(opt, xg, eps=eg)   # noqa: E731
    step()
    off = profile_sequence(m, step)
    assert not [n for n in off if "kl_shape" in n]
    m.kl_free_bits = 0.05
    on = profile_sequence(m, step)
    assert [n for n in on if "kl_shape" not in n] == off and len(on) == len(off) + 1
    m.kl_free_bits = 0.0
    m.kl_capacity = 3.0
    cap = profile_sequence(m, step)
    assert cap == on
    m.kl_capacity = None
    assert profile_sequence(m, step) == off
