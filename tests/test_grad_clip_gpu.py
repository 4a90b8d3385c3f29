"""Gradient-norm clipping and non-finite step skipping on the GPU (FusedAdamW(max_grad_norm=..., skip_nonfinite=...),
include/vae_step.h: vae_grad_norm / vae_adamw_step_clipped / vae_train_step_fused_clipped): against an f64 recomputation and
against torch's own clip_grad_norm_ + AdamW, split path against one-call path, skip semantics, checkpoints, the data-parallel
exchanges and train_one_epoch.  Small model throughout (H=64, L=16, B=6)."""
import ctypes as C
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.util import make_model, perturbed_params, rel_l2

pytestmark = pytest.mark.gpu

H, L, B, GEN = 64, 16, 6, True


def _cfg(**kw):
    base = dict(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.01, optimizer="AdamW", scheduler="OneCycle",
                epochs=1, freeze_encoder=False, log_wandb=False, print_interval=1000, log_interval=1000, global_rank=0)
    return Namespace(**{**base, **kw})


def _setup(dtype="f32", seed=61, **opt):
    from torch_vae_amd.train import build_optimizer
    m = make_model(H, L, GEN, dtype, perturbed_params(L, H, seed, GEN))
    o, s = build_optimizer(_cfg(**opt), m, steps_per_epoch=10)
    o._bind()
    return m, o, s


def _batch(i):
    x = torch.from_numpy(vo.synth_pianoroll(B, H, 30 + i)).cuda()
    eps = torch.from_numpy(vo.counter_normal(B * L, 30 + i, 5).reshape(B, L)).float().cuda()
    return x, eps


def _norm64(model, opt):
    g = model.flat_grads().double().cpu().numpy()
    return math.sqrt(sum(float((g[o:o + n] ** 2).sum()) for o, n in opt._ranges))


def _probe_norm(dtype):
    """The gradient norm of the first step, to place max_grad_norm where the clip is active."""
    m, o, _ = _setup(dtype)
    x, eps = _batch(1)
    m.fused_forward_backward(x, eps=eps)
    return _norm64(m, o)


def _state(m, o):
    return [t.detach().clone() for t in (m.flat_parameters(), o._m, o._v)]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_clipped_update_against_f64_recomputation(dtype):
    """Three one-call steps under OneCycle with the clip active: parameters and moments recomputed in f64 from the GPU's own
    gradients with torch's clip formula; the reported norm is the f64 norm of the optimised gradient ranges."""
    from torch_vae_amd import _lib
    from torch_vae_amd.train import fused_step
    mx = 0.25 * _probe_norm(dtype)
    m, opt, sched = _setup(dtype, max_grad_norm=mx)
    worst = {}
    f = lambda v: float(np.float32(v))        # noqa: E731  (torch's scalars: a double expression rounded once)
    for step in range(1, 4):
        x, eps = _batch(step)
        p0, m0, v0 = [t.double().cpu().numpy() for t in _state(m, opt)]
        hyper = [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in opt.param_groups]
        fused_step(m, opt, x, eps=eps)
        torch.cuda.synchronize()
        g = m.flat_grads().double().cpu().numpy()
        p1, m1, v1 = m.flat_parameters().double().cpu().numpy(), opt._m.double().cpu().numpy(), opt._v.double().cpu().numpy()
        norm = math.sqrt(sum(float((g[o:o + n] ** 2).sum()) for o, n in opt._ranges))
        got_norm = float(opt.last_grad_norm)
        assert abs(got_norm - norm) <= 1e-12 * norm, (got_norm, norm)
        coef = min(1.0, mx / (norm + 1e-6))
        assert coef < 0.9, coef                                    # the clip is active
        touched = np.zeros(p0.size, dtype=bool)
        for (lr, b1, b2, e, wd), (o, n) in zip(hyper, opt._ranges):
            sl = slice(o, o + n)
            touched[sl] = True
            gc = g[sl] * f(coef)
            mm = m0[sl] * f(b1) + f(1 - b1) * gc
            vv = v0[sl] * f(b2) + f(1 - b2) * gc * gc
            denom = np.sqrt(vv) * f(1 / np.sqrt(1 - b2 ** step)) + f(e)
            want = p0[sl] * f(1 - lr * wd) - f(lr / (1 - b1 ** step)) * (mm / denom)
            for name, a, b in (("param", p1[sl], want), ("exp_avg", m1[sl], mm), ("exp_avg_sq", v1[sl], vv)):
                worst[name] = max(worst.get(name, 0.0), rel_l2(a, b))
            worst["update"] = max(worst.get("update", 0.0), rel_l2(p1[sl] - p0[sl], want - p0[sl]))
        assert np.array_equal(p1[~touched], p0[~touched])          # fc_mu, fc_var, decoder_input, final_layer never move
        assert np.array_equal(g, m.flat_grads().double().cpu().numpy())   # the gradient buffer keeps the unclipped gradient
        sched.step()
    assert worst["param"] < 1e-6 and worst["exp_avg"] < 1e-6 and worst["exp_avg_sq"] < 1e-6 and worst["update"] < 1e-4, worst
    # the norm alone (vae_grad_norm), with a gradient scale
    n = len(opt._ranges)
    offs = (C.c_int64 * n)(*[r[0] for r in opt._ranges]); sizes = (C.c_int64 * n)(*[r[1] for r in opt._ranges])
    out = torch.zeros((), dtype=torch.float64, device="cuda")
    scratch = torch.empty(_lib.GRAD_CLIP_SCRATCH_BYTES, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vae_grad_norm(m.flat_grads().data_ptr(), n, offs, sizes, 4.0, out.data_ptr(), scratch.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "vae_grad_norm")
    g = m.flat_grads().double().cpu().numpy()
    want = math.sqrt(sum(float(((4.0 * g[o:o + n]) ** 2).sum()) for o, n in opt._ranges))
    assert abs(float(out) - want) <= 1e-12 * want


def test_split_path_equals_one_call_path():
    """fused_forward_backward + FusedAdamW.step() (VAE_ONE_CALL_STEP=0) and the one-call step give the same bits with the clip active."""
    from torch_vae_amd.train import fused_step
    mx = 0.25 * _probe_norm("f32")
    res = []
    for one_call in ("1", "0"):
        m, opt, sched = _setup("f32", max_grad_norm=mx)
        norms = []
        os.environ["VAE_ONE_CALL_STEP"] = one_call
        try:
            for step in range(1, 4):
                x, eps = _batch(step)
                fused_step(m, opt, x, eps=eps)
                norms.append(opt.last_grad_norm.clone())
                sched.step()
        finally:
            del os.environ["VAE_ONE_CALL_STEP"]
        res.append(_state(m, opt) + norms + [opt.state_dict()["state"][0]["step"]])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][-1]) == 3


def test_against_torch_clip_grad_norm_and_adamw():
    """f32 copies of the optimised parameters, given the model's flat gradients at every step, go through
    torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW under the same OneCycle schedule."""
    from torch_vae_amd.train import fused_step
    mx = 0.25 * _probe_norm("f32")
    m, opt, sched = _setup("f32", max_grad_norm=mx)
    groups = [[torch.nn.Parameter(p.detach().clone()) for p in g["params"]] for g in opt.param_groups]
    max_lrs = [g["max_lr"] for g in opt.param_groups]
    topt = torch.optim.AdamW([{"params": gp, "lr": lr} for gp, lr in zip(groups, max_lrs)], lr=max_lrs[0], weight_decay=0.01)
    tsched = torch.optim.lr_scheduler.OneCycleLR(topt, max_lrs, epochs=1, steps_per_epoch=10)
    assert [g["lr"] for g in topt.param_groups] == [g["lr"] for g in opt.param_groups]
    for step in range(1, 4):
        x, eps = _batch(step)
        fused_step(m, opt, x, eps=eps)
        for gp, g in zip(groups, opt.param_groups):
            for tp, p in zip(gp, g["params"]):
                tp.grad = p.grad.detach().clone()
        tnorm = torch.nn.utils.clip_grad_norm_([tp for gp in groups for tp in gp], mx)
        assert float(tnorm) > mx
        assert abs(float(opt.last_grad_norm) - float(tnorm)) <= 1e-6 * float(tnorm)
        topt.step()
        sched.step(); tsched.step()
    got = torch.cat([p.detach().reshape(-1) for g in opt.param_groups for p in g["params"]]).cpu().numpy()
    want = torch.cat([tp.detach().reshape(-1) for gp in groups for tp in gp]).cpu().numpy()
    assert rel_l2(got, want) < 1e-6, rel_l2(got, want)


def test_inactive_clip_matches_unclipped_optimiser():
    """max_grad_norm=1e30 with skip_nonfinite: the update of an optimiser built with neither option (expected bit-identical; at
    most one float ulp per element is allowed, the bias corrections being formed by the device's pow)."""
    from torch_vae_amd.train import fused_step
    res = []
    for kw in ({}, {"max_grad_norm": 1e30, "skip_nonfinite": True}):
        m, opt, sched = _setup("bf16", **kw)
        assert opt._clip_on == bool(kw)
        for step in range(1, 4):
            x, eps = _batch(step)
            fused_step(m, opt, x, eps=eps)
            sched.step()
        res.append([t.cpu().numpy() for t in _state(m, opt)])
    for a, b in zip(*res):
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))
        assert np.all(np.abs(a.astype(np.float64) - b) <= ulp), int((a != b).sum())


def test_nonfinite_step_is_skipped():
    """A batch with one NaN cell through the one-call step, then FusedAdamW.step() with a foreign gradient holding an inf: nothing
    moves, the step count holds, skipped_steps counts; the next clean step equals a twin's that never saw the bad batches."""
    from torch_vae_amd.train import fused_step
    m, opt, _ = _setup("f32", max_grad_norm=1.0, skip_nonfinite=True)
    twin, topt, _ = _setup("f32", max_grad_norm=1.0, skip_nonfinite=True)
    x1, e1 = _batch(1)
    for mm, oo in ((m, opt), (twin, topt)):
        fused_step(mm, oo, x1, eps=e1)
    before = _state(m, opt)
    assert int(opt.skipped_steps) == 0 and opt.state_dict()["state"][0]["step"] == 1
    xb, eb = _batch(2)
    xb[1, 0, 5, 7] = float("nan")
    fused_step(m, opt, xb, eps=eb)
    assert not math.isfinite(float(opt.last_grad_norm))
    assert int(opt.skipped_steps) == 1
    assert opt.state_dict()["state"][0]["step"] == 1
    for a, b in zip(_state(m, opt), before):
        assert torch.equal(a, b)
    # split path, foreign gradient tensors (staged into the flat buffer by step()), one inf among them
    x2, e2 = _batch(3)
    m.fused_forward_backward(x2, eps=e2)
    for g in opt.param_groups:
        for p in g["params"]:
            p.grad = p.grad.detach().clone()
    opt.param_groups[1]["params"][0].grad.view(-1)[3] = float("inf")
    opt.step()
    assert not math.isfinite(float(opt.last_grad_norm))
    assert int(opt.skipped_steps) == 2 and opt.state_dict()["state"][0]["step"] == 1
    for a, b in zip(_state(m, opt), before):
        assert torch.equal(a, b)
    # the next clean step: bit-identical to the twin's second step
    x3, e3 = _batch(4)
    for mm, oo in ((m, opt), (twin, topt)):
        fused_step(mm, oo, x3, eps=e3)
    for a, b in zip(_state(m, opt), _state(twin, topt)):
        assert torch.equal(a, b)
    assert torch.equal(opt.last_grad_norm, topt.last_grad_norm) and math.isfinite(float(opt.last_grad_norm))
    assert int(topt.skipped_steps) == 0 and opt.state_dict()["state"][0]["step"] == topt.state_dict()["state"][0]["step"] == 2


def test_checkpoint_carries_device_step_through_torch_adamw():
    """After a skip, state_dict() reports the device step; the state loads into torch.optim.AdamW and back, group keys equal."""
    from torch_vae_amd.train import fused_step
    m, opt, _ = _setup("f32", max_grad_norm=1.0, skip_nonfinite=True)
    for i in (1, 2):
        x, eps = _batch(i)
        fused_step(m, opt, x, eps=eps)
    xb, eb = _batch(3)
    xb[0, 0, 0, 0] = float("nan")
    fused_step(m, opt, xb, eps=eb)
    assert int(opt.skipped_steps) == 1
    sd = opt.state_dict()
    assert all(float(st["step"]) == 2 for st in sd["state"].values())
    topt = torch.optim.AdamW([{"params": list(g["params"])} for g in opt.param_groups])
    assert set(opt.defaults) == set(topt.defaults)            # the options are attributes, not group keys
    topt.load_state_dict(sd)
    assert [set(g) for g in topt.param_groups] == [set(g) for g in opt.param_groups]
    m2, opt2, _ = _setup("f32", max_grad_norm=1.0, skip_nonfinite=True)
    opt2.load_state_dict(topt.state_dict())
    assert int(opt2._clip_state()[0]) == 2 and float(opt2.state_dict()["state"][0]["step"]) == 2
    assert torch.equal(opt2._m, opt._m) and torch.equal(opt2._v, opt._v)
    # both continue identically from there
    m2.flat_parameters().copy_(m.flat_parameters())
    x4, e4 = _batch(4)
    for mm, oo in ((m, opt), (m2, opt2)):
        fused_step(mm, oo, x4, eps=e4)
    for a, b in zip(_state(m, opt), _state(m2, opt2)):
        assert torch.equal(a, b)


def test_clipped_exchanges_single_rank_rccl():
    """With the clip active, the in-line (1) and bucketed (2) gradient exchanges of the one-call step on a one-rank RCCL
    communicator leave the same bits as no exchange (0)."""
    import torch.distributed as dist
    from torch_vae_amd.train import enable_library_allreduce, fused_step
    mx = 0.25 * _probe_norm("f32")

    def run(mode):
        m, opt, _ = _setup("f32", max_grad_norm=mx, skip_nonfinite=True)
        if mode is not None:
            assert enable_library_allreduce(m)
        for i in (1, 2):
            x, eps = _batch(i)
            fused_step(m, opt, x, eps=eps, overlap=mode)
        if mode is not None:
            assert m.library_comm_world() == 1
        assert float(opt.last_grad_norm) > mx
        return _state(m, opt) + [opt.last_grad_norm.clone(), m.flat_grads().clone()]

    ref = run(None)
    env = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY", "GPU_MAX_HW_QUEUES")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29589", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) >= 8:
        os.environ["GPU_MAX_HW_QUEUES"] = "6"    # (train.fused_step refuses the bucketed exchange with eight queues)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for mode in (False, True):
            for a, b in zip(run(mode), ref):
                assert torch.equal(a, b), mode
    finally:
        dist.destroy_process_group()
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_train_one_epoch_clips_like_torch():
    """config.max_grad_norm through train_one_epoch: FusedAdamW (fused loop, clip on the device) and torch.optim.AdamW (autograd loop,
    torch's clip_grad_norm_) end three steps within 1e-5."""
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    mx = 0.25 * _probe_norm("f32")
    cfg = _cfg(max_grad_norm=mx)
    batches = [_batch(i) for i in (1, 2, 3)]
    loader = [(x.cpu(), torch.zeros(B, dtype=torch.long)) for x, _ in batches]
    p = perturbed_params(L, H, 61, GEN)
    m = make_model(H, L, GEN, "f32", p)
    opt, sched = build_optimizer(cfg, m, steps_per_epoch=10)
    it = iter([e for _, e in batches])
    orig = m.fused_train_step
    m.fused_train_step = lambda o, x, **k: orig(o, x, **{**k, "eps": next(it)})
    res, n_steps, _ = train_one_epoch(cfg, m, opt, sched, m.loss, loader, device="cuda", epoch=1)
    assert n_steps == 3 and "skipped_steps" not in res and float(opt.last_grad_norm) > mx
    m2 = make_model(H, L, GEN, "f32", p)
    topt = torch.optim.AdamW([{"params": m2.encoder.parameters(), "lr": cfg.lr}, {"params": m2.decoder.parameters(), "lr": cfg.lr}],
                             lr=cfg.lr, weight_decay=cfg.weight_decay)
    tsched = torch.optim.lr_scheduler.OneCycleLR(topt, [g["lr"] for g in topt.param_groups], epochs=1, steps_per_epoch=10)
    it2 = iter([e for _, e in batches])
    fwd = m2.forward

    def forward_with_eps(x):
        m2.set_next_eps(next(it2))
        return fwd(x)

    m2.forward = forward_with_eps
    res2, _, _ = train_one_epoch(cfg, m2, topt, tsched, m2.loss, loader, device="cuda", epoch=1)
    np.testing.assert_allclose(res2["loss"], res["loss"], rtol=1e-5)
    d = rel_l2(m2.flat_parameters().cpu().numpy(), m.flat_parameters().cpu().numpy())
    assert d < 1e-5, d
    # skip_nonfinite adds the count to the results
    m3, opt3, sched3 = _setup("f32", max_grad_norm=mx, skip_nonfinite=True)
    it3 = iter([e for _, e in batches])
    orig3 = m3.fused_train_step
    m3.fused_train_step = lambda o, x, **k: orig3(o, x, **{**k, "eps": next(it3)})
    res3, _, _ = train_one_epoch(_cfg(max_grad_norm=mx, skip_nonfinite=True), m3, opt3, sched3, m3.loss, loader, device="cuda", epoch=1)
    assert res3["skipped_steps"] == 0 and res3["loss"] == res["loss"]
