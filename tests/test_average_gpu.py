"""Weight averaging on the GPU: the kernels of include/vae_average.h on bare buffers against the float64 reference of
tests/average_ref.py and against torch.lerp, the gate, the exchange, and the Python layer (torch_vae_amd/averaging.py) on the
smallest model: the average beside the fused step, a step skipped on the device, applied(), checkpoints, the training loop and
update_bn.

The single-update bounds are derived from the formula, not measured.  With M = max(|e|, |s|) elementwise:
  against the reference (exact lerp, w in float64): one rounding of s - e (<= 2^-24 |s - e| <= 2^-23 M, then times |w| or |1 - w| <= 1),
  one of w to float32 (<= 2^-24 w |s - e| <= 2^-23 M) and one of the fused multiply-add (<= 2^-24 M): 2.5 * 2^-24 M < 2^-22 M;
  against torch.lerp in float32 on the CPU, which rounds in its own places: both sides' errors, 2^-21 M.
A trajectory of k updates stays within k * 2^-22 * M (M over the whole trajectory): the lerp is a contraction, it does not amplify
what earlier updates left."""
import copy
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from oracle.torch_cpu_step import TorchCpuStep
from tests import average_ref as R
from tests.util import make_model, perturbed_params

pytestmark = pytest.mark.gpu

GUARD = 64                         # floats: 256 bytes, so the payload keeps the 16-byte alignment
SIZES = [1, 3, 4, 255, 1029, (1 << 20) + 7]
STRIDE_SIZE = (1 << 21) + 9        # more than 2048 workgroups * 256 lanes * 4 floats: the stride loop takes a second pass
WEIGHTS = [0.001, 0.5, 0.9]
TOL_REF, TOL_TORCH = 2.0 ** -22, 2.0 ** -21
H, L, B = 32, 16, 4


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from torch_vae_amd import _lib
    return _lib.lib()


def ok(rc, what="vae_average"):
    assert rc == 0, (what, lib().vae_last_error().decode())


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = host(a) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def guarded(values, fill=-7.5):
    """(whole buffer, payload view) on the GPU: the float32 values between two guard bands"""
    values = np.asarray(values, np.float32)
    buf = torch.full((2 * GUARD + values.size,), fill, device="cuda")
    buf[GUARD:GUARD + values.size] = torch.from_numpy(values).cuda()
    return buf, buf[GUARD:GUARD + values.size]


def guards_intact(buf, n, fill=-7.5):
    g = host(buf)
    return bool((g[:GUARD] == fill).all() and (g[GUARD + n:] == fill).all())


def new_state(n_averaged=0, opt_step=None):
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    ok(lib().vae_average_state_init(state.data_ptr(), 0 if opt_step is None else opt_step.data_ptr(), n_averaged, st()), "state_init")
    return state


def read_state(state):
    raw = state.cpu()
    return int(raw[0]), int(raw[1]), float(raw.view(torch.float64)[2])


def call_update(avg0, src0, avg1, src1, state, *, kind=R.EMA, decay=0.999, warmup=0.0, opt_step=None, scale0=1.0, scale1=1.0):
    p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    n = lambda t: 0 if t is None else t.numel()  # noqa: E731
    return lib().vae_average_update(p(avg0), p(src0), n(avg0), scale0, p(avg1), p(src1), n(avg1), scale1, kind, decay, warmup, p(opt_step),
                                    state.data_ptr(), st())


def data(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def check_single_update(n, w, n2=5):
    """One EMA update with weight w = 1 - decay on segments of n and n2 floats; both gates of the module docstring."""
    decay = 1.0 - w
    (e0, s0), (e1, s1) = data(n, 10 * n + 1), data(n2, 10 * n + 2)
    abuf0, a0 = guarded(e0)
    abuf1, a1 = guarded(e1)
    d0, d1 = torch.from_numpy(s0).cuda(), torch.from_numpy(s1).cuda()
    state = new_state(n_averaged=5)
    ok(call_update(a0, d0, a1, d1, state, decay=decay))
    copy_, w64 = R.weight(R.EMA, 5, decay)
    assert not copy_ and read_state(state) == (-1, 6, float(np.float32(w64)))
    assert guards_intact(abuf0, n) and guards_intact(abuf1, n2), "a float outside avg was written"
    assert np.array_equal(bits(d0), bits(s0)) and np.array_equal(bits(d1), bits(s1)), "src was written"
    for e, s, got in ((e0, s0, host(a0)), (e1, s1, host(a1))):
        m = np.maximum(np.abs(e), np.abs(s)).astype(np.float64)
        err_ref = np.abs(got.astype(np.float64) - R.lerp(e, s, w64))
        lerp_cpu = torch.lerp(torch.from_numpy(e), torch.from_numpy(s), float(np.float32(w64))).numpy()
        err_torch = np.abs(got.astype(np.float64) - lerp_cpu.astype(np.float64))
        print(f"n={e.size} w={w}: largest error / M against the reference {np.max(err_ref / m):.3e} (bound {TOL_REF:.3e}), "
              f"against torch.lerp {np.max(err_torch / m):.3e} (bound {TOL_TORCH:.3e})")
        assert (err_ref <= TOL_REF * m).all(), (e.size, w, int(np.argmax(err_ref / m)))
        assert (err_torch <= TOL_TORCH * m).all(), (e.size, w, int(np.argmax(err_torch / m)))
        assert not np.array_equal(got, e)


# ---- 1. the C ABI on bare buffers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("n", SIZES)
def test_single_update_against_the_reference_and_torch_lerp(n, w):
    check_single_update(n, w)


def test_single_update_where_the_stride_loop_takes_a_second_pass():
    check_single_update(STRIDE_SIZE, 0.001, n2=1029)
    check_single_update(5, 0.9, n2=STRIDE_SIZE)          # (the long segment second)


def test_scaled_source_and_equal_weight():
    """src_scale != 1 (update_bn's 10.f) and VAE_AVG_EQUAL: s = fl(src * scale) in float32, w = 1 / (n + 1)."""
    e, s = data(1029, 77)
    for n_avg in (1, 2, 7):
        abuf, a = guarded(e)
        d = torch.from_numpy(s).cuda()
        state = new_state(n_averaged=n_avg)
        ok(call_update(a, d, None, None, state, kind=R.EQUAL, scale0=10.0))
        w64 = 1.0 / (n_avg + 1.0)
        s32 = s * np.float32(10.0)
        m = np.maximum(np.abs(e), np.abs(s32)).astype(np.float64)
        assert (np.abs(host(a).astype(np.float64) - R.lerp(e, s32, w64)) <= TOL_REF * m).all(), n_avg
        assert read_state(state) == (-1, n_avg + 1, float(np.float32(w64))) and guards_intact(abuf, e.size)


def test_trajectory_of_20_updates():
    n, n2, k = 1029, 5, 20
    rng = np.random.default_rng(4)
    srcs = [(rng.standard_normal(n).astype(np.float32), rng.standard_normal(n2).astype(np.float32)) for _ in range(k)]
    for kind, kw in ((R.EMA, dict(decay=0.99, warmup=10.0)), (R.EMA, dict(decay=0.9)), (R.EQUAL, {})):
        ref = R.AverageRef(kind, **kw)
        abuf0, a0 = guarded(np.full(n, np.nan, np.float32))          # (the first update copies: what avg held is gone)
        abuf1, a1 = guarded(np.full(n2, np.nan, np.float32))
        state = new_state()
        weights = []
        for s0, s1 in srcs:
            ok(call_update(a0, torch.from_numpy(s0).cuda(), a1, torch.from_numpy(s1).cuda(), state, kind=kind, **kw))
            ref.update([s0, s1])
            weights.append(ref.last_weight)
        assert read_state(state) == (-1, k, ref.last_weight)
        if kw.get("warmup"):
            assert max(weights[1:]) > 0.5 > min(weights)          # both branches of the lerp were taken
        M = max(np.abs(np.concatenate(p)).max() for p in srcs)
        for got, want in ((host(a0), ref.avg[0]), (host(a1), ref.avg[1])):
            err = np.abs(got.astype(np.float64) - want).max()
            print(f"trajectory kind={kind} {kw}: largest error {err:.3e}, bound {k * TOL_REF * M:.3e}")
            assert err <= k * TOL_REF * M
        assert guards_intact(abuf0, n) and guards_intact(abuf1, n2)


def test_the_first_update_is_a_bit_copy():
    n = 1029
    s = np.random.default_rng(2).standard_normal(n).astype(np.float32)
    sb = s.view(np.uint32).copy()
    sb[0], sb[5], sb[1027], sb[1028] = 0x7FC12345, 0x7F800000, 0xFF800000, 0x7F923456     # quiet NaN with a payload, +inf, -inf, signalling NaN
    sb[7], sb[8] = 0x80000000, 0x00000001                                                   # -0, the smallest subnormal
    s = sb.view(np.float32)
    d = torch.from_numpy(s.copy()).cuda()
    assert np.array_equal(bits(d), sb)
    for kind in (R.EMA, R.EQUAL):
        abuf, a = guarded(np.full(n, np.nan, np.float32))
        t2 = torch.from_numpy(s[:5].copy()).cuda()
        abuf2, a2 = guarded(np.zeros(5, np.float32))
        state = new_state()
        ok(call_update(a, d, a2, t2, state, kind=kind, decay=0.3, warmup=4.0))
        assert np.array_equal(bits(a), bits(d)) and np.array_equal(bits(a2), bits(t2)), kind
        assert read_state(state) == (-1, 1, 1.0) and guards_intact(abuf, n) and guards_intact(abuf2, 5)
    # a scaled first update is the float32 product, whatever avg held
    s = np.random.default_rng(8).standard_normal(n).astype(np.float32)
    s[0], s[5], s[1027], s[1028] = np.nan, np.inf, -np.inf, -0.0
    d = torch.from_numpy(s).cuda()
    abuf, a = guarded(np.full(n, np.inf, np.float32))
    ok(call_update(a, d, None, None, new_state(), kind=R.EQUAL, scale0=10.0))
    with np.errstate(invalid="ignore", over="ignore"):
        want = s * np.float32(10.0)
    fin = np.isfinite(want)
    got = host(a)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32)) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])


def test_the_gate():
    n = 1029
    e, s = data(n, 9)
    abuf, a = guarded(e)
    a2buf, a2 = guarded(e[:5])
    d, d2 = torch.from_numpy(s).cuda(), torch.from_numpy(s[:5].copy()).cuda()
    step = torch.full((), 7, dtype=torch.int64, device="cuda")
    state = new_state(n_averaged=3, opt_step=step)
    assert read_state(state) == (7, 3, 0.0)
    before = (bits(a).copy(), bits(a2).copy(), bits(state).copy())
    ok(call_update(a, d, a2, d2, state, kind=R.EQUAL, opt_step=step))               # the step the state has seen: nothing happens
    assert np.array_equal(bits(a), before[0]) and np.array_equal(bits(a2), before[1]) and np.array_equal(bits(state), before[2])
    step.fill_(8)
    ok(call_update(a, d, a2, d2, state, kind=R.EQUAL, opt_step=step))               # a new step: applied
    assert read_state(state) == (8, 4, 0.25)
    want = R.lerp(e, s, 0.25)
    assert (np.abs(host(a).astype(np.float64) - want) <= TOL_REF * np.maximum(np.abs(e), np.abs(s))).all()
    after = bits(a).copy()
    ok(call_update(a, d, a2, d2, state, kind=R.EQUAL, opt_step=step))               # the same step again: nothing
    assert np.array_equal(bits(a), after) and read_state(state) == (8, 4, 0.25)
    ok(call_update(a, d, a2, d2, state, kind=R.EQUAL, opt_step=None))               # no counter: always applied, seen_step kept
    assert read_state(state) == (8, 5, float(np.float32(0.2))) and not np.array_equal(bits(a), after)
    step.fill_(-1)
    fresh = new_state(opt_step=None)
    assert read_state(fresh) == (-1, 0, 0.0)
    ok(call_update(a, d, a2, d2, fresh, opt_step=step))                             # a counter that reads -1 is "seen" by a state without one
    assert read_state(fresh) == (-1, 0, 0.0)
    assert guards_intact(abuf, n) and guards_intact(a2buf, 5)


def test_identical_call_sequences_give_identical_bits():
    n = (1 << 20) + 7
    rng = np.random.default_rng(12)
    srcs = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda() for _ in range(3)]
    small = [torch.from_numpy(rng.standard_normal(5).astype(np.float32)).cuda() for _ in range(3)]
    runs = []
    for _ in range(2):
        a, a2, state = torch.empty(n, device="cuda"), torch.empty(5, device="cuda"), new_state()
        for s, s2 in zip(srcs, small):
            ok(call_update(a, s, a2, s2, state, decay=0.9))
        runs.append((bits(a), bits(a2), bits(state)))
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


@pytest.mark.parametrize("n,n2", [(1, 5), (3, 0), (4, 255), (1029, 5), ((1 << 20) + 7, 3), (5, STRIDE_SIZE)])
def test_swap(n, n2):
    rng = np.random.default_rng(n + n2)
    va, vb, vc, vd = (rng.standard_normal(k).astype(np.float32) for k in (n, n, n2, n2))
    va[0] = np.nan
    bufs = [guarded(v) for v in (va, vb, vc, vd)]
    (_, a), (_, b), (_, c), (_, d) = bufs
    p = lambda t: t.data_ptr() if t.numel() else 0  # noqa: E731
    ok(lib().vae_average_swap(p(a), p(b), n, p(c), p(d), n2, st()), "swap")
    assert np.array_equal(bits(a), bits(vb)) and np.array_equal(bits(b), bits(va)) and np.array_equal(bits(c), bits(vd)) and np.array_equal(bits(d), bits(vc))
    ok(lib().vae_average_swap(p(a), p(b), n, p(c), p(d), n2, st()), "swap")
    assert np.array_equal(bits(a), bits(va)) and np.array_equal(bits(b), bits(vb)) and np.array_equal(bits(c), bits(vc)) and np.array_equal(bits(d), bits(vd))
    assert all(guards_intact(buf, v.numel()) for buf, v in bufs)


def test_refused_calls_enqueue_nothing():
    n = 1029
    e, s = data(n, 3)
    abuf, a = guarded(e)
    d = torch.from_numpy(s).cuda()
    state = new_state(n_averaged=2)
    before = (bits(abuf).copy(), bits(d).copy(), bits(state).copy())
    L_ = lib()
    refused = [
        call_update(a, d, None, None, state, decay=1.5), call_update(a, d, None, None, state, decay=float("nan")),
        call_update(a, d, None, None, state, warmup=-1.0), call_update(a, d, None, None, state, kind=2),
        call_update(a, d, None, None, state, scale0=float("inf")), call_update(a, a, None, None, state),
        call_update(a[1:], d[1:], None, None, state), call_update(a, d, a[4:12], d[4:12], state),
        L_.vae_average_update(a.data_ptr(), d.data_ptr(), n, 1.0, 0, 0, 0, 1.0, 0, 0.9, 0.0, 0, 0, st()),
        L_.vae_average_update(a.data_ptr(), 0, n, 1.0, 0, 0, 0, 1.0, 0, 0.9, 0.0, 0, state.data_ptr(), st()),
        L_.vae_average_update(a.data_ptr(), d.data_ptr(), -1, 1.0, 0, 0, 0, 1.0, 0, 0.9, 0.0, 0, state.data_ptr(), st()),
        L_.vae_average_swap(a.data_ptr(), a.data_ptr(), n, 0, 0, 0, st()), L_.vae_average_swap(a.data_ptr(), d.data_ptr() + 4, n - 1, 0, 0, 0, st()),
        L_.vae_average_swap(a.data_ptr(), 0, n, 0, 0, 0, st()), L_.vae_average_state_init(state.data_ptr(), 0, -1, st()),
        L_.vae_average_state_init(0, 0, 0, st()),
    ]
    assert refused == [-1] * len(refused)
    assert L_.vae_last_error().decode().startswith("vae_average_state_init: ")
    assert ok(call_update(None, None, None, None, state)) is None                  # n == 0 twice: accepted, and nothing launched
    torch.cuda.synchronize()
    assert np.array_equal(bits(abuf), before[0]) and np.array_equal(bits(d), before[1]) and np.array_equal(bits(state), before[2])


# ---- 2. with a model -------------------------------------------------------------------------------------------------------------------
def batches(k, seed=40):
    return [torch.from_numpy(vo.synth_pianoroll(B, H, seed + i).astype(np.float32)).cuda() for i in range(k)]


def model_and_optimizer(dtype, seed=21, **opt_kw):
    from torch_vae_amd.optim import FusedAdamW
    model = make_model(H, L, False, dtype, perturbed_params(L, H, seed, False))
    opt = FusedAdamW([{"params": model.encoder.parameters()}, {"params": model.decoder.parameters()}], lr=1e-2, weight_decay=0.0, **opt_kw)
    return model, opt


def snapshot(model):
    return model._flat.clone(), model._bnflat.clone()


def param_slices(model, prefixes):
    from torch_vae_amd import _lib
    return [(n, model._offs[i], model._sizes[i]) for i, n in enumerate(_lib.PARAM_NAMES) if n.split(".")[0] in prefixes]


def assert_matches_reference(avg, ref, snaps, what):
    """the averager's two buffers against the float64 recursion on the snapshots [(parameters, buffers)] it averaged, within the
    trajectory bound of that many updates, elementwise (M: an element's largest magnitude over the snapshots)"""
    k = len(snaps)
    for i, (got, want) in enumerate(((host(avg._params), ref.avg[0]), (host(avg._buffers), ref.avg[1]))):
        both = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), both), what
        if not both.any():      # (a planted inf went through every BatchNorm: no finite statistic is left to compare)
            continue
        with np.errstate(invalid="ignore"):
            M = np.max([np.abs(host(s[i]).astype(np.float64)) for s in snaps], axis=0)
        err = np.abs(got[both].astype(np.float64) - want[both])
        print(f"{what}: largest error {err.max():.3e} at a bound of {k * TOL_REF * M[both][np.argmax(err)]:.3e}")
        assert (err <= k * TOL_REF * M[both]).all(), what


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind,kw", [("ema", dict(decay=0.9)), ("ema", dict(decay=0.99, warmup=3.0)), ("swa", {})])
def test_five_fused_steps_with_an_update_after_each(dtype, kind, kw):
    from torch_vae_amd.averaging import WeightAverage
    from torch_vae_amd.train import fused_step
    model, opt = model_and_optimizer(dtype)
    avg = WeightAverage(model, kind=kind, **kw)
    ref = R.AverageRef(kind, **kw)
    snaps = []
    torch.manual_seed(1)
    for x in batches(5):
        fused_step(model, opt, x, use_device_eps=False)
        avg.update(opt)
        snaps.append(snapshot(model))
    for flat, bn in snaps:                               # (read back after the loop: nothing synchronised inside it)
        assert ref.update([host(flat), host(bn)])
    assert int(avg.n_averaged) == 5 and float(avg.last_weight) == ref.last_weight
    assert_matches_reference(avg, ref, snaps, f"{dtype} {kind} {kw}")
    assert not np.array_equal(bits(avg._params), bits(model._flat)) and not np.array_equal(bits(avg._buffers), bits(model._bnflat))
    # fc_mu, fc_var, decoder_input and final_layer are never optimised: they average to themselves, bit for bit
    frozen = param_slices(model, ("fc_mu", "fc_var", "decoder_input", "final_layer"))
    assert len(frozen) == 12
    for name, o, n in frozen:
        assert np.array_equal(bits(avg._params[o:o + n]), bits(model._flat[o:o + n])), name
    moved = param_slices(model, ("encoder", "decoder"))
    assert all(not np.array_equal(bits(avg._params[o:o + n]), bits(model._flat[o:o + n])) for name, o, n in moved if name.endswith(".0.weight"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_step_skipped_on_the_device_is_invisible_to_the_average(dtype):
    from torch_vae_amd.averaging import WeightAverage
    from torch_vae_amd.train import fused_step
    model, opt = model_and_optimizer(dtype, skip_nonfinite=True)
    avg = WeightAverage(model, kind="ema", decay=0.9)
    avg.reset(opt)
    xs = batches(5)
    xs[2] = xs[2].clone()
    xs[2][0, 0, 3, 5] = float("inf")
    snaps = []
    torch.manual_seed(1)
    for x in xs:
        fused_step(model, opt, x, use_device_eps=False)
        avg.update(opt)
        snaps.append(snapshot(model))
    assert int(avg.n_averaged) == 4 and int(opt.skipped_steps) == 1 and int(avg._state[0]) == 4
    assert np.array_equal(bits(snaps[2][0]), bits(snaps[1][0]))          # the skipped step left the parameters alone
    ref = R.AverageRef("ema", decay=0.9, seen_step=0)
    applied = [ref.update([host(flat), host(bn)], opt_step=count) for (flat, bn), count in zip(snaps, (1, 2, 2, 3, 4))]
    assert applied == [True, True, False, True, True] and ref.n_averaged == 4
    # (the inf went through the forward's BatchNorm: the running statistics of the steps after it are not finite, in the model and in
    #  the reference alike; the parameters are)
    assert np.isfinite(host(avg._params)).all()
    assert_matches_reference(avg, ref, [snaps[i] for i in (0, 1, 3, 4)], f"{dtype} skipped step")
    # the average that counts the skipped step is another one
    wrong = R.AverageRef("ema", decay=0.9)
    for flat, bn in snaps:
        wrong.update([host(flat), host(bn)])
    assert np.abs(wrong.avg[0] - ref.avg[0]).max() > 10 * 4 * TOL_REF * np.abs(ref.avg[0]).max()


def test_the_gate_needs_no_optimiser_counter():
    """A FusedAdamW without clipping or skipping keeps its count on the host, a torch optimiser has none: every update applies."""
    from torch_vae_amd.averaging import WeightAverage
    model, opt = model_and_optimizer("f32")
    avg = WeightAverage(model, kind="swa")
    assert avg._step_counter(opt) is None and avg._step_counter(torch.optim.SGD(model.parameters(), lr=0.1)) is None and avg._step_counter(None) is None
    for _ in range(3):
        avg.update(opt)
    assert int(avg.n_averaged) == 3 and np.array_equal(bits(avg._params), bits(model._flat))      # the mean of three equal things


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_applied_runs_the_model_on_the_average_and_restores_it(dtype):
    from torch_vae_amd.averaging import WeightAverage
    from torch_vae_amd.evaluation import evaluate
    from torch_vae_amd.train import fused_step
    model, opt = model_and_optimizer(dtype)
    avg = WeightAverage(model, kind="ema", decay=0.5)
    torch.manual_seed(1)
    for x in batches(3):
        fused_step(model, opt, x, use_device_eps=False)
        avg.update(opt)
    twin = make_model(H, L, False, dtype)
    sd = avg.module_state_dict()
    assert list(sd) == list(model.state_dict()) and all(sd[k].shape == v.shape and sd[k].dtype == v.dtype for k, v in model.state_dict().items())
    twin.load_state_dict(sd)
    assert np.array_equal(bits(twin._flat), bits(avg._params)) and np.array_equal(bits(twin._bnflat), bits(avg._buffers))
    assert np.array_equal(host(twin._nbt), host(model._nbt))
    before = (bits(model._flat).copy(), bits(model._bnflat).copy(), host(model._nbt).copy(), bits(avg._params).copy(), bits(avg._buffers).copy())
    z = torch.randn(B, L, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    loader = [(x, torch.zeros(B, dtype=torch.long)) for x in batches(2, seed=90)]
    model.eval(); twin.eval()
    with torch.no_grad():
        own = model.decode(z).clone()
        want_decode = twin.decode(z).clone()
    torch.manual_seed(8)
    want_eval = evaluate(loader, twin, "cuda", verbosity=0)
    with avg.applied() as m:
        assert m is model and model._last is None
        with torch.no_grad():
            got_decode = model.decode(z).clone()
        torch.manual_seed(8)
        got_eval = evaluate(loader, model, "cuda", verbosity=0)
        with pytest.raises(RuntimeError, match="does not nest"):
            with avg.applied():
                pass
        for call in (avg.update, avg.state_dict, avg.module_state_dict, avg.copy_to):
            with pytest.raises(RuntimeError, match="inside applied"):
                call()
        assert model._last is not None
    assert model._last is None
    assert np.array_equal(bits(got_decode), bits(want_decode)) and not np.array_equal(bits(got_decode), bits(own))
    assert got_eval == want_eval, (got_eval, want_eval)

    def restored():
        now = (bits(model._flat), bits(model._bnflat), host(model._nbt), bits(avg._params), bits(avg._buffers))
        return all(np.array_equal(a, b) for a, b in zip(now, before))
    assert restored()
    with pytest.raises(KeyError, match="boom"):
        with avg.applied():
            assert np.array_equal(bits(model._flat), before[3])
            raise KeyError("boom")
    assert restored() and not avg._applied
    with avg.applied():                                  # (and it can be entered again)
        pass
    assert restored()
    # copy_to writes the average into a model for good
    avg.copy_to(twin)
    assert np.array_equal(bits(twin._flat), before[3]) and np.array_equal(bits(twin._bnflat), before[4])


def test_state_dict_round_trip_then_one_more_update():
    from torch_vae_amd.averaging import WeightAverage
    from torch_vae_amd.train import fused_step
    model, opt = model_and_optimizer("f32", skip_nonfinite=True)
    avg = WeightAverage(model, kind="ema", decay=0.99, warmup=2.0)
    avg.reset(opt)
    xs = batches(4)
    torch.manual_seed(1)
    for x in xs[:3]:
        fused_step(model, opt, x, use_device_eps=False)
        avg.update(opt)
    state = copy.deepcopy(avg.state_dict())
    assert (state["n_averaged"], state["seen_step"], state["kind"], state["decay"], state["warmup"]) == (3, 3, "ema", 0.99, 2.0)
    assert state["last_weight"] == R.weight_f32(R.EMA, 2, 0.99, 2.0)
    loaded = [WeightAverage(model, kind="swa"), WeightAverage(model, kind="swa")]
    loaded[0].load_state_dict(state, opt)                # the optimiser's own device count is marked as seen
    loaded[1].load_state_dict(state)                     # the checkpoint's seen_step is
    for other in loaded:
        assert (other.kind, other.decay, other.warmup) == ("ema", 0.99, 2.0) and np.array_equal(bits(other._state), bits(avg._state))
        other.update(opt)                                # no step since: the reloaded average does not take the current one for new
        assert int(other.n_averaged) == 3 and np.array_equal(bits(other._params), bits(avg._params))
    fused_step(model, opt, xs[3], use_device_eps=False)
    for a in [avg] + loaded:
        a.update(opt)
    for other in loaded:
        assert np.array_equal(bits(other._params), bits(avg._params)) and np.array_equal(bits(other._buffers), bits(avg._buffers))
        assert np.array_equal(bits(other._state), bits(avg._state)) and int(other.n_averaged) == 4
    with pytest.raises(ValueError, match="geometry"):
        loaded[0].load_state_dict(dict(state, params=state["params"][:-1]))


def base_config(**extra):
    return Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                     epochs=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0, **extra)


def epoch_loader(steps, seed=70):
    return [(torch.from_numpy(vo.synth_pianoroll(B, H, seed + s).astype(np.float32)), torch.zeros(B, dtype=torch.long)) for s in range(steps)]


@pytest.mark.parametrize("optimizer", ["AdamW", "Adam"])      # the fused optimiser, and a torch one (no device counter)
def test_train_one_epoch_follows_the_schedule(optimizer, tmp_path):
    from torch_vae_amd import utils
    from torch_vae_amd.averaging import WeightAverage
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    model = make_model(H, L, False, "f32", vo.init_params(L, H, 61, False))
    cfg = base_config(weight_average="ema", ema_decay=0.9, ema_warmup=1.0, avg_start_step=2, avg_every=2)
    cfg.optimizer = optimizer
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=10)
    keys = list(model.state_dict())
    seen = []
    orig = WeightAverage.update

    def spy(self, optimizer_=None):
        seen.append((optimizer_, model._flat.clone(), model._bnflat.clone()))
        return orig(self, optimizer_)
    WeightAverage.update = spy
    try:
        torch.manual_seed(5)
        _, total_step, _ = train_one_epoch(cfg, model, opt, sched, model.loss, epoch_loader(6), device="cuda", epoch=1)
    finally:
        WeightAverage.update = orig
    avg = model.weight_average
    assert isinstance(avg, WeightAverage) and total_step == 6 and int(avg.n_averaged) == 3 and len(seen) == 3
    assert all(o is opt for o, _, _ in seen) and list(model.state_dict()) == keys and "weight_average" not in dict(model.named_modules())
    assert (avg.kind, avg.decay, avg.warmup, avg.start_step, avg.every, avg.use_buffers) == ("ema", 0.9, 1.0, 2, 2, True)
    ref = R.AverageRef("ema", decay=0.9, warmup=1.0)
    for _, flat, bn in seen:
        ref.update([host(flat), host(bn)])
    assert_matches_reference(avg, ref, [(flat, bn) for _, flat, bn in seen], f"train_one_epoch {optimizer}")
    # the next epoch goes on with the model's own average, and the schedule with total_step
    _, total_step, _ = train_one_epoch(cfg, model, opt, sched, model.loss, epoch_loader(3, seed=80), device="cuda", epoch=2, total_step=total_step)
    assert model.weight_average is avg and total_step == 9 and int(avg.n_averaged) == 4          # total_step 8
    # the checkpoint carries it, and a fresh model gets it back
    mods = utils.checkpoint_modules(model, opt, sched, save_all_modules=True)
    assert "weight_average" in mods
    path = utils.safe_save_model(mods, checkpoint_path=str(tmp_path / "ckpt.pt"), total_step=total_step)
    model2 = make_model(H, L, False, "f32")
    opt2, sched2 = build_optimizer(cfg, model2, steps_per_epoch=10)
    assert utils.load_checkpoint(model2, opt2, sched2, path)["total_step"] == 9
    avg2 = model2.weight_average
    assert np.array_equal(bits(avg2._params), bits(avg._params)) and np.array_equal(bits(avg2._buffers), bits(avg._buffers))
    assert int(avg2.n_averaged) == 4 and (avg2.kind, avg2.decay, avg2.warmup, avg2.start_step, avg2.every) == ("ema", 0.9, 1.0, 2, 2)
    assert np.array_equal(bits(model2._flat), bits(model._flat))


def test_train_one_epoch_without_the_field_is_the_loop_as_it_is():
    from torch_vae_amd.train import build_optimizer, fused_step, train_one_epoch
    steps = 3
    p = vo.init_params(L, H, 61, False)
    loader = epoch_loader(steps)
    runs = []
    for how in ("train_one_epoch", "by hand"):
        model = make_model(H, L, False, "f32", p)
        cfg = base_config() if how == "by hand" else base_config(weight_average=None, ema_decay=0.9, avg_start_step=0, avg_every=1)
        opt, sched = build_optimizer(cfg, model, steps_per_epoch=10)
        torch.manual_seed(5)
        got = []
        if how == "by hand":          # the body of the loop as it was: the batch to the device, one fused_step, the scheduler
            for x, _ in loader:
                out3, _ = fused_step(model, opt, x.to("cuda"), use_device_eps=False)
                sched.step()
                got.append(out3.clone())
        else:
            orig = model.fused_train_step

            def step(o, x, **k):
                out = orig(o, x, **k)
                got.append(out[0].clone())
                return out
            model.fused_train_step = step
            train_one_epoch(cfg, model, opt, sched, model.loss, loader, device="cuda", epoch=1)
            assert getattr(model, "weight_average", None) is None
        runs.append((got, model.flat_parameters().clone(), model._bnflat.clone()))
    assert len(runs[0][0]) == len(runs[1][0]) == steps
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(runs[0][0], runs[1][0]))
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1])) and np.array_equal(bits(runs[0][2]), bits(runs[1][2]))


# ---- 3. update_bn ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_update_bn_over_three_batches(dtype):
    """The averaged model's buffers become the cumulative mean of the per-batch statistics.  Against the float64 mean of the
    per-batch 10 * running' values the bound is 2^-21 * M elementwise, M the largest of the three magnitudes: the first fold is a
    copy, the second and third are lerps with w = 1/2 and 1/3, each within 2^-22 * M, and the third shrinks what the second left by
    2/3: (2/3 + 1) * 2^-22 < 2^-21.  Against the CPU oracle (f32 only): the project's gate for BatchNorm statistics, rtol 1e-4, atol 1e-6."""
    from torch_vae_amd import _lib
    from torch_vae_amd.averaging import WeightAverage
    p = perturbed_params(L, H, 33, False)
    model = make_model(H, L, False, dtype, p)
    avg = WeightAverage(model, kind="swa", use_buffers=(dtype == "f32"))
    avg.update()                                          # the copy: the average is the model's weights
    xs = batches(3, seed=50)
    rng = np.random.default_rng(6)
    eps = [torch.from_numpy(rng.standard_normal((B, L)).astype(np.float32)).cuda() for _ in xs]
    # what each batch leaves in zeroed buffers, by hand (the model's own buffers put back afterwards)
    model.train()
    kept = (model._bnflat.clone(), model._nbt.clone())
    left = []
    with torch.no_grad():
        for x, e in zip(xs, eps):
            model._bnflat.zero_()
            model._run_forward(x, e, train=True, want_pre=False)
            left.append(host(model._bnflat).copy())
    model._bnflat.copy_(kept[0]); model._nbt.copy_(kept[1])
    model.eval()
    before = (bits(model._flat).copy(), bits(model._bnflat).copy(), host(model._nbt).copy(), bits(avg._params).copy())
    avg.update_bn([(x, None) for x in xs], eps=eps)
    assert not model.training and model._last is None
    now = (bits(model._flat), bits(model._bnflat), host(model._nbt), bits(avg._params))
    assert all(np.array_equal(a, b) for a, b in zip(now, before)), "update_bn changed the model or the averaged parameters"
    got = host(avg._buffers).astype(np.float64)
    stats = [R.recovered_bn_stat(v) for v in left]
    mean = np.mean(stats, axis=0)
    M = np.max(np.abs(stats), axis=0)
    err = np.abs(got - mean)
    print(f"update_bn {dtype}: largest error / M {np.max(err / np.maximum(M, 1e-300)):.3e}, bound {TOL_TORCH:.3e}")
    assert (err <= TOL_TORCH * M).all()
    assert np.abs(got - host(kept[0])).max() > 1e-3       # (they are not the buffers the model had)
    if dtype != "f32":
        return
    cpu = TorchCpuStep(p)
    want = np.zeros_like(mean)
    for x, e in zip(xs, eps):
        for k, v in cpu.bn.items():
            if not k.endswith("num_batches_tracked"):
                v.zero_()
        with torch.no_grad():
            cpu.forward(x.cpu(), e.cpu())
        for i, name in enumerate(_lib.BN_NAMES):
            c, o = model._bn_ch[i], model._bn_offs[i]
            want[o:o + c] += 10.0 * cpu.bn[name + ".running_mean"].double().numpy() / len(xs)
            want[o + c:o + 2 * c] += 10.0 * cpu.bn[name + ".running_var"].double().numpy() / len(xs)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
    # the loader may hand bare batches, and an empty one changes nothing
    avg.update_bn(xs, eps=eps)
    assert np.array_equal(bits(avg._buffers), got.astype(np.float32).view(np.uint32))
    avg.update_bn([])
    assert np.array_equal(bits(avg._buffers), got.astype(np.float32).view(np.uint32)) and np.array_equal(bits(model._bnflat), before[1])
