"""Attribute-regularised latents on the GPU (include/vae_attributes.h and its Python layer) against the numpy reference of
tests/attr_ref.py: the counters and the concordance sums for exact equality, the regulariser's f32 terms at the f32 layer-local gate,
the hook into the training step on the GPU's own tensors, and the stream contract of every entry point.  References are computed
once (functools caches) and shared."""
import functools
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests import attr_ref as R
from tests import stream_harness as sh
from tests import test_streams_gpu as streams
from tests.stream_harness import Bufs, Case
from tests.util import make_model, perturbed_params

pytestmark = pytest.mark.gpu

COUNTER_KEYS = list(R.counter_cases())       # (h, w, n): every shape x count
ID = {name: k for k, name in enumerate(R.NAMES)}


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from torch_vae_amd import _lib
    return _lib.lib()


def ok(rc, what="vae_attr"):
    assert rc == 0, (what, lib().vae_last_error().decode())


def host(t):
    return t.detach().cpu().numpy()


def i32(values):
    import ctypes
    return (ctypes.c_int32 * len(values))(*values)


# ---- 1. counters ------------------------------------------------------------------------------------------------------------------------
def run_counters(x, out=None, thr=R.THRESHOLD):
    n, h, w = x.shape
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if out is None:
        out = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    ok(lib().vae_attr_roll_counters(d.data_ptr(), n, h, w, thr, out.data_ptr(), st()))
    return out


@pytest.mark.parametrize("key", COUNTER_KEYS, ids=str)
def test_counters_equal_the_reference(key):
    h, w, n = key
    x, want = R.counter_cases()[key]
    got = host(run_counters(x))
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), f"first differences (roll, counter): {bad[:8].tolist()} got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"
    assert got.dtype == np.int32
    again = run_counters(x)
    assert sh.same_bits(again, torch.from_numpy(got).cuda())
    if w % 32 == 0:       # the first seven are columns 2..8 of the musical statistics of the same cells
        from torch_vae_amd.evaluation import music_statistics, roll_attributes
        from torch_vae_amd.generation import binarize_rolls
        xd = torch.from_numpy(x).cuda()
        feats = music_statistics(binarize_rolls(xd, R.THRESHOLD))["features"]
        assert np.array_equal(host(feats)[:, 2:9], got[:, :7])
        assert sh.same_bits(roll_attributes(xd[:, None], R.THRESHOLD), again)


@pytest.mark.parametrize("key", [(3, 65, 67), (128, 128, 3), (1, 1, 1), (1024, 64, 3)], ids=str)
def test_nothing_outside_the_counter_table_is_written(key):
    h, w, n = key
    x, want = R.counter_cases()[key]
    guard = 64
    buf = torch.full((guard + n * 8 + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    run_counters(x, out=buf[guard:guard + n * 8])
    got = host(buf)
    assert (got[:guard] == 0x5A5A5A5A).all() and (got[guard + n * 8:] == 0x5A5A5A5A).all()
    assert np.array_equal(got[guard:guard + n * 8].reshape(n, 8), want)


def test_no_rolls_and_another_threshold():
    x, want = R.counter_cases()[(13, 192, 3)]
    d = torch.from_numpy(x).cuda()
    out = torch.full((3, 8), -7, dtype=torch.int32, device="cuda")
    ok(lib().vae_attr_roll_counters(d.data_ptr(), 0, 13, 192, 0.5, out.data_ptr(), st()))
    assert (host(out) == -7).all()
    assert np.array_equal(host(run_counters(x, thr=0.75)), R.counters(x >= np.float32(0.75)))


# ---- 2. the regulariser -----------------------------------------------------------------------------------------------------------------
PAIR_SETS = {1: [("note_density", 0)], 3: [("mean_pitch", 0), ("note_density", 2), ("polyphony", 4)],
             8: [("note_density", 3), ("note_count", 0), ("pitch_range", 15), ("mean_pitch", 7), ("polyphony", 1), ("onset_steps", 8),
                 ("used_pitches", 2), ("note_density", 9)]}
SHAPES_LP = [(1, 1), (5, 1), (5, 3), (16, 1), (16, 3), (16, 8)]       # (L, pairs): every pair count that fits L
WEIGHT = 0.75
FLT_MIN = float(np.finfo(np.float32).tiny)


def run_regularizer(z, c, pairs, L, delta, weight, grad=True):
    """vae_attr_regularizer on numpy z [B, ldz] and counters -> (loss f64 [1 + K], g [B, L] or None) device tensors"""
    B, ldz = z.shape
    zd, cd = torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda()
    loss = torch.full((1 + len(pairs),), float("nan"), dtype=torch.float64, device="cuda")
    g = torch.full((B, L), float("nan"), device="cuda") if grad else None
    ok(lib().vae_attr_regularizer(zd.data_ptr(), ldz, L, cd.data_ptr(), B, len(pairs), i32([ID[n] for n, _ in pairs]), i32([d for _, d in pairs]),
                                  delta, weight, loss.data_ptr(), 0 if g is None else g.data_ptr(), st()))
    return loss, g


def check_regularizer(z, c, pairs, L, delta, tag):
    """The gates: loss relative error <= 1e-5, plus FLT_MIN absolute; per regularised column
    ||g - g_ref|| <= 1e-5 ||g_ref|| + 1e-7 (weight 2 delta / B) sqrt(B).  Returns (worst loss error, worst gradient error / gate).

    The FLT_MIN (1.18e-38, the smallest normal f32): the terms are formed in f32, and when every pair of a column is saturated in
    the right order (half of the B = 2 columns, many at delta = 100) the whole loss is a sum of 2 e^{-2|u|} that lies below what f32
    can hold with any relative precision, or at all (e^{-400}); the reference (f64, the saturated term formed without cancellation)
    is then 1e-100 where an f32 term can only be 0.  Everywhere above FLT_MIN the relative gate stands alone."""
    B = z.shape[0]
    want_loss, want_g = R.regularizer(z, c, pairs, delta, WEIGHT)
    loss, g = run_regularizer(z, c, pairs, L, delta, WEIGHT)
    loss_only, _ = run_regularizer(z, c, pairs, L, delta, WEIGHT, grad=False)
    loss2, g2 = run_regularizer(z, c, pairs, L, delta, WEIGHT)
    assert sh.same_bits(loss, loss2) and sh.same_bits(g, g2) and sh.same_bits(loss, loss_only), tag
    got_loss, got_g = host(loss), host(g).astype(np.float64)
    worst_l, worst_g = 0.0, 0.0
    for k in range(len(want_loss)):
        err = abs(got_loss[k] - want_loss[k])
        assert err <= 1e-5 * abs(want_loss[k]) + FLT_MIN, (tag, k, got_loss[k], want_loss[k])
        worst_l = max(worst_l, err / abs(want_loss[k]) if abs(want_loss[k]) > FLT_MIN else 0.0)
    named = [d for _, d in pairs]
    for d in range(L):
        if d not in named:
            assert not got_g[:, d].any() and not np.signbit(got_g[:, d]).any(), (tag, d)      # exactly +0
            continue
        err = np.linalg.norm(got_g[:, d] - want_g[:, d])
        gate = 1e-5 * np.linalg.norm(want_g[:, d]) + 1e-7 * (WEIGHT * 2 * delta / B) * math.sqrt(B)
        assert err <= gate, (tag, d, err, gate)
        worst_g = max(worst_g, err / gate)
    return worst_l, worst_g


# (the largest gaps measured on the MI355X are in the comment at the end of this section)
@pytest.mark.parametrize("delta", [1.0, 10.0, 100.0])
@pytest.mark.parametrize("B", [1, 2, 3, 64, 65, 257, 1024])
def test_regularizer_against_the_f64_reference(B, delta):
    worst = (0.0, 0.0)
    for L, npairs in SHAPES_LP:
        z, c = R.latent_case(B, L, seed=1000 + 16 * B + L)
        w = check_regularizer(z, c, PAIR_SETS[npairs], L, delta, f"B{B} L{L} pairs{npairs} delta{delta}")
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print(f"B{B} delta{delta}: worst loss relative error {worst[0]:.3g}, worst gradient error / gate {worst[1]:.3g}")


@pytest.mark.parametrize("kind", ["duplicate_rows", "all_tied"])
@pytest.mark.parametrize("B", [2, 65])
def test_regularizer_with_ties(B, kind):
    z, c = R.latent_case(B, 5, seed=7 + B, duplicates=kind == "duplicate_rows")
    if kind == "all_tied":
        c[:] = c[0]
    w = check_regularizer(z, c, PAIR_SETS[3], 5, 10.0, f"{kind} B{B}")
    print(f"{kind} B{B}: worst loss relative error {w[0]:.3g}, worst gradient error / gate {w[1]:.3g}")


# Measured on the MI355X (the lines the tests above print), worst over all cases:
#   loss      relative error 1.14e-07 (B = 2, delta = 1); below 6e-8 for B >= 3 and below 3e-9 for B >= 64; gate 1e-5
#   gradient  error / gate 0.018 (B = 2, delta = 1), 0.010 (B = 3, delta = 10), at most 0.0054 for B >= 64; with ties 0.0069
#   (duplicate rows at B = 2: loss and gradient exact.)


# ---- 3. the concordance sums --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def concordance_case(N, L, nattr):
    names = list(R.NAMES) if nattr == 7 else ["mean_pitch"]
    z, c = R.latent_case(N, L, seed=31 * N + L, duplicates=True)
    return z, c, names, R.concordance(z[:, :L], c, names)


def run_concordance(z, c, names, L):
    N, ldz = z.shape
    A = len(names)
    zd = torch.from_numpy(z).cuda() if N else torch.zeros(1, ldz, device="cuda")
    cd = torch.from_numpy(c).cuda() if N else torch.zeros(1, 8, dtype=torch.int32, device="cuda")
    S = torch.full((A, L), -7, dtype=torch.int64, device="cuda")
    tz, ta = torch.full((L,), -7, dtype=torch.int64, device="cuda"), torch.full((A,), -7, dtype=torch.int64, device="cuda")
    ok(lib().vae_attr_concordance(zd.data_ptr(), ldz, L, cd.data_ptr(), N, A, i32([ID[n] for n in names]), S.data_ptr(), tz.data_ptr(),
                                  ta.data_ptr(), st()))
    return S, tz, ta


@pytest.mark.parametrize("nattr", [1, 7])
@pytest.mark.parametrize("L", [1, 5, 16, 20])
@pytest.mark.parametrize("N", [0, 1, 2, 3, 67, 300, 1031])
def test_concordance_equals_the_reference(N, L, nattr):
    z, c, names, (S, tz, ta) = concordance_case(N, L, nattr)
    got = run_concordance(z, c, names, L)
    assert np.array_equal(host(got[0]), S) and np.array_equal(host(got[1]), tz) and np.array_equal(host(got[2]), ta)
    if N >= 3:
        assert tz.any() and ta.any() and (N < 67 or S.any())          # ties on both sides, and something to correlate
    again = run_concordance(z, c, names, L)
    assert all(sh.same_bits(a, b) for a, b in zip(got, again))
    if N and L in (5, 20):
        from torch_vae_amd.evaluation import attribute_correlation
        tau = attribute_correlation(torch.from_numpy(z[:, :L].copy()).cuda(), torch.from_numpy(c).cuda(), names).numpy()
        want = R.tau_b(S, tz, ta, N)
        assert tau.shape == (nattr, L) and np.array_equal(np.isnan(tau), np.isnan(want))
        assert np.all(np.abs(np.nan_to_num(tau) - np.nan_to_num(want)) <= 1e-12)


def test_attribute_correlation_of_no_points_and_of_a_monotone_dimension():
    from torch_vae_amd.evaluation import attribute_correlation
    z, c = R.latent_case(40, 3, seed=9, ld=3)
    z[:, 1] = R.attribute_values(c, ["note_density"])[:, 0].astype(np.float32)        # dimension 1 IS the attribute
    tau = attribute_correlation(torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda(), ["note_density", "polyphony"])
    assert tau[0, 1] == 1.0 and abs(tau[0, 0]) < 1.0
    none = attribute_correlation(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 8, dtype=torch.int32, device="cuda"), ["note_density"])
    assert none.shape == (1, 3) and bool(torch.isnan(none).all())


# ---- 4. the hook into the training step ---------------------------------------------------------------------------------------------------
REG = {"note_density": 1, "mean_pitch": 3, "polyphony": 0}
ATTR_W, ATTR_DELTA, BETA = 0.5, 10.0, 2.0


@functools.lru_cache(maxsize=None)
def step_inputs(H, L, B):
    gen = H != 32
    x = vo.synth_pianoroll(B, H, seed=40 + H)
    eps = vo.counter_normal(B * L, 41, 5).reshape(B, L).astype(np.float32)
    return gen, perturbed_params(L, H, 43, gen), x, eps


def attr_model(H, L, dtype, on=True):
    gen, p, _, _ = step_inputs(H, L, 8)
    m = make_model(H, L, gen, dtype, p, kld_weight=BETA)
    if on:
        m.attr_reg, m.attr_weight, m.attr_delta = dict(REG), ATTR_W, ATTR_DELTA
    return m


def dbg18(m, B, L):
    from torch_vae_amd import _lib
    t = torch.empty(B * 2 * L, device="cuda")
    _lib.check(_lib.lib().vae_debug_tensor(m._ctx.handle, 18, t.data_ptr(), B * 2 * L, st()), "vae_debug_tensor")
    return t.double().view(B, 2 * L)


@pytest.mark.parametrize("L", [4, 16])
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_the_hook_in_every_storage_type(dtype, H, L):
    from torch_vae_amd.attributes import attribute_regularizer, roll_attributes
    B = 8
    _, _, x, eps = step_inputs(H, L, B)
    xg, eg = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    off, on = attr_model(H, L, dtype, on=False), attr_model(H, L, dtype)
    out_off, _ = off.fused_forward_backward(xg, eps=eg)
    d_off, g_off = dbg18(off, B, L), off.flat_grads().clone()
    out_on, _ = on.fused_forward_backward(xg, eps=eg)
    d_on, g_on = dbg18(on, B, L), on.flat_grads().clone()
    last = on._last
    assert torch.equal(last["z"], off._last["z"]) and torch.equal(last["mu"], off._last["mu"])
    # what the hook must have added, from the GPU's own mu, log_var, z and the library's own regulariser on them
    loss, g_z = attribute_regularizer(last["z"], roll_attributes(xg, 0.5), [ID[n] for n in REG], list(REG.values()), ATTR_DELTA, ATTR_W)
    gmul = vo.f16_grad_scale(B, H) if dtype == "f16" else 1.0
    g64 = g_z.double()
    want = gmul * torch.cat([g64, g64 * eg.double() * torch.exp(0.5 * last["lv"].double()) * 0.5], dim=1)
    gap = float((d_on - d_off - want).norm() / d_on.norm())
    print(f"{dtype} {H}x{H} L{L}: latent-gradient gap {gap:.3g} of the on-tensor (|want| / |on| = {float(want.norm() / d_on.norm()):.3g})")
    assert float(want.norm()) > 0 and gap <= 1e-5, gap
    assert sh.same_bits(on.attribute_loss(), loss) and on.attribute_loss().dtype == torch.float64
    # the ELBO scalars
    o_on, o_off, l0 = out_on.tolist(), out_off.tolist(), float(loss[0])
    assert abs((o_on[0] - o_off[0]) - ATTR_W * l0) <= 4 * 2.0 ** -24 * max(abs(o_on[0]), abs(o_off[0]), ATTR_W * l0), (o_on, o_off, l0)
    assert sh.same_bits(out_on[1:], out_off[1:])
    assert bool(torch.isfinite(g_on).all())
    if dtype == "f32":     # the backward is linear in the upstream gradient: the difference of the steps is vae_backward of g_z alone
        from torch_vae_amd import _lib
        alone = attr_model(H, L, dtype, on=False)
        alone._run_forward(xg, eg, train=True, want_pre=False)
        buf = torch.full_like(alone._gflat, float("nan"))
        _lib.check(_lib.lib().vae_backward(alone._ctx.handle, alone._last["x"].data_ptr(), alone._flat.data_ptr(), buf.data_ptr(), 0, 0, 0, 0,
                                           g_z.data_ptr(), 0, BETA, 0, st()), "vae_backward")
        # (the conv biases in front of a train-mode BatchNorm have no gradient, tests/util.py PRE_BN_BIAS: the only tensors that may
        #  be left as they were, and 0 in both steps)
        from tests.util import PRE_BN_BIAS
        from torch_vae_amd._lib import PARAM_NAMES
        unwritten = [n for i, n in enumerate(PARAM_NAMES) if bool(torch.isnan(buf[alone._offs[i]:alone._offs[i] + alone._sizes[i]]).any())]
        assert set(unwritten) <= set(PRE_BN_BIAS), unwritten
        buf = torch.nan_to_num(buf, nan=0.0)
        gap = sh.rel_l2(g_on - g_off, buf)
        print(f"f32 {H}x{H} L{L}: flat-gradient difference against vae_backward(g_z) alone {gap:.3g}")
        assert gap <= 1e-5, gap


def test_two_part_backward_takes_the_same_g_z():
    H, L, B = 32, 16, 8
    _, _, x, eps = step_inputs(H, L, B)
    xg, eg = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    whole, parts = attr_model(H, L, "f32"), attr_model(H, L, "f32")
    out_w, _ = whole.fused_forward_backward(xg, eps=eg)
    seen = []
    out_p, _ = parts.fused_forward_backward(xg, eps=eg, on_decoder_grads=lambda: seen.append(1))
    assert seen == [1] and sh.same_bits(dbg18(whole, B, L), dbg18(parts, B, L))
    assert sh.rel_l2(parts.flat_grads(), whole.flat_grads()) <= 1e-6 and sh.same_bits(out_w, out_p)


def test_autograd_path_equals_the_fused_path():
    """forward -> loss -> backward against fused_forward_backward, at the gate of tests/test_parity_gpu.py's
    test_autograd_path_matches_fused_path (scalars rtol 1e-6; every parameter gradient rtol 1e-5, atol 1e-8)."""
    H, L, B = 32, 16, 8
    _, _, x, eps = step_inputs(H, L, B)
    xg, eg = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    m1, m2 = attr_model(H, L, "f32"), attr_model(H, L, "f32")
    out3, _ = m1.fused_forward_backward(xg, eps=eg)
    m2.set_next_eps(eg)
    out = m2.forward(xg)
    lo = m2.loss(out)
    assert lo["loss"].requires_grad
    lo["loss"].backward()
    np.testing.assert_allclose([lo["loss"].item(), lo["reconstruction_loss"].item(), lo["kld_loss"].item()], out3.tolist(), rtol=1e-6)
    assert sh.same_bits(m1.attribute_loss(), m2.attribute_loss())
    for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert b.grad is not None, n
        np.testing.assert_allclose(b.grad.cpu().numpy(), a.grad.cpu().numpy(), rtol=1e-5, atol=1e-8, err_msg=n)
    plain = attr_model(H, L, "f32", on=False)
    plain.set_next_eps(eg)
    assert abs(plain.loss(plain.forward(xg))["loss"].item() + ATTR_W * float(m2.attribute_loss()[0]) - lo["loss"].item()) <= 1e-6 * abs(lo["loss"].item())


def test_fused_step_takes_the_one_call_path_only_without_attr_reg():
    from torch_vae_amd.optim import FusedAdamW
    from torch_vae_amd.train import fused_step
    H, L, B = 32, 16, 8
    _, _, x, eps = step_inputs(H, L, B)
    xg, eg = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    for on in (False, True):
        m = attr_model(H, L, "bf16", on=on)
        opt = FusedAdamW([{"params": list(m.encoder.parameters())}, {"params": list(m.decoder.parameters())}], lr=1e-3, weight_decay=0.0)
        calls = {"one": 0, "split": 0}
        one, split = m.fused_train_step, m.fused_forward_backward

        def count_one(*a, _f=one, **k):
            calls["one"] += 1
            return _f(*a, **k)

        def count_split(*a, _f=split, **k):
            calls["split"] += 1
            return _f(*a, **k)
        m.fused_train_step, m.fused_forward_backward = count_one, count_split
        before = m.flat_parameters().clone()
        out3, _ = fused_step(m, opt, xg, eps=eg)
        assert calls == ({"one": 0, "split": 1} if on else {"one": 1, "split": 0}), (on, calls)
        assert bool(torch.isfinite(out3).all()) and not torch.equal(before, m.flat_parameters())      # the optimiser stepped
        if on:
            assert bool(torch.isfinite(m.attribute_loss()).all())
        else:
            with pytest.raises(RuntimeError, match="attr_reg"):
                m.attribute_loss()


def test_a_bad_value_raises_when_the_step_reads_it():
    H, L, B = 32, 16, 8
    _, _, x, eps = step_inputs(H, L, B)
    m = attr_model(H, L, "bf16")
    m.attr_reg = {"note_density": 16}
    with pytest.raises(ValueError, match="latent dimension"):
        m.fused_forward_backward(torch.from_numpy(x).cuda())
    m.attr_reg = {"loudness": 0}
    with pytest.raises(ValueError, match="unknown attribute"):
        m.loss(m.forward(torch.from_numpy(x).cuda()))


def test_loss_on_foreign_tensors_with_and_without_latents():
    """loss() on a plain dict that is not the model's forward: without attr_reg it never looks for 'latents' (the callers of before
    pass none); with attr_reg it takes the term from the given latents and refuses a dict that has none."""
    H, L, B = 32, 16, 8
    _, _, x, eps = step_inputs(H, L, B)
    xg, eg = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    m = attr_model(H, L, "f32", on=False)
    m.set_next_eps(eg)
    out = m.forward(xg)
    foreign = {"output": out["output"] * 1.0, "input": xg, "encoded": {"mu": out["encoded"]["mu"] * 1.0, "log_var": out["encoded"]["log_var"] * 1.0}}
    plain = m.loss(foreign)["loss"]
    assert bool(torch.isfinite(plain))
    m.attr_reg, m.attr_weight, m.attr_delta = dict(REG), ATTR_W, ATTR_DELTA
    with pytest.raises(ValueError, match="latents"):
        m.loss(foreign)
    z = (out["latents"] * 1.0).detach().requires_grad_(True)
    lo = m.loss({**foreign, "latents": z})["loss"]
    want = ATTR_W * float(m.attribute_loss()[0])
    assert abs(lo.item() - plain.item() - want) <= 1e-6 * abs(lo.item())
    lo.backward()
    _, g = run_regularizer(host(z), host(roll_counters_of(xg)), list(REG.items()), L, ATTR_DELTA, ATTR_W)
    assert sh.same_bits(z.grad, g)


def roll_counters_of(xg):
    from torch_vae_amd.evaluation import roll_attributes
    return roll_attributes(xg, 0.5)


# ---- 5. the Python surface --------------------------------------------------------------------------------------------------------------
def test_traverse():
    from torch_vae_amd.evaluation import roll_attributes
    from torch_vae_amd.generation import traverse
    m = attr_model(32, 16, "f32", on=False)
    z = torch.from_numpy(vo.counter_normal(3 * 16, 5, 5).reshape(3, 16)).float().cuda()
    values = [-2.0, 0.0, 0.5, 2.0, 3.0]
    was_training = m.training
    rolls, counters = traverse(m, z, 4, values)
    assert rolls.shape == (3, 5, 1, 32, 32) and counters.shape == (3, 5, 8) and counters.dtype == torch.int32
    assert rolls.is_cuda and counters.is_cuda and m.training == was_training
    assert sh.same_bits(counters.reshape(15, 8), roll_attributes(rolls.reshape(15, 1, 32, 32), 0.5))
    zz = z.clone()
    zz[:, 4] = 0.5
    assert sh.same_bits(rolls[:, 2], m._run_decode(zz, train=False))
    low, _ = traverse(m, z, 4, torch.tensor(values), threshold=0.0)
    assert sh.same_bits(low, rolls) and int(traverse(m, z, 4, values, threshold=0.0)[1][0, 0, 0]) == 32 * 32
    with pytest.raises(ValueError, match="latent dimension"):
        traverse(m, z, 16, values)
    with pytest.raises(ValueError, match="at least one"):
        traverse(m, z, 0, [])


def tiny_loader(n=40, batch=16, seed=23):
    from torch_vae_amd.data import DevicePianorollLoader, PianorollDataset
    rng = np.random.default_rng(seed)
    cells = np.stack([R.random_runs(rng, 32, 32, (0.02, 0.1, 0.3)[r % 3]) for r in range(n)])
    ds = PianorollDataset(torch.from_numpy(cells.astype(np.float32)), storage="bits")
    return cells, DevicePianorollLoader(ds, batch, train=False)


@pytest.mark.parametrize("with_reg", [False, True])
def test_evaluate_with_attributes(with_reg):
    from torch_vae_amd.evaluation import attribute_correlation, evaluate
    cells, loader = tiny_loader()
    m = attr_model(32, 16, "f32", on=with_reg)

    def run(**kw):
        torch.manual_seed(3)          # the eval forward draws eps from torch's device generator
        return evaluate(loader, m, "cuda", verbosity=0, **kw)

    plain, with_attr = run(), run(attributes=True)
    names = list(REG) if with_reg else list(R.NAMES)
    assert [k for k in with_attr if k not in plain] == [f"attr_tau_{n}" for n in names] and list(with_attr)[:len(plain)] == list(plain)
    assert {k: with_attr[k] for k in plain} == plain
    with torch.no_grad():
        mu = torch.cat([m.encode(x.float())["mu"] for x, _ in loader])
    counters = torch.from_numpy(R.counters(cells)).cuda()
    tau = attribute_correlation(mu.float().contiguous(), counters, names).numpy()
    for k, name in enumerate(names):
        got = with_attr[f"attr_tau_{name}"]
        want = tau[k, REG[name]] if with_reg else tau[k, int(np.nanargmax(np.abs(tau[k])))]
        assert abs(got - want) <= 1e-12 and -1.0 <= got <= 1.0, (name, got, want)
    ref = R.tau_b(*R.concordance(host(mu), R.counters(cells), names), len(cells))
    assert np.allclose(tau, ref, rtol=0, atol=1e-12, equal_nan=True)


def test_train_one_epoch_reads_the_config():
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    H, L, B = 32, 16, 8
    gen, p, _, _ = step_inputs(H, L, B)
    m = make_model(H, L, gen, "bf16", p)
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                    epochs=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0,
                    attr_reg={"note_density": 0, "pitch_range": 5}, attr_weight=2.0, attr_delta=5.0)
    opt, sched = build_optimizer(cfg, m, steps_per_epoch=10)
    loader = [(torch.from_numpy(vo.synth_pianoroll(B, H, seed=80 + s)), torch.zeros(B, dtype=torch.long)) for s in range(2)]
    res, total_step, _ = train_one_epoch(cfg, m, opt, sched, m.loss, loader, device="cuda", epoch=1)
    assert total_step == 2 and math.isfinite(res["loss"])
    assert (m.attr_reg, m.attr_weight, m.attr_delta) == ({"note_density": 0, "pitch_range": 5}, 2.0, 5.0)
    al = m.attribute_loss()
    assert al.shape == (3,) and al.dtype == torch.float64 and al.is_cuda and bool(torch.isfinite(al).all())
    assert 0.0 < float(al[1]) < 2.0 and abs(float(al[0]) - float(al[1]) - float(al[2])) <= 1e-15
    assert bool(torch.isfinite(m.flat_parameters()).all())


# ---- 6. the stream contract (include/vae_step.h, first paragraph) on the new entry points -------------------------------------------------
SKEY = (13, 192, 67)
S_N, S_L, S_LD = 300, 5, 8
S_PAIRS = PAIR_SETS[3]


def _make_counters():
    x, _ = R.counter_cases()[SKEY]
    b = Bufs()
    b.inp("rolls", torch.from_numpy(x))
    b.outp("counters", 67, 8, dtype=torch.int32)
    return b


def _counters(b):
    ok(lib().vae_attr_roll_counters(b["rolls"].data_ptr(), 67, 13, 192, 0.5, b["counters"].data_ptr(), st()))


def _make_latents():
    z, c = R.latent_case(S_N, S_L, seed=77, ld=S_LD)
    b = Bufs()
    b.inp("z", torch.from_numpy(np.nan_to_num(z)))        # (the poison is NaN: the true padding columns are zeros here)
    b.inp("counters", torch.from_numpy(c), poison=0)
    b.outp("loss", 1 + len(S_PAIRS), dtype=torch.float64)
    b.outp("g_z", S_N, S_L)
    b.outp("loss_only", 1 + len(S_PAIRS), dtype=torch.float64)
    b.outp("S", 7, S_L, dtype=torch.int64)
    b.outp("ties_z", S_L, dtype=torch.int64)
    b.outp("ties_a", 7, dtype=torch.int64)
    return b


def _regularizer(b):
    attr, dim = i32([ID[n] for n, _ in S_PAIRS]), i32([d for _, d in S_PAIRS])
    ok(lib().vae_attr_regularizer(b["z"].data_ptr(), S_LD, S_L, b["counters"].data_ptr(), S_N, len(S_PAIRS), attr, dim, 10.0, 0.5,
                                  b["loss"].data_ptr(), b["g_z"].data_ptr(), st()))
    ok(lib().vae_attr_regularizer(b["z"].data_ptr(), S_LD, S_L, b["counters"].data_ptr(), S_N, len(S_PAIRS), attr, dim, 10.0, 0.5,
                                  b["loss_only"].data_ptr(), 0, st()))


def _concordance(b):
    ok(lib().vae_attr_concordance(b["z"].data_ptr(), S_LD, S_L, b["counters"].data_ptr(), S_N, 7, i32(list(range(7))), b["S"].data_ptr(),
                                  b["ties_z"].data_ptr(), b["ties_a"].data_ptr(), st()))


STREAM_CASES = [
    Case("attr_roll_counters", ("vae_attr_roll_counters",), _make_counters, _counters),
    Case("attr_regularizer", ("vae_attr_regularizer",), _make_latents, _regularizer),
    Case("attr_concordance", ("vae_attr_concordance",), _make_latents, _concordance),
]


def _make_python():
    x, _ = R.counter_cases()[SKEY]
    z, _ = R.latent_case(67, S_L, seed=78, ld=S_L)
    b = Bufs()
    b.inp("rolls", torch.from_numpy(x))
    b.inp("z", torch.from_numpy(z))
    return b


def _python(b):
    from torch_vae_amd.attributes import attribute_regularizer
    from torch_vae_amd.evaluation import attribute_values, roll_attributes
    c = roll_attributes(b["rolls"], 0.5)
    b.out["counters"] = c
    b.out["values"] = attribute_values(c, R.NAMES)
    b.out["loss"], b.out["g_z"] = attribute_regularizer(b["z"], c, [ID[n] for n, _ in S_PAIRS], [d for _, d in S_PAIRS], 10.0, 0.5)


def _make_step():
    b = streams._py_model("bf16")
    b.keep[0].attr_reg, b.keep[0].attr_weight = {"note_density": 0, "mean_pitch": 2}, 0.5
    return b


def _step(b):
    from torch_vae_amd.train import fused_step
    m, opt = b.keep[0], b.keep[1]
    for i in range(2):
        out3, xhat = fused_step(m, opt, b["x"], eps=b["eps"])
        b.out[f"out3_{i}"] = out3.clone()
        b.out[f"attr_loss_{i}"] = m.attribute_loss().clone()
    b.out["xhat"] = xhat


def _traverse(b):
    from torch_vae_amd.generation import traverse
    b.out["rolls"], b.out["traverse_counters"] = traverse(b.keep[0], b["eps"][:2], 0, [-1.0, 1.0])


def _correlation(b):
    from torch_vae_amd.evaluation import attribute_correlation, roll_attributes
    c = roll_attributes(b["rolls"], 0.5)
    b.out["tau"] = attribute_correlation(b["z"], c, R.NAMES).cuda()


PY_STREAM_CASES = [
    Case("python/roll_attributes+attribute_regularizer", ("vae_attr_roll_counters", "vae_attr_regularizer"), _make_python, _python, warmups=2),
    Case("python/fused_step with attr_reg", ("vae_attr_roll_counters", "vae_attr_regularizer"), _make_step, _step, dtype="bf16",
         reset=streams._py_reset, warmups=2),
    Case("python/traverse", ("vae_attr_roll_counters",), _make_step, _traverse, dtype="bf16", reset=streams._py_reset, warmups=2),
    Case("python/attribute_correlation", ("vae_attr_concordance",), _make_python, _correlation, sync_free=False,
         reads_back="attribute_correlation reads the sums and tie counts back once"),
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_stream_contract(case):
    sh.check_case(case)
    if case.name == "attr_concordance":      # and what it computed is right
        b = case.make()
        sh.stage(b)
        case.run(b)
        z, c = R.latent_case(S_N, S_L, seed=77, ld=S_LD)
        S, tz, ta = R.concordance(z[:, :S_L], c, list(R.NAMES))
        assert np.array_equal(host(b["S"]), S) and np.array_equal(host(b["ties_z"]), tz) and np.array_equal(host(b["ties_a"]), ta)


@pytest.mark.parametrize("case", PY_STREAM_CASES, ids=repr)
def test_stream_contract_python_layer(case):
    sh.check_case(case)
