"""Denoising and infilling on the GPU: the corruption kernel (include/vae_denoise.h) bit for bit against the numpy reference of
tests/denoise_ref.py, the separate reconstruction target (vae_set_recon_target) on every step path against torch CPU f64 autograd
and the storage-emulating oracle, the Python layer on top, and the stream contract of the new entry points.  References are
computed once (functools caches) and shared."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from oracle.torch_cpu_step import TorchCpuStep
from tests import denoise_ref as R
from tests import stream_harness as sh
from tests import test_streams_gpu as streams
from tests.stream_harness import Bufs, Case
from tests.test_pos_weight_host import wbce_reference
from tests.test_recon_loss_gpu import _dbg, velocity_roll
from tests.util import PRE_BN_BIAS, flat_grad_dict, make_model, perturbed_params, rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(4, 128, 128), (3, 32, 32), (2, 5, 8), (1, 1, 200), (2, 128, 192)]      # (n, h, w): 200 and 8 are no multiple of 64
GRAD_TOL_F32 = 5e-3          # tests/test_parity_gpu.py GRAD_TOL["f32"] (LeakyReLU kink ties)
LAYER_TOL = 5e-4             # the layer-local gate of tests/test_parity_gpu.py
GUARD = 64
U64 = (1 << 64) - 1


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from torch_vae_amd import _lib
    return _lib.lib()


def ok(rc, what="vae_denoise"):
    assert rc == 0, (what, lib().vae_last_error().decode())


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the corruption kernel ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_roll_case():
    """The random roll of the issue: (clean, reference out, reference hidden, the reference's counts)."""
    x = np.ascontiguousarray(vo.synth_pianoroll(4, 128, 7)[:, 0], dtype=np.float32)
    info = {}
    out, hidden = R.corrupt_ref(x, p_drop=0.3, span=(16, 32), p_add=0.01, seed=11, counter0=5, counter_stride=3, info=info)
    return x, out, hidden, info


@functools.lru_cache(maxsize=None)
def roll(n, h, w, kind):
    """0/1 rolls or velocity rolls with runs of every length, runs across every multiple of 64, runs at both ends of a row, single
    cells one apart; the velocity kind also has cells exactly at the threshold, just below it, and NaNs."""
    rng = np.random.default_rng(1000 * n + 10 * h + w + (kind == "velocity"))
    on = rng.random((n, h, w)) < 0.25
    for b in range(n):
        for p in range(h):
            for _ in range(int(rng.integers(0, 3))):
                t0 = int(rng.integers(0, w)); on[b, p, t0:t0 + int(rng.integers(2, 40))] = True
            if w > 64 and p % 3 == 0:
                c = 64 * int(rng.integers(1, (w + 63) // 64)); on[b, p, max(c - int(rng.integers(1, 9)), 0):c + int(rng.integers(1, 9))] = True
        if h > 1:
            on[b, 0, :] = True
        if h > 2:
            on[b, 1, :3] = True; on[b, 1, w - 3:] = True; on[b, 2, :] = False
    x = on.astype(np.float32)
    if kind == "velocity":
        x = (x * rng.uniform(0.5, 1.0, x.shape)).astype(np.float32) + (~on * rng.uniform(0.0, 0.49, x.shape)).astype(np.float32)
        flat = x.reshape(-1)
        flat[::13] = 0.5; flat[5::29] = np.nextafter(np.float32(0.5), np.float32(0)); flat[7::31] = np.nan
    return np.ascontiguousarray(x)


def run_corrupt(x, *, threshold=0.5, p_drop=0.0, span=None, p_add=0.0, add_value=1.0, spans=None, seed=0, counter0=0, counter_stride=1,
                want_hidden=True):
    """vae_denoise_corrupt on numpy rolls, out and hidden inside guard bands -> (out, hidden) numpy; the bands are checked here."""
    n, h, w = x.shape
    d = torch.from_numpy(x).cuda()
    obuf = torch.full((GUARD + n * h * w + GUARD,), -7.5, device="cuda")
    hbuf = torch.full((GUARD + n * h * (w // 8) + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    o, hd = obuf[GUARD:GUARD + n * h * w], hbuf[GUARD:GUARD + n * h * (w // 8)]
    sp = None if spans is None else torch.tensor(np.asarray(spans, dtype=np.int64).reshape(n, 2), dtype=torch.int64).to(torch.int32).cuda()
    smin, smax = (0, 0) if span is None else span
    ok(lib().vae_denoise_corrupt(d.data_ptr(), o.data_ptr(), hd.data_ptr() if want_hidden else 0, n, h, w, threshold, p_drop, smin, smax, p_add,
                                 add_value, 0 if sp is None else sp.data_ptr(), seed & U64, counter0 & U64, counter_stride & U64, st()))
    og, hg = host(obuf), host(hbuf)
    assert (og[:GUARD] == -7.5).all() and (og[GUARD + n * h * w:] == -7.5).all(), "a float outside out was written"
    assert (hg[:GUARD] == 0xC3).all() and (hg[GUARD + n * h * (w // 8):] == 0xC3).all(), "a byte outside hidden was written"
    assert np.array_equal(bits(host(d)), bits(x)), "clean was written"
    if not want_hidden:
        assert (hg == 0xC3).all()
    return og[GUARD:GUARD + n * h * w].reshape(n, h, w), hg[GUARD:GUARD + n * h * (w // 8)].reshape(n, h, w // 8)


def assert_same(got, want, what):
    go, gh = got
    wo, wh = want
    bad = np.argwhere(bits(go) != bits(wo))
    assert bad.size == 0, f"{what}: out differs at (roll, row, column) {bad[:6].tolist()}: got {go[tuple(bad[0])]} want {wo[tuple(bad[0])]}"
    bad = np.argwhere(gh != wh)
    assert bad.size == 0, f"{what}: hidden differs at (roll, row, byte) {bad[:6].tolist()}: got {gh[tuple(bad[0])]:08b} want {wh[tuple(bad[0])]:08b}"


def test_the_random_roll_bit_for_bit():
    from torch_vae_amd.denoise import corrupt_rolls
    x, want_out, want_hidden, info = random_roll_case()
    assert info["crossing_dropped"] >= 1 and info["crossing_kept"] >= 1 and info["added"] >= 1      # (on the reference: the test has a subject)
    kw = dict(p_drop=0.3, span=(16, 32), p_add=0.01, seed=11, counter0=5, counter_stride=3)
    got = run_corrupt(x, **kw)
    assert_same(got, (want_out, want_hidden), "random roll")
    assert_same(run_corrupt(x, **kw), got, "second call")
    no_mask, _ = run_corrupt(x, want_hidden=False, **kw)
    assert np.array_equal(bits(no_mask), bits(want_out))
    xd = torch.from_numpy(x).cuda()
    o, hd = corrupt_rolls(xd[:, None], note_dropout=0.3, span=(16, 32), add_noise=0.01, seed=11, counter0=5, counter_stride=3, return_hidden=True)
    assert o.shape == (4, 1, 128, 128) and hd.shape == (4, 1, 128, 16) and hd.dtype == torch.uint8
    assert_same((host(o)[:, 0], host(hd)[:, 0]), (want_out, want_hidden), "corrupt_rolls")
    assert sh.same_bits(corrupt_rolls(xd, note_dropout=0.3, span=(16, 32), add_noise=0.01, seed=11, counter0=5, counter_stride=3), o[:, 0])


MODES = {"drop": dict(p_drop=0.4), "span": dict(span="draw"), "add": dict(p_add=0.05, add_value=0.75), "all": dict(p_drop=0.3, span="draw", p_add=0.02)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["binary", "velocity"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_corruption_against_the_reference(shape, kind, mode):
    n, h, w = shape
    x = roll(n, h, w, kind)
    kw = dict(MODES[mode], seed=21 + h, counter0=7, counter_stride=5)
    if kw.get("span") == "draw":
        kw["span"] = (max(1, w // 8), max(1, w // 4))
    info = {}
    want = R.corrupt_ref(x, info=info, **kw)
    if "p_drop" in kw and n * h > 4:
        assert info["dropped"] >= 1 and info["kept"] >= 1
        if w > 64:
            assert info["crossing_dropped"] >= 1 and info["crossing_kept"] >= 1, info
    assert_same(run_corrupt(x, **kw), want, f"{shape} {kind} {mode}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_all_off_is_a_copy_and_probability_one_is_everything(shape):
    n, h, w = shape
    x = roll(n, h, w, "velocity")
    out, hidden = run_corrupt(x, seed=5)
    assert np.array_equal(bits(out), bits(x)) and not hidden.any()
    assert_same(run_corrupt(x, p_drop=1.0, p_add=1.0, add_value=2.0, seed=5), R.corrupt_ref(x, p_drop=1.0, p_add=1.0, add_value=2.0, seed=5), "p = 1")
    # a threshold below every cell: one note per row, and a dropped cell is 0.f, which is still on - nothing hidden by the drop
    lo = np.nan_to_num(x, nan=0.25)
    assert_same(run_corrupt(lo, threshold=-1.0, p_drop=0.5, seed=6), R.corrupt_ref(lo, threshold=-1.0, p_drop=0.5, seed=6), "threshold -1")


def run_params(n, w, smin, smax, seed, counter0=0, counter_stride=1):
    buf = torch.full((GUARD + 2 * n + GUARD,), -77, dtype=torch.int32, device="cuda")
    ok(lib().vae_denoise_params(buf[GUARD:].data_ptr(), n, w, smin, smax, seed & U64, counter0 & U64, counter_stride & U64, st()))
    g = host(buf)
    assert (g[:GUARD] == -77).all() and (g[GUARD + 2 * n:] == -77).all()
    return g[GUARD:GUARD + 2 * n].reshape(n, 2)


@pytest.mark.parametrize("n,w,smin,smax", [(300, 128, 16, 32), (5, 8, 0, 8), (67, 200, 200, 200), (4, 192, 0, 0), (1, 32, 1, 1)])
def test_params_equal_the_reference_draws(n, w, smin, smax):
    for c0, cs in ((0, 1), (U64 - 10, 3), (1 << 63, (1 << 63) + 1)):
        want = R.spans_ref(n, w, smin, smax, 9, c0, cs)
        assert np.array_equal(run_params(n, w, smin, smax, 9, c0, cs), want), (c0, cs)
    assert (want[:, 0] >= 0).all() and (want[:, 0] + want[:, 1] <= w).all()


def test_given_spans_at_both_ends_and_out_of_range():
    n, h, w = 8, 5, 192
    x = roll(8, 5, 192, "velocity")
    big = (1 << 31) - 1
    spans = [[0, 17], [w - 9, 9], [-5, 10], [w - 3, 100], [500, 4], [-big - 1, big], [big, big], [3, -2]]
    want = R.corrupt_ref(x, spans=spans, p_drop=0.2, p_add=0.02, seed=4)
    assert_same(run_corrupt(x, spans=spans, p_drop=0.2, p_add=0.02, seed=4), want, "given spans")          # (guard bands: run_corrupt)
    hid = np.unpackbits(want[1], axis=-1).astype(bool)
    assert hid[0, :, :17].all() and hid[1, :, w - 9:].all() and hid[2, :, :5].all() and hid[3, :, w - 3:].all()
    # given spans replace the draw whatever span_min / span_max say, and the drawn ones given back are the drawn corruption
    drawn = run_params(n, w, 8, 40, 4)
    a = run_corrupt(x, span=(8, 40), seed=4)
    assert_same(run_corrupt(x, span=(0, 0), spans=drawn, seed=4), a, "drawn spans handed back")
    assert_same(run_corrupt(x, span=(1, 2), spans=drawn, seed=4), a, "span_min / span_max beside given spans")
    for s in (0, w):           # whole-roll and empty spans
        assert_same(run_corrupt(x, spans=[[0, s]] * n, seed=4), R.corrupt_ref(x, spans=[[0, s]] * n, seed=4), f"span of {s}")


def test_counters_wrap_as_the_reference_does():
    x = roll(3, 32, 32, "binary")
    for c0, cs in ((U64, 1), (U64 - 1, 1 << 63), ((1 << 64) // 32 // 32 - 1, 1), (12345678901234567890, 9876543210987654321)):
        kw = dict(p_drop=0.4, span=(4, 8), p_add=0.03, seed=(1 << 64) - 2, counter0=c0, counter_stride=cs)
        assert_same(run_corrupt(x, **kw), R.corrupt_ref(x, **kw), f"counter0 {c0} stride {cs}")
    # a stride of 0 gives every roll the same counter - the same draws on equal rolls - and a stride of 1 does not
    same = np.stack([x[0]] * 3)
    out, _ = run_corrupt(same, p_drop=0.4, p_add=0.03, seed=3, counter0=9, counter_stride=0)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2]) and not np.array_equal(out[0], same[0])
    out, _ = run_corrupt(same, p_drop=0.4, p_add=0.03, seed=3, counter0=9, counter_stride=1)
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])


def test_no_rolls_launch_nothing():
    o = torch.full((16,), -7.5, device="cuda")
    ok(lib().vae_denoise_corrupt(o.data_ptr(), o.data_ptr() + 32, 0, 0, 1, 8, 0.5, 0.5, 0, 0, 0.5, 1.0, 0, 1, 0, 1, st()))
    s = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    ok(lib().vae_denoise_params(s.data_ptr(), 0, 32, 2, 4, 1, 0, 1, st()))
    assert (host(o) == -7.5).all() and (host(s) == -77).all()
    from torch_vae_amd.denoise import corrupt_rolls, corruption_spans
    out, hid = corrupt_rolls(torch.empty(0, 4, 32, device="cuda"), note_dropout=0.5, return_hidden=True)
    assert out.shape == (0, 4, 32) and hid.shape == (0, 4, 4) and corruption_spans(0, 32, (2, 4)).shape == (0, 2)
    got = corruption_spans(50, 128, (16, 32), seed=3, counter0=U64 - 20, counter_stride=7)
    assert got.dtype == torch.int32 and np.array_equal(host(got), R.spans_ref(50, 128, 16, 32, 3, U64 - 20, 7))


# ---- 2. the separate reconstruction target ----------------------------------------------------------------------------------------------
def eps_of(B, L, seed):
    return vo.counter_normal(B * L, seed, 5).reshape(B, L).astype(np.float32)


@functools.lru_cache(maxsize=None)
def denoise_inputs(B, H, L, seed, velocity=False):
    """(clean [B,1,H,H], corrupt_ref(clean), eps) float32"""
    clean = velocity_roll(B, H, seed) if velocity else vo.synth_pianoroll(B, H, seed).astype(np.float32)
    cor, _ = R.corrupt_ref(clean[:, 0], p_drop=0.3, span=(H // 8, H // 4), p_add=0.01, seed=seed, counter0=3)
    assert not np.array_equal(cor, clean[:, 0])
    return clean, np.ascontiguousarray(cor[:, None]), eps_of(B, L, seed)


def cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def model_of(H, L, gen, dtype, p, recon="bce", w=None, kld_weight=1.0):
    m = make_model(H, L, gen, dtype, p, kld_weight=kld_weight)
    if recon == "mse":
        m.recon_loss = "mse"
    if w is not None:
        m.pos_weight = w
    return m


def adamw(m):
    from torch_vae_amd.optim import FusedAdamW
    return FusedAdamW([{"params": list(m.encoder.parameters())}, {"params": list(m.decoder.parameters())}], lr=1e-3, weight_decay=0.0)


def set_target(m, B, ptr):
    from torch_vae_amd import _lib
    _lib.check(_lib.lib().vae_set_recon_target(m._context(B).handle, ptr), "vae_set_recon_target")


def one_step(m, path, x, eps, target=None):
    """(out3, xhat, flat gradients, parameters after the step) of one step on `path`"""
    if path == "fused_train_step":
        out3, xhat = m.fused_train_step(adamw(m), x, eps=eps, target=target)
    else:
        out3, xhat = m.fused_forward_backward(x, eps=eps, target=target)
    return out3.clone(), xhat.clone(), m.flat_grads().clone(), m.flat_parameters().clone()


@pytest.mark.parametrize("path", ["fused_forward_backward", "fused_train_step"])
@pytest.mark.parametrize("dtype,H", [("f32", 32), ("bf16", 128), ("f16", 128)])
def test_off_is_off(dtype, H, path):
    """No target, target = a copy of x, and a pending target cleared with NULL: the same bits everywhere."""
    L, B, gen = 16, 4, H != 32
    p = perturbed_params(L, H, 31, gen)
    x, eps = cuda(vo.synth_pianoroll(B, H, 32).astype(np.float32), eps_of(B, L, 33))
    plain = one_step(model_of(H, L, gen, dtype, p), path, x, eps)
    copy = one_step(model_of(H, L, gen, dtype, p), path, x, eps, target=x.clone())
    m = model_of(H, L, gen, dtype, p)
    other = torch.rand_like(x)
    set_target(m, B, other.data_ptr())
    set_target(m, B, 0)
    cleared = one_step(m, path, x, eps)
    for name, got in (("target = x.clone()", copy), ("cleared with NULL", cleared)):
        for what, a, b in zip(("out3", "xhat", "gradients", "parameters"), got, plain):
            assert sh.same_bits(a, b), (name, what)
    assert not sh.same_bits(one_step(model_of(H, L, gen, dtype, p), path, x, eps, target=other)[0], plain[0])


@pytest.mark.parametrize("dtype,H", [("f32", 32), ("bf16", 128)])
def test_the_target_is_one_shot(dtype, H):
    L, B, gen = 16, 4, H != 32
    p = perturbed_params(L, H, 34, gen)
    clean, cor, eps = cuda(*denoise_inputs(B, H, L, 35))
    plain = one_step(model_of(H, L, gen, dtype, p), "fused_forward_backward", cor, eps)
    m = model_of(H, L, gen, dtype, p)
    with_target = one_step(m, "fused_forward_backward", cor, eps, target=clean)
    assert not sh.same_bits(with_target[0], plain[0])
    after = one_step(m, "fused_forward_backward", cor, eps)
    for what, a, b in zip(("out3", "xhat", "gradients"), after, plain):
        assert sh.same_bits(a, b), what
    # a target set before encode / decode / log_likelihood is consumed there and changes nothing, there or in the step after
    # (both calls on the same model: in train mode they move the running statistics, which none of these outputs reads back)
    z = torch.from_numpy(eps_of(B, L, 36)).cuda()
    calls = {"encode": lambda mm: mm.encode(cor)["mu"], "decode": lambda mm: mm.decode(z),
             "log_likelihood": lambda mm: mm.log_likelihood(cor, 2, seed=5)["log_likelihood"]}
    for name, call in calls.items():
        with torch.no_grad():
            want = call(m).clone()
            set_target(m, B, clean.data_ptr())
            got = call(m).clone()
        assert sh.same_bits(got, want), name
        after = one_step(m, "fused_forward_backward", cor, eps)
        for what, a, b in zip(("out3", "xhat", "gradients"), after, plain):
            assert sh.same_bits(a, b), (name, what)


def recon_term(xhat, t, recon, w):
    if recon == "mse":
        return F.mse_loss(xhat, t)
    return F.binary_cross_entropy(xhat, t, weight=None if w is None else 1 + (w - 1) * t)


def cpu_denoise_grads(p, cor, clean, eps, kld_weight, recon="bce", w=None, want_dx=False):
    """torch CPU f64 autograd of the denoising step: TorchCpuStep.forward(corrupted), the loss taken against the clean roll"""
    stp = TorchCpuStep(p, kld_weight=kld_weight, dtype=torch.float64)
    xc = torch.from_numpy(cor.astype(np.float64)).requires_grad_(want_dx)
    xhat, mu, lv, _ = stp.forward(xc, torch.from_numpy(eps.astype(np.float64)))
    rec = recon_term(xhat, torch.from_numpy(clean.astype(np.float64)), recon, w)
    kld = -0.5 * torch.mean(torch.sum(1 + lv - mu ** 2 - torch.exp(lv), dim=-1))
    loss = rec + kld_weight * kld
    loss.backward()
    out3 = [float(loss.detach()), float(rec.detach()), float(-kld.detach())]
    return out3, xhat.detach().numpy(), {k: v.grad.numpy() for k, v in stp.p.items()}, (xc.grad.numpy() if want_dx else None)


def check_f32_step(H, L, B, gen, recon, w, clean, cor, eps, seed):
    p = perturbed_params(L, H, seed, gen)
    want3, want_xhat, want_g, _ = cpu_denoise_grads(p, cor, clean, eps, 2.0, recon, w)
    m = model_of(H, L, gen, "f32", p, recon, w, kld_weight=2.0)
    xc, xt, e = cuda(cor, clean, eps)
    out3, xhat = m.fused_forward_backward(xc, eps=e, target=xt)
    torch.cuda.synchronize()
    got = flat_grad_dict(m)
    bad = {n: rel_l2(got[n], want_g[n].reshape(-1)) for n in got if n not in PRE_BN_BIAS}
    print("f32 denoising step", recon, w, out3.tolist(), want3, rel_l2(xhat.cpu().numpy(), want_xhat), max(bad.values()))
    np.testing.assert_allclose(out3.tolist(), want3, rtol=1e-4)
    assert rel_l2(xhat.cpu().numpy(), want_xhat) < 1e-4
    assert max(bad.values()) < GRAD_TOL_F32, {n: v for n, v in bad.items() if v >= GRAD_TOL_F32}
    return want3


@pytest.mark.parametrize("recon,w,velocity", [("bce", None, False), ("mse", None, True), ("bce", 8.0, False)], ids=["bce", "mse-velocity", "pos_weight-8"])
@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 32, False), (64, 16, 5, True), (128, 16, 3, True)])
def test_f32_denoising_step_against_torch_autograd(H, L, B, gen, recon, w, velocity):
    clean, cor, eps = denoise_inputs(B, H, L, 52, velocity)
    check_f32_step(H, L, B, gen, recon, w, clean, cor, eps, 51)


def test_f32_step_with_a_target_unrelated_to_the_input():
    """The target is another seed's roll: a kernel that still read x anywhere in the reconstruction term could not pass."""
    H, L, B, gen = 64, 16, 5, True
    x = vo.synth_pianoroll(B, H, 61).astype(np.float32)
    t = velocity_roll(B, H, 62)
    eps = eps_of(B, L, 63)
    assert not np.array_equal(x, t)
    with_t = check_f32_step(H, L, B, gen, "bce", None, t, x, eps, 64)
    own, _, _, _ = cpu_denoise_grads(perturbed_params(L, H, 64, gen), x, x, eps, 2.0)
    assert abs(with_t[1] - own[1]) > 1e-2 * own[1] and abs(with_t[2] - own[2]) <= 1e-12 * abs(own[2])        # another reconstruction term, the same KL


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("H,B,w", [(128, 3, None), (64, 5, 8.0), (256, 1, None), (128, 3, 8.0)])
def test_16bit_output_conv_with_a_target_on_its_own_inputs(dtype, H, B, w):
    """The fused output-conv kernels (128: row-streaming; 64 / 256: tiled) with a clean target against the storage-emulating oracle
    on the kernel's own input (the stored y7): xhat, dz7, final_layer.3's gradients and the reconstruction term - the scheme of
    test_16bit_output_conv_wbce_on_its_own_inputs, with a velocity target and its corruption as the input."""
    import math
    L, gen = 16, True
    p = perturbed_params(L, H, 41, gen)
    clean, cor, eps = denoise_inputs(B, H, L, 43, True)
    m = model_of(H, L, gen, dtype, p, "bce", w)
    xc, xt, e = cuda(cor, clean, eps)
    out3, xhat = m.fused_forward_backward(xc, eps=e, target=xt)
    torch.cuda.synchronize()
    ww = 1.0 if w is None else w
    gs = max(1.0, vo.f16_grad_scale(B, H) / 2.0 ** max(0, math.ceil(math.log2(ww)))) if dtype == "f16" else 1.0
    y7 = _dbg(m, 7, B * 32 * H * H).cpu().numpy().reshape(B, 32, H, H).astype(np.float64)
    dz7 = _dbg(m, 15, B * 32 * H * H).cpu().numpy().reshape(B, 32, H, H).astype(np.float64) / gs
    grads = flat_grad_dict(m)
    P = lambda k: p[k].astype(np.float64)                  # noqa: E731
    rs = lambda v: vo.round_storage(v, dtype)              # noqa: E731
    rg = lambda v: vo.round_storage(v, dtype, gs)          # noqa: E731
    z7, _ = vo.bn_train_fwd_stored(y7, P("final_layer.1.weight"), P("final_layer.1.bias"), dtype)
    a7, wt = rs(vo.lrelu(z7)), rs(P("final_layer.3.weight"))
    logit = vo.conv_fwd(a7, wt, P("final_layer.3.bias"), 1)
    gaps = {"xhat": rel_l2(vo.sigmoid(logit), xhat.cpu().numpy())}
    recon, dlogit = wbce_reference(xhat.double().cpu().numpy(), clean.astype(np.float64), ww)      # the backward from the GPU's own xhat
    _, dlogit_input = wbce_reference(xhat.double().cpu().numpy(), cor.astype(np.float64), ww)
    assert rel_l2(dlogit_input, dlogit) > 100 * LAYER_TOL                                            # (the gate tells the two targets apart)
    gaps["reconstruction_loss"] = abs(out3[1].item() - recon) / recon
    dw, _ = vo.conv_wgrad(a7, rg(dlogit), 1)
    gaps["final_layer.3.weight"] = rel_l2(dw, grads["final_layer.3.weight"].reshape(dw.shape))
    gaps["final_layer.3.bias"] = rel_l2(dlogit.sum(axis=(0, 2, 3)), grads["final_layer.3.bias"])
    gaps["dz7"] = rel_l2(rg(vo.lrelu_bwd(z7, vo.conv_dgrad(rg(dlogit), wt, 1, (H, H)))), dz7)
    print("own inputs with a target", dtype, H, B, w, gs, gaps)
    assert max(gaps.values()) < LAYER_TOL, gaps


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B,bands", [(3, 0), (5, 4)])
def test_streaming_and_tiled_output_conv_bit_identical_with_a_target(dtype, B, bands):
    from torch_vae_amd import _lib
    H, L = 128, 16
    p = perturbed_params(L, H, 13, True)
    clean, cor, eps = cuda(*denoise_inputs(B, H, L, 46, True))
    res = []
    for stream in (0, 1):
        m = model_of(H, L, True, dtype, p, kld_weight=1.5)
        h = m._context(B).handle
        _lib.check(_lib.lib().vae_set_option(h, b"use_convout_stream", stream), "set")
        _lib.check(_lib.lib().vae_set_option(h, b"knob_convout_bands", bands), "set")
        out3, xhat = m.fused_forward_backward(cor, eps=eps, target=clean)
        res.append((out3.clone(), xhat.clone(), _dbg(m, 15, B * 32 * H * H)))
    torch.cuda.synchronize()
    (o0, x0, d0), (o1, x1, d1) = res
    assert torch.equal(x0, x1) and torch.equal(d0, d1)
    np.testing.assert_allclose(o1.cpu().numpy(), o0.cpu().numpy(), rtol=2e-6)      # (the term's sum is partitioned differently)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_deferred_and_separate_output_conv_bit_identical_with_a_target(dtype):
    from torch_vae_amd import _lib
    H, L, B = 64, 16, 6
    p = perturbed_params(L, H, 11, True)
    clean, cor, eps = cuda(*denoise_inputs(B, H, L, 47, True))
    res = []
    for val in (0, 1):
        m = model_of(H, L, True, dtype, p, kld_weight=2.0)
        _lib.check(_lib.lib().vae_set_option(m._context(B).handle, b"use_fused_convout", val), "set")
        out3, xhat = m.fused_forward_backward(cor, eps=eps, target=clean)
        res.append((out3.clone(), xhat.clone(), _dbg(m, 15, B * 32 * H * H), m.flat_grads().clone()))
    torch.cuda.synchronize()
    for what, a, b in zip(("out3", "xhat", "dz7", "gradients"), *res):
        assert torch.equal(a, b), what


def test_every_loss_path_with_a_target():
    """model(x_c, target=x) -> loss() -> backward() equals fused_forward_backward and fused_train_step with the target, and loss() on
    foreign tensors with "input": x; an eval-mode forward's loss() is the f64 formula against the target."""
    H, L, B, gen = 32, 16, 16, False
    p = perturbed_params(L, H, 2, gen)
    clean, cor, eps = cuda(*denoise_inputs(B, H, L, 49))
    m1 = model_of(H, L, gen, "f32", p, kld_weight=4.0)
    out3, _ = m1.fused_forward_backward(cor, eps=eps, target=clean)
    g1 = m1.flat_grads().clone()
    m2 = model_of(H, L, gen, "f32", p, kld_weight=4.0)
    m2.set_next_eps(eps)
    out = m2.forward(cor, target=clean)
    assert out["input"] is clean and m2._last["x"].data_ptr() == cor.data_ptr()
    lo = m2.loss(out)
    assert type(lo["loss"].grad_fn).__name__.startswith("_FusedELBO")              # the HIP ELBO of the forward, not the generic one
    lo["loss"].backward()
    np.testing.assert_allclose([lo["loss"].item(), lo["reconstruction_loss"].item(), lo["kld_loss"].item()], out3.tolist(), rtol=1e-5)
    np.testing.assert_allclose(m2.flat_grads().cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-8)
    m3 = model_of(H, L, gen, "f32", p, kld_weight=4.0)
    o3, _ = m3.fused_train_step(adamw(m3), cor, eps=eps, target=clean)
    torch.cuda.synchronize()
    np.testing.assert_allclose(o3.tolist(), out3.tolist(), rtol=1e-5)
    np.testing.assert_allclose(m3.flat_grads().cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-8)
    m4 = model_of(H, L, gen, "f32", p, kld_weight=4.0)
    m4.set_next_eps(eps)
    out = m4.forward(cor, target=clean)
    foreign = {"output": out["output"] * 1.0, "input": clean, "encoded": {"mu": out["encoded"]["mu"] * 1.0, "log_var": out["encoded"]["log_var"] * 1.0}}
    lg, lf = m4.loss(foreign), m4.loss(out)
    for k in ("loss", "reconstruction_loss", "kld_loss"):
        np.testing.assert_allclose(lg[k].item(), lf[k].item(), rtol=1e-6)
    lg["loss"].backward()
    assert rel_l2(m4.flat_grads().cpu().numpy(), g1.cpu().numpy()) < 1e-5
    # the own output scored against the INPUT is another number: the target really is what the own path read
    against_input = m4.loss({**foreign, "input": cor})["reconstruction_loss"].item()
    assert abs(against_input - lf["reconstruction_loss"].item()) > 100 * 1e-5 * against_input
    m1.eval()
    with torch.no_grad():
        ev = m1.forward(cor, target=clean)
        le = m1.loss(ev)
    want = float(F.binary_cross_entropy(ev["output"].double().cpu(), clean.double().cpu()))
    np.testing.assert_allclose(le["reconstruction_loss"].item(), want, rtol=1e-5)
    with pytest.raises(RuntimeError, match="target must have the input's shape"):
        m1.forward(cor, target=clean[:-1])
    with pytest.raises(RuntimeError, match="expected input"):
        m1.fused_forward_backward(cor, target=clean[:, :, :-1])


def test_the_input_gradient_is_the_corrupted_input_s():
    H, L, B, gen = 32, 16, 5, False
    p = perturbed_params(L, H, 71, gen)
    clean, cor, eps = denoise_inputs(B, H, L, 72)
    want3, _, want_g, want_dx = cpu_denoise_grads(p, cor, clean, eps, 2.0, want_dx=True)
    m = model_of(H, L, gen, "f32", p, kld_weight=2.0)
    xc, xt, e = cuda(cor, clean, eps)
    xc.requires_grad_(True)
    m.set_next_eps(e)
    lo = m.loss(m.forward(xc, target=xt))
    lo["loss"].backward()
    torch.cuda.synchronize()
    assert xt.grad is None and xc.grad is not None
    gap = rel_l2(xc.grad.cpu().numpy(), want_dx)
    print("input gradient", lo["loss"].item(), want3[0], gap)
    np.testing.assert_allclose(lo["loss"].item(), want3[0], rtol=1e-4)
    assert gap < GRAD_TOL_F32
    got = flat_grad_dict(m)
    bad = {n: rel_l2(got[n], want_g[n].reshape(-1)) for n in got if n not in PRE_BN_BIAS}
    assert max(bad.values()) < GRAD_TOL_F32, bad


def test_attr_reg_counts_the_target():
    from torch_vae_amd.attributes import attribute_regularizer, roll_attributes
    H, L, B, gen = 32, 16, 8, False
    p = perturbed_params(L, H, 43, gen)
    clean, cor, eps = cuda(*denoise_inputs(B, H, L, 44))
    reg = {"note_density": 1, "polyphony": 0}
    assert not torch.equal(roll_attributes(clean, 0.5), roll_attributes(cor, 0.5))
    m = model_of(H, L, gen, "f32", p)
    m.attr_reg, m.attr_weight = dict(reg), 0.5
    m.fused_forward_backward(cor, eps=eps, target=clean)
    from torch_vae_amd._lib import ATTRIBUTES
    want, _ = attribute_regularizer(m._last["z"], roll_attributes(clean, 0.5), [ATTRIBUTES[n] for n in reg], list(reg.values()), 10.0, 0.5)
    assert sh.same_bits(m.attribute_loss(), want)
    m2 = model_of(H, L, gen, "f32", p)
    m2.attr_reg, m2.attr_weight = dict(reg), 0.5
    m2.set_next_eps(eps)
    m2.loss(m2.forward(cor, target=clean))
    assert sh.same_bits(m2.attribute_loss(), want)


# ---- 3. the Python layer ---------------------------------------------------------------------------------------------------------------
class DenoiseCpuStep(TorchCpuStep):
    """TorchCpuStep whose reconstruction term is taken against a clean roll."""

    def step(self, cor, clean, eps):
        xhat, mu, lv, z = self.forward(cor, eps)
        self.opt.zero_grad()
        recon = F.binary_cross_entropy(xhat, clean)
        kld = -0.5 * torch.mean(torch.sum(1 + lv - mu ** 2 - torch.exp(lv), dim=-1))
        loss = recon + self.kld_weight * kld
        loss.backward()
        self.opt.step()
        self.sched.step()
        return float(loss.detach()), float(recon.detach()), float(-kld.detach())


def base_config(B, **extra):
    return Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                     epochs=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0, **extra)


def config_corruption(x, step, B, seed=0):
    """corrupt_ref with denoise_note_dropout=0.3, denoise_span=(4, 8) and the counters of train_one_epoch's step `step`"""
    out, _ = R.corrupt_ref(x[:, 0], p_drop=0.3, span=(4, 8), seed=seed, counter0=step * B, counter_stride=1)
    return np.ascontiguousarray(out[:, None])


def test_train_one_epoch_with_the_denoise_config_against_the_cpu_loop():
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    H, L, B, steps, total, kw, first = 32, 16, 4, 3, 10, 1.0, 2
    p = vo.init_params(L, H, 61, False)
    batches = [(vo.synth_pianoroll(B, H, 70 + s).astype(np.float32), eps_of(B, L, 70 + s)) for s in range(steps)]
    cpu = DenoiseCpuStep(p, kld_weight=kw, batch=B, total_steps=total, dtype=torch.float64)
    f64 = lambda a: torch.from_numpy(a.astype(np.float64))      # noqa: E731
    want = [cpu.step(f64(config_corruption(x, first + s, B, seed=7)), f64(x), f64(e)) for s, (x, e) in enumerate(batches)]
    assert any(not np.array_equal(config_corruption(x, first + s, B, seed=7), x) for s, (x, _) in enumerate(batches))
    model = make_model(H, L, False, "f32", p, kld_weight=kw)
    cfg = base_config(B, denoise_note_dropout=0.3, denoise_span=(4, 8), denoise_seed=7)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=total)
    it = iter([torch.from_numpy(e).cuda() for _, e in batches])
    got, seen = [], []
    orig = model.fused_train_step

    def step(o, x, **k):
        seen.append((x.clone(), k["target"].clone()))
        out3, xhat = orig(o, x, **{**k, "eps": next(it)})
        got.append(out3.tolist())
        return out3, xhat
    model.fused_train_step = step
    loader = [(torch.from_numpy(x), torch.zeros(B, dtype=torch.long)) for x, _ in batches]
    res, total_step, _ = train_one_epoch(cfg, model, opt, sched, model.loss, loader, device="cuda", epoch=1, total_step=first)
    assert total_step == first + steps and len(got) == steps
    for s, ((xin, tgt), (x, _)) in enumerate(zip(seen, batches)):      # the step got the clean batch as target, corrupt_ref's bits as input
        assert np.array_equal(bits(host(tgt)), bits(x)) and np.array_equal(bits(host(xin)), bits(config_corruption(x, first + s, B, seed=7))), s
    print("train_one_epoch", got, want)
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-4)
    np.testing.assert_allclose(res["loss"], np.mean([x[0] for x in want]), rtol=2e-4)


def test_torch_optimiser_path_of_train_one_epoch_honours_the_denoise_config():
    from torch_vae_amd.train import train_one_epoch
    H, L, B, kw = 32, 16, 4, 1.0
    p = vo.init_params(L, H, 61, False)
    x, eps = vo.synth_pianoroll(B, H, 70).astype(np.float32), eps_of(B, L, 70)
    cor = config_corruption(x, 0, B)
    want3, _, _, _ = cpu_denoise_grads(p, cor, x, eps, kw)
    own3, _, _, _ = cpu_denoise_grads(p, x, x, eps, kw)
    assert abs(want3[0] - own3[0]) > 1e-3 * own3[0]
    model = make_model(H, L, False, "f32", p, kld_weight=kw)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    cfg = Namespace(world_size=1, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0,
                    denoise_note_dropout=0.3, denoise_span=(4, 8))
    model.set_next_eps(torch.from_numpy(eps).cuda())
    res, _, _ = train_one_epoch(cfg, model, opt, torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0), model.loss,
                                [(torch.from_numpy(x), torch.zeros(B, dtype=torch.long))], device="cuda", epoch=2)
    np.testing.assert_allclose(res["loss"], want3[0], rtol=1e-4)


def test_train_one_epoch_without_the_fields_is_the_loop_as_it_is():
    from torch_vae_amd.train import build_optimizer, fused_step, train_one_epoch
    H, L, B, steps = 32, 16, 4, 3
    p = vo.init_params(L, H, 61, False)
    loader = [(torch.from_numpy(vo.synth_pianoroll(B, H, 70 + s).astype(np.float32)), torch.zeros(B, dtype=torch.long)) for s in range(steps)]
    runs = []
    for how in ("train_one_epoch", "by hand"):
        model = make_model(H, L, False, "f32", p)
        cfg = base_config(B) if how == "by hand" else base_config(B, denoise_note_dropout=None, denoise_span=None, denoise_add_noise=None, denoise_seed=3)
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
                assert k.get("target") is None
                out = orig(o, x, **k)
                got.append(out[0].clone())
                return out
            model.fused_train_step = step
            train_one_epoch(cfg, model, opt, sched, model.loss, loader, device="cuda", epoch=1)
        runs.append((got, model.flat_parameters().clone()))
    assert len(runs[0][0]) == len(runs[1][0]) == steps
    assert all(sh.same_bits(a, b) for a, b in zip(runs[0][0], runs[1][0])) and sh.same_bits(runs[0][1], runs[1][1])


@functools.lru_cache(maxsize=None)
def small_model():
    return make_model(32, 16, False, "f32", perturbed_params(16, 32, 91, False))


def test_infill():
    from torch_vae_amd.generation import infill
    m = small_model()
    x = torch.from_numpy(velocity_roll(4, 32, 92)).cuda()
    was_training, t0, t1 = m.training, 8, 20
    filled, xhat = infill(m, x, t0, t1)
    assert m.training == was_training and filled.shape == x.shape == xhat.shape
    outside = torch.ones(32, dtype=torch.bool, device="cuda"); outside[t0:t1] = False
    assert sh.same_bits(filled[..., outside], x[..., outside])
    masked = x.clone(); masked[..., t0:t1] = 0
    m.eval()
    with torch.no_grad():
        m.set_next_eps(torch.zeros(4, 16, device="cuda"))          # z = mu: the decode of the posterior mean
        ev = m(masked)["output"]
    m.train(was_training)
    assert sh.same_bits(xhat, ev) and sh.same_bits(filled[..., t0:t1], ev[..., t0:t1])
    assert not torch.equal(filled[..., t0:t1], x[..., t0:t1])
    binary, raw = infill(m, x, t0, t1, threshold=0.5)
    assert sh.same_bits(raw, xhat) and sh.same_bits(binary[..., outside], x[..., outside])
    assert sh.same_bits(binary[..., t0:t1], (xhat[..., t0:t1] >= 0.5).float())
    whole, _ = infill(m, x, 0, 32)
    assert sh.same_bits(whole, infill(m, torch.rand_like(x), 0, 32)[1])      # everything masked: the input no longer matters
    with pytest.raises(ValueError, match="t0 < t1"):
        infill(m, x, 20, 20)


def test_infill_metrics():
    from torch_vae_amd.evaluation import infill_metrics, reconstruction_metrics
    rng = np.random.default_rng(5)
    xhat = torch.from_numpy(rng.random((6, 1, 32, 32)).astype(np.float32)).cuda()
    target = torch.from_numpy(velocity_roll(6, 32, 93)).cuda()
    for t0, t1 in ((8, 20), (0, 32), (31, 32)):
        got = infill_metrics(xhat, target, t0, t1, thresholds=(0.3, 0.5))
        want = reconstruction_metrics(xhat[..., t0:t1].contiguous(), target[..., t0:t1].contiguous(), thresholds=(0.3, 0.5))
        assert set(got.keys()) == set(want.keys())
        for k in want.keys():
            assert sh.same_bits(got[k], want[k]), (t0, t1, k)
        assert int(got["n_cells"]) == 6 * 32 * (t1 - t0)


def test_evaluate_with_an_infill_span():
    from torch_vae_amd.evaluation import evaluate, infill_metrics, ratios_from_counts
    from torch_vae_amd.generation import infill
    m = small_model()
    was_training = m.training
    loader = [(torch.from_numpy(vo.synth_pianoroll(8, 32, 94 + s).astype(np.float32)), torch.zeros(8, dtype=torch.long)) for s in range(2)]

    def run(**kw):
        torch.manual_seed(3)          # the eval forward draws eps from torch's device generator
        return evaluate(loader, m, "cuda", verbosity=0, **kw)
    plain, with_span = run(note_thresholds=0.5), run(note_thresholds=0.5, infill_span=(8, 20))
    assert [k for k in with_span if k not in plain] == ["infill_f1", "infill_precision", "infill_recall"]
    assert {k: with_span[k] for k in plain} == plain and list(with_span)[:len(plain)] == list(plain)
    assert {k: v for k, v in run(infill_span=(8, 20)).items() if not k.startswith("infill_")} == run()
    pos = tp = fp = n = 0
    for x, _ in loader:
        x = x.cuda()
        r = infill_metrics(infill(m, x, 8, 20)[1], x, 8, 20)
        pos, tp, fp, n = pos + int(r["positives"]), tp + int(r["tp"][0]), fp + int(r["fp"][0]), n + int(r["n_cells"])
    want = ratios_from_counts(n, pos, [tp], [fp])
    for k in ("f1", "precision", "recall"):
        assert abs(with_span[f"infill_{k}"] - 100.0 * want[k][0]) <= 1e-12, k
    assert pos > 0
    m.train(was_training)
    with pytest.raises(ValueError, match="t0 < t1"):
        evaluate(loader, m, "cuda", verbosity=0, infill_span=(8, 40))


# ---- 4. the stream contract (include/vae_step.h, first paragraph) on the new entry points -------------------------------------------------
S_SHAPE = (16, 128, 128)
S_KW = dict(p_drop=0.3, p_add=0.01, seed=11, counter0=5, counter_stride=3)


def _make_corrupt():
    b = Bufs()
    b.inp("clean", torch.from_numpy(roll(*S_SHAPE, "velocity")))
    b.inp("spans", torch.from_numpy(R.spans_ref(S_SHAPE[0], S_SHAPE[2], 16, 32, 2)), poison=0)
    for name in ("out", "out_given"):
        b.outp(name, *S_SHAPE)
    for name in ("hidden", "hidden_given"):
        b.outp(name, S_SHAPE[0], S_SHAPE[1], S_SHAPE[2] // 8, dtype=torch.uint8)
    b.outp("drawn", S_SHAPE[0], 2, dtype=torch.int32)
    return b


def _corrupt(b):
    n, h, w = S_SHAPE
    ok(lib().vae_denoise_corrupt(b["clean"].data_ptr(), b["out"].data_ptr(), b["hidden"].data_ptr(), n, h, w, 0.5, 0.3, 16, 32, 0.01, 1.0, 0,
                                 11, 5, 3, st()))
    ok(lib().vae_denoise_corrupt(b["clean"].data_ptr(), b["out_given"].data_ptr(), b["hidden_given"].data_ptr(), n, h, w, 0.5, 0.3, 0, 0, 0.01, 1.0,
                                 b["spans"].data_ptr(), 11, 5, 3, st()))


def _params(b):
    ok(lib().vae_denoise_params(b["drawn"].data_ptr(), S_SHAPE[0], S_SHAPE[2], 16, 32, 11, 5, 3, st()))


STREAM_CASES = [
    Case("denoise_corrupt", ("vae_denoise_corrupt",), _make_corrupt, _corrupt),
    Case("denoise_params", ("vae_denoise_params",), _make_corrupt, _params),
]


def _python(b):
    from torch_vae_amd.denoise import corrupt_rolls, corruption_spans
    b.out["out"], b.out["hidden"] = corrupt_rolls(b["clean"], note_dropout=0.3, span=(16, 32), add_noise=0.01, seed=11, counter0=5, counter_stride=3,
                                                  return_hidden=True)
    b.out["out_given"] = corrupt_rolls(b["clean"], spans=b["spans"], seed=11)
    b.out["drawn"] = corruption_spans(S_SHAPE[0], S_SHAPE[2], (16, 32), seed=11, counter0=5, counter_stride=3)


def _denoising_steps(b):
    from torch_vae_amd.denoise import corrupt_rolls
    from torch_vae_amd.train import fused_step
    m, opt = b.keep[0], b.keep[1]
    for i in range(2):
        cor = corrupt_rolls(b["x"], note_dropout=0.3, span=(4, 8), seed=3, counter0=i * b["x"].shape[0])
        out3, xhat = fused_step(m, opt, cor, eps=b["eps"], target=b["x"])
        b.out[f"out3_{i}"] = out3.clone()
    b.out["xhat"] = xhat


def _infill(b):
    from torch_vae_amd.generation import infill
    b.out["filled"], b.out["infill_xhat"] = infill(b.keep[0], b["x"], 8, 20)


PY_STREAM_CASES = [
    Case("python/corrupt_rolls+corruption_spans", ("vae_denoise_corrupt", "vae_denoise_params"), _make_corrupt, _python, warmups=2),
    Case("python/fused_step with a target", ("vae_denoise_corrupt",), streams._py_model, _denoising_steps, dtype="bf16", reset=streams._py_reset,
         warmups=2),
    Case("python/infill", (), streams._py_model, _infill, dtype="bf16", reset=streams._py_reset, warmups=2),
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_stream_contract(case):
    sh.check_case(case)
    b = case.make()          # and what it computed is right
    sh.stage(b)
    case.run(b)
    x = roll(*S_SHAPE, "velocity")
    if case.name == "denoise_params":
        assert np.array_equal(host(b["drawn"]), R.spans_ref(S_SHAPE[0], S_SHAPE[2], 16, 32, 11, 5, 3))
    else:
        assert_same((host(b["out"]), host(b["hidden"])), R.corrupt_ref(x, span=(16, 32), **S_KW), "drawn")
        assert_same((host(b["out_given"]), host(b["hidden_given"])), R.corrupt_ref(x, spans=R.spans_ref(S_SHAPE[0], S_SHAPE[2], 16, 32, 2), **S_KW), "given")


@pytest.mark.parametrize("case", PY_STREAM_CASES, ids=repr)
def test_stream_contract_python_layer(case):
    sh.check_case(case)
