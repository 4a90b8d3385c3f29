"""Note-event extraction on the GPU (vae_extract_notes, torch_vae_amd/generation.py, VanillaVAE.sample_notes / interpolate,
evaluate(..., note_events=...)) against tests/notes_ref.py.  Every comparison is exact.  In the kernel tests the source is a view into
the middle of a larger buffer of ones and every output a view into a larger buffer pre-filled with a sentinel: a missing guard shows
as a wrong value or a damaged sentinel, never as a stray access."""
import functools

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests import notes_ref as nr
from tests.util import make_model, perturbed_params
from torch_vae_amd import _lib, data, evaluation, generation

pytestmark = pytest.mark.gpu

PAD = 1024                                  # cells / slots / bytes of filler on either side of every buffer
EV_S, PK_S, OFF_S, CL_S = -77, -7.5, -99, 0xA5


def embed(x, shift=0):
    """x [n,h,w] float32 on the device as a view into the middle of a buffer of ones, `shift` more bytes in front."""
    assert shift % 4 == 0
    t = torch.from_numpy(np.array(x, np.float32))
    buf = torch.ones(2 * PAD + shift // 4 + t.numel(), dtype=torch.float32)
    lo = PAD + shift // 4
    buf[lo:lo + t.numel()] = t.reshape(-1)
    buf = buf.cuda()
    assert buf.data_ptr() % 16 == 0
    return buf[lo:lo + t.numel()].view(t.shape), buf


def framed(numel, dtype, sentinel, shift_items=0):
    """(view of `numel` items, whole buffer, start) inside a device buffer filled with `sentinel`."""
    buf = torch.full((2 * PAD + shift_items + numel,), sentinel, dtype=dtype, device="cuda")
    lo = PAD + shift_items
    return buf[lo:lo + numel], buf, lo


def intact(buf, lo, numel, sentinel):
    host = buf.cpu()
    return bool((host[:lo] == sentinel).all()) and bool((host[lo + numel:] == sentinel).all())


def raw(x, on, off, D, G, *, capacity=None, events=True, cleaned=True, shift=0, ev_shift=0, slack=3):
    """One call of the C entry point on embedded / framed buffers.  capacity None: the reference's total plus `slack` slots, which
    must stay untouched.  Returns host arrays (events and peaks cut to min(total, capacity)) after checking every sentinel."""
    x = np.asarray(x, np.float32)
    n, h, w = x.shape
    src, _keep = embed(x, shift)
    assert src.data_ptr() % 16 == shift % 16
    total = None
    if capacity is None:
        total = int(nr.extract(x, on, off, D, G)["offsets"][-1])
        capacity = total + slack
    ev, ev_buf, ev_lo = framed(4 * capacity, torch.int32, EV_S, ev_shift // 4)
    pk, pk_buf, pk_lo = framed(capacity, torch.float32, PK_S)
    of, of_buf, of_lo = framed(n + 1, torch.int64, OFF_S)
    cl, cl_buf, cl_lo = framed(n * h * (w // 8), torch.uint8, CL_S, 3)        # (an odd start: cleaned has no alignment to rely on)
    if events and capacity:
        assert ev.data_ptr() % 16 == ev_shift % 16
    rc = _lib.lib().vae_extract_notes(src.data_ptr(), n, h, w, on, off, D, G, ev.data_ptr() if events else None,
                                      pk.data_ptr() if events else None, capacity, of.data_ptr(), cl.data_ptr() if cleaned else None,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().vae_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(src.cpu().view(torch.int32), torch.from_numpy(np.array(x)).view(torch.int32)), "the source was written"
    assert intact(ev_buf, ev_lo, 4 * capacity, EV_S) and intact(pk_buf, pk_lo, capacity, PK_S), "events / peaks frame damaged"
    assert intact(of_buf, of_lo, n + 1, OFF_S) and intact(cl_buf, cl_lo, cl.numel(), CL_S), "offsets / cleaned frame damaged"
    offsets = of.cpu().numpy()
    written = min(int(offsets[-1]), capacity) if events else 0
    ev_h, pk_h = ev.cpu().numpy().reshape(capacity, 4), pk.cpu().numpy()
    assert (ev_h[written:] == EV_S).all() and (pk_h[written:] == PK_S).all(), "slots past the written events were touched"
    cl_h = cl.cpu().numpy().reshape(n, h, w // 8)
    if not cleaned:
        assert (cl_h == CL_S).all()
    if total is not None:
        assert int(offsets[-1]) == total
    return {"events": ev_h[:written], "peaks": pk_h[:written], "offsets": offsets, "cleaned": cl_h if cleaned else None}


def same(got, ref, tag, upto=None):
    np.testing.assert_array_equal(got["offsets"], ref["offsets"], err_msg=f"{tag} offsets")
    np.testing.assert_array_equal(got["events"], ref["events"][:upto], err_msg=f"{tag} events")
    np.testing.assert_array_equal(got["peaks"].view(np.int32), ref["peaks"][:upto].view(np.int32), err_msg=f"{tag} peaks")
    if got["cleaned"] is not None:
        np.testing.assert_array_equal(got["cleaned"], ref["cleaned"], err_msg=f"{tag} cleaned")


def test_sweep():
    """Every width at a 64-step chunk edge, by rows and rolls, by parameter set.  The witnesses: over the sweep each parameter set's
    reference output holds every effect its parameters allow (bridging needs G > 0, dropping D > 1, sustaining off < on), and the
    sets together hold all three - otherwise the comparison proves nothing."""
    rng = np.random.default_rng(0)
    seen = {ps: {"bridged": 0, "dropped": 0, "sustained": 0, "events": 0} for ps in nr.PARAM_SETS}
    for w in (8, 24, 64, 72, 128, 136, 200):
        for h in (1, 3):
            for n in (1, 5):
                x = nr.random_rolls(rng, n, h, w)
                for ps in nr.PARAM_SETS:
                    ref = nr.extract(x, *ps)
                    same(raw(x, *ps), ref, f"w={w} h={h} n={n} {ps}")
                    for k in ("bridged", "dropped", "sustained"):
                        seen[ps][k] += ref["stats"][k]
                    seen[ps]["events"] += len(ref["events"])
    print(seen)
    for (on, off, D, G), st in seen.items():
        assert st["events"] > 100
        assert (st["bridged"] > 0) == (G > 0) and (st["dropped"] > 0) == (D > 1) and (st["sustained"] > 0) == (off < on), ((on, off, D, G), st)
    assert all(any(st[k] > 10 for st in seen.values()) for k in ("bridged", "dropped", "sustained"))


def hand_rows(D, G):
    """Rows of 128 steps, each one edge of the contract (on = 0.5, off = 0.3)."""
    rows = []

    def row():
        r = np.zeros(128, np.float32)
        rows.append(r)
        return r
    row()[:] = 1.0                                             # one note over the whole row
    r = row(); r[:D + 1] = 0.7; r[128 - D:] = 0.9              # notes touching both ends
    r = row(); r[:G + 1] = 0.0; r[G + 1:G + 1 + D] = 1.0       # a silent run of G + 1 at the row's start is no gap
    r = row(); r[40:64 - G // 2] = 1.0; r[64 - G // 2 + G:90] = 0.6     # a gap of exactly G across 63|64 (G = 0: adjacent)
    r = row(); r[40:63 - G // 2] = 1.0; r[64 - G // 2 + G:90] = 0.6     # and one of G + 1
    if D > 1:
        r = row(); r[64 - (D - 1):64] = 1.0                    # a note of D - 1 ending at column 64: dropped
        r = row(); r[65 - (D - 1):65] = 1.0                    # ... its last cell in the second chunk
    r = row(); r[64 - D:64] = 1.0                              # a note of D ending at column 64: kept
    r = row(); r[65 - D:65] = 0.5
    row()[:] = np.nan                                          # a row of NaNs
    r = row(); r[10:15] = 0.7; r[15:15 + max(G, 1)] = np.nan; r[15 + max(G, 1):25] = 1.0    # a NaN gap: bridged when G >= 1, the peak skips it
    r = row(); r[60] = 1.0; r[61:70] = 0.4; r[70] = np.nan; r[71:80] = 0.4    # sustained across 63|64, ended by a NaN
    r = row(); r[0::2] = 1.0                                   # alternating
    r = row(); r[1::2] = 0.5
    return np.stack(rows)[None]


@pytest.mark.parametrize("D,G", [(1, 0), (2, 1), (3, 2), (5, 64), (70, 3)])
def test_hand_made_rows(D, G):
    x = hand_rows(D, G)
    ref = nr.extract(x, 0.5, 0.3, D, G)
    got = raw(x, 0.5, 0.3, D, G)
    same(got, ref, f"D={D} G={G}")
    by_row = lambda p: [tuple(e[2:]) for e in got["events"] if e[1] == p]
    assert by_row(0) == [(0, 128)]
    if (D, G) == (3, 2):
        assert by_row(1) == [(0, 4), (125, 3)] and by_row(2) == [(3, 3)]
        assert by_row(3) == [(40, 50)] and by_row(4) == [(40, 22), (65, 25)]
        assert by_row(5) == [] and by_row(6) == [] and by_row(7) == [(61, 3)] and by_row(8) == [(62, 3)]
        assert by_row(9) == []
        i = [k for k, e in enumerate(got["events"]) if e[1] == 10]
        assert by_row(10) == [(10, 15)] and got["peaks"][i[0]] == 1.0
        assert by_row(11) == [(60, 10)]
        assert by_row(12) == [(0, 127)]                        # every one-step gap bridged: one note, the last cell silent


def test_worst_case_and_capacity():
    n, h, w = 2, 3, 128
    x = nr.alternating(n, h, w)
    ref = nr.extract(x, 0.5, 0.5, 1, 0)
    total = n * h * 64
    assert len(ref["events"]) == total
    same(raw(x, 0.5, 0.5, 1, 0, capacity=total), ref, "exact capacity")
    same(raw(x, 0.5, 0.5, 1, 0, capacity=total - 5), ref, "capacity - 5", upto=total - 5)     # (raw checks the slots beyond)
    same(raw(x, 0.5, 0.5, 1, 0, capacity=1), ref, "capacity 1", upto=1)


@functools.lru_cache(maxsize=None)
def _scan_case(n, h, w, density, seed):
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((n, h, w)) < density, np.float32(1.0), np.float32(0.2)).astype(np.float32)
    x[rng.random((n, h, w)) < density / 2] = 0.4
    ref = nr.extract(x, 0.5, 0.3, 1, 1)
    x.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("n,h,w,density", [(70000, 1, 8, 0.01), (1400, 50, 8, 0.01), (5, 128, 128, 0.05)])
def test_scan_across_tiles(n, h, w, density):
    """More rows than one pass of the scan's workgroup (16384), with h = 1 (every row an offset) and h = 50 (rolls straddle tiles)."""
    x, ref = _scan_case(n, h, w, density, 3)
    assert len(ref["events"]) > 300
    same(raw(x, 0.5, 0.3, 1, 1), ref, f"{n}x{h}x{w}")


def test_count_only_and_cleaned_alone():
    x = nr.random_rolls(np.random.default_rng(5), 3, 4, 136)
    ref = nr.extract(x, 0.5, 0.3, 2, 1)
    got = raw(x, 0.5, 0.3, 2, 1, events=False, cleaned=False, capacity=0)
    np.testing.assert_array_equal(got["offsets"], ref["offsets"])
    got = raw(x, 0.5, 0.3, 2, 1, events=False, cleaned=True, capacity=0)
    np.testing.assert_array_equal(got["offsets"], ref["offsets"])
    np.testing.assert_array_equal(got["cleaned"], ref["cleaned"])
    got = raw(x, 0.5, 0.3, 2, 1, events=True, cleaned=False)
    same(got, ref, "no cleaned")


@pytest.mark.parametrize("shift,ev_shift", [(4, 0), (8, 0), (12, 0), (0, 4), (12, 4)])
def test_alignment(shift, ev_shift):
    x = nr.random_rolls(np.random.default_rng(6), 2, 3, 72)
    same(raw(x, 0.5, 0.3, 2, 1, shift=shift, ev_shift=ev_shift), nr.extract(x, 0.5, 0.3, 2, 1), f"shift {shift} / {ev_shift}")


def host(res):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def test_python_api_and_determinism():
    x = nr.random_rolls(np.random.default_rng(7), 4, 5, 200)
    ref = nr.extract(x, 0.5, 0.3, 2, 1)
    xd = torch.from_numpy(x).cuda()
    kw = dict(onset_threshold=0.5, sustain_threshold=0.3, min_duration=2, max_gap=1)
    a = generation.extract_notes(xd, cleaned=True, **kw)
    assert a["events"].dtype == torch.int32 and a["peaks"].dtype == torch.float32 and a["offsets"].dtype == torch.int64
    assert a["cleaned"].dtype == torch.uint8 and a["total"].dim() == 0 and int(a["total"]) == len(ref["events"])
    same(host(a), ref, "exact allocation")
    b = generation.extract_notes(xd.view(4, 1, 5, 200), cleaned=True, **kw)
    for k in ("events", "peaks", "offsets", "cleaned"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    big = generation.extract_notes(xd, max_notes=len(ref["events"]) + 100, **kw)
    assert big["events"].shape == (len(ref["events"]) + 100, 4) and big["cleaned"] is None
    N = int(big["total"])
    assert torch.equal(big["events"][:N], a["events"]) and torch.equal(big["peaks"][:N].view(torch.int32), a["peaks"].view(torch.int32))
    assert torch.equal(big["offsets"], a["offsets"])
    small = generation.extract_notes(xd, max_notes=7, **kw)
    assert int(small["total"]) == N and torch.equal(small["events"], a["events"][:7])
    none = generation.extract_notes(xd, max_notes=0, cleaned=True, **kw)
    assert none["events"].shape == (0, 4) and torch.equal(none["offsets"], a["offsets"]) and torch.equal(none["cleaned"], a["cleaned"])
    # defaults: plain thresholding at 0.5; a silent batch; an empty batch
    same(host(generation.extract_notes(xd)), {k: v for k, v in nr.extract(x).items() if k != "cleaned"} | {"cleaned": None}, "defaults")
    silent = generation.extract_notes(torch.zeros(2, 3, 16, device="cuda"), cleaned=True)
    assert silent["events"].shape == (0, 4) and silent["offsets"].tolist() == [0, 0, 0] and int(silent["cleaned"].sum()) == 0
    empty = generation.extract_notes(torch.zeros(0, 3, 16, device="cuda"))
    assert empty["events"].shape == (0, 4) and empty["offsets"].tolist() == [0] and int(empty["total"]) == 0
    assert generation.binarize_rolls(torch.zeros(0, 3, 16, device="cuda")).shape == (0, 3, 2)
    # host lists
    lists = generation.events_to_lists(a, pitch_offset=21)
    assert len(lists) == 4
    flat = [(r, p - 21, t0, d) for r, notes in enumerate(lists) for p, t0, d, _ in notes]
    assert flat == [tuple(e) for e in ref["events"].tolist()]
    vel = [v for notes in lists for *_, v in notes]
    assert vel == [int(round(127.0 * min(max(float(p), 0.0), 1.0))) for p in ref["peaks"]]
    secs = generation.events_to_lists(a, step_seconds=0.25)
    assert secs[0][0][1:3] == (lists[0][0][1] * 0.25, lists[0][0][2] * 0.25)
    for bad in (dict(onset_threshold=0.3, sustain_threshold=0.5), dict(min_duration=0), dict(max_gap=-1), dict(max_notes=-1),
                dict(onset_threshold=float("nan"))):
        with pytest.raises(ValueError):
            generation.extract_notes(xd, **bad)
    with pytest.raises(ValueError):
        generation.extract_notes(xd[:, :, ::2])
    with pytest.raises(TypeError):
        generation.extract_notes(xd.double())


@pytest.mark.parametrize("t", [0.3, 0.5])
def test_binarize_rolls(t):
    x = nr.random_rolls(np.random.default_rng(8), 3, 7, 136)
    got = generation.binarize_rolls(torch.from_numpy(x).cuda(), t)
    with np.errstate(invalid="ignore"):
        want = np.packbits(x >= np.float32(t), axis=-1)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def test_round_trip_through_the_resident_dataset():
    x = nr.random_rolls(np.random.default_rng(9), 6, 8, 72)
    first = generation.extract_notes(torch.from_numpy(x).cuda(), onset_threshold=0.7, sustain_threshold=0.1, min_duration=3, max_gap=2,
                                     cleaned=True)
    assert int(first["total"]) > 20
    ds = data.PianorollDataset.from_stored(first["cleaned"], "bits")
    assert (len(ds), ds.height, ds.width) == (6, 8, 72)
    back = data.gather_rolls(ds.data, "bits", 72, batch=6)
    assert back.shape == (6, 1, 8, 72)
    again = generation.extract_notes(back, cleaned=True)
    for k in ("events", "offsets", "cleaned"):
        assert torch.equal(again[k], first[k]), k
    assert bool((again["peaks"] == 1.0).all())


def _snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _unchanged(model, snap, training):
    assert model.training == training
    now = model.state_dict()
    assert list(now) == list(snap)
    for k, v in snap.items():
        assert torch.equal(now[k], v), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("training", [False, True])
def test_sample_notes(dtype, training):
    H, L, B = 32, 16, 4
    m = make_model(H, L, False, dtype, perturbed_params(L, H, 3, False))
    m.train(training)
    snap = _snapshot(m)
    assert any(k.endswith("num_batches_tracked") for k in snap) and any(k.endswith("running_var") for k in snap)
    probe = m.sample_notes(B, seed=11, return_rolls=True)
    rolls = probe["rolls"]
    assert rolls.shape == (B, 1, H, H) and rolls.dtype == torch.float32
    t = float(rolls.median())                      # a threshold that certainly cuts through the decoded values
    kw = dict(onset_threshold=t, sustain_threshold=0.98 * t, min_duration=2, max_gap=1)
    a = m.sample_notes(B, seed=11, return_rolls=True, cleaned=True, **kw)
    b = m.sample_notes(B, seed=11, return_rolls=True, cleaned=True, **kw)
    assert torch.equal(a["rolls"], rolls) and int(a["total"]) > 0
    for k in ("rolls", "events", "peaks", "offsets", "cleaned"):
        assert torch.equal(a[k], b[k]), k
    direct = generation.extract_notes(a["rolls"], cleaned=True, **kw)
    for k in ("events", "peaks", "offsets", "cleaned"):
        assert torch.equal(a[k], direct[k]), k
    same(host({k: a[k] for k in ("events", "peaks", "offsets", "cleaned")}),
         nr.extract(a["rolls"][:, 0].cpu().numpy(), t, np.float32(0.98 * t), 2, 1), "sample_notes")
    assert not torch.equal(m.sample_notes(B, seed=12, return_rolls=True)["rolls"], rolls)
    assert "rolls" not in m.sample_notes(B, seed=11)
    cold = m.sample_notes(B, temperature=0.0, seed=1, return_rolls=True)["rolls"]
    assert all(torch.equal(cold[0], cold[i]) for i in range(1, B))
    hot = m.sample_notes(B, temperature=2.0, seed=11, return_rolls=True)["rolls"]
    assert not torch.equal(hot, rolls)
    _unchanged(m, snap, training)


def _np_interp(a, b, steps, mode):
    a, b = a.astype(np.float64), b.astype(np.float64)
    out = np.empty((len(a), steps, a.shape[1]))
    for i in range(len(a)):
        om = np.arccos(np.clip(a[i] @ b[i] / (np.linalg.norm(a[i]) * np.linalg.norm(b[i])), -1, 1))
        for s in range(steps):
            t = s / (steps - 1) if steps > 1 else 0.0
            if mode == "lerp" or om < 1e-6:
                out[i, s] = (1 - t) * a[i] + t * b[i]
            else:
                out[i, s] = np.sin((1 - t) * om) / np.sin(om) * a[i] + np.sin(t * om) / np.sin(om) * b[i]
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_interpolate(dtype):
    H, L, B, steps = 32, 16, 4, 5
    m = make_model(H, L, False, dtype, perturbed_params(L, H, 4, False))
    m.train(True)
    snap = _snapshot(m)
    xa = torch.from_numpy(vo.synth_pianoroll(B, H, 21).astype(np.float32)).cuda()
    xb = torch.from_numpy(vo.synth_pianoroll(B, H, 22).astype(np.float32)).cuda()
    xb[3] = xa[3]                                  # one pair of equal rolls: angle 0, the straight-line fall-back
    out = {mode: m.interpolate(xa, xb, steps, mode) for mode in ("slerp", "lerp")}
    again = m.interpolate(xa, xb, steps)
    _unchanged(m, snap, True)
    m.eval()
    with torch.no_grad():
        mu_a, mu_b = m.encode(xa)["mu"].cpu().numpy(), m.encode(xb)["mu"].cpu().numpy()
    for mode, (rolls, z) in out.items():
        assert rolls.shape == (B, steps, 1, H, H) and z.shape == (B, steps, L) and z.dtype == torch.float32
        err = float(np.abs(z.cpu().numpy() - _np_interp(mu_a, mu_b, steps, mode)).max())
        print(f"{dtype} {mode}: max |z - formula| = {err:.3g} (gate 1e-6), max |mu| = {np.abs(mu_a).max():.3g}")
        assert err <= 1e-6
        assert np.array_equal(z[:, 0].cpu().numpy(), mu_a) or mode == "slerp"
        with torch.no_grad():
            assert torch.equal(rolls.reshape(B * steps, 1, H, H), m.decode(z.view(-1, L)))
    assert torch.equal(again[0], out["slerp"][0]) and torch.equal(again[1], out["slerp"][1])
    assert not torch.equal(out["slerp"][1][:3], out["lerp"][1][:3]) and torch.equal(out["slerp"][1][3], out["lerp"][1][3])
    one = m.interpolate(xa, xb, 1)
    assert one[0].shape == (B, 1, 1, H, H) and np.abs(one[1][:, 0].cpu().numpy() - mu_a).max() <= 1e-6
    with pytest.raises(ValueError):
        m.interpolate(xa, xb[:2], steps)


class _Loader:
    def __init__(self, batches):
        self.batches = list(batches)

    def __iter__(self):
        return iter(self.batches)


def test_evaluate_note_events(capsys):
    H, L = 32, 16
    m = make_model(H, L, False, "f32", perturbed_params(L, H, 5, False))
    rolls = torch.from_numpy(vo.synth_pianoroll(12, H, 77).astype(np.float32))
    loader = _Loader((rolls[a:a + 4], torch.zeros(4, dtype=torch.long)) for a in (0, 4, 8))
    torch.manual_seed(5)
    base = evaluation.evaluate(loader, m, "cuda", verbosity=0)
    assert list(base) == ["count", "cross-entropy", "mse", "mae"]
    torch.manual_seed(5)
    assert evaluation.evaluate(loader, m, "cuda", verbosity=0, note_events=None) == base
    torch.manual_seed(5)                           # the same eps again: the model's own outputs, batch by batch in loader order
    m.eval()
    with torch.no_grad():
        rec = torch.cat([m(x.cuda())["output"] for x, _ in loader]).cpu().numpy()[:, 0]
    t = float(np.median(rec))
    cfg = dict(onset_threshold=t, sustain_threshold=0.98 * t, min_duration=2, max_gap=1, onset_tolerance=1, target_threshold=0.5)
    torch.manual_seed(5)
    res = evaluation.evaluate(loader, m, "cuda", verbosity=1, note_events=cfg)
    printed = capsys.readouterr().out
    keys = ["notes_pred", "notes_true", "matched", "note_precision", "note_recall", "note_f1"]
    assert list(res) == list(base) + keys and {k: res[k] for k in base} == base
    counts = [0, 0, 0]
    for a in (0, 4, 8):        # per batch, as evaluate() numbers the rolls
        pred = nr.extract(rec[a:a + 4], t, np.float32(0.98 * t), 2, 1)["events"]
        true = nr.extract(rolls[a:a + 4, 0].numpy(), 0.5, 0.5, 1, 0)["events"]
        got = nr.event_metrics(pred, true, 1)
        for i, k in enumerate(keys[:3]):
            counts[i] += got[k]
    want = nr.ratios(counts[0], counts[1], counts[2])
    assert {k: res[k] for k in keys} == want
    assert want["notes_pred"] > 0 and want["notes_true"] > 0
    assert "note_f1" in printed and "notes_pred" in printed
    # composes with the cell-level metrics; an unknown key is refused
    torch.manual_seed(5)
    both = evaluation.evaluate(loader, m, "cuda", verbosity=0, note_thresholds=0.5, note_events=cfg)
    assert {k: both[k] for k in keys} == want and "f1" in both
    with pytest.raises(ValueError):
        evaluation.evaluate(loader, m, "cuda", verbosity=0, note_events={"threshold": 0.5})
