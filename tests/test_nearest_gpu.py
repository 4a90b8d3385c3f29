"""The nearest-roll search on the GPU (vae_nearest_rolls; evaluation.nearest_rolls, novelty_summary, sample_novelty) against
tests/nearest_ref.py.  Every comparison is exact.  In the kernel tests queries and rolls are views into the middle of larger buffers
of 0xFF bytes and every output a view into a larger buffer pre-filled with a sentinel: a missing zero fill picks up ones and changes
a distance, a missing guard damages a sentinel - never a stray access."""
import functools

import numpy as np
import pytest
import torch

from tests import nearest_ref as nf
from tests.util import make_model, perturbed_params
from torch_vae_amd import _lib, data, evaluation, generation

pytestmark = pytest.mark.gpu

PAD = 1024                                   # bytes / slots of filler on either side of every buffer
IDX_S, I32_S = -99, -77
QT, CT = _lib.NEAREST_QUERY_TILE, _lib.NEAREST_CAND_TILE
OUTS = ("index", "distance", "shift", "intersection", "query_cells")


def embed(planes, shift=0):
    """uint8 planes on the device as a view into the middle of a buffer of 0xFF bytes, `shift` more bytes in front."""
    t = torch.from_numpy(np.array(planes, np.uint8))
    buf = torch.full((2 * PAD + shift + t.numel(),), 0xFF, dtype=torch.uint8)
    lo = PAD + shift
    buf[lo:lo + t.numel()] = t.reshape(-1)
    buf = buf.cuda()
    assert buf.data_ptr() % 16 == 0
    return buf[lo:lo + t.numel()].view(t.shape), buf, lo


def framed(numel, dtype, sentinel, shift_items=0):
    buf = torch.full((2 * PAD + shift_items + numel,), sentinel, dtype=dtype, device="cuda")
    lo = PAD + shift_items
    return buf[lo:lo + numel], buf, lo


def intact(buf, lo, numel, sentinel):
    host = buf.cpu()
    return bool((host[:lo] == sentinel).all()) and bool((host[lo + numel:] == sentinel).all())


def raw(q, r, P, T, k, *, exclude=None, splits=0, roll_shift=0, out_shift=0):
    """One call of the C entry point on embedded / framed buffers; host arrays after checking sources and every sentinel."""
    Q, h, wb = q.shape
    N = r.shape[0]
    qv, q_buf, q_lo = embed(q)
    rv, r_buf, r_lo = embed(r, roll_shift)
    assert qv.data_ptr() % 16 == 0 and rv.data_ptr() % 16 == roll_shift % 16
    ex = None if exclude is None else torch.tensor(exclude, dtype=torch.int64).cuda()
    out, frames = {}, {}
    for name, n, dt, s in (("index", Q * k, torch.int64, IDX_S), ("distance", Q * k, torch.int32, I32_S), ("shift", 2 * Q * k, torch.int32, I32_S),
                           ("intersection", Q * k, torch.int32, I32_S), ("query_cells", Q, torch.int32, I32_S)):
        v, buf, lo = framed(n, dt, s, 0 if name == "index" else out_shift)
        if name != "index" and out_shift:
            assert v.data_ptr() % 16 == 4 * out_shift
        out[name], frames[name] = v, (buf, lo, n, s)
    rc = _lib.lib().vae_nearest_rolls(qv.data_ptr(), Q, rv.data_ptr(), N, h, wb * 8, P, T, _lib.ptr(ex), k, splits,
                                      *(out[name].data_ptr() for name in OUTS), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().vae_last_error().decode()
    torch.cuda.synchronize()
    for buf, lo, planes in ((q_buf, q_lo, q), (r_buf, r_lo, r)):
        host = buf.cpu().numpy()
        assert (host[:lo] == 0xFF).all() and (host[lo + planes.size:] == 0xFF).all(), "the padding of a source was written"
        assert np.array_equal(host[lo:lo + planes.size], planes.reshape(-1)), "a source was written"
    for name, f in frames.items():
        assert intact(*f), f"{name} frame damaged"
    res = {name: out[name].cpu().numpy() for name in OUTS}
    res["shift"] = res["shift"].reshape(Q, k, 2)
    for name in ("index", "distance", "intersection"):
        res[name] = res[name].reshape(Q, k)
    return res


def same(got, ref, tag):
    for name in OUTS:
        np.testing.assert_array_equal(got[name], ref[name], err_msg=f"{tag} {name}")


def test_sweep():
    """The reference's sweep plus the tile edges: N and Q at and either side of the candidate and query tiles, k in (1, 4, 32) and
    k > N.  The witnesses are asserted over the sweep in total: without non-zero shifts, shift ties and index ties in the
    reference's own output the comparison would prove little."""
    rng = np.random.default_rng(0)
    cases = list(nf.sweep_cases())
    cases += [(5, 64, 2, 3, 4, n, 4) for n in (CT - 1, CT, CT + 1)] + [(16, 128, 2, 3, q, 20, 4) for q in (QT - 1, QT, QT + 1)]
    cases += [(5, 64, 1, 2, 6, 40, k) for k in (1, 4, 32)] + [(3, 32, 1, 1, 3, 2 * CT + 3, 32), (4, 96, 0, 0, 2 * QT + 1, 5, 32)]
    tot = {"nonzero_shift": 0, "shift_ties": 0, "index_ties": 0}
    for h, w, P, T, Q, N, k in cases:
        q, r = nf.make_case(rng, Q, N, h, w, P, T)
        ref = nf.search(q, r, P, T, k)
        same(raw(q, r, P, T, k), ref, f"{h}x{w} window ({P},{T}) Q={Q} N={N} k={k}")
        if (P, T) == (0, 0):
            assert ref["stats"]["nonzero_shift"] == 0
        for key in tot:
            tot[key] += ref["stats"][key]
    print(tot)
    assert min(tot.values()) > 20, tot


@functools.lru_cache(maxsize=None)
def _case(seed, Q, N, h, w, P, T, k):
    q, r = nf.make_case(np.random.default_rng(seed), Q, N, h, w, P, T)
    ref = nf.search(q, r, P, T, k)
    for a in (q, r, *ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q, r, ref


@pytest.mark.parametrize("roll_shift,out_shift", [(4, 0), (0, 1), (12, 3)])
def test_alignment(roll_shift, out_shift):
    """The rolls' base moved by 4 bytes (no 16-byte loads then); the int32 outputs at a 4-byte but not 16-byte offset."""
    q, r, ref = _case(1, 5, 19, 16, 128, 2, 3, 4)
    same(raw(q, r, 2, 3, 4, roll_shift=roll_shift, out_shift=out_shift), ref, f"shift {roll_shift} / {out_shift}")
    q, r, ref = _case(2, 5, 19, 16, 128, 2, 0, 4)
    same(raw(q, r, 2, 0, 4, roll_shift=roll_shift, out_shift=out_shift), ref, f"T=0 shift {roll_shift} / {out_shift}")


def test_window_reaches_the_frame_small():
    """P = h - 1 and T = w - 1: every shift up to the one that leaves a single cell of the candidate in the frame."""
    q, r, ref = _case(3, 9, 20, 3, 32, 2, 31, 4)
    assert ref["stats"]["nonzero_shift"] > 0
    same(raw(q, r, 2, 31, 4), ref, "3x32 window (2,31)")
    q, r, ref = _case(4, 5, 7, 5, 64, 4, 40, 3)       # a time shift of more than one dword
    same(raw(q, r, 4, 40, 3), ref, "5x64 window (4,40)")


def test_the_workloads_own_augmentation_window():
    q, r, ref = _case(5, 9, 70, 128, 128, 6, 4, 4)
    assert ref["stats"]["nonzero_shift"] > 0 and ref["stats"]["shift_ties"] > 0
    same(raw(q, r, 6, 4, 4), ref, "128x128 window (6,4)")


@pytest.mark.parametrize("shape", [(128, 128, 2, 3, 9, 70, 4), (5, 64, 2, 3, 9, 5, 4), (5, 64, 2, 0, 9, 70, 32)])
def test_splits_give_the_same_bits(shape):
    """splits in (1, 2, 3, 7) and 0: bit-identical outputs, all equal to the reference; N = 5 < 7 leaves splits without a roll."""
    h, w, P, T, Q, N, k = shape
    q, r, ref = _case(6, Q, N, h, w, P, T, k)
    got = {s: raw(q, r, P, T, k, splits=s) for s in (1, 2, 3, 7, 0)}
    for s, g in got.items():
        same(g, ref, f"splits={s}")
        for name in OUTS:
            assert g[name].tobytes() == got[1][name].tobytes(), (s, name)
    again = raw(q, r, P, T, k)
    for name in OUTS:
        assert again[name].tobytes() == got[0][name].tobytes(), name


def test_exclude_entries():
    """Out-of-range and -1 entries exclude nothing; an entry in range leaves out exactly that roll."""
    q, r, ref = _case(7, 9, 20, 16, 128, 2, 3, 4)
    ex = [int(ref["index"][0, 0]), -1, 20, int(ref["index"][3, 1]), 2 ** 40, -2 ** 62, 0, 19, int(ref["index"][8, 0])]
    want = nf.search(q, r, 2, 3, 4, exclude=ex)
    assert want["index"][0, 0] != ref["index"][0, 0] and np.array_equal(want["index"][1], ref["index"][1])
    same(raw(q, r, 2, 3, 4, exclude=ex), want, "exclude")
    same(raw(q[:2], r[:1], 2, 3, 4, exclude=[0, 5]), nf.search(q[:2], r[:1], 2, 3, 4, exclude=[0, 5]), "every roll excluded")


def test_256x256_once():
    q, r, ref = _case(8, 3, 9, 256, 256, 1, 1, 4)
    same(raw(q, r, 1, 1, 4), ref, "256x256")


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def test_self_search_finds_planted_duplicates():
    rng = np.random.default_rng(9)
    cells = np.stack([nf.random_roll(rng, 16, 128) for _ in range(40)])
    cells[10], cells[25] = cells[2], nf.shifted(cells[7], 1, -2)
    planes = nf.pack(cells)
    ds = data.PianorollDataset(torch.from_numpy(cells), storage="bits")
    assert np.array_equal(ds.data.cpu().numpy(), planes)
    res = evaluation.nearest_rolls(ds, ds, 2, max_pitch_shift=1, max_time_shift=2, exclude="self")
    got = host(res)
    ref = nf.search(planes, planes, 1, 2, 2, exclude=np.arange(40))
    same(got, ref, "self")
    assert (got["index"] != np.arange(40)[:, None]).all()
    for a, b in ((2, 10), (10, 2)):
        assert got["index"][a, 0] == b and got["distance"][a, 0] == 0 and tuple(got["shift"][a, 0]) == (0, 0)
    lost = int(cells[7].sum() - cells[25].sum())             # what the plant pushed out of the frame stays lost on the way back
    assert got["index"][25, 0] == 7 and got["distance"][25, 0] == 0 and tuple(got["shift"][25, 0]) == (1, -2)
    assert got["index"][7, 0] == 25 and got["distance"][7, 0] == lost and tuple(got["shift"][7, 0]) == (-1, 2)
    # without the exclusion every roll finds itself first
    plain = host(evaluation.nearest_rolls(ds, ds, 1))
    assert np.array_equal(plain["index"][:, 0], np.minimum(np.arange(40), np.where(np.arange(40) == 10, 2, 40)))
    assert (plain["distance"] == 0).all() and (plain["jaccard"] == 1.0).all()


def test_python_layer():
    q, r, ref = _case(10, 9, 20, 16, 128, 2, 3, 4)
    ds = data.PianorollDataset.from_stored(torch.from_numpy(np.array(r)).cuda(), "bits")
    kw = dict(max_pitch_shift=2, max_time_shift=3)
    res = evaluation.nearest_rolls(torch.from_numpy(np.array(q)).cuda(), ds, 4, **kw)
    assert res["index"].dtype == torch.int64 and res["jaccard"].dtype == torch.float64 and res["shift"].shape == (9, 4, 2)
    assert all(v.is_cuda for v in res.values())
    got = host(res)
    same(got, ref, "planes")
    np.testing.assert_array_equal(got["neighbour_cells"], ref["neighbour"].sum(axis=(2, 3)))
    inter, union = ref["intersection"].astype(np.float64), (ref["distance"] + ref["intersection"]).astype(np.float64)
    np.testing.assert_array_equal(got["jaccard"], np.where(union > 0, inter / np.maximum(union, 1.0), 1.0))
    assert (got["jaccard"][7] == [1.0, 0.0, 0.0, 0.0]).all()          # the empty query: roll 0 is empty too, the others are not
    # float32 rolls go through binarize_rolls, [Q,h,w] or [Q,1,h,w]; 0.7 is a cell at threshold 0.6, not at 0.8
    cells = torch.from_numpy(nf.unpack(q).astype(np.float32) * 0.7).cuda()
    for x in (cells, cells.view(9, 1, 16, 128)):
        same(host(evaluation.nearest_rolls(x, ds, 4, threshold=0.6, **kw)), ref, "float32")
    assert int(evaluation.nearest_rolls(cells, ds, 4, threshold=0.8, **kw)["query_cells"].sum()) == 0
    # a dataset as queries; k beyond the dataset; no queries at all
    qds = data.PianorollDataset.from_stored(torch.from_numpy(np.array(q)).cuda(), "bits")
    same(host(evaluation.nearest_rolls(qds, ds, 4, **kw)), ref, "dataset")
    wide = host(evaluation.nearest_rolls(qds, ds, 32, **kw))
    assert (wide["index"][:, 20:] == -1).all() and (wide["distance"][:, 20:] == -1).all() and np.isnan(wide["jaccard"][:, 20:]).all()
    assert (wide["neighbour_cells"][:, 20:] == 0).all() and np.array_equal(wide["index"][:, :4], ref["index"])
    none = evaluation.nearest_rolls(torch.zeros(0, 16, 16, dtype=torch.uint8, device="cuda"), ds, 3)
    assert none["index"].shape == (0, 3) and evaluation.novelty_summary(none)["count"] == 0
    ex = torch.tensor([int(ref["index"][i, 0]) for i in range(9)], device="cuda")
    shut = host(evaluation.nearest_rolls(qds, ds, 4, exclude=ex, **kw))
    same(shut, nf.search(q, r, 2, 3, 4, exclude=ex.tolist()), "exclude tensor")
    with pytest.raises(ValueError):
        evaluation.nearest_rolls(qds, ds, 4, exclude=ex[:5])
    with pytest.raises(ValueError):
        evaluation.nearest_rolls(torch.zeros(2, 16, 8, dtype=torch.uint8, device="cuda"), ds)
    with pytest.raises(_lib.VaeLibError, match="max_pitch_shift must be in 0..h-1"):
        evaluation.nearest_rolls(qds, ds, max_pitch_shift=16)
    s = evaluation.novelty_summary(res)
    assert s == evaluation.novelty_summary({k: v.cpu() for k, v in res.items()}) and s["count"] == 9 and s["without_neighbour"] == 0


def test_sample_novelty():
    """An untrained model's decoded values sit in a narrow band that 0.5 need not cut, so the extraction threshold is lowered (or
    raised) to the median of a probe batch: about half the cells sound, and no sample is empty."""
    H, L, B = 32, 16, 8
    m = make_model(H, L, False, "f32", perturbed_params(L, H, 3, False))
    t = float(m.sample_notes(B, seed=11, return_rolls=True)["rolls"].median())
    rng = np.random.default_rng(11)
    train = data.PianorollDataset(torch.from_numpy(np.stack([nf.random_roll(rng, H, H, 0.3) for _ in range(12)])), storage="bits")
    kw = dict(seed=11, k=2, max_pitch_shift=1, max_time_shift=1, onset_threshold=t)
    summary, near, notes = evaluation.sample_novelty(m, train, B, **kw)
    planes = notes["cleaned"].cpu().numpy()
    assert planes.shape == (B, H, H // 8) and (nf.unpack(planes).sum(axis=(1, 2)) > 0).all()
    ref = nf.search(planes, train.data.cpu().numpy(), 1, 1, 2)
    same(host(near), ref, "sample_novelty")
    want = evaluation.novelty_summary(evaluation._nearest_result(*(torch.from_numpy(ref[name]) for name in OUTS)))
    assert summary == want and summary["count"] == B
    summary2, near2, notes2 = evaluation.sample_novelty(m, train, B, **kw)
    assert summary2 == summary and all(torch.equal(near[k], near2[k]) for k in OUTS) and torch.equal(notes["cleaned"], notes2["cleaned"])
    # a "training set" of the model's own samples, transposed by two rows: every sample is a copy, found only inside the window.
    # Two of the 32 rows leave the frame with about a sixteenth of the cells, so the copies sit near jaccard 15/16, above the
    # default bar of 0.9
    params = torch.tensor([[2, 0]] * B, dtype=torch.int32, device="cuda")
    moved = generation.binarize_rolls(data.gather_rolls(notes["cleaned"], "bits", H, batch=B, params=params))
    own = data.PianorollDataset.from_stored(moved, "bits")
    inside, near_in, _ = evaluation.sample_novelty(m, own, B, seed=11, max_pitch_shift=2, onset_threshold=t)
    outside, near_out, _ = evaluation.sample_novelty(m, own, B, seed=11, max_pitch_shift=0, onset_threshold=t)
    print(inside, outside, near_in["jaccard"][:, 0].tolist(), near_out["jaccard"][:, 0].tolist())
    assert inside["copies"] == 1.0 and inside["shifted_copies"] == 1.0
    assert outside["copies"] < inside["copies"] and outside["shifted_copies"] == 0.0
