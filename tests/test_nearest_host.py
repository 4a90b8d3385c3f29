"""Host side of the nearest-roll search (torch_vae_amd/evaluation.py: nearest_rolls, novelty_summary; vae_nearest_rolls): the numpy
reference pinned against a second statement of the pair distance (tests/augment_ref.gather) and against hand-made cases, the argument
refusals of the entry point (fake, never dereferenced addresses: every check comes before anything is enqueued), the Python-side
refusals and novelty_summary on hand-built CPU tensors."""
import os

import numpy as np
import pytest
import torch

from tests import nearest_ref as nf
from torch_vae_amd import _lib, data, evaluation

A = 4096          # a fake device address, 16-byte aligned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_against_the_gather_statement():
    rng = np.random.default_rng(0)
    seen = {"nonzero_shift": 0, "shift_ties": 0}
    for h, w, P, T in ((1, 32, 0, 2), (3, 32, 2, 3), (5, 64, 1, 2), (4, 96, 2, 0), (3, 32, 2, 31)):
        q, r = nf.make_case(rng, 5, 6, h, w, P, T)
        ref = nf.search(q, r, P, T, k=6)
        qc, rc = nf.unpack(q), nf.unpack(r)
        for i in range(5):
            for s in range(6):
                j = ref["index"][i, s]
                d, shift, inter = nf.pair_by_gather(qc[i], rc[j], P, T)
                assert (d, shift, inter) == (ref["distance"][i, s], tuple(ref["shift"][i, s]), ref["intersection"][i, s]), (h, w, P, T, i, j)
                assert ref["neighbour"][i, s].sum() == d + 2 * inter - ref["query_cells"][i]
        for key in seen:
            seen[key] += ref["stats"][key]
    assert min(seen.values()) > 20, seen


def test_reference_sweep_witnesses():
    """The generator's cases hold what the GPU sweep relies on: over the sweep in total, many non-zero shifts, shift ties and index ties."""
    rng = np.random.default_rng(0)
    tot = {"nonzero_shift": 0, "shift_ties": 0, "index_ties": 0}
    for h, w, P, T, Q, N, k in nf.sweep_cases():
        st = nf.search(*nf.make_case(rng, Q, N, h, w, P, T), P, T, k)["stats"]
        if (P, T) == (0, 0):
            assert st["nonzero_shift"] == 0
        for key in tot:
            tot[key] += st[key]
    assert min(tot.values()) > 20, tot


def _roll(h, w, cells):
    c = np.zeros((h, w), np.uint8)
    for y, x in cells:
        c[y, x] = 1
    return c


def test_hand_made_cases():
    h, w, P, T = 6, 32, 2, 3
    base = _roll(h, w, [(2, 5), (2, 6), (3, 10), (1, 20), (4, 31), (0, 0)])
    empty = np.zeros((h, w), np.uint8)
    # an empty candidate: every shift ties and (0, 0) wins; the distance is the query's cell count
    ref = nf.search(nf.pack(base[None]), nf.pack(empty[None]), P, T)
    assert ref["distance"][0, 0] == 6 and tuple(ref["shift"][0, 0]) == (0, 0) and ref["intersection"][0, 0] == 0
    assert ref["stats"]["shift_ties"] == 1
    # a duplicate roll: the lower index first
    other = _roll(h, w, [(5, 5)])
    ref = nf.search(nf.pack(base[None]), nf.pack(np.stack([other, base, empty, base])), 0, 0, k=3)
    assert ref["index"][0].tolist() == [1, 3, 2] and ref["distance"][0].tolist() == [0, 0, 6]
    # a copy shifted by (P, -T) is found at distance 0 with that shift - when nothing leaves the frame
    inner = _roll(h, w, [(2, 5), (2, 6), (3, 10), (1, 20)])
    q = nf.shifted(inner, P, -T)
    assert q.sum() == inner.sum()
    ref = nf.search(nf.pack(q[None]), nf.pack(inner[None]), P, T)
    assert ref["distance"][0, 0] == 0 and tuple(ref["shift"][0, 0]) == (P, -T) and ref["intersection"][0, 0] == 4
    # one row further is outside the window
    ref = nf.search(nf.pack(nf.shifted(inner, P + 1, 0)[None]), nf.pack(inner[None]), P, T)
    assert ref["distance"][0, 0] > 0
    # cells shifted out of the frame are lost: against the query that kept them, the distance is the number lost
    q = nf.shifted(base, -1, 1)          # (0, 0) leaves at the top, (4, 31) at the right
    assert q.sum() == 4
    ref = nf.search(nf.pack(q[None]), nf.pack(base[None]), P, T)
    assert ref["distance"][0, 0] == 0 and tuple(ref["shift"][0, 0]) == (-1, 1)
    ref = nf.search(nf.pack(base[None]), nf.pack(q[None]), P, T)      # the other way round the two cells stay lost
    assert ref["distance"][0, 0] == 2 and tuple(ref["shift"][0, 0]) == (1, -1) and ref["intersection"][0, 0] == 4
    # exclude leaves out exactly that roll; k > N leaves -1 slots
    rolls = nf.pack(np.stack([other, base, empty, base]))
    ref = nf.search(nf.pack(np.stack([base, base])), rolls, 0, 0, k=5, exclude=[1, 7])
    assert ref["index"].tolist() == [[3, 2, 0, -1, -1], [1, 3, 2, 0, -1]]
    assert ref["distance"][0].tolist() == [0, 6, 7, -1, -1] and ref["intersection"][0].tolist() == [6, 0, 0, 0, 0]
    assert ref["shift"][0, 3:].tolist() == [[0, 0], [0, 0]]


def near(L, queries=A, nq=2, rolls=A, n=5, h=4, w=32, P=0, T=0, exclude=None, k=1, splits=0, index=A, distance=A, shift=A, inter=A,
         cells=A):
    return L.vae_nearest_rolls(queries, nq, rolls, n, h, w, P, T, exclude, k, splits, index, distance, shift, inter, cells, None)


NULL = "null pointer (queries, rolls, index, distance, shift, intersection, query_cells)"
W32 = "w must be a positive multiple of 32"
PS = "max_pitch_shift must be in 0..h-1"
TS = "max_time_shift must be in 0..w-1"
A4 = "distance, shift, intersection and query_cells must be 4-byte aligned"
CASES = {
    "null_queries": (lambda L: near(L, queries=None), NULL),
    "null_rolls": (lambda L: near(L, rolls=None), NULL),
    "null_index": (lambda L: near(L, index=None), NULL),
    "null_distance": (lambda L: near(L, distance=None), NULL),
    "null_shift": (lambda L: near(L, shift=None), NULL),
    "null_intersection": (lambda L: near(L, inter=None), NULL),
    "null_query_cells": (lambda L: near(L, cells=None), NULL),
    "n_queries_-1": (lambda L: near(L, nq=-1), "n_queries must be >= 0"),
    "n_rolls_0": (lambda L: near(L, n=0), "n_rolls must be in 1..2^40"),
    "n_rolls_2^40+1": (lambda L: near(L, n=2 ** 40 + 1), "n_rolls must be in 1..2^40"),
    "h_0": (lambda L: near(L, h=0), "h must be >= 1"),
    "w_0": (lambda L: near(L, w=0), W32),
    "w_48": (lambda L: near(L, w=48), W32),
    "w_-32": (lambda L: near(L, w=-32), W32),
    "roll_8196_bytes": (lambda L: near(L, h=2049, w=32), "a roll (h * w / 8 bytes) must fit 8192 bytes"),
    "roll_256x288": (lambda L: near(L, h=256, w=288), "a roll (h * w / 8 bytes) must fit 8192 bytes"),
    "P_-1": (lambda L: near(L, P=-1), PS),
    "P_h": (lambda L: near(L, P=4), PS),
    "T_-1": (lambda L: near(L, T=-1), TS),
    "T_w": (lambda L: near(L, T=32), TS),
    "shifts_1025": (lambda L: near(L, h=32, w=64, P=20, T=12), "(2 max_pitch_shift + 1) * (2 max_time_shift + 1) must be <= 1023"),
    "k_0": (lambda L: near(L, k=0), "k must be in 1..32"),
    "k_33": (lambda L: near(L, k=33), "k must be in 1..32"),
    "splits_-1": (lambda L: near(L, splits=-1), "splits must be in 0..64"),
    "splits_65": (lambda L: near(L, splits=65), "splits must be in 0..64"),
    "grid_2^31": (lambda L: near(L, nq=2 ** 31 - 1, splits=64), "query tiles * splits must stay below 2^31"),
    "queries_plus_2": (lambda L: near(L, queries=A + 2), "queries and rolls must be 4-byte aligned"),
    "rolls_plus_1": (lambda L: near(L, rolls=A + 1), "queries and rolls must be 4-byte aligned"),
    "index_plus_4": (lambda L: near(L, index=A + 4), "index and exclude must be 8-byte aligned"),
    "exclude_plus_4": (lambda L: near(L, exclude=A + 4), "index and exclude must be 8-byte aligned"),
    "distance_plus_2": (lambda L: near(L, distance=A + 2), A4),
    "shift_plus_1": (lambda L: near(L, shift=A + 1), A4),
    "intersection_plus_3": (lambda L: near(L, inter=A + 3), A4),
    "query_cells_plus_2": (lambda L: near(L, cells=A + 2), A4),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = CASES[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == "vae_nearest_rolls: " + want


def test_no_queries_and_the_caps_pass_every_check():
    """n_queries == 0 returns 0 and launches nothing, whatever else is asked within the limits: 256x256, 13 x 9 shifts and more, k = 32,
    64 splits."""
    L = _lib.lib()
    assert near(L, nq=0) == 0
    assert near(L, nq=0, h=256, w=256, P=6, T=4, k=32, splits=64, exclude=A + 8, queries=A + 4, index=A + 8, distance=A + 4) == 0
    assert near(L, nq=0, h=128, w=128, P=15, T=16) == 0          # 31 x 33 = 1023 shifts
    assert _lib.NEAREST_MAX_SHIFTS == 1023 >= 13 * 9 and _lib.NEAREST_MAX_ROLL_BYTES == 256 * 256 // 8
    assert (_lib.NEAREST_MAX_K, _lib.NEAREST_MAX_SPLITS) == (32, 64)


def test_exported():
    L = _lib.lib()
    assert "vae_nearest_rolls" in _lib.EXPORTS and hasattr(L, "vae_nearest_rolls")
    with open(os.path.join(ROOT, "include", "vae_step.h")) as f:
        header = f.read()
    assert "int vae_nearest_rolls(const uint8_t* queries /*[n_queries][h][w/8]*/, int n_queries," in header
    with open(os.path.join(ROOT, "torch_vae_amd", "csrc", "nearest_rolls.cuh")) as f:
        src = f.read()
    for name, value in (("NR_QUERY_TILE", _lib.NEAREST_QUERY_TILE), ("NR_CAND_TILE", _lib.NEAREST_CAND_TILE),
                        ("NR_TILE_ROLL_BYTES", _lib.NEAREST_TILE_ROLL_BYTES), ("NR_LARGE_TILE", _lib.NEAREST_LARGE_TILE),
                        ("NR_MAX_ROLL_BYTES", _lib.NEAREST_MAX_ROLL_BYTES),
                        ("NR_MAX_SHIFTS", _lib.NEAREST_MAX_SHIFTS), ("NR_MAX_K", _lib.NEAREST_MAX_K), ("NR_MAX_SPLITS", _lib.NEAREST_MAX_SPLITS)):
        assert f"constexpr int {name} = {value};" in src, name
    import torch_vae_amd
    for name in ("nearest_rolls", "novelty_summary", "sample_novelty"):
        assert name in torch_vae_amd.__all__ and getattr(torch_vae_amd, name) is getattr(evaluation, name)


def _host_dataset(n=3, h=4, w=32, storage="bits"):
    cells = torch.zeros(n, h, w // 8 if storage == "bits" else w, dtype=torch.uint8)
    return data.PianorollDataset.from_stored(cells, storage)


def test_python_refusals_need_no_device():
    ds = _host_dataset()
    with pytest.raises(TypeError, match="PianorollDataset"):
        evaluation.nearest_rolls(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="'bits' storage"):
        evaluation.nearest_rolls(ds, _host_dataset(storage="bytes"))
    with pytest.raises(ValueError, match="'bits' storage"):
        evaluation.nearest_rolls(_host_dataset(storage="bytes"), ds)
    with pytest.raises(ValueError, match="once per query tile"):          # host memory (what "pinned" storage is): refused, with the reason
        evaluation.nearest_rolls(ds, ds)
    with pytest.raises(ValueError, match="4x64"):
        evaluation.nearest_rolls(_host_dataset(w=64), ds)
    with pytest.raises(ValueError, match="5x32"):
        evaluation.nearest_rolls(_host_dataset(h=5), ds)
    with pytest.raises(ValueError, match="needs the dataset itself"):
        evaluation.nearest_rolls(_host_dataset(), ds, exclude="self")
    with pytest.raises(ValueError, match="exclude must be"):
        evaluation.nearest_rolls(ds, ds, exclude="other")
    for k in (0, -1, 33, 1.5, True):
        with pytest.raises(ValueError, match="k must be"):
            evaluation.nearest_rolls(ds, ds, k)
    with pytest.raises(ValueError, match="max_pitch_shift"):
        evaluation.nearest_rolls(ds, ds, max_pitch_shift=-1)
    with pytest.raises(ValueError, match="on the GPU"):
        evaluation.nearest_rolls(torch.zeros(1, 4, 4, dtype=torch.uint8), ds)
    with pytest.raises(ValueError, match="on the GPU"):
        evaluation.nearest_rolls(torch.zeros(1, 4, 32), ds)
    with pytest.raises(TypeError):
        evaluation.nearest_rolls(np.zeros((1, 4, 4), np.uint8), ds)


def _result(index, distance, shift, inter, cells):
    return evaluation._nearest_result(torch.tensor(index, dtype=torch.int64), torch.tensor(distance, dtype=torch.int32),
                                      torch.tensor(shift, dtype=torch.int32), torch.tensor(inter, dtype=torch.int32),
                                      torch.tensor(cells, dtype=torch.int32))


def test_novelty_summary_on_hand_built_tensors():
    # six queries, k = 2: an exact copy, a transposed copy at jaccard 0.9, a near miss (0.8), both empty (jaccard 1.0, distance 0),
    # a far one, and one with no neighbour at all
    res = _result(index=[[4, 1], [2, 0], [7, 3], [0, 5], [9, 8], [-1, -1]],
                  distance=[[0, 9], [2, 30], [4, 8], [0, 3], [30, 31], [-1, -1]],
                  shift=[[[0, 0], [1, 0]], [[-2, 0], [0, 0]], [[0, 1], [0, 0]], [[0, 0], [0, 0]], [[0, 0], [3, 3]], [[0, 0], [0, 0]]],
                  inter=[[10, 4], [18, 1], [16, 10], [0, 0], [0, 1], [0, 0]],
                  cells=[10, 19, 18, 0, 12, 7])
    assert res["jaccard"].dtype == torch.float64
    j = res["jaccard"]
    assert j[0, 0] == 1.0 and j[1, 0] == 18 / 20 and j[2, 0] == 16 / 20 and j[3, 0] == 1.0 and j[4, 0] == 0.0
    assert j[3, 1] == 0.0 and bool(torch.isnan(j[5]).all())
    assert res["neighbour_cells"].tolist() == [[10, 7], [19, 13], [18, 10], [0, 3], [18, 21], [0, 0]]
    s = evaluation.novelty_summary(res)
    assert s == {"count": 5, "without_neighbour": 1, "copies": 3 / 5, "shifted_copies": 1 / 5, "median_jaccard": 18 / 20,
                 "mean_distance": 36 / 5}
    assert evaluation.novelty_summary(res, copy_jaccard=0.8)["copies"] == 4 / 5
    assert evaluation.novelty_summary(res, copy_jaccard=0.8)["shifted_copies"] == 2 / 5
    assert evaluation.novelty_summary(res, copy_jaccard=1.0)["copies"] == 2 / 5
    four = {k: v[:4] for k, v in res.items()}                             # an even count: the median is the mean of the middle two
    assert evaluation.novelty_summary(four)["median_jaccard"] == (18 / 20 + 1.0) / 2
    none = {k: v[5:] for k, v in res.items()}
    assert evaluation.novelty_summary(none) == {"count": 0, "without_neighbour": 1, "copies": 0.0, "shifted_copies": 0.0,
                                                "median_jaccard": 0.0, "mean_distance": 0.0}
    with pytest.raises(ValueError):
        evaluation.novelty_summary(res, copy_jaccard=1.5)
