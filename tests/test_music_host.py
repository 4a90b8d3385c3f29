"""Host side (no GPU) of the musical-statistics tests: the numpy reference (tests/music_ref.py) against identities and hand-made rolls
with known answers, its summary / compare functions, the refusals of include/vae_music.h through fake, never dereferenced
pointers, the header / export bookkeeping, the coverage the GPU cases must have, and the argument checks of the Python layer."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import music_ref as R
from tests import test_music_gpu as gpu_cases
from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_music.h")
P = 4096          # a fake device address, 16-byte aligned
C = R.COL


def one(cells, off=0):
    return R.roll_features(np.asarray(cells, dtype=np.uint8), off)


def blk(f, name):
    return f[C[name]:C[name] + R.WIDTH[name]].tolist()


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in R.gpu_cases() if k[2] != 3], ids=str)
def test_reference_identities(key):
    h, w, n, off = key
    for f in R.gpu_cases()[key][1].astype(np.int64):
        assert sum(blk(f, "pc_cells")) == f[C["cells"]]
        assert sum(blk(f, "pc_notes")) == f[C["notes"]] == sum(blk(f, "duration"))
        assert sum(blk(f, "polyphony")) == w
        assert sum(blk(f, "ioi")) == max(f[C["onset_steps"]] - 1, 0)
        assert f[C["rolls"]] == 1 and f[C["nonempty"]] == (f[C["cells"]] > 0) and f[74] == f[75] == 0
        assert f[C["sounding_steps"]] == w - f[C["polyphony"]]
        assert (f[C["lowest"]] < 0) == (f[C["highest"]] < 0) == (f[C["cells"]] == 0)


def test_empty_roll():
    f = one(np.zeros((5, 64)))
    want = np.zeros(R.F, dtype=np.int64)
    want[C["rolls"]], want[C["lowest"]], want[C["highest"]], want[C["polyphony"]] = 1, -1, -1, 64
    assert f.tolist() == want.tolist()


def test_full_row_is_one_note():
    cells = np.zeros((13, 64), np.uint8)
    cells[7] = 1
    f = one(cells, off=21)
    assert (f[C["cells"]], f[C["notes"]], f[C["used_pitches"]], f[C["lowest"]], f[C["highest"]]) == (64, 1, 1, 7, 7)
    assert (f[C["sounding_steps"]], f[C["onset_steps"]], f[C["max_polyphony"]]) == (64, 1, 1)
    assert blk(f, "duration") == [0] * 6 + [1] + [0] * 5            # 64 = 2^6
    assert blk(f, "pc_cells")[(7 + 21) % 12] == 64 and blk(f, "pc_notes")[(7 + 21) % 12] == 1
    assert blk(f, "polyphony")[1] == 64 and sum(blk(f, "ioi")) == 0


def test_alternating_bits():
    cells = np.zeros((3, 32), np.uint8)
    cells[1, 0::2] = 1
    f = one(cells)
    assert (f[C["cells"]], f[C["notes"]], f[C["onset_steps"]], f[C["sounding_steps"]]) == (16, 16, 16, 16)
    assert blk(f, "duration") == [16] + [0] * 11
    assert blk(f, "ioi") == [0, 15] + [0] * 10                        # every gap is 2 steps: bucket floor(log2 2) = 1
    assert blk(f, "polyphony")[:2] == [16, 16]
    cells[2, 1::2] = 1                                                # the other row fills the odd steps: an onset on every step
    f = one(cells)
    assert blk(f, "ioi") == [31] + [0] * 11 and f[C["onset_steps"]] == 32


def test_notes_across_word_boundaries():
    cells = np.zeros((2, 288), np.uint8)
    cells[0, 30:34] = 1                       # across the 32-bit boundary at 32
    cells[1, 120:140] = 1                     # across the 128-bit boundary at 128
    cells[1, 255:257] = 1                     # and the one at 256
    f = one(cells)
    assert (f[C["cells"]], f[C["notes"]]) == (4 + 20 + 2, 3)
    assert blk(f, "duration") == [0, 1, 1, 0, 1] + [0] * 7            # lengths 2, 4, 20
    assert f[C["onset_steps"]] == 3
    assert blk(f, "ioi") == [0] * 6 + [1, 1] + [0] * 4                # 120 - 30 = 90 (bucket 6), 255 - 120 = 135 (bucket 7)


def test_a_note_at_either_edge_is_a_note():
    cells = np.zeros((1, 64), np.uint8)
    cells[0, :3] = 1
    cells[0, 61:] = 1
    f = one(cells)
    assert (f[C["notes"]], f[C["onset_steps"]]) == (2, 2) and blk(f, "duration")[1] == 2 and blk(f, "ioi")[5] == 1   # gap 61


def test_column_of_twenty_cells():
    cells = np.zeros((24, 32), np.uint8)
    cells[2:22, 5] = 1
    cells[0, 9] = 1
    f = one(cells)
    assert f[C["max_polyphony"]] == 20 and blk(f, "polyphony") == [30, 1] + [0] * 13 + [1]
    assert (f[C["lowest"]], f[C["highest"]], f[C["used_pitches"]]) == (0, 21, 21)


def test_totals_rules():
    empty, a, b = np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8)
    a[1, :4] = 1
    b[2:4, 7] = 1
    feats = np.stack([one(c) for c in (empty, a, b)])
    t = R.totals(feats)
    assert (t[C["rolls"]], t[C["nonempty"]], t[C["cells"]], t[C["lowest"]], t[C["highest"]], t[C["max_polyphony"]]) == (3, 2, 6, 1, 3, 2)
    first = R.totals(feats[:1])
    assert (first[C["lowest"]], first[C["highest"]], first[C["max_polyphony"]]) == (-1, -1, 0)
    assert R.totals(feats[1:], into=first).tolist() == t.tolist()      # -1 means "none yet"


# ---- summary and compare ------------------------------------------------------------------------------------------------------------
def c_major_roll():
    cells = np.zeros((24, 32), np.uint8)
    for p in (0, 2, 4, 5, 7, 9, 11, 12, 14):
        cells[p, p:p + 3] = 1
    return cells


def test_identical_sets():
    feats = R.gpu_cases()[(13, 64, 67, 0)][1]
    c = R.compare(feats, feats)
    for name in R.DISTRIBUTIONS:
        assert c[f"js_{name}"] == 0.0 and c[f"overlap_{name}"] == pytest.approx(1.0, abs=1e-15)
    for name in R.SCALARS:
        assert c[f"w1_{name}"] == 0.0 and c[f"mean_{name}_a"] == c[f"mean_{name}_b"]


def test_disjoint_pitch_classes():
    a, b = np.zeros((12, 32), np.uint8), np.zeros((12, 32), np.uint8)
    a[0, :8] = 1
    a[4, 3] = 1
    b[7, 20:22] = 1
    c = R.compare(one(a), one(b))
    assert c["js_pitch_class"] == pytest.approx(1.0, abs=1e-15) and c["overlap_pitch_class"] == 0.0
    assert c["js_pitch_class_onsets"] == pytest.approx(1.0, abs=1e-15)
    assert c["w1_cells"] == 7.0 and c["w1_notes"] == 1.0               # 9 cells against 2, 2 notes against 1


def test_c_major():
    s = R.summary(one(c_major_roll()), 24, 32)
    assert s["scale_consistency"] == 1.0 and s["key"] == 0
    s = R.summary(one(c_major_roll(), off=7), 24, 32)                   # row 0 is a G: G major
    assert s["scale_consistency"] == 1.0 and s["key"] == 7
    chromatic = np.zeros((12, 32), np.uint8)
    chromatic[:, 0] = 1
    s = R.summary(one(chromatic), 12, 32)
    assert s["scale_consistency"] == pytest.approx(7 / 12) and s["key"] == 0       # every root ties: the lowest wins
    assert s["pitch_class_entropy"] == pytest.approx(math.log2(12))


def test_summary_numbers():
    cells = np.zeros((3, 4, 32), np.uint8)
    cells[0, 1, :4] = 1
    cells[0, 3, 2:4] = 1
    cells[1, 2, 8] = 1
    s = R.summary(R.features(R.pack(cells)), 4, 32)
    assert s["rolls"] == 3 and s["empty_roll_rate"] == pytest.approx(1 / 3) and s["notes_per_roll"] == 1.0
    assert s["note_density"] == pytest.approx(7 / (3 * 4 * 32)) and s["mean_duration"] == pytest.approx(7 / 3)
    assert s["mean_polyphony"] == pytest.approx(7 / 5) and s["empty_step_rate"] == pytest.approx(91 / 96)
    assert s["used_pitches"] == 1.5 and s["pitch_range"] == 2.0        # (3 + 1) / 2 over the two non-empty rolls
    assert sum(s["duration"]) == pytest.approx(1.0) and s["duration"][:3] == [pytest.approx(1 / 3)] * 3


def test_empty_side_is_nan():
    empty, some = R.features(R.pack(np.zeros((2, 4, 32), np.uint8))), one(c_major_roll())
    s = R.summary(empty, 4, 32)
    for k in ("notes_per_roll", "note_density", "empty_roll_rate"):
        assert not math.isnan(s[k])
    for k in ("mean_duration", "mean_polyphony", "used_pitches", "pitch_range", "pitch_class_entropy", "scale_consistency"):
        assert math.isnan(s[k]), k
    assert s["key"] == -1 and all(math.isnan(v) for v in s["pitch_class"]) and s["polyphony"][0] == 1.0
    c = R.compare(empty, some)
    for name in ("pitch_class", "pitch_class_onsets", "duration", "ioi"):
        assert math.isnan(c[f"js_{name}"]) and math.isnan(c[f"overlap_{name}"])
    assert not math.isnan(c["js_polyphony"]) and c["mean_cells_a"] == 0.0 and math.isnan(c["scale_consistency_a"])
    none = R.compare(np.zeros((0, R.F), np.int32), some)
    assert math.isnan(none["mean_notes_a"]) and math.isnan(none["w1_notes"]) and math.isnan(none["js_polyphony"])


def test_package_host_math_matches_the_reference():
    """evaluation's host-side pieces (no device involved) against the numpy versions."""
    from torch_vae_amd import evaluation as E
    fa, fb = R.gpu_cases()[(13, 64, 67, 0)][1], R.gpu_cases()[(13, 64, 67, 21)][1][:40]
    ta, tb = R.totals(fa), R.totals(fb)
    for name, source in R.DISTRIBUTIONS.items():
        got, want = E._js_and_overlap(R.block(ta, source), R.block(tb, source)), R.js_overlap(R.block(ta, source), R.block(tb, source))
        np.testing.assert_allclose(got, want, rtol=1e-12)
    for name, values in R.per_roll(fa).items():
        got = E._wasserstein1(torch.from_numpy(values), torch.from_numpy(R.per_roll(fb)[name]))
        np.testing.assert_allclose(got, R.wasserstein1(values, R.per_roll(fb)[name]), rtol=1e-12)
    assert E._scale_consistency(R.block(ta, "pc_cells")) == R.scale_consistency(R.block(ta, "pc_cells"))
    assert {k: (s.start, s.stop - s.start) for k, s in E.MUSIC_COLUMNS.items()} == {k: (v, R.WIDTH.get(k, 1)) for k, v in C.items()}
    assert dict(E.MUSIC_DISTRIBUTIONS) == R.DISTRIBUTIONS and tuple(E.MUSIC_SCALARS) == R.SCALARS and tuple(E.MAJOR_SCALE) == R.MAJOR


# ---- what the GPU cases must cover (checked here, before anything is sent to a device) -------------------------------------------------
def test_gpu_cases_cover_every_column():
    cases = R.gpu_cases()
    for h, w in R.SHAPES:
        for n in R.COUNTS:
            for off in R.OFFSETS:
                assert (h, w, n, off) in cases
    feats = np.concatenate([f for _, f in cases.values()])
    assert [c for c in range(74) if not feats[:, c].any()] == []
    assert not feats[:, 74:].any()
    for name in ("duration", "polyphony", "ioi"):
        assert feats[:, C[name] + R.WIDTH[name] - 1].any(), name
    for (h, w, n, off), (planes, f) in cases.items():
        assert planes.shape == (n, h, w // 8) and f.shape == (n, R.F)
        if n >= 3:       # the all-zero and the all-ones roll
            assert (f[:, C["cells"]] == 0).any() and (f[:, C["cells"]] == h * w).any()
    assert gpu_cases.CASE_KEYS == list(cases)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def stats(L, planes=P, n=3, h=4, w=32, off=0, features=P, totals=P, accumulate=0):
    return L.vae_music_roll_stats(planes, n, h, w, off, features, totals, accumulate, None)


REFUSALS = {
    "null_planes": (lambda L: stats(L, planes=None), "null pointer (planes, features)"),
    "null_features": (lambda L: stats(L, features=None), "null pointer (planes, features)"),
    "negative_n": (lambda L: stats(L, n=-1), "n must be >= 0"),
    "h_0": (lambda L: stats(L, h=0), "h must be >= 1"),
    "w_0": (lambda L: stats(L, w=0), "w must be a positive multiple of 32"),
    "w_48": (lambda L: stats(L, w=48), "w must be a positive multiple of 32"),
    "w_negative": (lambda L: stats(L, w=-32), "w must be a positive multiple of 32"),
    "roll_8224_bytes": (lambda L: stats(L, h=257, w=256), "a roll (h * w / 8 bytes) must fit 8192 bytes"),
    "roll_wide": (lambda L: stats(L, h=1, w=65568), "a roll (h * w / 8 bytes) must fit 8192 bytes"),
    "pitch_offset_negative": (lambda L: stats(L, off=-1), "pitch_offset must be in 0..2^20"),
    "pitch_offset_above_2^20": (lambda L: stats(L, off=(1 << 20) + 1), "pitch_offset must be in 0..2^20"),
    "n_above_2^40_features": (lambda L: stats(L, n=(1 << 40) // 76 + 1), "n * 76 features must stay within 2^40"),
    "planes_plus_2": (lambda L: stats(L, planes=P + 2), "planes and features must be 4-byte aligned"),
    "features_plus_1": (lambda L: stats(L, features=P + 1), "planes and features must be 4-byte aligned"),
    "totals_plus_4": (lambda L: stats(L, totals=P + 4), "totals must be 8-byte aligned"),
    "refused_with_n_0_too": (lambda L: stats(L, n=0, w=40), "w must be a positive multiple of 32"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = REFUSALS[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == "vae_music_roll_stats: " + want


def test_limits_are_accepted_up_to_the_refusal():
    """(nothing is launched: n = 0 without totals returns before any device work)"""
    L = _lib.lib()
    assert stats(L, n=0, h=256, w=256, off=1 << 20, totals=None) == 0
    assert stats(L, n=0, h=1, w=65536, totals=None, accumulate=1) == 0
    assert stats(L, n=0, h=2048, w=32, totals=P, accumulate=1) == 0


# ---- the header, the exports and the stream-case table ------------------------------------------------------------------------------
def _header(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def test_header_declares_exactly_the_music_exports():
    declared = set(re.findall(r"\b(vae_[a-z0-9_]+)\s*\(", _header(HEADER)))
    assert declared == set(_lib.MUSIC_EXPORTS) == {"vae_music_roll_stats"}
    assert all(n.startswith("vae_music_") for n in _lib.MUSIC_EXPORTS)
    L = _lib.lib()
    assert not [n for n in _lib.MUSIC_EXPORTS if not hasattr(L, n)]
    assert not set(_lib.MUSIC_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.MIXTURE_EXPORTS))
    assert L.vae_abi_version() == 1
    assert int(re.search(r"#define VAE_MUSIC_FEATURES (\d+)", open(HEADER).read()).group(1)) == _lib.MUSIC_FEATURES == R.F


def test_the_other_headers_declare_no_music_function():
    for name in ("vae_step.h", "vae_mixture.h"):
        assert "vae_music_" not in _header(os.path.join(ROOT, "include", name)), name


def stream_entry_points():
    found = [m.group(1) for m in re.finditer(r"\b(vae_\w+)\s*\(([^;{}]*?)\)\s*;", _header(HEADER)) if re.search(r"\bvae_stream_t\b", m.group(2))]
    assert len(found) == len(set(found))
    return found


def test_every_stream_entry_point_of_the_header_has_a_stream_case():
    """The rule of tests/test_streams_host.py on the new header and its own case table: every function of include/vae_music.h that
    takes a stream is called by a sync-free case of tests/test_music_gpu.py, and `covers` names calls the module really makes."""
    names = stream_entry_points()
    assert sorted(names) == sorted(_lib.MUSIC_EXPORTS)
    covered = set()
    for c in gpu_cases.STREAM_CASES:
        assert c.sync_free and c.reads_back is None, c.name
        covered |= set(c.covers)
    assert not [n for n in names if n not in covered]
    assert not [n for n in covered if n not in names]
    called = {a or b for a, b in re.findall(r"lib\(\)\.(vae_\w+)\(|L_\.(vae_\w+)\(", inspect.getsource(gpu_cases))}
    for c in gpu_cases.STREAM_CASES:
        assert not [n for n in c.covers if n not in called], c.name
    all_names = [c.name for c in gpu_cases.STREAM_CASES + gpu_cases.PY_STREAM_CASES]
    assert len(set(all_names)) == len(all_names)
    for c in gpu_cases.PY_STREAM_CASES:
        assert c.sync_free and c.reads_back is None, c.name      # music_statistics and the accumulator read nothing back


# ---- Python argument checks (all raised before anything touches a device) ------------------------------------------------------------
def test_python_argument_checks():
    from torch_vae_amd.evaluation import MusicStatsAccumulator, music_statistics, sample_music_stats
    planes = torch.zeros(2, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="must be on the GPU"):
        music_statistics(planes)
    with pytest.raises(TypeError, match="tensor or a PianorollDataset"):
        music_statistics(planes.numpy())
    for bad in (-1, (1 << 20) + 1, 1.5, True):
        with pytest.raises(ValueError, match="pitch_offset"):
            music_statistics(planes, pitch_offset=bad)
        with pytest.raises(ValueError, match="pitch_offset"):
            MusicStatsAccumulator(pitch_offset=bad)
    with pytest.raises(RuntimeError, match="update"):
        MusicStatsAccumulator().compute()
    with pytest.raises(TypeError, match="PianorollDataset"):
        sample_music_stats(None, planes, 4)


def test_python_shape_checks():
    from torch_vae_amd.evaluation import music_statistics
    for shape, dtype, err, word in (((2, 4, 4), torch.int32, TypeError, "uint8 bit planes or float32"),
                                    ((2, 4), torch.uint8, ValueError, r"\[n, h, w/8\]"),
                                    ((2, 4, 5), torch.uint8, ValueError, "multiple of 32"),
                                    ((2, 0, 4), torch.uint8, ValueError, "at least one pitch row"),
                                    ((2, 257, 32), torch.uint8, ValueError, "8224 bytes"),
                                    ((2, 4, 48), torch.float32, ValueError, "multiple of 32"),
                                    ((2, 2, 4, 32), torch.float32, ValueError, r"\[n, 1, h, w\]"),
                                    ((4, 32), torch.float32, ValueError, r"\[n, h, w\]"),
                                    ((1, 512, 256), torch.float32, ValueError, "16384 bytes")):
        with pytest.raises(err, match=word):
            music_statistics(torch.zeros(*shape, dtype=dtype))
    with pytest.raises(ValueError, match="must be on the GPU"):
        music_statistics(torch.zeros(2, 4, 32))
