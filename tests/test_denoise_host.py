"""Host side (no GPU) of the denoising tests: the numpy reference (tests/denoise_ref.py) pinned on hand-built rows and on the random
roll the GPU test compares the kernel on; the refusals of include/vae_denoise.h through fake, never dereferenced pointers; the
header / export bookkeeping of both headers; the stream-case table of tests/test_denoise_gpu.py; and the argument checks of the
Python layer."""
import inspect
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests import denoise_ref as R
from tests import test_denoise_gpu as gpu_cases
from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_denoise.h")
STEP_HEADER = os.path.join(ROOT, "include", "vae_step.h")
OTHER_HEADERS = ("vae_step.h", "vae_mixture.h", "vae_music.h", "vae_fidelity.h", "vae_attributes.h")
P, Q, HID = 4096, 1 << 30, 1 << 40          # fake device addresses, 16-byte aligned and far apart


# ---- the reference on hand-built rows ------------------------------------------------------------------------------------------------
def drop_pattern(notes, k, h, w, seed, p_drop):
    """Which of ``notes`` [(p, t0, t1)] of the roll with counter k are dropped: the draw at the onset's counter, taken from the
    oracle's own counter_uniform (not from the reference under test)."""
    u = vo.counter_uniform((k * h + h) * w, seed, R.STREAM_DROP)
    return [bool(u[(k * h + p) * w + t0] < p_drop) for p, t0, _ in notes]


def hand_rows():
    """[1, 8, 128] and the notes [(p, t0, t1)] in it: a run ending at column 63, one starting at 64, one spanning 60..70, a run
    touching each end of the row, two runs one cell apart, a NaN cell inside what would be one run, a velocity cell exactly at the
    threshold next to one just below it."""
    x = np.zeros((1, 8, 128), np.float32)
    notes = []

    def put(p, t0, t1, v=1.0):
        x[0, p, t0:t1] = v
        notes.append((p, t0, t1))
    put(0, 50, 64); put(1, 64, 80); put(2, 60, 71); put(3, 0, 5); put(3, 120, 128); put(4, 10, 12); put(4, 13, 15)
    put(5, 20, 24); x[0, 5, 22] = np.nan; notes[-1:] = [(5, 20, 22), (5, 23, 24)]
    put(6, 30, 31, 0.5); x[0, 6, 31] = np.nextafter(np.float32(0.5), np.float32(0)); x[0, 6, 29] = 0.75; notes[-1:] = [(6, 29, 31)]
    put(7, 0, 128, 0.9)
    return x, notes


def test_runs_of_the_hand_built_rows():
    x, notes = hand_rows()
    with np.errstate(invalid="ignore"):
        on = x[0] >= np.float32(0.5)
    found = [(p, t0, t1) for p in range(8) for t0, t1 in R.row_runs(on[p])]
    assert found == sorted(notes)
    assert R.row_runs(np.zeros(8, bool)) == [] and R.row_runs(np.ones(8, bool)) == [(0, 8)]


DROP_SEEDS = (0, 1, 3)       # between them every note of the hand-built rows is dropped once and kept once (checked below)


def test_the_seeds_of_the_hand_built_rows_drop_and_keep_every_note():
    x, notes = hand_rows()
    patterns = [drop_pattern(sorted(notes), 9, 8, 128, seed, 0.5) for seed in DROP_SEEDS]
    assert all(any(col) and not all(col) for col in zip(*patterns)), patterns


@pytest.mark.parametrize("seed", DROP_SEEDS)
def test_note_dropout_is_per_note_on_hand_built_rows(seed):
    x, notes = hand_rows()
    notes = sorted(notes)
    assert R.roll_counter(0, 9, 4) == 9
    pattern = drop_pattern(notes, 9, 8, 128, seed, 0.5)
    info = {}
    out, hidden = R.corrupt_ref(x, p_drop=0.5, seed=seed, counter0=9, counter_stride=4, info=info)
    want = x.copy()
    hid = np.zeros(x.shape, bool)
    for (p, t0, t1), d in zip(notes, pattern):
        if d:
            want[0, p, t0:t1] = 0.0
            hid[0, p, t0:t1] = True
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))        # (bit patterns: the NaN cell is kept as it is)
    assert np.array_equal(hidden, np.packbits(hid, axis=-1)) and hidden.shape == (1, 8, 16)
    assert info["notes"] == len(notes) and info["dropped"] == sum(pattern) and info["kept"] == len(notes) - sum(pattern)
    assert info["crossing_dropped"] + info["crossing_kept"] == 2            # the run 60..70 and the full row
    # the cell just below the threshold is not part of the note and stays, the one exactly at it goes with its note
    assert out[0, 6, 31] == x[0, 6, 31] and (out[0, 6, 30] == 0.0) == pattern[notes.index((6, 29, 31))]
    # every probability of 0 draws nothing; p_drop = 1 drops every note and nothing else
    same, none = R.corrupt_ref(x, seed=seed)
    assert np.array_equal(same.view(np.uint32), x.view(np.uint32)) and not none.any()
    gone, _ = R.corrupt_ref(x, p_drop=1.0, seed=seed)
    with np.errstate(invalid="ignore"):
        assert not (gone >= np.float32(0.5)).any() and np.array_equal(np.isnan(gone), np.isnan(x)) and gone[0, 6, 31] == x[0, 6, 31]


def test_span_and_spurious_cells_on_hand_built_rows():
    x, _ = hand_rows()
    out, hidden = R.corrupt_ref(x, spans=[[60, 10]])
    want = x.copy(); want[0, :, 60:70] = 0.0
    hid = np.zeros(x.shape, bool); hid[0, :, 60:70] = True
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(hidden, np.packbits(hid, axis=-1))
    for spans, lo, hi in (([[-5, 10]], 0, 5), ([[120, 100]], 120, 128), ([[500, 4]], 0, 0), ([[-(1 << 31), (1 << 31) - 1]], 0, 0),
                          ([[3, -2]], 0, 0), ([[(1 << 31) - 1, (1 << 31) - 1]], 0, 0), ([[-4, 1000]], 0, 128)):
        out, hidden = R.corrupt_ref(x, spans=spans)
        want = x.copy(); want[0, :, lo:hi] = 0.0
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), spans
        assert int(np.unpackbits(hidden).sum()) == 8 * (hi - lo), spans
    # p_add = 1: every cell that is off (the NaN and the cell below the threshold too) and outside the span becomes add_value
    out, hidden = R.corrupt_ref(x, p_add=1.0, add_value=0.75, spans=[[0, 64]])
    with np.errstate(invalid="ignore"):
        off = ~(x[0] >= np.float32(0.5))
    assert (out[0, :, :64] == 0.0).all() and (out[0, :, 64:][off[:, 64:]] == np.float32(0.75)).all()
    assert np.array_equal(out[0, :, 64:][~off[:, 64:]], x[0, :, 64:][~off[:, 64:]])
    hid = np.zeros(x.shape, bool); hid[0, :, :64] = True; hid[0, :, 64:] = off[:, 64:]
    assert np.array_equal(hidden, np.packbits(hid, axis=-1))
    # an add_value below the threshold changes the value and not the on/off state: nothing is hidden by it
    _, hidden = R.corrupt_ref(x, p_add=1.0, add_value=0.25)
    assert not hidden.any()


def test_drawn_spans_are_inside_the_roll_and_wrap_like_the_counters():
    for w, lo, hi in ((8, 0, 8), (32, 4, 8), (128, 16, 32), (200, 200, 200), (64, 0, 0)):
        s = R.spans_ref(50, w, lo, hi, seed=3, counter0=(1 << 64) - 20, counter_stride=7)
        assert s.dtype == np.int32 and (s[:, 1] >= lo).all() and (s[:, 1] <= hi).all() and (s[:, 0] >= 0).all() and (s[:, 0] + s[:, 1] <= w).all()
        if 0 < lo < hi:
            assert len(set(s[:, 1].tolist())) > 1 and len(set(s[:, 0].tolist())) > 1
    # roll 3 of a batch that starts 20 below 2^64 with stride 7 has the counter 1: the same draw as roll 1 of a batch from 0
    a = R.spans_ref(4, 128, 16, 32, seed=3, counter0=(1 << 64) - 20, counter_stride=7)
    b = R.spans_ref(2, 128, 16, 32, seed=3)
    assert a[3].tolist() == b[1].tolist()
    u = vo.counter_uniform(6, 3, R.STREAM_SPAN)
    assert b[1].tolist() == [int(u[3] * (128 - (16 + int(u[2] * 17)) + 1)), 16 + int(u[2] * 17)]


@pytest.fixture(scope="module")
def random_case():
    return gpu_cases.random_roll_case()


def test_the_random_roll_carries_the_cases(random_case):
    """The counts a sketch of the same formulas gave when the issue was written: the reference disagrees with none of them, and it
    reports dropped and kept notes that cross a 64-column boundary - what the kernel's carry between words is tested on."""
    x, out, hidden, info = random_case
    assert x.shape == (4, 128, 128) and x.dtype == np.float32
    counts = {k: int(info[k]) for k in ("notes", "dropped", "crossing_dropped", "crossing_kept", "added")}
    assert counts == dict(notes=821, dropped=255, crossing_dropped=21, crossing_kept=49, added=488)
    assert info["crossing_dropped"] >= 1 and info["crossing_kept"] >= 1
    assert (info["spans"][:, 1] >= 16).all() and (info["spans"][:, 1] <= 32).all()
    assert hidden.shape == (4, 128, 16) and int(np.unpackbits(hidden).sum()) >= 488 + 128 * int(info["spans"][:, 1].sum())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def corrupt(L, clean=P, out=Q, hidden=HID, n=3, h=4, w=32, thr=0.5, p_drop=0.3, smin=2, smax=8, p_add=0.01, add=1.0, spans=None,
            seed=1, c0=0, cs=1):
    return L.vae_denoise_corrupt(clean, out, hidden, n, h, w, thr, p_drop, smin, smax, p_add, add, spans, seed, c0, cs, None)


def params(L, spans=P, n=3, w=32, smin=2, smax=8, seed=1, c0=0, cs=1):
    return L.vae_denoise_params(spans, n, w, smin, smax, seed, c0, cs, None)


NAN, INF = float("nan"), float("inf")
W_MSG, SPAN_MSG = "w must be a multiple of 8 in 8..2^20", "the span needs 0 <= span_min <= span_max <= w"
P_MSG, F_MSG = "p_drop and p_add must lie in [0, 1]", "threshold and add_value must be finite"
ALIGN, OVER = "clean and out must be 16-byte, spans 4-byte aligned", "clean, out and hidden must not overlap"
REFUSALS = {
    "corrupt/null_clean": (lambda L: corrupt(L, clean=None), "null pointer (clean, out)"),
    "corrupt/null_out": (lambda L: corrupt(L, out=None), "null pointer (clean, out)"),
    "corrupt/in_place": (lambda L: corrupt(L, out=P), OVER),
    "corrupt/out_inside_clean": (lambda L: corrupt(L, out=P + 3 * 4 * 32 * 4 - 16), OVER),
    "corrupt/clean_inside_out": (lambda L: corrupt(L, clean=Q + 16), OVER),
    "corrupt/hidden_inside_out": (lambda L: corrupt(L, hidden=Q + 3 * 4 * 32 * 4 - 1), OVER),
    "corrupt/hidden_inside_clean": (lambda L: corrupt(L, hidden=P), OVER),
    "corrupt/negative_n": (lambda L: corrupt(L, n=-1), "n must be >= 0"),
    "corrupt/w_0": (lambda L: corrupt(L, w=0, smin=0, smax=0), W_MSG),
    "corrupt/w_12": (lambda L: corrupt(L, w=12), W_MSG),
    "corrupt/w_negative": (lambda L: corrupt(L, w=-8), W_MSG),
    "corrupt/w_above_2^20": (lambda L: corrupt(L, w=(1 << 20) + 8), W_MSG),
    "corrupt/h_0": (lambda L: corrupt(L, h=0), "h must be in 1..2^20"),
    "corrupt/h_above_2^20": (lambda L: corrupt(L, h=(1 << 20) + 1), "h must be in 1..2^20"),
    "corrupt/n_h_w": (lambda L: corrupt(L, n=(1 << 6) + 1, h=1 << 20, w=1 << 20), "n * h * w must stay within 2^46"),
    "corrupt/p_drop_negative": (lambda L: corrupt(L, p_drop=-1e-9), P_MSG),
    "corrupt/p_drop_above_1": (lambda L: corrupt(L, p_drop=1.0000001), P_MSG),
    "corrupt/p_drop_nan": (lambda L: corrupt(L, p_drop=NAN), P_MSG),
    "corrupt/p_add_inf": (lambda L: corrupt(L, p_add=INF), P_MSG),
    "corrupt/p_add_negative": (lambda L: corrupt(L, p_add=-0.5), P_MSG),
    "corrupt/p_add_nan": (lambda L: corrupt(L, p_add=NAN), P_MSG),
    "corrupt/span_min_negative": (lambda L: corrupt(L, smin=-1), SPAN_MSG),
    "corrupt/span_min_above_max": (lambda L: corrupt(L, smin=9, smax=8), SPAN_MSG),
    "corrupt/span_max_above_w": (lambda L: corrupt(L, smax=33), SPAN_MSG),
    "corrupt/threshold_nan": (lambda L: corrupt(L, thr=NAN), F_MSG),
    "corrupt/threshold_inf": (lambda L: corrupt(L, thr=INF), F_MSG),
    "corrupt/add_value_inf": (lambda L: corrupt(L, add=-INF), F_MSG),
    "corrupt/add_value_nan": (lambda L: corrupt(L, add=NAN), F_MSG),
    "corrupt/clean_plus_4": (lambda L: corrupt(L, clean=P + 4), ALIGN),
    "corrupt/out_plus_8": (lambda L: corrupt(L, out=Q + 8), ALIGN),
    "corrupt/spans_plus_2": (lambda L: corrupt(L, spans=HID + 4096 + 2), ALIGN),
    "corrupt/refused_with_n_0_too": (lambda L: corrupt(L, n=0, w=12), W_MSG),
    "params/null_spans": (lambda L: params(L, spans=None), "null pointer (spans)"),
    "params/negative_n": (lambda L: params(L, n=-1), "n must be >= 0"),
    "params/n_above_2^40": (lambda L: params(L, n=(1 << 40) + 1), "n must stay within 2^40"),
    "params/w_4": (lambda L: params(L, w=4, smin=0, smax=0), W_MSG),
    "params/w_20": (lambda L: params(L, w=20), W_MSG),
    "params/span_min_negative": (lambda L: params(L, smin=-1), SPAN_MSG),
    "params/span_min_above_max": (lambda L: params(L, smin=5, smax=4), SPAN_MSG),
    "params/span_max_above_w": (lambda L: params(L, smax=40), SPAN_MSG),
    "params/spans_plus_1": (lambda L: params(L, spans=P + 1), "spans must be 4-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = REFUSALS[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == "vae_denoise_" + case.split("/")[0] + ": " + want


def test_limits_are_accepted_up_to_the_refusal():
    """(nothing is launched: n = 0 returns before any device work)"""
    L = _lib.lib()
    assert corrupt(L, n=0, h=1 << 20, w=1 << 20, smax=1 << 20) == 0
    assert corrupt(L, n=0, h=1, w=8, smin=0, smax=0, p_drop=0.0, p_add=1.0, hidden=None) == 0
    assert corrupt(L, n=0, p_drop=1.0, smin=32, smax=32, spans=HID + 4096) == 0
    assert params(L, n=0, w=1 << 20, smin=0, smax=1 << 20) == 0


def test_set_recon_target_refuses_a_null_context():
    L = _lib.lib()
    assert L.vae_set_recon_target(None, P) == -1 and L.vae_last_error().decode() == "vae_set_recon_target: null ctx"
    assert L.vae_set_recon_target(None, None) == -1


# ---- the headers, the exports and the stream-case table -----------------------------------------------------------------------------
def _header(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def test_header_declares_exactly_the_denoise_exports():
    declared = set(re.findall(r"\b(vae_[a-z0-9_]+)\s*\(", _header(HEADER)))
    assert declared == set(_lib.DENOISE_EXPORTS) == {"vae_denoise_corrupt", "vae_denoise_params"}
    assert all(n.startswith("vae_denoise_") for n in _lib.DENOISE_EXPORTS)
    L = _lib.lib()
    assert not [n for n in _lib.DENOISE_EXPORTS if not hasattr(L, n)]
    others = set(_lib.EXPORTS) | set(_lib.MIXTURE_EXPORTS) | set(_lib.MUSIC_EXPORTS) | set(_lib.FIDELITY_EXPORTS) | set(_lib.ATTR_EXPORTS)
    assert not set(_lib.DENOISE_EXPORTS) & others
    assert L.vae_abi_version() == 1
    text = open(HEADER).read()
    for name, value in (("STREAM_DROP", _lib.DENOISE_STREAM_DROP), ("STREAM_SPAN", _lib.DENOISE_STREAM_SPAN), ("STREAM_ADD", _lib.DENOISE_STREAM_ADD)):
        assert int(re.search(rf"#define VAE_DENOISE_{name} (\d+)", text).group(1)) == value, name
    assert (_lib.DENOISE_STREAM_DROP, _lib.DENOISE_STREAM_SPAN, _lib.DENOISE_STREAM_ADD) == (R.STREAM_DROP, R.STREAM_SPAN, R.STREAM_ADD) == (902, 903, 904)
    for name, value in (("MAX_ROWS", _lib.DENOISE_MAX_ROWS), ("MAX_COLS", _lib.DENOISE_MAX_COLS)):
        assert re.search(rf"#define VAE_DENOISE_{name} \(1 << (\d+)\)", text).group(1) == str(value.bit_length() - 1), name


def test_the_other_headers_declare_no_denoise_function():
    for name in OTHER_HEADERS:
        assert "vae_denoise_" not in _header(os.path.join(ROOT, "include", name)), name


def test_the_step_header_declares_the_target_setter():
    m = re.search(r"\bint\s+vae_set_recon_target\s*\(([^)]*)\)\s*;", _header(STEP_HEADER))
    assert m and [a.strip() for a in m.group(1).split(",")] == ["vae_ctx* ctx", "const float* target"]
    assert "vae_set_recon_target" in _lib.EXPORTS and hasattr(_lib.lib(), "vae_set_recon_target")
    doc = open(STEP_HEADER).read()
    about = doc[doc.index("A reconstruction target apart from the input"):doc.index("int vae_set_recon_target")]
    for word in ("vae_encode", "vae_decode", "vae_log_likelihood", "consume and ignore", "One-shot", "NULL"):
        assert word in about, word


def stream_entry_points():
    found = [m.group(1) for m in re.finditer(r"\b(vae_\w+)\s*\(([^;{}]*?)\)\s*;", _header(HEADER)) if re.search(r"\bvae_stream_t\b", m.group(2))]
    assert len(found) == len(set(found))
    return found


def test_every_stream_entry_point_of_the_header_has_a_stream_case():
    """The rule of tests/test_music_host.py on this header and its own case table."""
    names = stream_entry_points()
    assert sorted(names) == sorted(_lib.DENOISE_EXPORTS)
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
        assert c.sync_free and c.reads_back is None, c.name
    assert any("corrupt_rolls" in c.name for c in gpu_cases.PY_STREAM_CASES)


def test_the_gpu_shapes_are_the_ones_the_issue_names():
    assert gpu_cases.SHAPES == [(4, 128, 128), (3, 32, 32), (2, 5, 8), (1, 1, 200), (2, 128, 192)]
    assert any(w % 64 for _, _, w in gpu_cases.SHAPES)


# ---- Python argument checks (all raised before anything touches a device) ------------------------------------------------------------
def test_python_argument_checks():
    from torch_vae_amd.denoise import Corruption, corrupt_rolls, corruption_spans
    x = torch.zeros(2, 4, 32)
    with pytest.raises(ValueError, match="must be on the GPU"):
        corrupt_rolls(x)
    for shape, dtype, err, word in (((2, 4), torch.float32, ValueError, r"\[n, h, w\]"), ((2, 2, 4, 8), torch.float32, ValueError, r"\[n, 1, h, w\]"),
                                    ((2, 4, 8), torch.uint8, TypeError, "float32"), ((1, 4, 12), torch.float32, ValueError, "multiple of 8"),
                                    ((1, 4, 0), torch.float32, ValueError, "multiple of 8")):
        with pytest.raises(err, match=word):
            corrupt_rolls(torch.zeros(*shape, dtype=dtype))
    with pytest.raises(TypeError, match="tensor"):
        corrupt_rolls(x.numpy())
    for kw, word in ((dict(note_dropout=1.5), "note_dropout"), (dict(note_dropout=float("nan")), "note_dropout"), (dict(add_noise=-0.1), "add_noise"),
                     (dict(add_noise="0.1"), "add_noise"), (dict(threshold=float("inf")), "threshold"), (dict(add_value=float("nan")), "add_value"),
                     (dict(seed=1.5), "seed"), (dict(counter0=None), "counter0"), (dict(counter_stride=True), "counter_stride")):
        with pytest.raises(ValueError, match=word):
            corrupt_rolls(x, **kw)
    from torch_vae_amd.denoise import _checked_span      # (corrupt_rolls checks the span against the roll's width, after the device)
    assert _checked_span(None, 32) == (0, 0) and _checked_span(8, 32) == (8, 8) and _checked_span([0, 32], 32) == (0, 32)
    for span in ((4, 2), (-1, 3), (0, 33), (1, 2, 3), "4", (1.0, 2), 2.5, True):
        with pytest.raises(ValueError, match="span"):
            _checked_span(span, 32)
    with pytest.raises(ValueError, match="n must be"):
        corruption_spans(-1, 32, (2, 4))
    with pytest.raises(ValueError, match="w must be"):
        corruption_spans(4, 12, (2, 4))
    with pytest.raises(ValueError, match="GPU only"):
        corruption_spans(4, 32, (2, 4), device="cpu")
    with pytest.raises(ValueError, match="denoise_note_dropout"):
        Corruption(note_dropout=2.0)
    with pytest.raises(ValueError, match="span"):
        Corruption(span=(5, 2))


def test_corruption_from_config():
    from torch_vae_amd.denoise import Corruption
    assert Corruption.from_config(Namespace()) is None
    assert Corruption.from_config(Namespace(denoise_seed=4, denoise_note_dropout=None)) is None       # a seed alone asks for nothing
    c = Corruption.from_config(Namespace(denoise_note_dropout=0.3, denoise_span=[4, 8]))
    assert (c.note_dropout, c.span, c.add_noise, c.seed, c.threshold, c.add_value) == (0.3, (4, 8), 0.0, 0, 0.5, 1.0)
    c = Corruption.from_config(Namespace(denoise_add_noise=0.01, denoise_seed=(1 << 64) + 5))
    assert (c.note_dropout, c.span, c.add_noise, c.seed) == (0.0, None, 0.01, 5)
    c = Corruption.from_config(Namespace(denoise_span=16))
    assert c.span == 16 and c.note_dropout == 0.0


def test_signatures_and_config_fields():
    from torch_vae_amd import evaluation, generation, train
    from torch_vae_amd.denoise import corrupt_rolls
    from torch_vae_amd.models import VanillaVAE
    sig = inspect.signature(corrupt_rolls)
    assert {k: v.default for k, v in sig.parameters.items() if k != "x"} == dict(
        note_dropout=0.0, span=None, add_noise=0.0, threshold=0.5, add_value=1.0, seed=0, counter0=0, counter_stride=1, spans=None, return_hidden=False)
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.parameters.items() if k != "x")
    for f in (VanillaVAE.forward, VanillaVAE.fused_forward_backward, VanillaVAE.fused_train_step, train.fused_step):
        assert inspect.signature(f).parameters["target"].default is None, f
    assert inspect.signature(evaluation.evaluate).parameters["infill_span"].default is None
    assert list(inspect.signature(generation.infill).parameters) == ["model", "x", "t0", "t1", "threshold"]
    assert list(inspect.signature(evaluation.infill_metrics).parameters)[:5] == ["xhat", "target", "t0", "t1", "thresholds"]
    src = inspect.getsource(train.train_one_epoch)
    assert "Corruption.from_config(config)" in src and "(total_step * world + rank) * batch_size_this_gpu" in src
    import torch_vae_amd
    for name in ("corrupt_rolls", "corruption_spans", "infill"):
        assert name in torch_vae_amd.__all__ and callable(getattr(torch_vae_amd, name))


def test_infill_and_target_argument_checks():
    from torch_vae_amd.evaluation import infill_metrics
    from torch_vae_amd.generation import checked_time_span, infill
    from torch_vae_amd.models import VanillaVAE
    m = VanillaVAE(1, 16, 32)
    with pytest.raises(RuntimeError, match="HIP device"):
        infill(m, torch.zeros(2, 1, 32, 32), 4, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.forward(torch.zeros(2, 1, 32, 32), target=torch.zeros(2, 1, 32, 32))
    assert checked_time_span(0, 32, 32) == (0, 32)
    for t0, t1 in ((4, 4), (-1, 4), (8, 33), (9, 8), (1.0, 4), (True, 4)):
        with pytest.raises(ValueError):
            checked_time_span(t0, t1, 32)
    with pytest.raises(ValueError, match="same shape"):
        infill_metrics(torch.zeros(2, 4, 32), torch.zeros(2, 4, 16), 0, 8)
    with pytest.raises(ValueError, match="t0 < t1"):
        infill_metrics(torch.zeros(2, 4, 32), torch.zeros(2, 4, 32), 8, 8)
