"""Host side of the note-event extraction (torch_vae_amd/generation.py, vae_extract_notes): the numpy reference pinned against an
independent per-cell formulation and against the two-ballot form the kernel uses, the contract's properties, note_event_metrics
against an exhaustive maximum matching, and the argument refusals of the entry point (fake, never dereferenced addresses, as in
test_augment_host.py)."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import notes_ref as nr
from torch_vae_amd import _lib, evaluation

P = 4096          # a fake device address, 16-byte aligned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force_kept(x, on, off, D, G):
    """Per cell, by scanning left and right from it: the hysteresis state, whether a silent cell is bridged, whether a sounding
    cell belongs to a run of at least D."""
    x = np.asarray(x, np.float32)
    on, off = np.float32(on), np.float32(off)
    w = len(x)
    s = np.zeros(w, bool)
    for t in range(w):
        for u in range(t, -1, -1):          # the last cell at or before t that decides
            if x[u] >= on:
                s[t] = True
                break
            if not (x[u] >= off):
                break
    b = s.copy()
    for t in range(w):
        if not s[t]:
            left = next((u for u in range(t - 1, -1, -1) if s[u]), None)
            right = next((u for u in range(t + 1, w) if s[u]), None)
            b[t] = left is not None and right is not None and right - left - 1 <= G
    kept = np.zeros(w, bool)
    for t in range(w):
        if b[t]:
            lo = t
            while lo > 0 and b[lo - 1]:
                lo -= 1
            hi = t
            while hi + 1 < w and b[hi + 1]:
                hi += 1
            kept[t] = hi - lo + 1 >= D
    return kept


def test_reference_against_per_cell_formulation():
    rng = np.random.default_rng(0)
    seen = {"bridged": 0, "dropped": 0, "sustained": 0}
    for case in range(120):
        w = int(rng.choice([8, 24, 64, 72, 136]))
        row = nr.random_rolls(rng, 1, 1, w)[0, 0]
        for on, off, D, G in nr.PARAM_SETS + [(0.5, 0.1, 4, 5)]:
            notes, kept, st = nr.row_notes(row, on, off, D, G)
            assert np.array_equal(kept, brute_force_kept(row, on, off, D, G)), (case, on, off, D, G)
            assert [(t0, n) for t0, n, _ in notes] == nr.runs(kept)
            for t0, n, pk in notes:
                assert pk == np.nanmax(row[t0:t0 + n]) and pk in row[t0:t0 + n]
            for k in seen:
                seen[k] += st[k]
    assert min(seen.values()) > 50, seen


def ballot_hysteresis(x, on, off):
    """The kernel's form: per 64-step chunk two masks; cell i takes onm's bit at the highest set bit of (onm | offm) & bits 0..i,
    or the state carried in from the previous chunk when that is empty."""
    x = np.asarray(x, np.float32)
    out, carry = np.zeros(len(x), bool), False
    for c0 in range(0, len(x), 64):
        v = x[c0:c0 + 64]
        with np.errstate(invalid="ignore"):
            onm = sum(1 << i for i in range(len(v)) if v[i] >= np.float32(on))
            offm = sum(1 << i for i in range(len(v)) if not (v[i] >= np.float32(off)))
        for i in range(len(v)):
            m = (onm | offm) & ((2 << i) - 1)
            out[c0 + i] = carry if m == 0 else bool((onm >> (m.bit_length() - 1)) & 1)
        carry = out[c0 + len(v) - 1]
    return out


def test_ballot_form_equals_the_state_machine():
    rng = np.random.default_rng(1)
    for case in range(200):
        row = nr.random_rolls(rng, 1, 1, int(rng.choice([64, 72, 128, 200])))[0, 0]
        for on, off in ((0.5, 0.5), (0.5, 0.3), (0.7, 0.1), (1.0, 0.0)):
            assert np.array_equal(ballot_hysteresis(row, on, off), nr.hysteresis(row, on, off))


def test_plain_thresholding_is_packbits():
    rng = np.random.default_rng(2)
    x = nr.random_rolls(rng, 3, 4, 72)
    for t in (0.3, 0.5, 0.7):
        with np.errstate(invalid="ignore"):
            want = np.packbits(x >= np.float32(t), axis=-1)
        assert np.array_equal(nr.extract(x, t, t, 1, 0)["cleaned"], want)


@pytest.mark.parametrize("w", [8, 24, 64, 72, 200])
def test_events_per_row_bound(w):
    rng = np.random.default_rng(3)
    x = nr.random_rolls(rng, 2, 5, w)
    for on, off, D, G in nr.PARAM_SETS:
        ev = nr.extract(x, on, off, D, G)["events"]
        for r in range(2):
            for p in range(5):
                assert np.sum((ev[:, 0] == r) & (ev[:, 1] == p)) <= (w + 1) // 2
    alt = nr.extract(nr.alternating(1, 2, w), 0.5, 0.5, 1, 0)
    assert alt["offsets"].tolist() == [0, 2 * ((w + 1) // 2)]
    assert np.all(alt["events"][:, 3] == 1) and np.all(alt["peaks"] == 1.0)


def test_cleaned_planes_reextract_to_the_same_notes():
    rng = np.random.default_rng(4)
    x = nr.random_rolls(rng, 3, 3, 136)
    for on, off, D, G in nr.PARAM_SETS:
        first = nr.extract(x, on, off, D, G)
        planes = np.unpackbits(first["cleaned"], axis=-1).astype(np.float32)
        again = nr.extract(planes, 0.5, 0.5, 1, 0)
        assert np.array_equal(again["events"], first["events"]) and np.array_equal(again["offsets"], first["offsets"])
        assert np.array_equal(again["cleaned"], first["cleaned"])


def max_matching(a, b, tol):
    """Exhaustive: the largest set of pairs (i, j), |a_i - b_j| <= tol, no index twice."""
    best = 0
    for k in range(min(len(a), len(b)), 0, -1):
        for ia in itertools.combinations(range(len(a)), k):
            for jb in itertools.permutations(range(len(b)), k):
                if all(abs(a[i] - b[j]) <= tol for i, j in zip(ia, jb)):
                    return k
    return best


@pytest.mark.parametrize("tol", [0, 1, 2])
def test_note_event_metrics_against_exhaustive_matching(tol):
    rng = np.random.default_rng(5 + tol)
    for case in range(12):
        pred, ref, want = [], [], 0
        for r in range(2):
            for p in range(3):
                a = sorted(rng.choice(12, size=int(rng.integers(0, 7)), replace=False).tolist())
                b = sorted(rng.choice(12, size=int(rng.integers(0, 7)), replace=False).tolist())
                pred += [(r, p, t, 1) for t in a]
                ref += [(r, p, t, 2) for t in b]
                want += max_matching(a, b, tol)
        got = evaluation.note_event_metrics(np.array(pred, np.int32).reshape(-1, 4), np.array(ref, np.int32).reshape(-1, 4), onset_tolerance=tol)
        assert got == nr.ratios(len(pred), len(ref), want), case
        assert got == nr.event_metrics(pred, ref, tol)
        assert got == evaluation.note_event_metrics(torch.tensor(pred, dtype=torch.int32).reshape(-1, 4), ref, onset_tolerance=tol)


def test_note_event_metrics_edges():
    empty = np.zeros((0, 4), np.int32)
    some = np.array([[0, 1, 2, 3], [0, 1, 5, 1]], np.int32)
    zero = {"notes_pred": 0, "notes_true": 0, "matched": 0, "note_precision": 0.0, "note_recall": 0.0, "note_f1": 0.0}
    assert evaluation.note_event_metrics(empty, empty) == zero
    assert evaluation.note_event_metrics(some, empty) == dict(zero, notes_pred=2)
    assert evaluation.note_event_metrics(empty, some) == dict(zero, notes_true=2)
    same = evaluation.note_event_metrics(some, some, onset_tolerance=0)
    assert (same["matched"], same["note_precision"], same["note_recall"], same["note_f1"]) == (2, 1.0, 1.0, 1.0)
    # another pitch or another roll never matches; one step off matches at tolerance 1 only
    other = some + np.array([0, 1, 0, 0], np.int32)
    assert evaluation.note_event_metrics(some, other)["matched"] == 0
    shifted = some + np.array([0, 0, 1, 0], np.int32)
    assert evaluation.note_event_metrics(some, shifted, onset_tolerance=0)["matched"] == 0
    assert evaluation.note_event_metrics(some, shifted, onset_tolerance=1)["matched"] == 2
    with pytest.raises(ValueError):
        evaluation.note_event_metrics(some, some, onset_tolerance=-1)


def notes(L, rolls=P, n=2, h=4, w=16, on=0.5, off=0.5, D=1, G=0, events=P, peaks=P, capacity=8, offsets=P, cleaned=None):
    return L.vae_extract_notes(rolls, n, h, w, on, off, D, G, events, peaks, capacity, offsets, cleaned, None)


W8 = "w must be a multiple of 8 in 8..65536"
BOTH = "events and peaks must both be given or both be null"
ALIGN4 = "rolls, events and peaks must be 4-byte aligned"
CASES = {
    "null_rolls": (lambda L: notes(L, rolls=None), "null pointer (rolls, offsets)"),
    "null_offsets": (lambda L: notes(L, offsets=None), "null pointer (rolls, offsets)"),
    "events_without_peaks": (lambda L: notes(L, peaks=None), BOTH),
    "peaks_without_events": (lambda L: notes(L, events=None), BOTH),
    "n_-1": (lambda L: notes(L, n=-1), "n must be >= 0"),
    "h_0": (lambda L: notes(L, h=0), "h must be >= 1"),
    "w_0": (lambda L: notes(L, w=0), W8),
    "w_12": (lambda L: notes(L, w=12), W8),
    "w_-8": (lambda L: notes(L, w=-8), W8),
    "w_65544": (lambda L: notes(L, w=65544), W8),
    "rows_2^31": (lambda L: notes(L, n=2 ** 20, h=2 ** 11), "n * h must stay below 2^31"),
    "onset_nan": (lambda L: notes(L, on=float("nan")), "the thresholds must be finite"),
    "onset_inf": (lambda L: notes(L, on=float("inf")), "the thresholds must be finite"),
    "sustain_-inf": (lambda L: notes(L, off=float("-inf")), "the thresholds must be finite"),
    "sustain_above_onset": (lambda L: notes(L, on=0.3, off=0.5), "sustain_threshold must be <= onset_threshold"),
    "min_duration_0": (lambda L: notes(L, D=0), "min_duration must be >= 1"),
    "max_gap_-1": (lambda L: notes(L, G=-1), "max_gap must be >= 0"),
    "capacity_-1": (lambda L: notes(L, capacity=-1), "capacity must be >= 0"),
    "rolls_plus_2": (lambda L: notes(L, rolls=P + 2), ALIGN4),
    "peaks_plus_1": (lambda L: notes(L, peaks=P + 1), ALIGN4),
    "events_plus_2": (lambda L: notes(L, events=P + 2), ALIGN4),
    "offsets_plus_4": (lambda L: notes(L, offsets=P + 4), "offsets must be 8-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = CASES[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == "vae_extract_notes: " + want


def test_no_rolls_pass_every_argument_check():
    """n == 0 zeroes offsets[0] and returns 0.  Zeroing is a device operation: where there is a device it is checked on real memory;
    where there is none the call gets past every argument check (its failure is the runtime's, not a refusal of vae_extract_notes)."""
    L = _lib.lib()
    if torch.cuda.is_available():
        offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        assert notes(L, n=0, offsets=offsets.data_ptr(), events=None, peaks=None) == 0
        assert notes(L, n=0, h=7, w=64, offsets=offsets.data_ptr() + 8) == 0
        torch.cuda.synchronize()
        assert offsets.tolist() == [0, 0, -1]
    else:
        rc = notes(L, n=0)
        assert rc == 0 or not L.vae_last_error().decode().startswith("vae_extract_notes:")


def test_exported():
    L = _lib.lib()
    assert "vae_extract_notes" in _lib.EXPORTS and hasattr(L, "vae_extract_notes")
    assert L.vae_abi_version() == 1
    with open(os.path.join(ROOT, "include", "vae_step.h")) as f:
        assert "int vae_extract_notes(const float* rolls, int64_t n, int h, int w," in f.read()
    import torch_vae_amd
    from torch_vae_amd import generation
    for name in ("extract_notes", "binarize_rolls", "events_to_lists"):
        assert name in torch_vae_amd.__all__ and getattr(torch_vae_amd, name) is getattr(generation, name)
    from torch_vae_amd.models import VanillaVAE
    assert callable(VanillaVAE.sample_notes) and callable(VanillaVAE.interpolate)


def test_python_refusals_need_no_device():
    from torch_vae_amd import generation
    with pytest.raises(ValueError, match="on the GPU"):
        generation.extract_notes(torch.zeros(1, 4, 16))
    with pytest.raises(TypeError):
        generation.extract_notes(np.zeros((1, 4, 16), np.float32))
    with pytest.raises(ValueError):
        generation.interpolate_latents(torch.zeros(2, 4), torch.zeros(2, 4), 3, mode="cubic")
    z = generation.interpolate_latents(torch.tensor([[1.0, 0.0]]), torch.tensor([[0.0, 1.0]]), 3)
    assert torch.allclose(z[0, 1], torch.tensor([0.5 ** 0.5, 0.5 ** 0.5]), atol=1e-6)
    # parallel vectors: the angle is 0, the row falls back to the straight line
    z = generation.interpolate_latents(torch.tensor([[1.0, 1.0]]), torch.tensor([[3.0, 3.0]]), 3)
    assert torch.allclose(z[0], torch.tensor([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]))
