"""A plain numpy restatement of include/vae_music.h (vae_music_roll_stats) and of evaluation.music_summary / compare_music, written
from the header's table with loops over rows and columns of the unpacked cells - no bit tricks - plus the rolls the tests use.
Importing it touches no GPU."""
import math

import numpy as np

F = 76
COL = {"rolls": 0, "nonempty": 1, "cells": 2, "notes": 3, "used_pitches": 4, "lowest": 5, "highest": 6, "sounding_steps": 7,
       "onset_steps": 8, "max_polyphony": 9, "pc_cells": 10, "pc_notes": 22, "duration": 34, "polyphony": 46, "ioi": 62}
WIDTH = {"pc_cells": 12, "pc_notes": 12, "duration": 12, "polyphony": 16, "ioi": 12}
DISTRIBUTIONS = {"pitch_class": "pc_cells", "pitch_class_onsets": "pc_notes", "duration": "duration", "polyphony": "polyphony", "ioi": "ioi"}
SCALARS = ("notes", "cells", "used_pitches", "pitch_range", "max_polyphony")
MAJOR = (0, 2, 4, 5, 7, 9, 11)
SHAPES = [(1, 32), (3, 32), (13, 64), (5, 288), (128, 128), (256, 256)]
COUNTS = [1, 3, 67]
OFFSETS = [0, 21, 1000003 % (1 << 20)]


def log2_bucket(v):
    return min(int(math.floor(math.log2(v))), 11)


def roll_rows(cells):
    """What one roll's cells [h, w] of 0 / 1 hold, before rows are binned by pitch class: per row its cells and notes, the note
    lengths, the cells per column and the columns that hold an onset."""
    h, w = cells.shape
    row_cells, row_notes, lengths = [], [], []
    onset_at = np.zeros(w, dtype=bool)
    for p in range(h):
        edge = np.diff(np.concatenate(([0], cells[p].astype(np.int64), [0])))
        starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)      # a note is cells[p, start:end]
        onset_at[starts] = True
        row_cells.append(int(cells[p].sum()))
        row_notes.append(len(starts))
        lengths += [int(e - s) for s, e in zip(starts, ends)]
    return dict(row_cells=row_cells, row_notes=row_notes, lengths=lengths, column=[int(k) for k in cells.sum(axis=0)],
                onset_steps=[t for t in range(w) if onset_at[t]])


def roll_features(cells, pitch_offset=0, rows=None):
    """One feature row from cells [h, w] of 0 / 1 (rows: roll_rows(cells), when the caller has it already)."""
    rows = roll_rows(cells) if rows is None else rows
    f = np.zeros(F, dtype=np.int64)
    f[COL["rolls"]] = 1
    used = [p for p, c in enumerate(rows["row_cells"]) if c]
    for p in used:
        pc = (p + pitch_offset) % 12
        f[COL["cells"]] += rows["row_cells"][p]
        f[COL["notes"]] += rows["row_notes"][p]
        f[COL["pc_cells"] + pc] += rows["row_cells"][p]
        f[COL["pc_notes"] + pc] += rows["row_notes"][p]
    for length in rows["lengths"]:
        f[COL["duration"] + log2_bucket(length)] += 1
    f[COL["nonempty"]] = 1 if used else 0
    f[COL["used_pitches"]] = len(used)
    f[COL["lowest"]] = used[0] if used else -1
    f[COL["highest"]] = used[-1] if used else -1
    for k in rows["column"]:
        f[COL["polyphony"] + min(k, 15)] += 1
        f[COL["sounding_steps"]] += k > 0
        f[COL["max_polyphony"]] = max(f[COL["max_polyphony"]], k)
    steps = rows["onset_steps"]
    f[COL["onset_steps"]] = len(steps)
    for before, after in zip(steps, steps[1:]):
        f[COL["ioi"] + log2_bucket(after - before)] += 1
    return f


def unpack(planes):
    return np.unpackbits(np.asarray(planes, dtype=np.uint8), axis=-1)


def features(planes, pitch_offset=0, rows=None):
    """int32 [n, 76] from uint8 planes [n, h, w/8] (rows: the rolls' roll_rows, to share them between pitch offsets)"""
    cells = unpack(planes)
    out = np.zeros((cells.shape[0], F), dtype=np.int32)
    for r in range(cells.shape[0]):
        out[r] = roll_features(cells[r], pitch_offset, None if rows is None else rows[r])
    return out


def empty_totals():
    t = np.zeros(F, dtype=np.int64)
    t[COL["lowest"]] = t[COL["highest"]] = -1
    return t


def totals(feat, into=None):
    """int64 [76]: sums, the minimum of `lowest` over non-empty rolls, the maxima of `highest` and `max_polyphony`; `into`: totals to
    combine with (accumulate != 0)."""
    t = empty_totals() if into is None else np.array(into, dtype=np.int64)
    for f in np.asarray(feat, dtype=np.int64):
        for c in range(F):
            if c == COL["lowest"]:
                if f[1] and (t[c] < 0 or f[c] < t[c]):
                    t[c] = f[c]
            elif c in (COL["highest"], COL["max_polyphony"]):
                t[c] = max(t[c], f[c])
            else:
                t[c] += f[c]
    return t


def block(t, name):
    return [int(v) for v in t[COL[name]:COL[name] + WIDTH[name]]]


def ratio(a, b):
    return a / b if b else float("nan")


def pitch_range(feat):
    feat = np.asarray(feat, dtype=np.int64).reshape(-1, F)
    return (feat[:, 6] - feat[:, 5] + 1) * feat[:, 1]


def scale_consistency(pc_cells):
    cells = sum(pc_cells)
    if not cells:
        return float("nan"), -1
    shares = [sum(pc_cells[(root + s) % 12] for s in MAJOR) / cells for root in range(12)]
    best = max(shares)
    return best, shares.index(best)


def summary(feat, h, w):
    feat = np.asarray(feat, dtype=np.int64).reshape(-1, F)
    t = totals(feat)
    rolls, nonempty, cells, notes = (int(t[c]) for c in range(4))
    poly = block(t, "polyphony")
    out = {"rolls": rolls, "empty_roll_rate": ratio(rolls - nonempty, rolls), "notes_per_roll": ratio(notes, rolls),
           "note_density": ratio(cells, rolls * h * w), "mean_duration": ratio(cells, notes),
           "mean_polyphony": ratio(cells, int(t[COL["sounding_steps"]])), "empty_step_rate": ratio(poly[0], sum(poly)),
           "used_pitches": ratio(int(t[COL["used_pitches"]]), nonempty), "pitch_range": ratio(int(pitch_range(feat).sum()), nonempty)}
    for name, source in DISTRIBUTIONS.items():
        counts = block(t, source)
        out[name] = [ratio(c, sum(counts)) for c in counts]
    p = np.array(out["pitch_class"], dtype=np.float64)
    out["pitch_class_entropy"] = float(-(p[p > 0] * np.log2(p[p > 0])).sum()) if cells else float("nan")
    out["scale_consistency"], out["key"] = scale_consistency(block(t, "pc_cells"))
    return out


def js_overlap(a, b):
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    if not a.sum() or not b.sum():
        return float("nan"), float("nan")
    p, q = a / a.sum(), b / b.sum()
    m = 0.5 * (p + q)
    js = 0.0
    for i in range(len(p)):
        js += (0.5 * p[i] * np.log2(p[i] / m[i]) if p[i] > 0 else 0.0) + (0.5 * q[i] * np.log2(q[i] / m[i]) if q[i] > 0 else 0.0)
    return float(js), float(np.minimum(p, q).sum())


def wasserstein1(x, y):
    if not len(x) or not len(y):
        return float("nan")
    x, y = np.asarray(x), np.asarray(y)
    total = 0.0
    for v in range(0, int(max(x.max(), y.max())) + 1):
        total += abs((x <= v).sum() / len(x) - (y <= v).sum() / len(y))
    return total


def per_roll(feat):
    feat = np.asarray(feat, dtype=np.int64).reshape(-1, F)
    return {"notes": feat[:, 3], "cells": feat[:, 2], "used_pitches": feat[:, 4], "pitch_range": pitch_range(feat), "max_polyphony": feat[:, 9]}


def compare(fa, fb):
    ta, tb = totals(np.asarray(fa).reshape(-1, F)), totals(np.asarray(fb).reshape(-1, F))
    out = {}
    for name, source in DISTRIBUTIONS.items():
        out[f"js_{name}"], out[f"overlap_{name}"] = js_overlap(block(ta, source), block(tb, source))
    ra, rb = per_roll(fa), per_roll(fb)
    for name in SCALARS:
        out[f"mean_{name}_a"] = ratio(int(ra[name].sum()), len(ra[name]))
        out[f"mean_{name}_b"] = ratio(int(rb[name].sum()), len(rb[name]))
        out[f"w1_{name}"] = wasserstein1(ra[name], rb[name])
    out["scale_consistency_a"] = scale_consistency(block(ta, "pc_cells"))[0]
    out["scale_consistency_b"] = scale_consistency(block(tb, "pc_cells"))[0]
    return out


# ---- rolls ---------------------------------------------------------------------------------------------------------------------------
def pack(cells):
    return np.packbits(np.asarray(cells, dtype=np.uint8), axis=-1)


def random_runs(rng, h, w, density=0.05):
    """Cells [h, w]: notes of geometric length (mean about 4 steps) dropped until about `density` of the cells are set."""
    cells = np.zeros((h, w), dtype=np.uint8)
    target = max(1, int(round(density * h * w)))
    count = 0
    while count < target:
        p, t = int(rng.integers(h)), int(rng.integers(w))
        note = cells[p, t:t + int(rng.geometric(0.25))]
        count += note.size - int(note.sum())
        note[:] = 1
    return cells


def hand_made(h, w):
    """The rolls with known answers, each where the shape has room for it: (name, cells [h, w])."""
    out = [("empty", np.zeros((h, w), np.uint8)), ("full", np.ones((h, w), np.uint8))]
    row = np.zeros((h, w), np.uint8)
    row[h // 2] = 1
    out.append(("full_row", row))
    alt = np.zeros((h, w), np.uint8)
    alt[0, 0::2] = 1
    out.append(("alternating", alt))
    if w >= 64:
        c = np.zeros((h, w), np.uint8)
        c[h - 1, 30:34] = 1                      # across a 32-bit boundary
        if w >= 256:
            c[0, 120:140] = 1                    # across a 128-bit boundary
        out.append(("crossing", c))
    if h >= 20:
        c = np.zeros((h, w), np.uint8)
        c[h - 20:, w - 1] = 1                    # a column of 20 cells: the >= 15 bucket
        out.append(("column20", c))
    if w >= 288:
        c = np.zeros((h, w), np.uint8)
        c[0, 0] = 1
        c[h - 1, 280] = 1                        # onsets 280 steps apart: ioi bucket 8
        out.append(("far_onsets", c))
    return out


def case_planes(h, w, n, seed, single="random"):
    """uint8 planes [n, h, w/8] of one GPU case.  n >= 3: the all-zero and the all-ones roll, the hand-made rolls while there is
    room (always at least one roll of random runs), random runs at 2, 5 and 10 % for the rest.  n == 1: `single` = "random",
    "empty" or "full"."""
    rng = np.random.default_rng(seed)
    if n == 1:
        rolls = [dict(hand_made(h, w))[single]] if single != "random" else [random_runs(rng, h, w)]
    else:
        rolls = [c for _, c in hand_made(h, w)][:n - 1]
    while len(rolls) < n:
        rolls.append(random_runs(rng, h, w, density=float(rng.choice([0.02, 0.05, 0.1]))))
    return pack(np.stack(rolls))


def long_roll():
    """2 x 8192, for the buckets no listed shape is long enough to reach: notes of 3000, 600 and 1100 steps (duration buckets 11, 9,
    10) and onsets at steps 4, 3100, 3800, 5000 and 8100 (gaps 3096, 700, 1200, 3100: ioi buckets 11, 9, 10, 11)."""
    c = np.zeros((1, 2, 8192), np.uint8)
    c[0, 0, 4:3004] = 1
    c[0, 1, 3100:3700] = 1
    c[0, 1, 3800:4900] = 1
    c[0, 1, 5000] = 1
    c[0, 0, 8100] = 1
    return pack(c)


SINGLE = ["random", "full", "empty"]      # what the n = 1 case of pitch offset i holds
_cases = {}


def gpu_cases():
    """{(h, w, n, pitch_offset): (planes, features)} of the whole GPU comparison, computed once: every shape, count and pitch
    offset, plus one 2 x 8192 roll whose notes and gaps reach the upper duration and ioi buckets (no listed shape is that long)."""
    if not _cases:
        for si, (h, w) in enumerate(SHAPES):
            for ni, n in enumerate(COUNTS):
                shared = None
                for oi, off in enumerate(OFFSETS):
                    if n == 1 or shared is None:
                        planes = case_planes(h, w, n, 100 * si + ni, SINGLE[oi])
                        shared = (planes, [roll_rows(c) for c in unpack(planes)])
                    _cases[(h, w, n, off)] = (shared[0], features(shared[0], off, shared[1]))
        planes = long_roll()
        _cases[(2, 8192, 1, 21)] = (planes, features(planes, 21))
    return _cases
