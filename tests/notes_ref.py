"""numpy restatement of vae_extract_notes (include/vae_step.h) and of evaluation.note_event_metrics: a sequential state machine per
row, written for clarity, and the helpers the note tests share (the value set, the alternating row, the witnesses that a case
exercises bridging, dropping and sustaining at all)."""
import numpy as np

VALUES = np.array([0.0, 0.1, 0.3, 0.5, 0.7, 1.0, np.nan], np.float32)
PARAM_SETS = [(0.5, 0.5, 1, 0), (0.5, 0.3, 1, 0), (0.5, 0.3, 2, 1), (0.7, 0.1, 3, 2)]


def hysteresis(x, on, off):
    """s[t] of one row: on at x >= on, off at not (x >= off), else as before; float32 comparisons."""
    x = np.asarray(x, np.float32)
    on, off = np.float32(on), np.float32(off)
    s = np.zeros(len(x), bool)
    state = False
    for t, v in enumerate(x):
        if v >= on:
            state = True
        elif not (v >= off):
            state = False
        s[t] = state
    return s


def runs(mask):
    """[(start, length)] of the maximal runs of ones."""
    out, t, w = [], 0, len(mask)
    while t < w:
        if mask[t]:
            t0 = t
            while t < w and mask[t]:
                t += 1
            out.append((t0, t - t0))
        else:
            t += 1
    return out


def bridge(s, G):
    """Zero runs of length <= G with a one on both sides become ones."""
    s = s.copy()
    for t0, n in runs(~s):
        if n <= G and t0 > 0 and t0 + n < len(s):
            s[t0:t0 + n] = True
    return s


def row_notes(x, on, off, D, G):
    """([(onset, duration, peak)], kept mask, stats) of one row; stats counts bridged gaps, dropped notes and cells that are on
    only because of the sustain threshold."""
    x = np.asarray(x, np.float32)
    s = hysteresis(x, on, off)
    b = bridge(s, G)
    kept = np.zeros(len(x), bool)
    notes, dropped = [], 0
    for t0, n in runs(b):
        if n < D:
            dropped += 1
            continue
        kept[t0:t0 + n] = True
        cells = x[t0:t0 + n]
        notes.append((t0, n, np.float32(np.max(cells[~np.isnan(cells)]))))
    with np.errstate(invalid="ignore"):
        sustained = int(np.sum(s & ~(x >= np.float32(on))))
    stats = {"bridged": len(runs(~s)) - len(runs(~b)), "dropped": dropped, "sustained": sustained}
    return notes, kept, stats


def extract(rolls, on=0.5, off=None, D=1, G=0):
    """The whole contract on [n, h, w] float32: dict of events int32 [N, 4], peaks f32 [N], offsets int64 [n + 1], cleaned uint8
    [n, h, w/8] and the summed stats."""
    rolls = np.asarray(rolls, np.float32)
    off = on if off is None else off
    n, h, w = rolls.shape
    events, peaks, offsets = [], [], [0]
    kept = np.zeros((n, h, w), bool)
    stats = {"bridged": 0, "dropped": 0, "sustained": 0}
    for r in range(n):
        for p in range(h):
            with np.errstate(invalid="ignore"):
                if not (rolls[r, p] >= np.float32(on)).any():     # nothing ever switches the row on
                    continue
            notes, kept[r, p], st = row_notes(rolls[r, p], on, off, D, G)
            for k in stats:
                stats[k] += st[k]
            for t0, d, pk in notes:
                events.append((r, p, t0, d))
                peaks.append(pk)
        offsets.append(len(events))
    return {"events": np.array(events, np.int32).reshape(-1, 4), "peaks": np.array(peaks, np.float32),
            "offsets": np.array(offsets, np.int64), "cleaned": np.packbits(kept, axis=-1), "stats": stats}


def random_rolls(rng, n, h, w):
    """Rolls over VALUES with per-row mixing weights; the weights favour rows with long stretches above and below the thresholds."""
    out = np.empty((n, h, w), np.float32)
    for r in range(n):
        for p in range(h):
            wts = rng.dirichlet(np.full(len(VALUES), 0.7))
            out[r, p] = VALUES[rng.choice(len(VALUES), size=w, p=wts)]
    return out


def alternating(n, h, w):
    x = np.zeros((n, h, w), np.float32)
    x[..., 0::2] = 1.0
    return x


def match_row(pred_onsets, ref_onsets, tol):
    """Two-pointer sweep over two ascending onset lists: the number of pairs |p - r| <= tol with every note used at most once."""
    i = j = m = 0
    while i < len(pred_onsets) and j < len(ref_onsets):
        d = int(pred_onsets[i]) - int(ref_onsets[j])
        if abs(d) <= tol:
            m += 1
            i += 1
            j += 1
        elif d < 0:
            i += 1
        else:
            j += 1
    return m


def event_metrics(pred, ref, tol=1):
    """The six keys of evaluation.note_event_metrics from two event arrays [N, 4], by grouping the rows in a dict."""
    def rows(ev):
        d = {}
        for r, p, t0, _ in np.asarray(ev).reshape(-1, 4).tolist():
            d.setdefault((r, p), []).append(t0)
        return {k: sorted(v) for k, v in d.items()}
    a, b = rows(pred), rows(ref)
    matched = sum(match_row(a[k], b[k], tol) for k in a if k in b)
    return ratios(sum(map(len, a.values())), sum(map(len, b.values())), matched)


def ratios(n_pred, n_true, matched):
    div = lambda x, y: x / y if y else 0.0
    return {"notes_pred": n_pred, "notes_true": n_true, "matched": matched, "note_precision": div(matched, n_pred),
            "note_recall": div(matched, n_true), "note_f1": div(2 * matched, n_pred + n_true)}
