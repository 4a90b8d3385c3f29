"""A plain numpy restatement of include/vae_attributes.h, written from the header with loops over rows and columns - no bit tricks -
plus the inputs the tests use.  Counters from a boolean array, attribute values in f64, the regulariser's loss and gradient in f64
from the f32 z, the concordance sums by the O(N^2) definition.  Importing it touches no GPU."""
import functools

import numpy as np

COUNTERS = ("cells", "notes", "used_pitches", "lowest", "highest", "sounding_steps", "onset_steps", "pitch_sum")
NAMES = ("note_density", "note_count", "pitch_range", "mean_pitch", "polyphony", "onset_steps", "used_pitches")   # VAE_ATTR_* 0..6
SHAPES = [(1, 1), (1, 32), (3, 63), (3, 64), (3, 65), (5, 100), (13, 192), (128, 128), (1024, 64)]
COUNTS = [1, 3, 67]
THRESHOLD = 0.5


# ---- counters -------------------------------------------------------------------------------------------------------------------------
def roll_counters(cells):
    """int64 [8] of one boolean roll [h, w]"""
    cells = np.asarray(cells, dtype=bool)
    h, w = cells.shape
    before = np.concatenate([np.zeros((h, 1), dtype=bool), cells[:, :-1]], axis=1)      # the cell one step earlier (none at t = 0)
    onset = cells & ~before                                                               # a note's first cell
    used = [p for p in range(h) if cells[p].any()]
    return np.array([cells.sum(), onset.sum(), len(used), used[0] if used else -1, used[-1] if used else -1, cells.any(axis=0).sum(),
                     onset.any(axis=0).sum(), sum(p * int(cells[p].sum()) for p in range(h))], dtype=np.int64)


def counters(cells):
    """int32 [n, 8] of boolean rolls [n, h, w]"""
    return np.stack([roll_counters(c) for c in cells]).astype(np.int32) if len(cells) else np.zeros((0, 8), np.int32)


def attribute_values(c, names):
    """f64 [n, len(names)] from counters [n, 8]: one IEEE operation each"""
    c = np.asarray(c, dtype=np.int64).reshape(-1, 8)
    out = np.zeros((c.shape[0], len(names)), dtype=np.float64)
    for r, (cells, notes, used, lo, hi, sounding, onsets, psum) in enumerate(c.tolist()):
        for k, name in enumerate(names):
            out[r, k] = {"note_density": float(cells), "note_count": float(notes), "pitch_range": float(hi - lo + 1) if cells else 0.0,
                         "mean_pitch": np.float64(psum) / np.float64(cells) if cells else -1.0,
                         "polyphony": np.float64(cells) / np.float64(sounding) if cells else 0.0, "onset_steps": float(onsets),
                         "used_pitches": float(used)}[name]
    return out


def random_runs(rng, h, w, density):
    """boolean [h, w]: notes of random length scattered over the roll"""
    cells = np.zeros((h, w), dtype=bool)
    for _ in range(max(1, int(density * h * w / 4))):
        p, t, n = rng.integers(h), rng.integers(w), 1 + rng.integers(8)
        cells[p, t:t + n] = True
    return cells


@functools.lru_cache(maxsize=None)
def counter_cases():
    """{(h, w, n): (x f32 [n, h, w], counters int32 [n, 8])}: every shape x count.  Roll 0 is random with the required content
    forced in (a run from t = 0 to w - 1, runs across columns 63/64 and 127/128 where they exist, a cell exactly at the threshold,
    a NaN, values just below the threshold); with n >= 3 roll 1 is empty and roll 2 full; the rest are random at mixed densities."""
    rng = np.random.default_rng(20)
    cases = {}
    for h, w in SHAPES:
        for n in COUNTS:
            cells = np.zeros((n, h, w), dtype=bool)
            for r in range(n):
                cells[r] = random_runs(rng, h, w, (0.02, 0.1, 0.4)[r % 3])
            cells[0, h // 2, :] = True                       # a run from t = 0 to w - 1
            for edge in (63, 127):
                if w > edge + 1:
                    cells[0, 0, edge - 1:edge + 3] = True    # across the word boundary
                    cells[0, 0, edge - 2] = False
                    if h > 2:
                        cells[0, h - 1, edge + 1] = True     # an onset exactly on the first column of the next word
                        cells[0, h - 1, edge] = False
            if n >= 3:
                cells[1], cells[2] = False, True
            x = np.where(cells, rng.uniform(0.5, 1.0, cells.shape), rng.uniform(0.0, 0.4999, cells.shape)).astype(np.float32)
            x[0, h // 2, 0] = THRESHOLD                      # exactly the threshold: set
            if w > 1 and h > 1:                              # a NaN: not set (and its roll's reference cell cleared to match)
                x[0, 0, w - 1] = np.nan
                cells[0, 0, w - 1] = False
            cases[(h, w, n)] = (x, counters(cells))
    return cases


def to_music_columns(c):
    """the first seven counters are columns 2..8 of a vae_music_roll_stats feature row"""
    return np.asarray(c)[:, :7]


# ---- regulariser ------------------------------------------------------------------------------------------------------------------------
def sgn(x):
    return (x > 0).astype(np.float64) - (x < 0).astype(np.float64)


def regularizer(z, c, pairs, delta, weight):
    """z f32 [B, >= L], c counters [B, 8], pairs [(name, dim)] -> (loss f64 [1 + K], g f64 [B, L... the columns of z])"""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    B = z64.shape[0]
    loss, g = np.zeros(1 + len(pairs)), np.zeros_like(z64)
    for k, (name, d) in enumerate(pairs):
        a = attribute_values(c, [name])[:, 0]
        u = np.float64(np.float32(delta)) * (z64[:, None, d] - z64[None, :, d])
        # |tanh u - s| and sign(tanh u - s) as exact arithmetic has them (|tanh u| < 1 for every finite u), not as a rounded tanh does:
        # an f64 tanh IS 1.0 from |u| = 19.1 on, which would make a saturated pair's term and sign exactly 0 where the true term is
        # 2 e^{-2|u|} - and a reference that says 0 cannot be met to any relative error.  Elsewhere the two agree to an ulp of 1.
        s, su, e = sgn(a[:, None] - a[None, :]), sgn(u), np.exp(-2.0 * np.abs(u))
        term = np.where(s == 0, np.tanh(np.abs(u)), np.where(s * su > 0, 2.0 * e / (1.0 + e), 2.0 / (1.0 + e)))
        loss[1 + k] = term.sum() / (B * B)
        sech2 = 4.0 * e / (1.0 + e) ** 2
        g[:, d] = np.float64(np.float32(weight)) * (2.0 / (B * B)) * (np.where(s == 0, su, -s) * np.float64(np.float32(delta)) * sech2).sum(axis=1)
    loss[0] = loss[1:].sum()
    return loss, g


# ---- concordance ------------------------------------------------------------------------------------------------------------------------
def concordance(z, c, names):
    """(S int64 [A, L], ties_z [L], ties_a [A]) over the pairs i < j by the definition"""
    z = np.asarray(z, dtype=np.float32)
    a = attribute_values(c, names)
    N, L = z.shape
    A = len(names)
    S, tz, ta = np.zeros((A, L), np.int64), np.zeros(L, np.int64), np.zeros(A, np.int64)
    for i in range(N - 1):
        sz = sgn(z[i][None, :].astype(np.float64) - z[i + 1:].astype(np.float64)).astype(np.int64)      # [N-i-1, L]
        sa = sgn(a[i][None, :] - a[i + 1:]).astype(np.int64)                                              # [N-i-1, A]
        S += sa.T @ sz
        tz += (sz == 0).sum(axis=0)
        ta += (sa == 0).sum(axis=0)
    return S, tz, ta


def tau_b_direct(zcol, a):
    """Kendall tau-b of two vectors by the textbook O(N^2) loop (NaN when either is constant)"""
    n, conc, disc, tie_x, tie_y = len(zcol), 0, 0, 0, 0
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy = np.sign(float(zcol[i]) - float(zcol[j])), np.sign(float(a[i]) - float(a[j]))
            if dx == 0:
                tie_x += 1
            if dy == 0:
                tie_y += 1
            if dx * dy > 0:
                conc += 1
            elif dx * dy < 0:
                disc += 1
    n0 = n * (n - 1) // 2
    den = np.sqrt(float(n0 - tie_x) * float(n0 - tie_y))
    return (conc - disc) / den if den > 0 else float("nan")


def tau_b(S, tz, ta, n):
    n0 = n * (n - 1) // 2
    den = np.sqrt((n0 - np.asarray(ta, np.float64))[:, None] * (n0 - np.asarray(tz, np.float64))[None, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, np.asarray(S, np.float64) / np.where(den > 0, den, 1.0), np.nan)


def latent_case(n, L, seed, ld=None, duplicates=False):
    """z f32 [n, ld] ~ N(0, 1) (ld > L: the columns past L are NaN - nothing may read them) and counters of n random 8x24 rolls"""
    rng = np.random.default_rng(seed)
    ld = L + 3 if ld is None else ld
    z = np.full((n, ld), np.nan, dtype=np.float32)
    z[:, :L] = rng.standard_normal((n, L)).astype(np.float32)
    if duplicates and n > 1:
        z[n // 2:, :L] = z[:n - n // 2, :L]                  # duplicate rows: ties in every dimension
        z[:, 0] = np.round(z[:, 0])                           # and a coarse column
    cells = np.stack([random_runs(rng, 8, 24, (0.02, 0.1, 0.3)[r % 3]) for r in range(n)]) if n else np.zeros((0, 8, 24), bool)
    if n > 2:
        cells[1] = False                                      # an empty roll (mean_pitch -1, polyphony 0)
        cells[2] = cells[0]                                   # ties in every attribute
    return z, counters(cells)
