"""Reference for the nearest-roll search (include/vae_step.h: vae_nearest_rolls), plain numpy on unpacked cells: for every shift in
rank order the shifted dataset is a slice copied into a zero array, the distance and intersection are counted per pair, argmin over
the shift axis takes the first minimum (the lowest rank), and candidates are sorted by (d, j).  `pair_by_gather` states the pair
distance a second time through tests/augment_ref.gather.  Every comparison against it is exact."""
import numpy as np

from tests import augment_ref as ar

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def shifts(P, T):
    """The window's (dy, dt) in rank order: (0, 0), then the others ascending by (dy, dt)."""
    rest = [(dy, dt) for dy in range(-P, P + 1) for dt in range(-T, T + 1) if (dy, dt) != (0, 0)]
    return [(0, 0)] + rest


def shifted(cells, dy, dt):
    """C'(..., y, x) = C(..., y - dy, x - dt) inside the frame, 0 outside; cells [..., h, w]."""
    h, w = cells.shape[-2:]
    out = np.zeros_like(cells)
    if abs(dy) >= h or abs(dt) >= w:
        return out
    out[..., max(0, dy):h + min(0, dy), max(0, dt):w + min(0, dt)] = cells[..., max(0, -dy):h - max(0, dy), max(0, -dt):w - max(0, dt)]
    return out


def unpack(planes):
    return np.unpackbits(np.asarray(planes, np.uint8), axis=-1)


def pack(cells):
    return np.packbits(np.asarray(cells, np.uint8), axis=-1)


def search(queries, rolls, P=0, T=0, k=1, exclude=None):
    """queries [Q,h,w/8], rolls [N,h,w/8] uint8 planes -> the outputs of vae_nearest_rolls as numpy arrays, `neighbour` (the shifted
    neighbour's cells [Q,k,h,w], zeros in empty slots) and `stats`, the witness counts over the top-k entries: nonzero_shift
    (entries whose shift is not (0, 0)), shift_ties (entries where several shifts reach the minimum) and index_ties (queries with
    equal distances inside the top-k or across its cut)."""
    queries, rolls = np.asarray(queries, np.uint8), np.asarray(rolls, np.uint8)
    Q, N = len(queries), len(rolls)
    qc, rc = unpack(queries), unpack(rolls)
    table = shifts(P, T)
    dist = np.empty((len(table), Q, N), np.int64)
    inter = np.empty((len(table), Q, N), np.int64)
    for s, (dy, dt) in enumerate(table):
        sp = pack(shifted(rc, dy, dt))                              # counted on the packed bytes: same cells, fewer of them
        dist[s] = _POP[queries[:, None] ^ sp[None]].sum(axis=(2, 3))
        inter[s] = _POP[queries[:, None] & sp[None]].sum(axis=(2, 3))
    best = dist.argmin(axis=0)                                      # the first minimum: the lowest rank
    d = np.take_along_axis(dist, best[None], 0)[0]
    it = np.take_along_axis(inter, best[None], 0)[0]
    ties = (dist == d[None]).sum(axis=0) > 1
    out = {"index": np.full((Q, k), -1, np.int64), "distance": np.full((Q, k), -1, np.int32), "shift": np.zeros((Q, k, 2), np.int32),
           "intersection": np.zeros((Q, k), np.int32), "query_cells": qc.sum(axis=(1, 2)).astype(np.int32),
           "neighbour": np.zeros((Q, k) + qc.shape[1:], np.uint8)}
    stats = {"nonzero_shift": 0, "shift_ties": 0, "index_ties": 0}
    for i in range(Q):
        cand = [j for j in range(N) if exclude is None or j != int(exclude[i])]
        cand.sort(key=lambda j: (d[i, j], j))
        for s, j in enumerate(cand[:k]):
            dy, dt = table[best[i, j]]
            out["index"][i, s], out["distance"][i, s], out["shift"][i, s], out["intersection"][i, s] = j, d[i, j], (dy, dt), it[i, j]
            out["neighbour"][i, s] = shifted(rc[j], dy, dt)
            stats["nonzero_shift"] += (dy, dt) != (0, 0)
            stats["shift_ties"] += bool(ties[i, j])
        ds = [d[i, j] for j in cand[:k + 1]]
        stats["index_ties"] += any(a == b for a, b in zip(ds, ds[1:]))
    out["stats"] = stats
    return out


def pair_by_gather(q_cells, c_cells, P, T):
    """(d, (dy, dt), intersection) of one pair, the shifted candidate taken from augment_ref.gather with params (dy, c0 = -dt)."""
    h, w = q_cells.shape
    best = None
    for dy, dt in shifts(P, T):
        cs = ar.gather(c_cells[None], [0], [(dy, -dt)], w)[0, 0].astype(np.uint8)
        d = int((cs != q_cells).sum())
        if best is None or d < best[0]:
            best = (d, (dy, dt), int((cs & q_cells).sum()))
    return best


def random_roll(rng, h, w, density=0.04):
    """Short notes: runs of 1 to 8 steps in one row, a few percent of the cells."""
    c = np.zeros((h, w), np.uint8)
    for _ in range(max(1, int(density * h * w / 4.5))):
        y, t0, n = int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(1, 9))
        c[y, t0:t0 + n] = 1
    return c


def make_case(rng, Q, N, h, w, P, T):
    """(query planes [Q,h,w/8], roll planes [N,h,w/8]).  Roll 0 is empty, roll 3 a copy of roll 1, roll N-1 full.  Queries cycle
    through: a roll shifted by a draw inside the window with three cells flipped; a roll shifted by (P+1, -(T+1)), just outside
    it; a fresh random roll; an exact shifted copy - and every eighth query is empty."""
    rolls = np.stack([random_roll(rng, h, w) for _ in range(N)])
    if N > 1:
        rolls[N - 1] = 1
    if N > 3:
        rolls[3] = rolls[1]
    rolls[0] = 0
    queries = np.zeros((Q, h, w), np.uint8)
    for i in range(Q):
        j = int(rng.integers(N))
        dy, dt = int(rng.integers(-P, P + 1)), int(rng.integers(-T, T + 1))
        if i % 8 == 7:
            continue
        if i % 4 == 0:
            q = shifted(rolls[j], dy, dt)
            for _ in range(3):
                q[int(rng.integers(h)), int(rng.integers(w))] ^= 1
        elif i % 4 == 1:
            q = shifted(rolls[j], P + 1, -(T + 1))
        elif i % 4 == 2:
            q = random_roll(rng, h, w)
        else:
            q = shifted(rolls[j], dy, dt)
        queries[i] = q
    return pack(queries), pack(rolls)


SHAPES = [(1, 32), (3, 32), (5, 64), (4, 96), (16, 128), (128, 128)]
WINDOWS = [(0, 0), (2, 0), (0, 3), (2, 3)]
SIZES = [(1, 1, 1), (5, 7, 3), (9, 70, 4)]


def sweep_cases():
    """(h, w, P, T, Q, N, k) of the sweep; a window is clipped to the frame (P <= h-1); 128x128 runs window (2, 3) at (9, 70, 4) only."""
    for h, w in SHAPES:
        for P, T in WINDOWS:
            for Q, N, k in SIZES:
                if (h, w) == (128, 128) and ((P, T) != (2, 3) or (Q, N, k) != (9, 70, 4)):
                    continue
                yield h, w, min(P, h - 1), T, Q, N, k
