"""numpy float64 reference of the set-level fidelity metrics (include/vae_fidelity.h, torch_vae_amd/fidelity.py), computed from the
float32 inputs by brute force, and the inputs of the GPU tests: generated once per process and shared (gpu_cases()), never changed.

Error bounds of the device against this reference, u = 2^-24 (derived in DESIGN.md, "Set-level fidelity"):
  d2                within (D + 2) u relative
  radii2, nearest_d2  within TOL(D) = 2 (D + 2) u relative (an order statistic moves by no more than its elements do)
  sums[g] / pairs   within ((D + 3) / e + 4) u absolute;  sums[G] within (D + 3) u relative
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
DIMS = (1, 3, 16, 67, 128)
SHAPES = ((193, 131), (65, 64), (7, 300), (2, 1))      # (n, m): points of A, points of B
KS = (1, 3, 8)
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
UNDECIDED_CAP = 1e-3                                   # share of a Gaussian case's pairs that may sit within TOL of a ball's boundary
# seeds of the self-consistency sets A ~ N(0, I) [193, D]: for k in KS the k-th and (k+1)-th neighbour distances of every row differ by
# more than 2 TOL(D) relative (found by trying 2000 + D, 2001 + D, ...; tests/test_fidelity_host.py asserts the condition)
CONSISTENCY_N = 193
CONSISTENCY_SEEDS = {1: 2001, 3: 2003, 16: 2016, 67: 2067, 128: 2131}


def tol(D):
    return 2 * (D + 2) * U


def kernel_bound(D):
    return ((D + 3) / math.e + 4) * U


def dist_sum_bound(D):
    return (D + 3) * U


def d2(a, b):
    """[n, m] float64 squared distances of float32 points; non-finite coordinates give what IEEE arithmetic gives"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = a[:, None, :] - b[None, :, :]
        return (diff * diff).sum(-1)


def _without_diagonal(m, fill):
    m = m.copy()
    k = min(m.shape)
    m[np.arange(k), np.arange(k)] = fill
    return m


def radii(x, k):
    """the k-th smallest d2(x_i, x_j) over j != i: np.partition(row, k) of the row with itself included (the published PRDC
    code) when every distance is finite; by index exclusion, NaN never a neighbour, when not"""
    m = d2(x, x)
    if np.isfinite(m).all():
        return np.partition(m, k, axis=1)[:, k]
    return radii_by_exclusion(x, k)


def radii_by_exclusion(x, k):
    m = _without_diagonal(d2(x, x), np.inf)
    m[np.isnan(m)] = np.inf
    return np.partition(m, k - 1, axis=1)[:, k - 1]


def counts(dist, rad, exclude=False, scale=1.0, strict=False):
    """[m] number of j with dist[i, j] <= rad[j] * scale (< when strict); a NaN is in no ball"""
    with np.errstate(invalid="ignore"):
        inside = dist < rad[None, :] * scale if strict else dist <= rad[None, :] * scale
    if exclude:
        inside = _without_diagonal(inside, False)
    return inside.sum(1).astype(np.int64)


def nearest(dist, exclude=False):
    """(index [m] (lowest on a tie; -1 if no distance is finite), distance [m], second smallest distance [m])"""
    m = dist.copy()
    m[np.isnan(m)] = np.inf
    if exclude:
        m = _without_diagonal(m, np.inf)
    idx = m.argmin(1)
    best = m[np.arange(m.shape[0]), idx]
    second = np.partition(m, 1, axis=1)[:, 1] if m.shape[1] > 1 else np.full(m.shape[0], np.inf)
    return np.where(np.isfinite(best), idx, -1), best, second


def kernel_sums(dist, gammas, exclude=False):
    """[G + 1]: sum exp(-gamma d2) per gamma, then sum d2"""
    keep = np.ones(dist.shape, dtype=bool)
    if exclude:
        keep = _without_diagonal(keep, False)
    v = dist[keep]
    with np.errstate(invalid="ignore"):
        return np.array([np.exp(-g * v).sum() for g in gammas] + [v.sum()])


def pairs(n, m, exclude=False):
    return n * m - (min(n, m) if exclude else 0)


def default_gammas(dist):
    return [1.0 / (s * dist.mean()) for s in SCALES]


def mmd2(x, y, gammas=None):
    """per gamma: sum' K_xx / (n (n-1)) + sum' K_yy / (m (m-1)) - 2 sum K_xy / (n m)"""
    n, m = len(x), len(y)
    xy = d2(x, y)
    gammas = default_gammas(xy) if gammas is None else gammas
    G = len(gammas)
    return (kernel_sums(d2(x, x), gammas, True)[:G] / (n * (n - 1)) + kernel_sums(d2(y, y), gammas, True)[:G] / (m * (m - 1))
            - 2 * kernel_sums(xy, gammas)[:G] / (n * m))


def prdc(real, fake, k, r_real=None, r_fake=None):
    """precision, recall, density, coverage; the radii default to radii(., k) rounded to float32 (what the device holds)"""
    r_real = radii(real, k).astype(np.float32).astype(np.float64) if r_real is None else r_real
    r_fake = radii(fake, k).astype(np.float32).astype(np.float64) if r_fake is None else r_fake
    fr, rf = d2(fake, real), d2(real, fake)
    in_real, in_fake = counts(fr, r_real), counts(rf, r_fake)
    return dict(precision=(in_real > 0).mean(), recall=(in_fake > 0).mean(), density=in_real.sum() / (k * len(fake)),
                coverage=(nearest(rf)[1] <= r_real).mean())


def moments(x):
    """mean and the covariance about it (divided by n, as the mixture's M-step has it)"""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(0)
    c = x - mean
    return mean, c.T @ c / len(x)


def _sqrt_psd(s):
    w, v = np.linalg.eigh((s + s.T) / 2)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet(m1, s1, m2, s2):
    h = _sqrt_psd(s1)
    inner = h @ s2 @ h
    w = np.linalg.eigvalsh((inner + inner.T) / 2)
    return float((m1 - m2) @ (m1 - m2) + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(w, 0.0, None)).sum())


def frechet_distance(x, y):
    return frechet(*moments(x), *moments(y))


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def lattice(rng, n, D):
    """integers over 8: every difference, square and sum below is exact in float32 in any order (|c| <= 16: a d2 is at most
    128 * 1024 / 64).  A narrow range where D is large, so that ties stay common; every fifth point repeats an earlier one."""
    top = 16 if D <= 3 else 2
    x = rng.integers(-top, top + 1, size=(n, D)).astype(np.float32) / 8
    for i in range(4, n, 5):
        x[i] = x[rng.integers(0, i)]
    return x


def gaussian_pair(D, n, m):
    rng = np.random.default_rng(1000 + D)
    return rng.standard_normal((n, D)).astype(np.float32), (0.9 * rng.standard_normal((m, D)) + 0.3).astype(np.float32)


def consistency_set(D, seed=None):
    seed = CONSISTENCY_SEEDS[D] if seed is None else seed
    return np.random.default_rng(seed).standard_normal((CONSISTENCY_N, D)).astype(np.float32)


def consistency_gap_ok(x, D):
    """for every k of KS: the k-th and (k+1)-th neighbour distances of every row differ by more than 2 TOL relative"""
    m = np.sort(_without_diagonal(d2(x, x), np.inf), axis=1)
    return all(((m[:, k] - m[:, k - 1]) > 2 * tol(D) * m[:, k]).all() for k in KS)


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _case(kind, D, n, m):
    if kind == "lattice":
        rng = np.random.default_rng(77 + 1000 * D + n)
        a, b = lattice(rng, n, D), lattice(rng, m, D)
        b[: min(m, 3)] = a[: min(m, 3)]                      # points the two sets share: distance 0 across the sets
    else:
        a, b = gaussian_pair(D, n, m)
    ab, aa = d2(a, b), d2(a, a)
    c = dict(kind=kind, D=D, n=n, m=m, a=a, b=b, ab=ab, aa=aa, radii={}, ball_radii={}, counts={}, self_counts={})
    for k in KS:
        if k < n:
            c["radii"][k] = radii(a, k)
        # the balls around B's points: B's own k-NN radii where B has more than k points, else a quantile of the cross distances;
        # float32, so that the device and the reference hold the same numbers
        rb = radii(b, k) if k < m else np.full(m, np.quantile(ab, 0.3))
        rb = _f32(rb)
        c["ball_radii"][k] = rb
        c["counts"][k] = counts(ab, rb.astype(np.float64))
        if k < n:
            ra = _f32(c["radii"][k])
            c["self_counts"][k] = counts(aa, ra.astype(np.float64), exclude=True)
    c["nearest"], c["nearest_self"] = nearest(ab), nearest(aa, exclude=True)
    c["gammas"] = default_gammas(ab) + [0.0, 0.01, 3.0 / max(ab.mean(), 1e-30)]           # 8 bandwidths, one of them 0
    c["sums"], c["sums_self"] = kernel_sums(ab, c["gammas"]), kernel_sums(aa, c["gammas"], exclude=True)
    return c


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """{(kind, D, n, m): case}: the inputs and every reference result the GPU tests compare against"""
    return {(kind, D, n, m): _case(kind, D, n, m) for kind in ("lattice", "gaussian") for D in DIMS for n, m in SHAPES}


def undecided(c, k):
    """cross-set pairs of a case within TOL of a ball's boundary: their membership may differ between the device and the reference.
    (Within a set the k-th neighbour of every point sits ON the boundary of that point's ball by construction.)"""
    t = tol(c["D"])
    rb = c["ball_radii"][k].astype(np.float64)
    return int((np.abs(c["ab"] - rb[None, :]) <= t * rb[None, :]).sum())


@functools.lru_cache(maxsize=None)
def frechet_cases():
    """two well-conditioned pairs [512, 16]: Gaussians whose covariances have eigenvalues in [0.25, 4]"""
    out = []
    for seed in (31, 32):
        rng = np.random.default_rng(seed)
        sets = []
        for _ in range(2):
            q, _ = np.linalg.qr(rng.standard_normal((16, 16)))
            root = (q * np.sqrt(rng.uniform(0.25, 4.0, 16))) @ q.T
            sets.append((rng.standard_normal((512, 16)) @ root + rng.uniform(-1, 1, 16)).astype(np.float32))
        out.append(tuple(sets))
    return out
