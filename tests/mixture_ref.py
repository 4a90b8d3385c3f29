"""numpy float64 restatement of the latent mixture (include/vae_mixture.h): factor, log_prob, M-step, sample, EM and the initial
state of ``LatentMixture.fit``, plus the data generator of the mixture tests.  ``f32=True`` emulates the kernels' float32 steps -
x - m, the products and sums of y = W (x - m) and q = |y|^2 (sequential, no FMA), the f32 log_resp, and the M-step's f32 products
summed in f32 over 64-point chunks - so that the distance between the two runs measures what float32 costs at a shape.

    python -m tests.mixture_ref        prints the gaps the GPU tests' gates are built from (tests/test_mixture_gpu.py)
"""
import functools

import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))
TINY = 10.0 * np.finfo(np.float64).eps
STREAM_U, STREAM_EPS = 811, 812
REG = 1e-6

# (n, L, K, kind) -> EM iterations of the test mixture.  The four middle full shapes (and the diagonal ones) run EM on the device.
SHAPES = {
    (64, 1, 1, "full"): 2,
    (257, 3, 2, "full"): 8,
    (300, 16, 5, "full"): 8,
    (515, 33, 4, "full"): 6,
    (400, 128, 3, "full"): 4,
    (70, 5, 64, "full"): 2,
    (300, 16, 5, "diag"): 6,
    (130, 200, 3, "diag"): 3,
}
EM_SHAPES = [(257, 3, 2, "full"), (300, 16, 5, "full"), (515, 33, 4, "full"), (400, 128, 3, "full"), (300, 16, 5, "diag"),
             (130, 200, 3, "diag")]


def shape_id(s):
    return f"{s[3]}-n{s[0]}-L{s[1]}-K{s[2]}"


@functools.lru_cache(maxsize=None)
def make_data(n, L, K, seed=0):
    """K Gaussian clusters (at most 8) with random full maps, float32 [n, L].  Point i belongs to cluster i mod (the clusters
    used), except that the points ``initial_state`` takes as the first means (seed 0) belong to one cluster each and lie near its
    centre (a twentieth of the cluster's spread).  With the data covariance as every component's first covariance the first
    E-step is a nearest-mean rule in the whitened space, where a typical member is sqrt(2 L) from a mean that is itself a typical
    member and the centres are only ~sqrt(2 K) apart: from such a start components collapse onto a handful of points."""
    from torch_vae_amd.data import epoch_indices
    rng = np.random.default_rng(1000 + seed)
    kc = min(K, 8)
    centres = 1.5 * rng.standard_normal((kc, L))
    maps = np.eye(L) + 0.5 * rng.standard_normal((kc, L, L)) / np.sqrt(L)     # singular values in about [0.5, 1.5]
    which = np.arange(n) % kc
    first = epoch_indices(n, seed=0, epoch=0)[:kc].numpy()
    which[first] = np.arange(kc)
    e = rng.standard_normal((n, L))
    e[first] *= 0.05
    x = centres[which] + np.einsum("nij,nj->ni", maps[which], e)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def factor(S, kind="full"):
    """-> C, W, logdet, status (1-based index of the first pivot <= 0, the pivot then taken as 1)."""
    S = np.asarray(S, np.float64)
    K = S.shape[0]
    status = np.zeros(K, np.int32)
    if kind == "diag":
        bad = ~(S > 0)
        for k in range(K):
            if bad[k].any():
                status[k] = int(np.argmax(bad[k])) + 1
        C = np.sqrt(np.where(bad, 1.0, S))
        return C, 1.0 / C, -np.log(C).sum(1), status
    L = S.shape[1]
    C = np.zeros_like(S)
    W = np.zeros_like(S)
    for k in range(K):
        c = C[k]
        for j in range(L):
            v = S[k, j:, j] - c[j:, :j] @ c[j, :j]
            piv = v[0]
            if not piv > 0:
                if not status[k]:
                    status[k] = j + 1
                piv = 1.0
            c[j, j] = np.sqrt(piv)
            c[j + 1:, j] = v[1:] / c[j, j]
        w = W[k]
        for i in range(L):
            rhs = np.zeros(L)
            rhs[i] = 1.0
            w[i] = (rhs - c[i, :i] @ w[:i]) / c[i, i]
    logdet = -np.log(np.einsum("kdd->kd", C)).sum(1)
    return C, W, logdet, status


def _q(x, m, W, kind, f32):
    """q[n, k] = |W_k (x_n - m_k)|^2"""
    K = m.shape[0]
    n, L = x.shape
    q = np.empty((n, K), np.float32 if f32 else np.float64)
    if not f32:
        x = x.astype(np.float64)
        for k in range(K):
            d = x - m[k]
            y = d * W[k] if kind == "diag" else d @ W[k].T
            q[:, k] = (y * y).sum(1)
        return q
    x = x.astype(np.float32)
    for k in range(K):
        d = x - m[k].astype(np.float32)
        w = W[k].astype(np.float32)
        acc = np.zeros(n, np.float32)
        if kind == "diag":
            y = d * w
            for j in range(L):
                acc = acc + y[:, j] * y[:, j]
        else:
            y = np.zeros((n, L), np.float32)
            for j in range(L):
                y = y + d[:, j:j + 1] * w[None, :, j]
            for j in range(L):
                acc = acc + y[:, j] * y[:, j]
        q[:, k] = acc
    return q


def log_prob(x, pi, m, W, logdet, kind="full", f32=False):
    """-> log_prob [n] f64, log_resp [n, K] (f32 when emulating), mean log_prob"""
    L = x.shape[1]
    q = _q(x, m, W, kind, f32).astype(np.float64)
    with np.errstate(divide="ignore"):
        lp = np.log(pi)[None, :] + logdet[None, :] - 0.5 * L * LOG2PI - 0.5 * q
    mx = lp.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(lp - mx).sum(1, keepdims=True)))[:, 0]
    lr = lp - lse[:, None]
    return lse, (lr.astype(np.float32) if f32 else lr), float(lse.mean())


def _chunk_sum(prod, f32):
    """sum over axis 0; emulation: f32 within 64-point chunks, f64 across"""
    if not f32:
        return prod.astype(np.float64).sum(0)
    n = prod.shape[0]
    pad = (-n) % 64
    if pad:
        prod = np.concatenate([prod, np.zeros((pad,) + prod.shape[1:], prod.dtype)])
    prod = prod.reshape((-1, 64) + prod.shape[1:])
    acc = np.zeros((prod.shape[0],) + prod.shape[2:], np.float32)
    for i in range(64):                      # in order, as the kernels' chains run
        acc = acc + prod[:, i]
    return acc.astype(np.float64).sum(0)


def mstep(log_resp, x, reg=REG, kind="full", f32=False):
    """-> pi [K], m [K, L], S ([K, L, L] or the variances [K, L])"""
    n, L = x.shape
    r = np.exp(log_resp.astype(np.float64))
    K = r.shape[1]
    N = r.sum(0) + TINY
    pi = N / n
    m = np.empty((K, L))
    S = np.empty((K, L, L) if kind == "full" else (K, L))
    for k in range(K):
        if f32:
            r32, x32 = r[:, k].astype(np.float32), x.astype(np.float32)
            m[k] = _chunk_sum(r32[:, None] * x32, True) / N[k]
            d = x32 - m[k].astype(np.float32)
            rd = r32[:, None] * d
            S[k] = (_chunk_sum(rd[:, :, None] * d[:, None, :], True) if kind == "full" else _chunk_sum(rd * d, True)) / N[k]
        else:
            x64 = x.astype(np.float64)
            m[k] = (r[:, k, None] * x64).sum(0) / N[k]
            d = x64 - m[k]
            S[k] = ((r[:, k, None] * d).T @ d if kind == "full" else (r[:, k, None] * d * d).sum(0)) / N[k]
        S[k] += reg * np.eye(L) if kind == "full" else reg
    return pi, m, S


def pick(pi, u):
    """component of every u: the first k whose cumulative weight exceeds u, the last one taking the remainder"""
    cum = np.cumsum(pi)
    return np.minimum((u[:, None] >= cum[None, :]).sum(1), len(pi) - 1).astype(np.int32), cum


def sample(pi, m, C, kind, temperature, u, eps):
    """-> z [n, L] f64, component [n], and the per-element bound scale |m_d| + t sum_j |C_dj eps_j|"""
    comp, _ = pick(pi, u)
    e = eps.astype(np.float64)
    if kind == "diag":
        ce, ace = C[comp] * e, np.abs(C[comp] * e)
    else:
        ce, ace = np.einsum("ndj,nj->nd", C[comp], e), np.einsum("ndj,nj->nd", np.abs(C[comp]), np.abs(e))
    return m[comp] + temperature * ce, comp, np.abs(m[comp]) + abs(temperature) * ace


def generated_draws(n, L, seed):
    """the u and eps the device generator gives (oracle.counter_uniform / counter_normal on the mixture's two streams)"""
    from oracle import vae_oracle as vo
    return vo.counter_uniform(n, seed, STREAM_U), vo.counter_normal(n * L, seed, STREAM_EPS).astype(np.float32).reshape(n, L)


def initial_state(x, K, reg=REG, kind="full", seed=0):
    """what LatentMixture.fit starts from: means at the first K indices of the epoch-0 permutation, the data covariance + reg I for
    every component (one M-step with a single component and log_resp = 0), uniform weights"""
    from torch_vae_amd.data import epoch_indices
    n = x.shape[0]
    first = epoch_indices(n, seed=seed, epoch=0)[:K].numpy()
    _, _, S1 = mstep(np.zeros((n, 1), np.float32), x, reg, kind)
    return np.full(K, 1.0 / K), x[first].astype(np.float64), np.repeat(S1, K, axis=0)


def em(x, pi, m, S, kind="full", iters=1, reg=REG, f32=False):
    """-> pi, m, S, ll_history [iters]"""
    hist = np.empty(iters)
    for it in range(iters):
        _, W, logdet, status = factor(S, kind)
        assert not status.any(), status
        _, lr, hist[it] = log_prob(x, pi, m, W, logdet, kind, f32)
        pi, m, S = mstep(lr, x, reg, kind, f32)
    return pi, m, S, hist


@functools.lru_cache(maxsize=None)
def case(shape):
    """Everything the tests of one shape share, computed once: data, initial state, the f64 EM result (the test mixture) with its
    factors, f64 log_prob / log_resp at it, the f32-emulated ones, the emulated EM trajectory, and the gaps."""
    n, L, K, kind = shape
    iters = SHAPES[shape]
    x = make_data(n, L, K)
    pi0, m0, S0 = initial_state(x, K, REG, kind)
    pi, m, S, hist = em(x, pi0, m0, S0, kind, iters)
    C, W, logdet, status = factor(S, kind)
    lp, lr, mean = log_prob(x, pi, m, W, logdet, kind)
    lp32, lr32, mean32 = log_prob(x, pi, m, W, logdet, kind, f32=True)
    epi, em_, eS, ehist = em(x, pi0, m0, S0, kind, iters, f32=True)
    sd = np.sqrt(np.einsum("kdd->kd", S) if kind == "full" else S)
    sc = sd[:, :, None] * sd[:, None, :] if kind == "full" else S
    gaps = dict(log_prob=float(np.abs(lp32 - lp).max()), log_resp=float(np.abs(lr32.astype(np.float64) - lr).max()),
                em_ll=float(np.abs(ehist - hist).max()), em_pi=float(np.abs(epi - pi).max()),
                em_mean=float((np.abs(em_ - m) / sd).max()), em_cov=float((np.abs(eS - S) / sc).max()))
    return dict(x=x, init=(pi0, m0, S0), pi=pi, m=m, S=S, hist=hist, C=C, W=W, logdet=logdet, status=status, log_prob=lp, log_resp=lr,
                mean=mean, log_resp32=lr32, gaps=gaps, iters=iters, min_weight=float(pi.min()))


if __name__ == "__main__":
    for s in SHAPES:
        c = case(s)
        g = c["gaps"]
        print(f"{shape_id(s)}: iters {c['iters']}  max|log p| {np.abs(c['log_prob']).max():.1f}  min weight {c['min_weight']:.3f}  "
              f"min ll step {np.diff(c['hist']).min() if c['iters'] > 1 else 0.0:.2e}")
        print("    G: " + "  ".join(f"{k} {v:.2e}" for k, v in g.items()))
