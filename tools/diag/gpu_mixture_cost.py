"""Diagnostic (GPU box): cost of the latent mixture (include/vae_mixture.h) - one EM iteration (factor, E-step, M-step) and one
sample() of n draws - at (n, L, K) = (50 000, 16, 10) and (50 000, 128, 10), full covariances, against a torch-on-GPU restatement
of the same arithmetic (torch.linalg.cholesky / solve_triangular, einsum, logsumexp; f32 products, f64 constants).  Device events
around whole calls after a warm-up of every shape; the two routes alternate inside one process and the spread over the repeats is
printed with the median.  An EM iteration is the difference between an EM call of 1 + ITERS iterations and one of 1, over ITERS
(the call's closing factorisation drops out).  Writes profiles/latent_mixture_cost.txt (or MIXTURE_COST_OUT), with the float32
emulation gaps the GPU tests' tolerances come from (tests/test_mixture_gpu.py: GAPS).  No ratio is promised by anything; the file is
the record.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diag/gpu_mixture_cost.py`
(MIXTURE_REPS=1 keeps the trace short)."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from torch_vae_amd import _lib
from torch_vae_amd.mixture import LatentMixture

REPS = int(os.environ.get("MIXTURE_REPS", "7"))
ITERS = 10
OUT = os.environ.get("MIXTURE_COST_OUT", os.path.join(ROOT, "profiles", "latent_mixture_cost.txt"))
LOG2PI = math.log(2 * math.pi)
MATRIX_F32_FLOPS = 157.3e12      # exact-f32 MFMA peak (the f32 vector rate)


def clusters(n, L, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = 1.5 * torch.randn(K, L, device="cuda", generator=g)
    maps = torch.eye(L, device="cuda") + 0.5 * torch.randn(K, L, L, device="cuda", generator=g) / math.sqrt(L)
    which = torch.arange(n, device="cuda") % K
    e = torch.randn(n, L, device="cuda", generator=g)
    x = torch.empty(n, L, device="cuda")
    for k in range(K):
        sel = which == k
        x[sel] = centres[k] + e[sel] @ maps[k].T
    return x.contiguous()


def em_call(x, mix, iters, hist):
    n, L = x.shape
    dev = x.device
    _lib.check(_lib.lib().vae_mixture_em(x.data_ptr(), n, L, mix.components, 0, iters, 1e-6, mix.weights.data_ptr(), mix.means.data_ptr(),
                                         mix.covariances.data_ptr(), mix.cholesky.data_ptr(), mix._winv.data_ptr(), mix._winv32.data_ptr(),
                                         mix._logdet.data_ptr(), mix._status.data_ptr(), hist.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream), "vae_mixture_em")


def torch_iteration(x, pi, m, S, reg=1e-6):
    """one EM iteration in plain torch on the device: f64 factor, f32 pairwise products, f64 logsumexp, f32 weighted sums"""
    n, L = x.shape
    K = pi.shape[0]
    C = torch.linalg.cholesky(S)
    W = torch.linalg.solve_triangular(C, torch.eye(L, device=x.device, dtype=torch.float64).expand(K, L, L), upper=False)
    logdet = -torch.log(torch.diagonal(C, dim1=1, dim2=2)).sum(1)
    d = x[:, None, :] - m.float()[None, :, :]                                  # [n, K, L]
    y = torch.einsum("kdj,nkj->nkd", W.float(), d)
    lp = (torch.log(pi) + logdet - 0.5 * L * LOG2PI)[None, :] - 0.5 * (y * y).sum(-1).double()
    lse = torch.logsumexp(lp, 1)
    r = torch.exp(lp - lse[:, None]).float()
    N = r.double().sum(0) + 10 * torch.finfo(torch.float64).eps
    m2 = (r.T @ x).double() / N[:, None]
    d2 = x[:, None, :] - m2.float()[None, :, :]
    S2 = torch.einsum("nki,nkj->kij", r[:, :, None] * d2, d2).double() / N[:, None, None] + reg * torch.eye(L, device=x.device, dtype=torch.float64)
    return N / n, m2, S2, lse.mean()


def torch_sample(pi, m, C, n, gen):
    comp = torch.multinomial(pi.float(), n, replacement=True, generator=gen)
    eps = torch.randn(n, m.shape[1], device=m.device, generator=gen)
    return m.float()[comp] + torch.einsum("ndj,nj->nd", C.float()[comp], eps)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def summary(ts):
    return f"median {statistics.median(ts):8.3f} ms  (min {min(ts):8.3f}, max {max(ts):8.3f}, {len(ts)} repeats)"


lines = ["latent mixture: one EM iteration and one sample() against a torch-on-GPU restatement; device events around whole calls,",
         f"routes alternating in one process, {REPS} repeats after a warm-up of each.  tools/diag/gpu_mixture_cost.py", ""]
for n, L, K in ((50000, 16, 10), (50000, 128, 10)):
    x = clusters(n, L, K, 5 + L)
    mix0 = LatentMixture.fit(x, K, iters=2)
    hist = torch.empty(1 + ITERS, device="cuda", dtype=torch.float64)

    def ours(iters):
        mix = LatentMixture(mix0.weights.clone(), mix0.means.clone(), mix0.covariances.clone())
        return timed(lambda: em_call(x, mix, iters, hist))[0], mix

    def theirs():
        pi, m, S = mix0.weights.clone(), mix0.means.clone(), mix0.covariances.clone()

        def run():
            nonlocal pi, m, S
            for _ in range(2):
                pi, m, S, ll = torch_iteration(x, pi, m, S)
            return pi, m, S
        return timed(run)[0] / 2, (pi, m, S)

    ours(1); ours(1 + ITERS); theirs()
    t1, tn, tt = [], [], []
    for _ in range(REPS):
        t1.append(ours(1)[0]); tn.append(ours(1 + ITERS)[0]); tt.append(theirs()[0])
    per_iter = [(b - a) / ITERS for a, b in zip(t1, tn)]
    # agreement of the two routes after two iterations from the same state
    _, mix2 = ours(2)
    _, (pi_t, m_t, S_t) = theirs()
    flops = 2.0 * n * K * L * L            # E-step (triangular: half of 2 n K L^2) + SYRK (lower tiles: the other half)
    lines += [f"(n, L, K) = ({n}, {L}, {K}), full covariances",
              f"  EM iteration, HIP   : {summary(per_iter)}",
              f"  EM call, 1 iteration: {summary(t1)}   (factor, E-step, M-step, factor)",
              f"  EM iteration, torch : {summary(tt)}",
              f"  torch / HIP (medians): {statistics.median(tt) / statistics.median(per_iter):.2f}",
              f"  n K L^2 multiply-adds of E-step + M-step at the f32 matrix peak: {1e3 * flops / MATRIX_F32_FLOPS:.4f} ms "
              f"({100 * 1e3 * flops / MATRIX_F32_FLOPS / statistics.median(per_iter):.1f} % of the HIP iteration)",
              f"  after 2 iterations, HIP vs torch: max |d weights| {float((mix2.weights - pi_t).abs().max()):.2e}, "
              f"max |d means| {float((mix2.means - m_t).abs().max()):.2e}, max |d cov| {float((mix2.covariances - S_t).abs().max()):.2e}"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    mix0.sample(n); torch_sample(mix0.weights, mix0.means, mix0.cholesky, n, gen)
    ts, tq = [], []
    for r in range(REPS):
        ts.append(timed(lambda: mix0.sample(n, seed=r))[0]); tq.append(timed(lambda: torch_sample(mix0.weights, mix0.means, mix0.cholesky, n, gen))[0])
    lines += [f"  sample({n}), HIP     : {summary(ts)}   (counter generator, f64 accumulation)",
              f"  sample({n}), torch   : {summary(tq)}   (multinomial + randn + gathered einsum, f32)", ""]
    print("\n".join(lines[-11:]), flush=True)

from tests.test_mixture_gpu import GAPS     # noqa: E402  (constants only: nothing runs at import)

lines += ["float32-emulation gaps of the numpy reference (python -m tests.mixture_ref), from which the GPU tests' tolerances are built:",
          "log_prob / log_resp gate 4 G + 1e-6 |ref|; EM against the reference's float64 trajectory at 10 x the em_* gap (+ 1e-12 on the weights)"]
for shape, g in GAPS.items():
    lines.append(f"  {shape}: " + "  ".join(f"{k} {v:.3e}" for k, v in g.items()))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", OUT)
