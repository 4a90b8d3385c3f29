"""Diagnostic (GPU box): time of evaluation.latent_statistics (vae_latent_stats) against a torch-on-GPU restatement of the same
estimator (f32, queries in chunks, torch.logsumexp over the components) at N in {4096, 16384}, L in {16, 128}, S = 1.  Device events
around whole calls after warm-up; prints one JSON line per shape with both times, the HIP path's share of the arithmetic floor
(N^2 L triples at 4.9e12 per second: 6 plain VALU + one v_exp_f32 each over 1024 SIMDs at 2.4 GHz) and the largest
differences between the two routes.  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diag/gpu_latent_stats.py` (LSTAT_REPS=1 keeps the trace short)."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from torch_vae_amd.evaluation import latent_statistics

REPS = int(os.environ.get("LSTAT_REPS", "5"))
FLOOR_TRIPLES_PER_S = 4.9e12
LOG_2PI = math.log(2 * math.pi)


def torch_route(mu, lv, eps):
    N, L = mu.shape
    z = (eps[0] * torch.exp(0.5 * lv) + mu)
    iv, c = torch.exp(-lv), -0.5 * (LOG_2PI + lv)
    cq = max(1, (1 << 28) // (N * L))          # 1 GiB of f32 per [cq, N, L] temporary
    lq, lqd = torch.empty(N, device=mu.device), torch.empty(N, L, device=mu.device)
    for q0 in range(0, N, cq):
        a = c - 0.5 * (z[q0:q0 + cq, None, :] - mu) ** 2 * iv
        lq[q0:q0 + cq] = torch.logsumexp(a.sum(-1), 1) - math.log(N)
        lqd[q0:q0 + cq] = torch.logsumexp(a, 1) - math.log(N)
    return lq, lqd


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n, out


for N in (4096, 16384):
    for L in (16, 128):
        g = torch.Generator(device="cuda").manual_seed(N + L)
        mu = torch.randn(N, L, device="cuda", generator=g) * torch.rand(L, device="cuda", generator=g) * 2
        lv = torch.rand(N, L, device="cuda", generator=g) * 4 - 3
        eps = torch.randn(1, N, L, device="cuda", generator=g)
        ours = lambda: latent_statistics(mu, lv, eps=eps)
        theirs = lambda: torch_route(mu, lv, eps)
        timed(ours, 1)
        timed(theirs, 1)
        t_ours, res = timed(ours, REPS)
        t_torch, (lq, lqd) = timed(theirs, max(1, REPS // 2))
        floor_ms = 1e3 * N * N * L / FLOOR_TRIPLES_PER_S
        print(json.dumps({"N": N, "L": L, "S": 1, "reps": REPS, "latent_stats_ms": t_ours, "torch_chunked_logsumexp_ms": t_torch,
                          "speedup": t_torch / t_ours, "floor_ms": floor_ms, "fraction_of_floor": floor_ms / t_ours,
                          "max_abs_diff_log_qz": float((res["log_qz"][0] - lq.double()).abs().max()),
                          "max_abs_diff_log_qz_dims": float((res["log_qz_dims"][0] - lqd.double()).abs().max()),
                          "mi": float(res["mi"]), "tc": float(res["tc"]), "dwkl": float(res["dwkl"]), "kl": float(res["kl"]),
                          "active_units": res["active_units"]}), flush=True)
