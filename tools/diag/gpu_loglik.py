"""Diagnostic (GPU box): time of VanillaVAE.log_likelihood at 128x128, L=16, B=256, K=64 in bf16, against the torch route to the
same numbers - K eval-mode model(x) calls plus a per-sample torch BCE on each reconstruction.  Device events around whole calls
after warm-up; prints one JSON line (ms per call of each route, their ratio).  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diag/gpu_loglik.py` (LOGLIK_REPS=1 keeps the trace short)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.nn.functional as F

from torch_vae_amd.models import VanillaVAE
from torch_vae_amd.train import SyntheticPianorollLoader

H, L, B, K = 128, 16, 256, 64
REPS = int(os.environ.get("LOGLIK_REPS", "5"))

model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).cuda()
x = SyntheticPianorollLoader(B, H, 1, seed=3, device="cuda").batch(0)[0]


def ours():
    return model.log_likelihood(x, K, seed=11)


def torch_route():
    model.eval()
    acc = torch.zeros(B, device="cuda", dtype=torch.float64)
    with torch.no_grad():
        for _ in range(K):
            xhat = model(x)["output"]
            acc += F.binary_cross_entropy(xhat, x, reduction="none").sum((1, 2, 3)).double()
    return acc


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n, out


timed(ours, 1)
timed(torch_route, 1)
t_ours, res = timed(ours, REPS)
t_torch, _ = timed(torch_route, REPS)
ll = res["log_likelihood"]
assert bool(torch.isfinite(ll).all()), ll
print(json.dumps({"config": f"{H}x{H} L={L} B={B} K={K} bf16", "reps": REPS, "log_likelihood_ms": t_ours,
                  "torch_K_forwards_plus_bce_ms": t_torch, "speedup": t_torch / t_ours,
                  "mean_nll_nats": float(-ll.mean()), "mean_elbo_nats": float(res["elbo"].mean())}), flush=True)
