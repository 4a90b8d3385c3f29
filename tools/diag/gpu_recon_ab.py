"""Diagnostic (GPU box): step time of the BCE and MSE reconstruction terms at the bench configuration (128x128, L=16, B=256,
bf16).  One process, one model; fused_train_step timed with device events in alternating BCE / MSE blocks after warm-up, so
clock and thermal drift fall on both alike.  Prints one JSON line: ms/step per block, medians and the MSE / BCE ratio."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from torch_vae_amd.models import VanillaVAE
from torch_vae_amd.optim import FusedAdamW
from torch_vae_amd.train import SyntheticPianorollLoader

H, L, B = 128, 16, 256
BLOCKS = int(os.environ.get("RECON_AB_BLOCKS", "5"))
STEPS = int(os.environ.get("RECON_AB_STEPS", "200"))
WARMUP = 30

model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).cuda()
opt = FusedAdamW([{"params": model.encoder.parameters()}, {"params": model.decoder.parameters()}], lr=1e-4, weight_decay=0.0)
x = SyntheticPianorollLoader(B, H, 1, seed=3, device="cuda").batch(0)[0]
vel = x * torch.rand_like(x).mul_(0.8).add_(0.2)        # velocity-valued targets for the MSE blocks


def block(kind, n):
    model.recon_loss = kind
    xb = vel if kind == "mse" else x
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        model.fused_train_step(opt, xb)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


for kind in ("bce", "mse"):
    block(kind, WARMUP)
res = {"bce": [], "mse": []}
for i in range(BLOCKS):
    for kind in (("bce", "mse") if i % 2 == 0 else ("mse", "bce")):
        res[kind].append(block(kind, STEPS))
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
out3, _ = model.fused_train_step(opt, x)
torch.cuda.synchronize()
assert all(map(lambda v: v == v, out3.tolist())), out3
print(json.dumps({"config": f"{H}x{H} L={L} B={B} bf16", "steps_per_block": STEPS, "ms_per_step": res, "median": med,
                  "mse_over_bce": med["mse"] / med["bce"]}), flush=True)
