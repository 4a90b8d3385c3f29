"""Diagnostic (GPU box): step time of the plain and the positive-class-weighted BCE (pos_weight=None / 8) at the bench
configuration (128x128, L=16, B=256, bf16).  One process, one model, one batch; fused_train_step timed with device events in
alternating blocks after warm-up, so clock and thermal drift fall on both alike.  Prints one JSON line: ms/step per block, median,
spread (max - min over the blocks) per mode and the weighted / plain ratio of the medians."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from torch_vae_amd.models import VanillaVAE
from torch_vae_amd.optim import FusedAdamW
from torch_vae_amd.train import SyntheticPianorollLoader

H, L, B = 128, 16, 256
BLOCKS = int(os.environ.get("POS_WEIGHT_BLOCKS", "7"))
STEPS = int(os.environ.get("POS_WEIGHT_STEPS", "300"))
WARMUP = 50
MODES = {"plain": None, "weighted": 8.0}

model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).cuda()
opt = FusedAdamW([{"params": model.encoder.parameters()}, {"params": model.decoder.parameters()}], lr=1e-4, weight_decay=0.0)
x = SyntheticPianorollLoader(B, H, 1, seed=3, device="cuda").batch(0)[0]


def block(mode, n):
    model.pos_weight = MODES[mode]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        model.fused_train_step(opt, x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


for mode in MODES:
    block(mode, WARMUP)
res = {m: [] for m in MODES}
for i in range(BLOCKS):
    for mode in (("plain", "weighted") if i % 2 == 0 else ("weighted", "plain")):
        res[mode].append(block(mode, STEPS))
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
spread = {k: max(v) - min(v) for k, v in res.items()}
out3, _ = model.fused_train_step(opt, x)
torch.cuda.synchronize()
assert all(map(lambda v: v == v, out3.tolist())), out3
print(json.dumps({"config": f"{H}x{H} L={L} B={B} bf16 pos_weight 8 vs None", "steps_per_block": STEPS, "ms_per_step": res, "median": med,
                  "spread": spread, "weighted_minus_plain_us": 1e3 * (med["weighted"] - med["plain"]),
                  "weighted_over_plain": med["weighted"] / med["plain"]}), flush=True)
