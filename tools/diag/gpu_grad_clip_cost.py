"""Diagnostic: cost of gradient-norm clipping / non-finite skipping on the one-call training step (train.fused_step) at the
bench shape (H=128, L=16, B=256, bf16).  ms/step from HIP events around 200 timed steps after warm-up, options off and on.
Usage: python tools/diag/gpu_grad_clip_cost.py [off|on|both]   (prints one JSON line per mode)"""
import json
import os
import sys
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from torch_vae_amd.models import VanillaVAE  # noqa: E402
from torch_vae_amd.train import SyntheticPianorollLoader, build_optimizer, fused_step  # noqa: E402

H, L, B, WARMUP, STEPS, REPEATS = 128, 16, 256, 30, 200, 3


def measure(on: bool):
    torch.manual_seed(0)
    model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).cuda()
    extra = dict(max_grad_norm=1.0, skip_nonfinite=True) if on else {}
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                    epochs=1, freeze_encoder=False, **extra)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=100000)
    x = SyntheticPianorollLoader(B, H, 1, device="cuda").batch(0)[0]
    for _ in range(WARMUP):
        fused_step(model, opt, x); sched.step()
    torch.cuda.synchronize()
    runs = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            fused_step(model, opt, x); sched.step()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) / STEPS)
    rec = {"mode": "on" if on else "off", "ms_per_step": sorted(runs)[len(runs) // 2], "runs": runs, "steps": STEPS}
    if on:
        rec["last_grad_norm"] = float(opt.last_grad_norm)
        rec["skipped_steps"] = int(opt.skipped_steps)
    return rec


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    for on in {"off": (False,), "on": (True,), "both": (False, True)}[which]:
        print(json.dumps(measure(on)), flush=True)
