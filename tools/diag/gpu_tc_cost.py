"""Diagnostic: cost of the total-correlation objective (VanillaVAE.tc_weight, VAE_KL_TC) on the one-call training step
(train.fused_step) at the bench shape (H=128, L=16, B=256, bf16) and the beta-VAE shape (H=128, L=128, B=512, f16).  ms/step from
HIP events around 200 timed steps after warm-up, median of 3; modes off / tc / off in the same process.  Then one profiled TC step's
timeline (vae_profile_timeline: label, start ms, end ms), which shows whether the tc_* launches on the side stream end inside the
decoder forward's window.
Usage: python tools/diag/gpu_tc_cost.py [bench|beta|both]   (prints one JSON line per shape and mode, then the timeline)"""
import ctypes
import json
import os
import sys
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from torch_vae_amd import _lib  # noqa: E402
from torch_vae_amd.models import VanillaVAE  # noqa: E402
from torch_vae_amd.train import SyntheticPianorollLoader, build_optimizer, fused_step  # noqa: E402

WARMUP, STEPS, REPEATS = 30, 200, 3
SHAPES = {"bench": (128, 16, 256, "bf16"), "beta": (128, 128, 512, "f16")}


def measure(shape: str):
    H, L, B, dtype = SHAPES[shape]
    torch.manual_seed(0)
    model = VanillaVAE(1, L, H, kld_weight=4.0, generalised=True, compute_dtype=dtype, max_batch=B).cuda()
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                    epochs=1, freeze_encoder=False)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=100000)
    x = SyntheticPianorollLoader(B, H, 1, device="cuda").batch(0)[0]
    for mode in ("off", "tc", "off"):
        model.tc_weight = 6.0 if mode == "tc" else None
        for _ in range(WARMUP):
            fused_step(model, opt, x); sched.step()
        torch.cuda.synchronize()
        runs = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(STEPS):
                out3, _ = fused_step(model, opt, x); sched.step()
            e1.record()
            e1.synchronize()
            runs.append(e0.elapsed_time(e1) / STEPS)
        yield {"shape": shape, "H": H, "L": L, "B": B, "dtype": dtype, "mode": mode, "ms_per_step": sorted(runs)[len(runs) // 2],
               "runs": runs, "steps": STEPS, "out3": out3.tolist(), "tc": model.total_correlation().item(),
               "grads_finite": bool(torch.isfinite(model.flat_grads()).all())}
    # one profiled TC step: the launches in start order
    model.tc_weight = 6.0
    for _ in range(3):
        fused_step(model, opt, x)
    L_, h = _lib.lib(), model._ctx.handle
    L_.vae_profile(h, 1)
    fused_step(model, opt, x)
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 20)
    assert L_.vae_profile_timeline(h, buf, len(buf)) == 0
    L_.vae_profile(h, 0)
    rows = sorted(json.loads(buf.value.decode()), key=lambda r: r[1])
    yield {"shape": shape, "timeline": [[r[0], round(r[1], 4), round(r[2], 4)] for r in rows]}


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    for shape in {"bench": ("bench",), "beta": ("beta",), "both": ("bench", "beta")}[which]:
        for rec in measure(shape):
            print(json.dumps(rec), flush=True)
