"""Diagnostic (GPU box): cost record of the denoising objective (include/vae_denoise.h, vae_set_recon_target; torch_vae_amd/denoise.py).
Parts, written as text to profiles/denoise_cost.txt (or --out); nothing here is a gate:
  1. device code - registers, scratch and LDS of the kernels from a device-only compile of csrc/vae_denoise.hip with
     -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU);
  2. default path unchanged - bench.py --gpus 1 --steps 200 --warmup 20 in a built checkout of the parent commit (--parent DIR) and
     in this tree, one process per run, alternating; skipped when no parent tree is given;
  3. the one-call training step - ms/step of train.fused_step at the bench workload (128x128, latent 16, batch 256, bf16) in the parent
     tree, in this tree without a target, in this tree with a target (the corrupted batches made beforehand), and in this tree with
     the corruption launch inside the loop; each figure from a process of its own (this file with --step-timing), --rounds rounds,
     the rows alternating within a round, so that the parent's own spread is on the page beside every difference;
  4. vae_denoise_corrupt on its own at 256 rolls of 128x128, every corruption alone and all together, and the bytes per second that is.
Device times are events around back-to-back calls, the median of --blocks blocks after warm-up."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), help="tree whose package is imported")
ap.add_argument("--out", default=None)
ap.add_argument("--parent", default=None, help="built checkout of the parent commit")
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--step-timing", default=None, metavar="MODE", help="internal: print the ms/step of fused_step; MODE plain, target or corrupt+target")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
CORRUPTION = dict(note_dropout=0.3, span=(16, 32), add_noise=0.01)


def med(v):
    return sorted(v)[len(v) // 2]


def step_timing(mode, steps=200, warmup=20):
    """bench.py's loop (same model, optimiser, batches) through train.fused_step"""
    from argparse import Namespace
    import torch
    from torch_vae_amd.models import VanillaVAE
    from torch_vae_amd.train import SyntheticPianorollLoader, build_optimizer, fused_step
    H, L, B, dev = 128, 16, 256, torch.device("cuda:0")
    torch.manual_seed(0)
    model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).to(dev)
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle", epochs=1,
                    freeze_encoder=False)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=steps + warmup + 8)
    pool = SyntheticPianorollLoader(B, H, n_batches=4, seed=0, device=dev, pool=4)
    batches = [pool.batch(i)[0] for i in range(4)]
    model.eps_seed = 7919
    if mode == "plain":
        def step(i):
            return fused_step(model, opt, batches[i % 4])
    else:
        from torch_vae_amd.denoise import corrupt_rolls
        made = [corrupt_rolls(x, counter0=B * i, **CORRUPTION) for i, x in enumerate(batches)]
        if mode == "target":
            def step(i):
                return fused_step(model, opt, made[i % 4], target=batches[i % 4])
        else:
            def step(i):
                return fused_step(model, opt, corrupt_rolls(batches[i % 4], counter0=B * i, **CORRUPTION), target=batches[i % 4])
    for i in range(warmup):
        step(i); sched.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out3, _ = step(i); sched.step()
    host = 1e3 * (time.perf_counter() - t0) / steps
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    print(json.dumps({"mode": mode, "ms_per_step": round(ms, 4), "host_enqueue_ms_per_step": round(host, 4), "loss": out3.tolist()}))


if args.step_timing is not None:
    step_timing(args.step_timing)
    sys.exit(0)

OUT = args.out or os.path.join(ROOT, "profiles", "denoise_cost.txt")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def last_json(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


# ---- 1. device code
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
csrc = os.path.join(ROOT, "torch_vae_amd", "csrc")
flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result"]
say(f"Device code (no GPU; hipcc {' '.join(flags)} --cuda-device-only -Rpass-analysis=kernel-resource-usage, csrc/vae_denoise.hip):")
try:
    err = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "vae_denoise.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, timeout=600, check=True).stderr
    fields = {"VGPRs": r" VGPRs: (\d+)", "SGPRs": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
              "static LDS": r"LDS Size \[bytes/block\]: (\d+)", "waves/SIMD": r"Occupancy \[waves/SIMD\]: (\d+)"}
    say("  kernel                        " + "  ".join(f"{k:<10s}" for k in fields))
    for blk in re.split(r"remark: Function Name: ", err)[1:]:
        m = re.search(r"(denoise_\w+_kernel)", blk.split()[0])
        if m:
            say(f"  {m.group(1):<30s}" + "  ".join(f"{re.search(p, blk).group(1):<10s}" for p in fields.values()))
except (OSError, subprocess.SubprocessError) as e:
    say(f"  not available in this run ({type(e).__name__})")
say()

# ---- 2. and 3.: processes of their own, before this one opens the GPU
if args.parent:
    res = {"parent": [], "new": []}
    for i in range(args.bench_runs):
        for tag in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=args.parent if tag == "parent" else ROOT,
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            res[tag].append(last_json(out))
            print(f"bench {tag} run {i + 1}: {res[tag][-1]['ms_per_step']} ms/step", file=sys.stderr, flush=True)
    say("Default path: python bench.py --gpus 1 --steps 200 --warmup 20, parent and this commit each in its own built tree, one process per run,")
    say(f"processes alternating; {args.bench_runs} runs each.")
    say("  run   parent ms_per_step  samples/s  |  new ms_per_step  samples/s")
    for a, b in zip(res["parent"], res["new"]):
        say(f"        {a['ms_per_step']:<18.4f} {a['value']:<10.1f} |  {b['ms_per_step']:<16.4f} {b['value']:.1f}")
    pm, nm = med([r["ms_per_step"] for r in res["parent"]]), med([r["ms_per_step"] for r in res["new"]])
    lo, hi = min(r["ms_per_step"] for r in res["parent"]), max(r["ms_per_step"] for r in res["parent"])
    say(f"  median  {pm:.4f} | {nm:.4f};  parent's own band (min .. max) {lo:.4f} .. {hi:.4f};  new median - parent median {nm - pm:+.4f} "
        f"({'inside' if lo <= nm <= hi else 'outside'} the band)")
    say()

rows = ([("parent, one call per step", args.parent, "plain")] if args.parent else []) + [
    ("this tree, no target", ROOT, "plain"), ("this tree, target (corruption made beforehand)", ROOT, "target"),
    ("this tree, corrupt_rolls + target in the loop", ROOT, "corrupt+target")]


def timing(tree, mode):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--step-timing", mode], check=True, capture_output=True,
                         text=True, timeout=300).stdout
    return last_json(out)


say("One-call training step: train.fused_step, 128x128, latent 16, batch 256, bf16, 200 steps after 20 (bench.py's loop), a process per figure,")
say(f"{args.rounds} rounds, the rows in turn within a round (ms/step wall clock, host enqueue ms/step in brackets); corruption: {CORRUPTION}:")
got = {name: [] for name, *_ in rows}
for _ in range(args.rounds):
    for name, tree, mode in rows:
        got[name].append(timing(tree, mode))
for name, *_ in rows:
    v = [r["ms_per_step"] for r in got[name]]
    say(f"  {name:<50s}" + "   ".join(f"{r['ms_per_step']:.4f} ({r['host_enqueue_ms_per_step']:.4f})" for r in got[name]) +
        f"   median {med(v):.4f}, spread {max(v) - min(v):.4f}")
base_name = rows[0][0]
base = med([r["ms_per_step"] for r in got[base_name]])
for name, *_ in rows[1:]:
    say(f"  {name}: {med([r['ms_per_step'] for r in got[name]]) - base:+.4f} ms/step against '{base_name}' (medians)")
say(f"  expected from the code for a target: one more read of B*H*W*4 = {256 * 128 * 128 * 4 / 1e6:.1f} MB per step")
say()

import torch  # noqa: E402

from torch_vae_amd.denoise import corrupt_rolls  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps, blocks=args.blocks):
    """median over blocks of the mean ms of `reps` back-to-back calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return med(out)


# ---- 4. the corruption launch on its own
from torch_vae_amd.train import SyntheticPianorollLoader  # noqa: E402

x = SyntheticPianorollLoader(256, 128, n_batches=1, seed=0, device=dev).batch(0)[0]
say("vae_denoise_corrupt (corrupt_rolls: the output allocated per call), 256 synthetic rolls of 128x128 f32, one launch:")
for name, kw in (("copy (everything off)", {}), ("note dropout 0.3", dict(note_dropout=0.3)), ("span 16..32", dict(span=(16, 32))),
                 ("spurious cells 0.01", dict(add_noise=0.01)), ("all three", CORRUPTION), ("all three + hidden mask", dict(CORRUPTION, return_hidden=True))):
    ms = timed(lambda: corrupt_rolls(x, **kw), 200)
    say(f"  {name:<26s} {ms * 1e3:8.1f} us per call   {2 * x.numel() * 4 / ms / 1e6:8.1f} GB/s (read + written)")

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
