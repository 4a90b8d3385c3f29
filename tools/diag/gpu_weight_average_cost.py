"""Diagnostic (GPU box): cost record of the weight averaging (include/vae_average.h; torch_vae_amd/averaging.py).
Parts, written as text to profiles/weight_average_cost.txt (or --out); nothing here is a gate:
  1. device code - registers, scratch and LDS of the kernels from a device-only compile of csrc/vae_average.hip with
     -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU);
  2. default path unchanged - bench.py --gpus 1 --steps 200 --warmup 20 in a built checkout of the parent commit (--parent DIR) and
     in this tree, one process per run, alternating; skipped when no parent tree is given;
  3. the one-call training step - ms/step of train.fused_step at the bench workload (128x128, latent 16, batch 256, bf16) in the parent
     tree, in this tree without an average, with WeightAverage.update() after every step and after every 10th; each figure from a
     process of its own (this file with --step-timing), --rounds rounds, the rows alternating within a round, so that the parent's
     own spread is on the page beside every difference;
  4. vae_average_update on its own on the flagship model's two buffers, with the byte count the code predicts, 12 * (N + N_bn)
     (4 of src and 4 of avg read, 4 of avg written per float), beside the measured time; and vae_average_swap.
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
ap.add_argument("--step-timing", default=None, metavar="MODE", help="internal: print the ms/step of fused_step; MODE plain, avg1 or avg10")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
H, L, B = 128, 16, 256


def med(v):
    return sorted(v)[len(v) // 2]


def bench_model():
    import torch
    from torch_vae_amd.models import VanillaVAE
    torch.manual_seed(0)
    return VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).to(torch.device("cuda:0"))


def step_timing(mode, steps=200, warmup=20):
    """bench.py's loop (same model, optimiser, batches) through train.fused_step, with the averaging update behind the scheduler"""
    from argparse import Namespace
    import torch
    from torch_vae_amd.train import SyntheticPianorollLoader, build_optimizer, fused_step
    dev = torch.device("cuda:0")
    model = bench_model()
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle", epochs=1,
                    freeze_encoder=False)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=steps + warmup + 8)
    pool = SyntheticPianorollLoader(B, H, n_batches=4, seed=0, device=dev, pool=4)
    batches = [pool.batch(i)[0] for i in range(4)]
    model.eps_seed = 7919
    every = {"plain": 0, "avg1": 1, "avg10": 10}[mode]
    avg = None
    if every:
        from torch_vae_amd.averaging import WeightAverage
        avg = WeightAverage(model, kind="ema", decay=0.999)

    def step(i):
        out = fused_step(model, opt, batches[i % 4])
        sched.step()
        if every and (i + 1) % every == 0:
            avg.update(opt)
        return out
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out3, _ = step(i)
    host = 1e3 * (time.perf_counter() - t0) / steps
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    print(json.dumps({"mode": mode, "ms_per_step": round(ms, 4), "host_enqueue_ms_per_step": round(host, 4), "loss": out3.tolist(),
                      "n_averaged": None if avg is None else int(avg.n_averaged)}))


if args.step_timing is not None:
    step_timing(args.step_timing)
    sys.exit(0)

OUT = args.out or os.path.join(ROOT, "profiles", "weight_average_cost.txt")
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
say(f"Device code (no GPU; hipcc {' '.join(flags)} --cuda-device-only -Rpass-analysis=kernel-resource-usage, csrc/vae_average.hip):")
try:
    err = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "vae_average.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, timeout=600, check=True).stderr
    fields = {"VGPRs": r" VGPRs: (\d+)", "SGPRs": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
              "static LDS": r"LDS Size \[bytes/block\]: (\d+)", "waves/SIMD": r"Occupancy \[waves/SIMD\]: (\d+)"}
    say("  kernel                        " + "  ".join(f"{k:<10s}" for k in fields))
    for blk in re.split(r"remark: Function Name: ", err)[1:]:
        m = re.search(r"(average_\w+_kernel)", blk.split()[0])
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
    ("this tree, no average", ROOT, "plain"), ("this tree, update() after every step", ROOT, "avg1"),
    ("this tree, update() after every 10th step", ROOT, "avg10")]


def timing(tree, mode):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--step-timing", mode], check=True, capture_output=True,
                         text=True, timeout=300).stdout
    return last_json(out)


say("One-call training step: train.fused_step, 128x128, latent 16, batch 256, bf16, 200 steps after 20 (bench.py's loop), a process per figure,")
say(f"{args.rounds} rounds, the rows in turn within a round (ms/step wall clock, host enqueue ms/step in brackets); EMA, decay 0.999:")
got = {name: [] for name, *_ in rows}
for _ in range(args.rounds):
    for name, tree, mode in rows:
        got[name].append(timing(tree, mode))
for name, *_ in rows:
    v = [r["ms_per_step"] for r in got[name]]
    say(f"  {name:<44s}" + "   ".join(f"{r['ms_per_step']:.4f} ({r['host_enqueue_ms_per_step']:.4f})" for r in got[name]) +
        f"   median {med(v):.4f}, spread {max(v) - min(v):.4f}")
base_name = rows[0][0]
base = med([r["ms_per_step"] for r in got[base_name]])
for name, *_ in rows[1:]:
    say(f"  {name}: {med([r['ms_per_step'] for r in got[name]]) - base:+.4f} ms/step against '{base_name}' (medians)")
say()

import torch  # noqa: E402

from torch_vae_amd import _lib  # noqa: E402
from torch_vae_amd.averaging import WeightAverage  # noqa: E402


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


# ---- 4. the update and the exchange on their own
model = bench_model()
avg = WeightAverage(model, kind="ema", decay=0.999)
N, NBN = model._flat.numel(), model._bnflat.numel()
predicted = 12 * (N + NBN)
say(f"vae_average_update on the flagship model's buffers (N = {N} parameters, N_bn = {NBN} BatchNorm floats), two launches per call")
say(f"(the streaming kernel and the single-thread commit).  Bytes the code predicts per update: 12 * (N + N_bn) = {predicted} ({predicted / 1e6:.2f} MB):")
ms = timed(avg.update, 200)
say(f"  {'WeightAverage.update(), eager (host-bound?)':<44s} {ms * 1e3:8.1f} us per call   {predicted / ms / 1e6:8.1f} GB/s of the predicted bytes")
try:      # 50 updates captured once and replayed: no host between the launches, and the state still advances on every replay
    CAPTURED = 50
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        avg.update()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    n0 = int(avg.n_averaged)
    with torch.cuda.graph(graph):
        for _ in range(CAPTURED):
            avg.update()
    n1 = int(avg.n_averaged)
    ms = timed(graph.replay, 4) / CAPTURED
    n2 = int(avg.n_averaged)
    say(f"  {'the same, 50 calls captured and replayed':<44s} {ms * 1e3:8.1f} us per call   {predicted / ms / 1e6:8.1f} GB/s of the predicted bytes")
    say(f"    (n_averaged {n0} before the capture, {n1} after it, {n2} after {3 + 4 * args.blocks} replays: every replayed update applied)")
except Exception as e:  # noqa: BLE001
    say(f"  graph replay not available in this run ({type(e).__name__}: {e})")
step = torch.zeros((), dtype=torch.int64, device="cuda")
avg.reset()
L_ = _lib.lib()
st = torch.cuda.current_stream().cuda_stream


def gated():
    _lib.check(L_.vae_average_update(avg._params.data_ptr(), model._flat.data_ptr(), N, 1.0, avg._buffers.data_ptr(), model._bnflat.data_ptr(), NBN, 1.0,
                                     _lib.AVG_EMA, 0.999, 0.0, step.data_ptr(), avg._state.data_ptr(), st), "vae_average_update")


gated()      # (seen_step becomes 0: every call below finds the step it has seen and applies nothing)
ms = timed(gated, 200)
say(f"  {'update, gate closed (a skipped step)':<44s} {ms * 1e3:8.1f} us per call   (nothing read but the state, nothing written)")
ms = timed(avg._swap, 200)
say(f"  {'vae_average_swap (one launch)':<44s} {ms * 1e3:8.1f} us per call   {16 * (N + NBN) / ms / 1e6:8.1f} GB/s (16 bytes per float: both read, both written)")
say("  Between back-to-back calls both buffers stay in the last-level cache: these are cache figures, not HBM figures.")

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
