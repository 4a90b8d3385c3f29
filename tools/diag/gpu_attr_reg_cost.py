"""Diagnostic (GPU box): cost record of the attribute-regularised latents (include/vae_attributes.h; torch_vae_amd/attributes.py).
Parts, written as text to profiles/attribute_reg_cost.txt (or --out); nothing here is a gate:
  1. device code - registers, scratch and LDS of the kernels from a device-only compile of csrc/vae_attributes.hip with
     -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU);
  2. default path unchanged - bench.py --gpus 1 --steps 200 --warmup 20 in a built checkout of the parent commit (--parent DIR) and
     in this tree, one process per run, alternating; skipped when no parent tree is given;
  3. the training step with the regulariser - ms/step of train.fused_step at the bench workload (128x128, latent 16, batch 256, bf16)
     with one and with four regularised pairs in this tree, against the PARENT's split path (VAE_ONE_CALL_STEP=0) and one-call path;
     each figure from a process of its own (this file with --step-timing);
  4. the streaming bandwidth tools/bw_probe.hip reaches in the same visit (--bw-probe BINARY); skipped when no binary is given;
  5. vae_attr_roll_counters at 256 and 65536 rolls of 128x128, and the bytes per second that is;
  6. vae_attr_regularizer at B = 256 and 4096 (L = 16; 1 and 8 pairs);
  7. vae_attr_concordance at N = 16384, L = 16, 7 attributes against a torch restatement on the same card (checked equal once);
  8. evidence, not a test: Kendall tau of (z_0, cells) after --train-steps steps of a 32x32 model with and without
     attr_reg={"note_density": 0}.
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
ap.add_argument("--bw-probe", default=None, help="binary built from tools/bw_probe.hip")
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--train-steps", type=int, default=300)
ap.add_argument("--step-timing", type=int, default=None, metavar="PAIRS", help="internal: print the ms/step of fused_step with PAIRS regularised pairs")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
PAIRS4 = {"note_density": 0, "pitch_range": 1, "mean_pitch": 2, "onset_steps": 3}


def med(v):
    return sorted(v)[len(v) // 2]


def step_timing(pairs, steps=200, warmup=20):
    """bench.py's loop (same model, optimiser, batches) through train.fused_step; attr_reg only where pairs > 0"""
    from argparse import Namespace
    import torch
    from torch_vae_amd.models import VanillaVAE
    from torch_vae_amd.train import SyntheticPianorollLoader, build_optimizer, fused_step
    H, L, B, dev = 128, 16, 256, torch.device("cuda:0")
    torch.manual_seed(0)
    model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).to(dev)
    if pairs:
        model.attr_reg = dict(list(PAIRS4.items())[:pairs])
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle", epochs=1,
                    freeze_encoder=False)
    opt, sched = build_optimizer(cfg, model, steps_per_epoch=steps + warmup + 8)
    pool = SyntheticPianorollLoader(B, H, n_batches=4, seed=0, device=dev, pool=4)
    batches = [pool.batch(i)[0] for i in range(4)]
    model.eps_seed = 7919
    for i in range(warmup):
        fused_step(model, opt, batches[i % 4]); sched.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out3, _ = fused_step(model, opt, batches[i % 4]); sched.step()
    host = 1e3 * (time.perf_counter() - t0) / steps
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    print(json.dumps({"pairs": pairs, "ms_per_step": round(ms, 4), "host_enqueue_ms_per_step": round(host, 4), "loss": out3.tolist()}))


if args.step_timing is not None:
    step_timing(args.step_timing)
    sys.exit(0)

OUT = args.out or os.path.join(ROOT, "profiles", "attribute_reg_cost.txt")
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
say(f"Device code (no GPU; hipcc {' '.join(flags)} --cuda-device-only -Rpass-analysis=kernel-resource-usage, csrc/vae_attributes.hip):")
try:
    err = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "vae_attributes.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, timeout=600, check=True).stderr
    fields = {"VGPRs": r" VGPRs: (\d+)", "SGPRs": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
              "static LDS": r"LDS Size \[bytes/block\]: (\d+)", "waves/SIMD": r"Occupancy \[waves/SIMD\]: (\d+)"}
    say("  kernel                        " + "  ".join(f"{k:<10s}" for k in fields))
    for blk in re.split(r"remark: Function Name: ", err)[1:]:
        m = re.search(r"(attr_\w+_kernel)", blk.split()[0])
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

    def timing(tree, pairs, env=None):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--step-timing", str(pairs)], check=True, capture_output=True,
                             text=True, timeout=300, env={**os.environ, **(env or {})}).stdout
        return last_json(out)
    say("Training step with the regulariser: train.fused_step, 128x128, latent 16, batch 256, bf16, 200 steps after 20 (bench.py's loop), a process")
    say("per figure, two rounds (ms/step wall clock, host enqueue ms/step):")
    rows = [("parent, one call per step", args.parent, 0, None), ("parent, split path (VAE_ONE_CALL_STEP=0)", args.parent, 0, {"VAE_ONE_CALL_STEP": "0"}),
            ("this tree, attr_reg off", ROOT, 0, None), ("this tree, 1 pair (split path)", ROOT, 1, None), ("this tree, 4 pairs (split path)", ROOT, 4, None)]
    got = {name: [] for name, *_ in rows}
    for _ in range(2):
        for name, tree, pairs, env in rows:
            got[name].append(timing(tree, pairs, env))
    for name, *_ in rows:
        say(f"  {name:<44s}" + "   ".join(f"{r['ms_per_step']:.4f} ({r['host_enqueue_ms_per_step']:.4f})" for r in got[name]))
    base = min(r["ms_per_step"] for r in got["parent, split path (VAE_ONE_CALL_STEP=0)"])
    for name in ("this tree, 1 pair (split path)", "this tree, 4 pairs (split path)"):
        say(f"  {name}: {min(r['ms_per_step'] for r in got[name]) - base:+.4f} ms/step over the parent's split path (best of two each)")
    say()
else:
    say("Default path and step cost: not measured in this run (no parent tree given).")
    say()

# ---- 4. what a plain stream reaches on this card in this visit
read_bw = None
if args.bw_probe:
    out = subprocess.run([args.bw_probe], check=True, capture_output=True, text=True, timeout=300).stdout
    say("Streaming bandwidth in the same visit (tools/bw_probe.hip):")
    for ln in out.splitlines():
        m = re.match(r"(.+?)\s+([\d.]+) GB/s", ln)
        if m and m.group(1).startswith(("read-only", "copy grid-stride")):
            say("  " + ln)
            if m.group(1).startswith("read-only"):
                read_bw = max(read_bw or 0.0, float(m.group(2)))
    say()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_vae_amd import _lib  # noqa: E402
from torch_vae_amd.attributes import ATTRIBUTE_NAMES, attribute_correlation, attribute_regularizer, attribute_values, roll_attributes  # noqa: E402

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


# ---- 5. counters
say("vae_attr_roll_counters, rolls of 128x128 f32 (uniform values, 5 % of the cells at or above the threshold):")
g = torch.Generator(device=dev).manual_seed(1)
for n, reps in ((256, 200), (65536, 5)):
    x = (torch.rand(n, 128, 128, device=dev, generator=g) * 0.5263).contiguous()
    ms = timed(lambda: roll_attributes(x, 0.5), reps)
    gbs = x.numel() * 4 / ms / 1e6
    say(f"  n = {n:<6d} {ms * 1e3:10.1f} us per call   {gbs:8.1f} GB/s of rolls read" +
        (f"   {100 * gbs / read_bw:5.1f} % of the probe's read-only figure" if read_bw else ""))
    del x
say()

# ---- 6. regulariser
say("vae_attr_regularizer, L = 16, delta 10 (z ~ N(0,1), counters of random rolls), with the gradient:")
for B in (256, 4096):
    z = torch.randn(B, 16, device=dev, generator=g)
    c = roll_attributes((torch.rand(B, 32, 32, device=dev, generator=g) * torch.rand(B, 1, 1, device=dev, generator=g)).contiguous(), 0.5)
    for pairs in (1, 8):
        ids, dims = [k % 7 for k in range(pairs)], list(range(pairs))
        ms = timed(lambda: attribute_regularizer(z, c, ids, dims, 10.0, 1.0), 50)
        say(f"  B = {B:<5d} {pairs} pair(s)  {ms * 1e3:9.1f} us per call   ({B * B * pairs / ms / 1e6:8.1f} G pair-terms/s)")
say()

# ---- 7. concordance against torch on the device
N, L = 16384, 16
z = torch.randn(N, L, device=dev, generator=g)
z[:, 0] = torch.round(z[:, 0] * 4) / 4      # ties in one dimension
c = roll_attributes((torch.rand(N, 32, 32, device=dev, generator=g) * torch.rand(N, 1, 1, device=dev, generator=g)).contiguous(), 0.5)
names = list(ATTRIBUTE_NAMES)
ids = (__import__("ctypes").c_int32 * 7)(*range(7))
buf = torch.empty(7 * L + L + 7, dtype=torch.int64, device=dev)


def kernel():
    _lib.check(_lib.lib().vae_attr_concordance(z.data_ptr(), L, L, c.data_ptr(), N, 7, ids, buf[:7 * L].data_ptr(), buf[7 * L:8 * L].data_ptr(),
                                               buf[8 * L:].data_ptr(), torch.cuda.current_stream().cuda_stream), "vae_attr_concordance")


def torch_form(chunk=256):
    a = attribute_values(c, names)
    S = torch.zeros(7, L, dtype=torch.float64, device=dev)
    tz, ta = torch.zeros(L, dtype=torch.float64, device=dev), torch.zeros(7, dtype=torch.float64, device=dev)
    idx = torch.arange(N, device=dev)
    for i0 in range(0, N, chunk):
        upper = (idx[None, :] > idx[i0:i0 + chunk, None]).float()                     # [c, N]: j > i
        sz = torch.sign(z[i0:i0 + chunk, None, :] - z[None, :, :]) * upper[:, :, None]  # [c, N, L]
        sa = (torch.sign(a[i0:i0 + chunk, None, :] - a[None, :, :])).float() * upper[:, :, None]
        S += torch.einsum("cna,cnl->al", sa, sz).double()
        tz += (upper.sum() - (sz * sz).sum(dim=(0, 1))).double()
        ta += (upper.sum() - (sa * sa).sum(dim=(0, 1))).double()
    return S, tz, ta


kernel()
S, tz, ta = torch_form()
same = bool((buf[:7 * L].view(7, L).double() == S).all() and (buf[7 * L:8 * L].double() == tz).all() and (buf[8 * L:].double() == ta).all())
k_ms, t_ms = timed(kernel, 5), timed(torch_form, 1, blocks=3)
say(f"vae_attr_concordance, N = {N}, L = {L}, 7 attributes ({N * (N - 1) // 2} pairs):")
say(f"  kernel  {k_ms:9.3f} ms per call;  torch on the same card (sign differences and an einsum, chunks of 256 queries)  {t_ms:9.1f} ms;  results equal: {same}")
tau = attribute_correlation(z, c, names)
say(f"  attribute_correlation (the call, one read-back and tau-b on the host): largest |tau| {float(tau.abs().max()):.4f} on random latents")
say()

# ---- 8. evidence: does dimension 0 come to order the rolls by note density?
from argparse import Namespace  # noqa: E402

from torch_vae_amd.models import VanillaVAE  # noqa: E402
from torch_vae_amd.train import build_optimizer, fused_step  # noqa: E402

rolls = (torch.rand(4096, 1, 32, 32, device=dev, generator=g) < torch.rand(4096, 1, 1, 1, device=dev, generator=g) * 0.3).float()
counters = roll_attributes(rolls, 0.5)
say(f"Evidence (not a test): 32x32 model, latent 16, bf16, batch 256, {args.train_steps} steps of fused_step on 4096 random rolls of mixed density;")
say("Kendall tau-b of (posterior mean of dimension 0, cells) over the 4096 rolls afterwards:")
for reg in (None, {"note_density": 0}):
    torch.manual_seed(0)
    m = VanillaVAE(1, 16, 32, compute_dtype="bf16", max_batch=256, attr_reg=reg).to(dev)
    cfg = Namespace(batch_size_per_gpu=256, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle", epochs=1,
                    freeze_encoder=False)
    opt, sched = build_optimizer(cfg, m, steps_per_epoch=args.train_steps + 8)
    for s in range(args.train_steps):
        i0 = (s * 256) % 4096
        fused_step(m, opt, rolls[i0:i0 + 256]); sched.step()
    m.eval()
    with torch.no_grad():
        mu = torch.cat([m.encode(rolls[i:i + 256])["mu"].float() for i in range(0, 4096, 256)])
    t = attribute_correlation(mu.contiguous(), counters, ["note_density"])[0]
    say(f"  attr_reg = {str(reg):<22s} tau(z_0, cells) = {float(t[0]):+.4f}   largest |tau| over the other 15 dimensions = {float(t[1:].abs().max()):.4f}")

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
