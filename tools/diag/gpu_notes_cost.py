"""Diagnostic (GPU box): cost record of the note-event extraction (torch_vae_amd/generation.py, vae_extract_notes).  Three parts in one
visit, written as text to profiles/note_events_cost.txt (or --out):
  1. device code - registers, scratch and LDS of the three kernels from a device-only compile of csrc/vae_util.hip with
     -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU);
  2. default path unchanged - bench.py --gpus 1 --steps 200 --warmup 20 in a built checkout of the parent commit (--parent DIR) and
     in this tree, one process per run, alternating, 5 runs each; skipped when no parent tree is given;
  3. time per call at 256 x 128 x 128 with device events in alternating blocks after warm-up: vae_extract_notes (events, peaks and
     cleaned planes; the count-only call; the planes alone, which is binarize_rolls) on a sparse roll (vae_synth_pianoroll blurred
     along time into [0, 1], with noise) and on the alternating worst case, against vae_recon_metrics on the same tensor (the
     in-project yardstick for one streaming read of it) and against the torch formulation of binarize_rolls (x >= t, then a
     packbits by shifts and a sum)."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "note_events_cost.txt"))
ap.add_argument("--parent", default=None, help="built checkout of the parent commit (its bench.py is run from there)")
ap.add_argument("--bench-runs", type=int, default=5)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--calls", type=int, default=200, help="calls per block")
args = ap.parse_args()

N, H, W = 256, 128, 128
ON, OFF, D, G = 0.5, 0.3, 2, 1
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


# ---- 1. device code
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
csrc = os.path.join(ROOT, "torch_vae_amd", "csrc")
flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result"]
say(f"Device code (no GPU; hipcc {' '.join(flags)} --cuda-device-only -Rpass-analysis=kernel-resource-usage, csrc/vae_util.hip):")
try:
    err = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "vae_util.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, timeout=600, check=True).stderr
    fields = {"VGPRs": r" VGPRs: (\d+)", "SGPRs": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
              "static LDS": r"LDS Size \[bytes/block\]: (\d+)", "waves/SIMD": r"Occupancy \[waves/SIMD\]: (\d+)"}
    say("  kernel                              " + "  ".join(f"{k:<10s}" for k in fields))
    for blk in re.split(r"remark: Function Name: ", err)[1:]:
        name = blk.split()[0]
        names = {"note_count_kernelILb0E": "note_count_kernel<counts>", "note_count_kernelILb1E": "note_count_kernel<counts, planes>",
                 "note_scan_kernel": "note_scan_kernel", "note_emit_kernel": "note_emit_kernel",
                 "recon_metrics_kernelILi1E": "recon_metrics_kernel<1> (yardstick)"}
        short = next((v for k, v in names.items() if k in name), None)
        if short is None:
            continue
        vals = [re.search(p, blk).group(1) for p in fields.values()]
        say(f"  {short:<36s}" + "  ".join(f"{v:<10s}" for v in vals))
        if short.startswith("note_"):
            assert vals[2] == "0", f"{short} uses scratch"
    say(f"  note_count_kernel and note_emit_kernel add dynamic LDS: 4 rows x ceil(w/64) mask words x 8 bytes = {4 * ((W + 63) // 64) * 8} bytes at w = {W}.")
except (OSError, subprocess.SubprocessError) as e:
    say(f"  not available in this run ({type(e).__name__})")
say()

# ---- 2. default path: the benchmark in the parent's tree and in this one, before this process opens the GPU
if args.parent:
    res = {"parent": [], "new": []}
    for i in range(args.bench_runs):
        for tag in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
            cwd = args.parent if tag == "parent" else ROOT
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=cwd, check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            res[tag].append(rec)
            print(f"bench {tag} run {i + 1}: {rec['ms_per_step']} ms/step", file=sys.stderr, flush=True)
    say("Default path: python bench.py --gpus 1 --steps 200 --warmup 20, parent and this commit each in its own built tree, one process per run,")
    say(f"processes alternating; {args.bench_runs} runs each.")
    say("  run   parent ms_per_step  host_enqueue_ms   samples/s  |  new ms_per_step  host_enqueue_ms   samples/s")
    for i in range(args.bench_runs):
        a, b = res["parent"][i], res["new"][i]
        say(f"  {i + 1}     {a['ms_per_step']:<18.4f} {a['host_enqueue_ms_per_step']:<16.4f} {a['value']:<10.1f} |  {b['ms_per_step']:<16.4f} "
            f"{b['host_enqueue_ms_per_step']:<16.4f} {b['value']:.1f}")
    pm, nm = med([r["ms_per_step"] for r in res["parent"]]), med([r["ms_per_step"] for r in res["new"]])
    lo, hi = min(r["ms_per_step"] for r in res["parent"]), max(r["ms_per_step"] for r in res["parent"])
    say(f"  median  {pm:<18.4f}                             |  {nm:.4f}")
    say(f"  parent's own band (min .. max): ms_per_step {lo:.4f} .. {hi:.4f} (max - min {hi - lo:.4f}, {100 * (hi - lo) / pm:.2f} % of its median)")
    say(f"  new median {nm:.4f}: {'inside' if lo <= nm <= hi else 'OUTSIDE'} the parent's band; new median - parent median {nm - pm:+.4f}")
    say()
else:
    say("Default path: not measured in this run (no parent tree given).")
    say()

import ctypes  # noqa: E402

import torch  # noqa: E402

from torch_vae_amd import _lib, generation  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
lib = _lib.lib()
stream = torch.cuda.current_stream().cuda_stream
torch.manual_seed(0)

# ---- 3. time per call
sparse = torch.empty(N, H, W, device="cuda")
_lib.check(lib.vae_synth_pianoroll(sparse.data_ptr(), N, H, 7, stream), "synth")
sparse = 0.25 * torch.roll(sparse, 1, -1) + 0.5 * sparse + 0.25 * torch.roll(sparse, -1, -1)     # lines blurred along time
sparse = (sparse * (0.6 + 0.4 * torch.rand_like(sparse)) + 0.25 * torch.rand_like(sparse)).clamp_(0.0, 1.0).contiguous()
worst = torch.zeros(N, H, W, device="cuda")
worst[..., 0::2] = 1.0
CASES = {"sparse": (sparse, (ON, OFF, D, G)), "alternating": (worst, (0.5, 0.5, 1, 0))}
cap = N * H * (W // 2)
events = torch.empty(cap, 4, dtype=torch.int32, device="cuda")
peaks = torch.empty(cap, dtype=torch.float32, device="cuda")
offsets = torch.empty(N + 1, dtype=torch.int64, device="cuda")
planes = torch.empty(N, H, W // 8, dtype=torch.uint8, device="cuda")
th = (ctypes.c_float * 1)(0.5)
roll_sums = torch.empty(N, 3, dtype=torch.float64, device="cuda")
roll_counts = torch.empty(N, 3, dtype=torch.int64, device="cuda")
totals = torch.empty(8, dtype=torch.float64, device="cuda")
total_counts = torch.empty(3, dtype=torch.int64, device="cuda")
shifts = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device="cuda")
stall_a = torch.randn(8192, 8192, device="cuda")


def extract(x, prm, ev, cl):
    _lib.check(lib.vae_extract_notes(x.data_ptr(), N, H, W, *prm, events.data_ptr() if ev else None, peaks.data_ptr() if ev else None, cap if ev else 0,
                                     offsets.data_ptr(), planes.data_ptr() if cl else None, stream), "vae_extract_notes")


def recon(x):
    _lib.check(lib.vae_recon_metrics(x.data_ptr(), x.data_ptr(), N, H * W, th, 1, 0.5, roll_sums.data_ptr(), roll_counts.data_ptr(),
                                     totals.data_ptr(), total_counts.data_ptr(), 0, stream), "vae_recon_metrics")


def torch_binarize(x, t):
    return ((x >= t).view(N, H, W // 8, 8).to(torch.uint8) * shifts).sum(-1, dtype=torch.uint8)


KERNELS = {}
for tag, (x, prm) in CASES.items():
    KERNELS[f"{tag}: events+peaks+planes"] = lambda i, x=x, prm=prm: extract(x, prm, True, True)
    KERNELS[f"{tag}: events+peaks"] = lambda i, x=x, prm=prm: extract(x, prm, True, False)
    KERNELS[f"{tag}: count only"] = lambda i, x=x, prm=prm: extract(x, prm, False, False)
    KERNELS[f"{tag}: planes (binarize)"] = lambda i, x=x, prm=prm: extract(x, (prm[0], prm[0], 1, 0), False, True)
    KERNELS[f"{tag}: recon_metrics"] = lambda i, x=x: recon(x)
    KERNELS[f"{tag}: torch binarize"] = lambda i, x=x, prm=prm: torch_binarize(x, prm[0])

late = {}


def block(fn, n, key=None):
    """us per call.  The calls take less device time than the host needs to enqueue them, so the stream is first kept busy with
    matrix products while the host queues the whole block: the device then runs the calls back to back."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        torch.mm(stall_a, stall_a)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    late[key] = late.get(key, 0) + int(e0.query())      # the window began before the last call was queued: the host may be in the figure
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


# what the calls compute, checked once: binarize against torch, totals for the record
info = {}
for tag, (x, prm) in CASES.items():
    extract(x, prm, True, True)
    torch.cuda.synchronize()
    info[tag] = int(offsets[N])
    assert info[tag] <= cap
    assert torch.equal(generation.binarize_rolls(x, prm[0]), torch_binarize(x, prm[0])), "binarize_rolls differs from the torch formulation"
assert info["alternating"] == cap
for fn in KERNELS.values():
    block(fn, 50)
kt = {k: [] for k in KERNELS}
order = list(KERNELS)
for i in range(args.blocks):
    for k in (order if i % 2 == 0 else order[::-1]):
        kt[k].append(block(KERNELS[k], args.calls, k))
mb = N * H * W * 4 / 1e6
say(f"Time per call, rolls {N} x {H} x {W} float32 ({mb:.1f} MB) resident on the device (they fit the memory-side cache: every variant reads")
say(f"them from there); device events around {args.calls} calls per block, queued while the stream is held busy so that the device runs them")
say(f"back to back (`late`: blocks of the {args.blocks} whose window began before their last call was queued - harmless where the device is the")
say(f"slower side, host time in the figure where it is not); {args.blocks} alternating blocks after 50 warm-up calls.")
say(f"sparse: vae_synth_pianoroll blurred along time, scaled and with noise, (on, off, D, G) = ({ON}, {OFF}, {D}, {G}): {info['sparse']} events;")
say(f"alternating: every second cell 1.0, (0.5, 0.5, 1, 0): {info['alternating']} events = the capacity bound n*h*w/2.  recon_metrics reads the tensor as")
say("xhat and as target (the second read hits the cache).  us per call:")
say(f"  {'variant':<34s}" + "".join(f"block {i + 1:<4d}" for i in range(args.blocks)) + "median    spread    late")
for k in KERNELS:
    say(f"  {k:<34s}" + "".join(f"{v:<10.2f}" for v in kt[k]) + f"{med(kt[k]):<10.2f}{max(kt[k]) - min(kt[k]):<10.2f}{late.get(k, 0)}")
say()
for tag in CASES:
    m = {k.split(": ")[1]: med(v) for k, v in kt.items() if k.startswith(tag)}
    say(f"  {tag}: full call {m['events+peaks+planes']:.2f} us = {mb / m['events+peaks+planes']:.2f} TB/s of roll read once "
        f"(the call reads it twice); count only {m['count only']:.2f} us; recon_metrics {m['recon_metrics']:.2f} us "
        f"(x{m['events+peaks+planes'] / m['recon_metrics']:.2f}); planes alone {m['planes (binarize)']:.2f} us against torch's "
        f"{m['torch binarize']:.2f} us (torch / planes = {m['torch binarize'] / m['planes (binarize)']:.2f})")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
