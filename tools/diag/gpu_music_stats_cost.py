"""Diagnostic (GPU box): cost record of the per-roll musical statistics (torch_vae_amd/evaluation.py: music_statistics;
vae_music_roll_stats, include/vae_music.h).  Five parts in one visit, written as text to profiles/music_stats_cost.txt (or --out):
  1. device code - registers, scratch and LDS of the kernels from a device-only compile of csrc/vae_music.hip with
     -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU); scratch must be 0;
  2. default path unchanged - bench.py --gpus 1 --steps 200 --warmup 20 in a built checkout of the parent commit (--parent DIR) and
     in this tree, one process per run, alternating, 5 runs each; skipped when no parent tree is given;
  3. the streaming bandwidth tools/bw_probe.hip reaches in the same visit (--bw-probe BINARY, built with
     hipcc --offload-arch=gfx950 -O3 tools/bw_probe.hip -o tools/bw_probe); skipped when no binary is given;
  4. time per call at N = 65536 rolls of 128 x 128 (runs of four cells, density about 5 %), with and without totals: device events
     around back-to-back calls, the median of 7 alternating blocks after warm-up, and the bytes per second that is;
  5. a torch formulation on the same card, in chunks of 4096 rolls: unpack the planes to bytes, sums over rows / columns / pitch
     classes, shifted differences for the onsets, the polyphony histogram by scatter_add - it leaves out the note lengths and the
     gaps between onset steps, which have no short torch form; its columns are checked against the kernel's once."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "music_stats_cost.txt"))
ap.add_argument("--parent", default=None, help="built checkout of the parent commit (its bench.py is run from there)")
ap.add_argument("--bw-probe", default=None, help="binary built from tools/bw_probe.hip")
ap.add_argument("--bench-runs", type=int, default=5)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--rolls", type=int, default=65536)
args = ap.parse_args()

N, H, W, F, CHUNK = args.rolls, 128, 128, 76, 4096
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
say(f"Device code (no GPU; hipcc {' '.join(flags)} --cuda-device-only -Rpass-analysis=kernel-resource-usage, csrc/vae_music.hip):")
try:
    err = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "vae_music.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, timeout=600, check=True).stderr
    fields = {"VGPRs": r" VGPRs: (\d+)", "SGPRs": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
              "static LDS": r"LDS Size \[bytes/block\]: (\d+)", "waves/SIMD": r"Occupancy \[waves/SIMD\]: (\d+)"}
    say("  kernel                        " + "  ".join(f"{k:<10s}" for k in fields))
    for blk in re.split(r"remark: Function Name: ", err)[1:]:
        m = re.search(r"(music_\w+_kernel)", blk.split()[0])
        if not m:
            continue
        vals = [re.search(p, blk).group(1) for p in fields.values()]
        assert vals[2] == "0", f"{m.group(1)} uses scratch"
        say(f"  {m.group(1):<30s}" + "  ".join(f"{v:<10s}" for v in vals))
    per_wave = (H * (W // 32) + 3) // 4 * 4 + (W // 32 + 3) // 4 * 4 + F
    say(f"  dynamic LDS of music_roll_stats_kernel (one wave per workgroup): roundup4(h x w/32) + roundup4(w/32) + 76 dwords = {per_wave} x 4 = "
        f"{4 * per_wave} bytes at {H} x {W}.")
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

# ---- 3. what a plain stream reaches on this card in this visit
probe = {}
if args.bw_probe:
    out = subprocess.run([args.bw_probe], check=True, capture_output=True, text=True, timeout=300).stdout
    say("Streaming bandwidth in the same visit (tools/bw_probe.hip, 1 GiB buffers, 10 launches per figure):")
    for ln in out.splitlines():
        m = re.match(r"(.+?)\s+([\d.]+) GB/s", ln)
        if m and m.group(1).startswith(("read-only", "copy grid-stride")):
            probe[m.group(1).strip()] = float(m.group(2))
            say("  " + ln)
    say()
else:
    say("Streaming bandwidth: not measured in this run (no bw_probe binary given).")
    say()

import torch  # noqa: E402

from torch_vae_amd import _lib  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
lib = _lib.lib()
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(0)
BITS = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device="cuda")
PC = (torch.arange(H, device="cuda") % 12)


def random_planes(n):
    """About 5 % of the cells, as runs of four along time."""
    out = torch.empty(n, H, W // 8, dtype=torch.uint8, device="cuda")
    for a in range(0, n, CHUNK):
        m = min(CHUNK, n - a)
        cells = (torch.rand(m, H, W // 4, generator=g, device="cuda") < 0.05).repeat_interleave(4, dim=-1)
        out[a:a + m] = (cells.view(m, H, W // 8, 8).to(torch.uint8) * BITS).sum(-1, dtype=torch.uint8)
    return out


planes = random_planes(N)
features = torch.empty(N, F, dtype=torch.int32, device="cuda")
totals = torch.empty(F, dtype=torch.int64, device="cuda")


def kernel(with_totals=True):
    _lib.check(lib.vae_music_roll_stats(planes.data_ptr(), N, H, W, 0, features.data_ptr(), totals.data_ptr() if with_totals else None, 0, stream),
               "vae_music_roll_stats")


def torch_chunk(p):
    """The columns torch has a short form for, of one chunk of planes: int32 [m, 62] laid out as the kernel's first 62."""
    m = len(p)
    cells = ((p.view(m, H, W // 8, 1) & BITS) != 0).view(m, H, W)
    before = torch.zeros_like(cells)
    before[:, :, 1:] = cells[:, :, :-1]
    onsets = cells & ~before
    row_cells, row_notes = cells.sum(2, dtype=torch.int32), onsets.sum(2, dtype=torch.int32)
    column = cells.sum(1, dtype=torch.int32)
    out = torch.zeros(m, 62, dtype=torch.int32, device=p.device)
    used = row_cells > 0
    rows = torch.arange(H, device=p.device, dtype=torch.int32)
    out[:, 0] = 1
    out[:, 2], out[:, 3], out[:, 4] = row_cells.sum(1), row_notes.sum(1), used.sum(1)
    out[:, 1] = out[:, 2] > 0
    out[:, 5] = torch.where(used, rows, torch.full_like(rows, H)).amin(1)
    out[:, 5] = torch.where(out[:, 1] > 0, out[:, 5], torch.full_like(out[:, 5], -1))
    out[:, 6] = torch.where(used, rows, torch.full_like(rows, -1)).amax(1)
    out[:, 7], out[:, 8], out[:, 9] = (column > 0).sum(1), onsets.any(1).sum(1), column.amax(1)
    out[:, 10:22].index_add_(1, PC, row_cells)
    out[:, 22:34].index_add_(1, PC, row_notes)
    out[:, 46:62].scatter_add_(1, column.clamp(max=15).long(), torch.ones_like(column))
    return out


torch_out = torch.empty(N, 62, dtype=torch.int32, device="cuda")


def torch_all():
    for a in range(0, N, CHUNK):
        torch_out[a:a + CHUNK] = torch_chunk(planes[a:a + CHUNK])
    return torch_out.sum(0, dtype=torch.int64)


def block(fn, n):
    """ms per call: device events around n calls queued back to back."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


# what is timed computes the same thing, checked once
kernel()
torch_all()
torch.cuda.synchronize()
same = [c for c in list(range(34)) + list(range(46, 62)) if not torch.equal(torch_out[:, c], features[:, c])]
assert not same, f"the torch formulation's columns {same} differ from the kernel's"
density = float(features[:, 2].sum()) / (N * H * W)
notes_per_roll = float(features[:, 3].sum()) / N

VARIANTS = {"kernel: features + totals": (kernel, 10), "kernel: features only": (lambda: kernel(False), 10), "torch: unpack, sums, onsets": (torch_all, 1)}
for fn, n in VARIANTS.values():
    block(fn, 1)
times = {k: [] for k in VARIANTS}
order = list(VARIANTS)
for i in range(args.blocks):
    for k in (order if i % 2 == 0 else order[::-1]):
        times[k].append(block(*VARIANTS[k]))

plane_bytes, feature_bytes = N * H * W // 8, N * F * 4
say(f"Time per call: N = {N} rolls of {H} x {W} ({plane_bytes / 1e6:.0f} MB of bit planes on the device), runs of four cells, density {100 * density:.2f} %,")
say(f"{notes_per_roll:.1f} notes per roll; the call writes {feature_bytes / 1e6:.1f} MB of features, and with totals reads them once more.  Device events around")
say(f"back-to-back calls (10 per block; torch 1); {args.blocks} alternating blocks after a warm-up call of each.  The torch formulation, in chunks of")
say(f"{CHUNK} rolls: cells = (planes & bit) != 0; onsets = cells & ~shifted cells; sums over rows, columns and pitch classes; the polyphony")
say("histogram by scatter_add.  It computes 50 of the 74 columns (not the note lengths, not the gaps between onset steps); those 50 equal")
say("the kernel's exactly.  ms per call:")
say(f"  {'variant':<30s}" + "".join(f"block {i + 1:<4d}" for i in range(args.blocks)) + "median    spread")
for k in VARIANTS:
    say(f"  {k:<30s}" + "".join(f"{v:<10.3f}" for v in times[k]) + f"{med(times[k]):<10.3f}{max(times[k]) - min(times[k]):<10.3f}")
say()
m = {k: med(v) for k, v in times.items()}
kt, kf, tt = m["kernel: features + totals"], m["kernel: features only"], m["torch: unpack, sums, onsets"]
say(f"  features only: {kf:.3f} ms = {N / kf / 1e6:.2f} G rolls/s = {(plane_bytes + feature_bytes) / kf / 1e9:.3f} TB/s of planes read and features written")
say(f"  with totals:   {kt:.3f} ms = {(plane_bytes + 2 * feature_bytes) / kt / 1e9:.3f} TB/s (the totals pass reads the features again: {kt - kf:+.3f} ms)")
if probe:
    best = max(v for k, v in probe.items() if k.startswith("read-only"))
    say(f"  the probe's best read-only stream: {best / 1e3:.2f} TB/s; the features-only call reaches {100 * (plane_bytes + feature_bytes) / kf / 1e6 / best:.0f} % of it")
say(f"  torch: {tt:.3f} ms; kernel with totals / torch = {kt / tt:.4f}: the kernel is {'no slower' if kt <= tt else 'SLOWER'} than the torch formulation including its unpack")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
