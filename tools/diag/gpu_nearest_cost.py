"""Diagnostic (GPU box): cost record of the nearest-roll search (torch_vae_amd/evaluation.py: nearest_rolls; vae_nearest_rolls).  Four
parts in one visit, written as text to profiles/nearest_rolls_cost.txt (or --out):
  1. device code - registers, scratch and LDS of the kernels from a device-only compile of csrc/vae_util.hip with
     -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU); scratch must be 0;
  2. default path unchanged - bench.py --gpus 1 --steps 200 --warmup 20 in a built checkout of the parent commit (--parent DIR) and
     in this tree, one process per run, alternating, 5 runs each; skipped when no parent tree is given;
  3. time per call at Q = 256 queries against N = 65536 rolls of 128 x 128 (density about 5 %), k = 4, for the windows (0,0), (6,0)
     and (6,4): device events around back-to-back calls, the median of 7 alternating blocks after warm-up;
  4. a torch formulation of the (0,0) window on the same card: unpack the planes to 16-bit floats, inter = q @ c.T accumulated in
     float32, d = |q| + |c| - 2 inter, topk - the unpack of the dataset timed separately and together with the rest, and the bytes
     it needs beside the planes."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_rolls_cost.txt"))
ap.add_argument("--parent", default=None, help="built checkout of the parent commit (its bench.py is run from there)")
ap.add_argument("--bench-runs", type=int, default=5)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--rolls", type=int, default=65536)
args = ap.parse_args()

Q, N, H, W, K = args.queries, args.rolls, 128, 128, 4
WINDOWS = {(0, 0): 10, (6, 0): 3, (6, 4): 1}      # window -> calls per block
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
    say("  kernel                                          " + "  ".join(f"{k:<10s}" for k in fields))
    modes = ("T = 0, 16-byte reads", "T = 0, dwords", "any window, dwords", "|dt| < 32, 16-byte reads", "|dt| < 32, w = 128")
    rows = []
    for blk in re.split(r"remark: Function Name: ", err)[1:]:
        name = blk.split()[0]
        m = re.search(r"nearest_rolls_kernelILi(\d)ELi(\d)ELi(\d)E", name)
        if m:
            short = f"nearest_rolls_kernel<{m.group(1)} q/wave, {m.group(2)} waves; {modes[int(m.group(3))]}>"
        elif "nearest_merge_kernel" in name:
            short = "nearest_merge_kernel"
        else:
            continue
        vals = [re.search(p, blk).group(1) for p in fields.values()]
        assert vals[2] == "0", f"{short} uses scratch"
        rows.append(f"  {short:<72s}" + "  ".join(f"{v:<10s}" for v in vals))
    for r in sorted(rows):
        say(r)
    words = H * W // 32
    stride = (words + 7) // 8 * 8 + 4
    say(f"  dynamic LDS of nearest_rolls_kernel: (query tile + candidate tile) x (roundup(words, 8) + 4) dwords = "
        f"(16 + 16) x {stride} x 4 = {32 * stride * 4} bytes at {H} x {W}.")
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

import torch  # noqa: E402

from torch_vae_amd import _lib  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
lib = _lib.lib()
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda")
g.manual_seed(0)
BITS = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device="cuda")


def random_planes(n):
    """About 5 % of the cells, as runs of four along time."""
    out = torch.empty(n, H, W // 8, dtype=torch.uint8, device="cuda")
    for a in range(0, n, 4096):
        m = min(4096, n - a)
        cells = (torch.rand(m, H, W // 4, generator=g, device="cuda") < 0.05).repeat_interleave(4, dim=-1)
        out[a:a + m] = (cells.view(m, H, W // 8, 8).to(torch.uint8) * BITS).sum(-1, dtype=torch.uint8)
    return out


rolls = random_planes(N)
queries = random_planes(Q)
queries[::2] = rolls[torch.randint(0, N, (len(queries[::2]),), generator=g, device="cuda")]     # half the queries are training rolls
index = torch.empty(Q, K, dtype=torch.int64, device="cuda")
distance = torch.empty(Q, K, dtype=torch.int32, device="cuda")
shift = torch.empty(Q, K, 2, dtype=torch.int32, device="cuda")
inter = torch.empty(Q, K, dtype=torch.int32, device="cuda")
cells = torch.empty(Q, dtype=torch.int32, device="cuda")


def search(P, T):
    _lib.check(lib.vae_nearest_rolls(queries.data_ptr(), Q, rolls.data_ptr(), N, H, W, P, T, None, K, 0, index.data_ptr(), distance.data_ptr(),
                                     shift.data_ptr(), inter.data_ptr(), cells.data_ptr(), stream), "vae_nearest_rolls")


def unpack(planes):
    """[n, H*W] float16 cells and their count per roll."""
    c = ((planes.view(len(planes), -1, 1) & BITS) != 0).view(len(planes), -1).to(torch.float16)
    return c, c.sum(1, dtype=torch.float32)


def torch_search(qc, qn, cc, cn):
    try:
        it = torch.mm(qc, cc.T, out_dtype=torch.float32)
    except (TypeError, RuntimeError):
        it = torch.mm(qc, cc.T).float()          # (the product accumulates in float32 either way; counts up to 2048 are exact in float16)
    d = qn[:, None] + cn[None] - 2.0 * it
    return torch.topk(d, K, dim=1, largest=False, sorted=True)


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
qc, qn = unpack(queries)
cc, cn = unpack(rolls)
search(0, 0)
td, ti = torch_search(qc, qn, cc, cn)
torch.cuda.synchronize()
assert torch.equal(td.to(torch.int32), distance), "the torch formulation's distances differ from the kernel's"
agree = float((ti == index).double().mean())
extra = cc.numel() * cc.element_size() + cn.numel() * cn.element_size()

state = {}


def t_unpack():
    state["c"] = unpack(rolls)


def t_gemm():
    torch_search(qc, qn, cc, cn)


def t_both():
    torch_search(*unpack(queries), *unpack(rolls))


del cc, cn
VARIANTS = {f"kernel, window ({P},{T})": ((lambda P=P, T=T: search(P, T)), n) for (P, T), n in WINDOWS.items()}
cc, cn = unpack(rolls)
VARIANTS["torch: unpack the dataset"] = (t_unpack, 2)
VARIANTS["torch: product, distance, topk"] = (t_gemm, 3)
VARIANTS["torch: unpack + product + topk"] = (t_both, 2)
for fn, n in VARIANTS.values():
    block(fn, 1)
times = {k: [] for k in VARIANTS}
order = list(VARIANTS)
for i in range(args.blocks):
    for k in (order if i % 2 == 0 else order[::-1]):
        times[k].append(block(*VARIANTS[k]))

say(f"Time per call: Q = {Q} queries against N = {N} rolls of {H} x {W} ({N * H * W // 8 / 1e6:.0f} MB of bit planes on the device), runs of four cells,")
say(f"density about 5 %, half the queries taken from the rolls, k = {K}, splits chosen by the library.  Device events around back-to-back calls")
say(f"(calls per block: {', '.join(f'{k[0]},{k[1]}: {v}' for k, v in WINDOWS.items())}; torch 2 to 3); {args.blocks} alternating blocks after a warm-up call of each.")
say("The torch formulation of the (0,0) window: cells = ((planes & bit) != 0).half(); inter = q @ c.T (float32 accumulation);")
say(f"d = |q| + |c| - 2 inter; topk(k, smallest).  Its distances equal the kernel's exactly; its indices agree in {100 * agree:.1f} % of the slots (topk")
say(f"breaks equal distances its own way).  Beside the planes it needs {extra / 1e9:.2f} GB for the unpacked dataset.  ms per call:")
say(f"  {'variant':<34s}" + "".join(f"block {i + 1:<4d}" for i in range(args.blocks)) + "median    spread")
for k in VARIANTS:
    say(f"  {k:<34s}" + "".join(f"{v:<10.3f}" for v in times[k]) + f"{med(times[k]):<10.3f}{max(times[k]) - min(times[k]):<10.3f}")
say()
m = {k: med(v) for k, v in times.items()}
k00 = m["kernel, window (0,0)"]
pairs = Q * N
say(f"  window (0,0): {k00:.3f} ms = {pairs / k00 / 1e6:.2f} G pairs/s = {pairs * (H * W // 32) / k00 / 1e9:.2f} T dword XOR+popcounts/s, "
    f"{N * H * W // 8 * ((Q + 15) // 16) / k00 / 1e9:.2f} TB/s of rolls into LDS (each roll once per tile of 16 queries)")
for (P, T) in list(WINDOWS)[1:]:
    ns = (2 * P + 1) * (2 * T + 1)
    t = m[f"kernel, window ({P},{T})"]
    say(f"  window ({P},{T}): {t:.3f} ms for {ns} shifts = {t / ns:.3f} ms per shift = {t / ns / k00:.2f} x the (0,0) call")
say(f"  torch: unpack {m['torch: unpack the dataset']:.3f} ms, product + topk {m['torch: product, distance, topk']:.3f} ms, together "
    f"{m['torch: unpack + product + topk']:.3f} ms; kernel (0,0) / torch together = {k00 / m['torch: unpack + product + topk']:.2f}, "
    f"kernel (0,0) / product + topk alone = {k00 / m['torch: product, distance, topk']:.2f}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
