"""Diagnostic (GPU box): cost record of the set-level fidelity metrics (torch_vae_amd/fidelity.py; include/vae_fidelity.h).  Three
parts in one visit, written as text to profiles/set_fidelity_cost.txt (or --out):
  1. device code - registers, scratch and LDS of the kernels from a device-only compile of csrc/vae_fidelity.hip with
     -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU);
  2. time per call of the three entry points at n = m = 16384 points with D = 16 and D = 128 (k = 5; 5 bandwidths; splits chosen by
     the library), and beside each the plain torch formulation a user would otherwise write on the same card - torch.cdist, squared,
     then topk / a comparison and a row minimum / exp().sum() per bandwidth - which materialises the 1 GiB distance matrix: device
     events around back-to-back calls, the median of 7 alternating blocks after a warm-up call of each; the two are compared once
     (cdist takes the expanded form, so only to 1e-3);
  3. the Frechet distance of the two test pairs (tests/fidelity_ref.frechet_cases) on the device against the float64 reference: the
     measured error behind the gate of tests/test_fidelity_gpu.py::test_frechet_distance.
A record, not a gate: no test reads a time from it."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_fidelity_cost.txt"))
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--points", type=int, default=16384)
args = ap.parse_args()

N, K, SCALES = args.points, 5, (0.25, 0.5, 1.0, 2.0, 4.0)
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
say(f"Device code (no GPU; hipcc {' '.join(flags)} --cuda-device-only -Rpass-analysis=kernel-resource-usage, csrc/vae_fidelity.hip):")
try:
    err = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "vae_fidelity.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True, timeout=600, check=True).stderr
    fields = {"VGPRs": r" VGPRs: (\d+)", "AGPRs": r" AGPRs: (\d+)", "spilled": r"VGPRs Spill: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
              "static LDS": r"LDS Size \[bytes/block\]: (\d+)", "waves/SIMD": r"Occupancy \[waves/SIMD\]: (\d+)"}
    say("  kernel (DP: the padded dimension)  " + "  ".join(f"{k:<10s}" for k in fields))
    for blk in re.split(r"remark: Function Name: ", err)[1:]:
        m = re.search(r"(sd_\w+_kernel)(?:ILi(\d+)E)?", blk.split()[0])
        if not m:
            continue
        name = m.group(1) + (f" DP={m.group(2)}" if m.group(2) else "")
        say(f"  {name:<35s}" + "  ".join(f"{re.search(p, blk).group(1):<10s}" for p in fields.values()))
except (OSError, subprocess.SubprocessError) as e:
    say(f"  not available in this run ({type(e).__name__})")
say()

import torch  # noqa: E402

from torch_vae_amd import fidelity as F  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"


def block(fn, n):
    """ms per call: device events around n calls queued back to back."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


# ---- 2. time per call
say(f"Time per call at n = m = {N} points (A ~ N(0, I), B ~ 0.9 N(0, I) + 0.3; k = {K}; {len(SCALES)} bandwidths 1 / (s * mean d2); splits chosen by the")
say(f"library).  Device events around back-to-back calls (10 per block; torch 3); {args.blocks} alternating blocks after a warm-up call of each.  The torch")
say("formulation materialises d = torch.cdist(a, b) ** 2 (1 GiB at this size) in every call: knn - d.topk(k + 1, largest=False); balls -")
say("(d <= radii).sum(1) and d.min(1); sums - exp(-gamma * d).sum() per bandwidth and d.sum().  ms per call:")
g = torch.Generator(device="cuda")
g.manual_seed(0)
for D in (16, 128):
    a = torch.randn(N, D, generator=g, device="cuda")
    b = 0.9 * torch.randn(N, D, generator=g, device="cuda") + 0.3
    radii = F.knn_radii(b, K)
    gammas = (1.0 / (torch.tensor(SCALES, device="cuda", dtype=torch.float64) * (F.kernel_sums(a, b, None)[0] / (N * N)))).contiguous()
    gam32 = gammas.float()
    keep = {}

    def t_knn():
        keep["t_knn"] = (torch.cdist(a, a) ** 2).topk(K + 1, largest=False).values[:, K]

    def t_balls():
        d = torch.cdist(a, b) ** 2
        keep["t_counts"] = (d <= radii[None, :]).sum(1)
        keep["t_near"] = d.min(1)

    def t_sums():
        d = torch.cdist(a, b) ** 2
        keep["t_sums"] = torch.stack([torch.exp(-gam * d).sum(dtype=torch.float64) for gam in gam32] + [d.sum(dtype=torch.float64)])

    def k_knn():
        keep["k_knn"] = F.knn_radii(a, K)

    def k_balls():
        keep["k_counts"], keep["k_near"], keep["k_near_d2"] = F.ball_membership(a, b, radii)

    def k_sums():
        keep["k_sums"] = F.kernel_sums(a, b, gammas)

    variants = {"kernel: knn_radii": (k_knn, 10), "torch:  cdist + topk": (t_knn, 3), "kernel: balls": (k_balls, 10), "torch:  cdist, <=, min": (t_balls, 3),
                "kernel: kernel_sums": (k_sums, 10), "torch:  cdist, exp().sum()": (t_sums, 3)}
    for fn, _ in variants.values():
        block(fn, 1)
    torch.cuda.synchronize()
    # what is timed computes the same thing (cdist takes the expanded |a|^2 + |b|^2 - 2ab: agreement to 1e-3 only)
    assert torch.allclose(keep["k_knn"], keep["t_knn"], rtol=1e-3, atol=1e-4)
    assert (keep["k_counts"] - keep["t_counts"]).abs().float().mean() < 0.01 and torch.allclose(keep["k_near_d2"], keep["t_near"].values, rtol=1e-3, atol=1e-4)
    assert torch.allclose(keep["k_sums"], keep["t_sums"], rtol=1e-3)
    times = {k: [] for k in variants}
    order = list(variants)
    for i in range(args.blocks):
        for k in (order if i % 2 == 0 else order[::-1]):
            times[k].append(block(*variants[k]))
    say(f"  D = {D}")
    say(f"  {'variant':<30s}" + "".join(f"block {i + 1:<4d}" for i in range(args.blocks)) + "median    spread")
    for k in variants:
        say(f"  {k:<30s}" + "".join(f"{v:<10.3f}" for v in times[k]) + f"{med(times[k]):<10.3f}{max(times[k]) - min(times[k]):<10.3f}")
    m = {k: med(v) for k, v in times.items()}
    names = list(variants)
    for kern, tor in zip(names[0::2], names[1::2]):
        say(f"    {kern[8:]}: {N * N * D * 3 / m[kern] / 1e9:.2f} TFLOP/s of distance arithmetic (3 per term); kernel / torch = {m[kern] / m[tor]:.3f}")
    say()
    del a, b, keep

# ---- 3. the Frechet distance against float64
from tests import fidelity_ref as R  # noqa: E402

say("Frechet distance, device moments (vae_mixture_mstep, one component) against the float64 reference, on the two pairs [512, 16] of")
say("tests/fidelity_ref.frechet_cases():")
worst = 0.0
for i, (x, y) in enumerate(R.frechet_cases()):
    got, want = F.frechet_distance(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()), R.frechet_distance(x, y)
    worst = max(worst, abs(got - want) / want)
    say(f"  pair {i}: device {got!r}  reference {want!r}  relative error {abs(got - want) / want:.3e}")
say(f"  worst relative error {worst:.3e}; tests/test_fidelity_gpu.py::test_frechet_distance allows 8 times its FRECHET_MEASURED, at most 1e-4")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
