"""Diagnostic: what the reconstruction reductions cost in an evaluation pass, and what the metrics kernels reach.

evaluate() over a SyntheticPianorollLoader at the bench workload (128x128, latent 16, batch 256, bf16; the batches are generated once
and pooled, so the loader costs the same nothing in both passes), with the default torch reductions and with
note_thresholds=(0.5, 0.3) (one vae_recon_metrics call per batch, one read-back per pass): the two alternate in one process, after
warm-up passes of both, and each pass is timed with a host clock from its start to a device synchronise after it.

Then vae_recon_metrics alone (ReconMetricsAccumulator.update: the pass over the cells plus the fold launch) between two
device events, over distinct batches of more bytes together than the 256 MiB memory-side cache holds, as bytes read (2 N 4) over time
and as a share of the 8.0 TB/s HBM peak: once with every call queued behind two large matrix products before the device reaches the
first (device time), once issued as a pass issues them.

Usage: python tools/diag/gpu_eval_cost.py [--batches 32] [--repeats 7] [--out profiles/eval_metrics_cost.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from torch_vae_amd.evaluation import ReconMetricsAccumulator, evaluate  # noqa: E402
from torch_vae_amd.models import VanillaVAE  # noqa: E402
from torch_vae_amd.train import SyntheticPianorollLoader  # noqa: E402

H, L, B, DTYPE = 128, 16, 256, "bf16"
HBM_PEAK = 8.0e12
NOTE_THRESHOLDS = (0.5, 0.3)
SWEEP8 = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)


def timed_pass(loader, model, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = evaluate(loader, model, "cuda", verbosity=0, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def kernel_time(pairs, thresholds, rounds, ballast=None):
    """Seconds per update() between two device events.  With `ballast` (a big matrix) two products of it are enqueued first, so
    the host has every call queued before the device reaches the first: the figure is then device time (the two launches and the
    gap between them), not the rate at which Python issues calls."""
    acc = ReconMetricsAccumulator(thresholds)
    for x, t in pairs[:2]:
        acc.update(x, t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if ballast is not None:
        torch.mm(ballast, ballast)
        torch.mm(ballast, ballast)
    e0.record()
    for _ in range(rounds):
        for x, t in pairs:
            acc.update(x, t)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / (rounds * len(pairs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_eval_cost.py measures on the GPU; there is none here")
    torch.manual_seed(0)
    model = VanillaVAE(1, L, H, generalised=True, compute_dtype=DTYPE, max_batch=B).cuda()
    loader = SyntheticPianorollLoader(B, H, a.batches, seed=3, device="cuda", pool=a.batches)
    for _ in range(a.warmup):
        timed_pass(loader, model)
        timed_pass(loader, model, note_thresholds=NOTE_THRESHOLDS)
    runs = {"default": [], "notes": []}
    for _ in range(a.repeats):
        torch.manual_seed(1)
        ms, base = timed_pass(loader, model)
        runs["default"].append(ms)
        torch.manual_seed(1)
        ms, res = timed_pass(loader, model, note_thresholds=NOTE_THRESHOLDS)
        runs["notes"].append(ms)
    lines = [f"evaluate() at {H}x{H}, latent {L}, batch {B}, {DTYPE}, {a.batches} pooled batches per pass; {a.warmup} warm-up passes of each kind, "
             f"then {a.repeats} timed passes of each, alternating; host clock from the start of the pass to a device synchronise after it.",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    stat = {}
    for k, label in (("default", "default pass (torch reductions, four host reads per batch)"),
                     ("notes", f"note_thresholds={NOTE_THRESHOLDS} (one metrics call per batch, one read per pass)")):
        per = [ms / a.batches for ms in runs[k]]
        stat[k] = (statistics.median(per), max(per) - min(per))
        lines.append(f"{label}\n    ms per batch: " + "  ".join(f"{v:.4f}" for v in per)
                     + f"\n    median {stat[k][0]:.4f}   spread (max - min) {stat[k][1]:.4f}")
    excess = stat["notes"][0] - stat["default"][0]
    lines.append(f"notes pass minus default pass, medians: {excess:+.4f} ms per batch ({100 * excess / stat['default'][0]:+.1f} %); "
                 f"the default pass's own spread is {stat['default'][1]:.4f}: "
                 + ("not slower beyond the spread" if excess <= stat["default"][1] else "SLOWER beyond the spread"))
    lines.append(f"same pass, both ways: mse {base['mse']:.9f} / {res['mse']:.9f} %, mae {base['mae']:.9f} / {res['mae']:.9f} %; "
                 f"bce {res['bce']:.6f} nat, f1 {res['f1']:.3f} %, note density {res['note_density']:.3f} %")
    lines.append("")
    # the kernels alone: distinct (output, stimulus) pairs, 2 x 16.8 MB each, 32 of them = 1.07 GB per round
    model.eval()
    pairs = []
    with torch.no_grad():
        for x, _ in loader:
            pairs.append((model(x)["output"].clone(), x))
    nbytes = 2 * pairs[0][0].numel() * 4
    ballast = torch.randn(8192, 8192, device="cuda")
    torch.mm(ballast, ballast)
    lines.append(f"vae_recon_metrics alone (cell pass + fold; device events around {4 * len(pairs)} calls on {len(pairs)} distinct batches, "
                 f"{nbytes / 1e6:.1f} MB read per call; medians of three runs):")
    for queued in (True, False):
        lines.append("  every call queued before the first runs (device time):" if queued else
                     "  calls issued as a pass issues them (device time or the host's issue rate, whichever is longer):")
        for name, th in (("1 threshold", (0.5,)), ("2 thresholds", NOTE_THRESHOLDS), ("8 thresholds", SWEEP8)):
            rates = [kernel_time(pairs, th, 4, ballast if queued else None) for _ in range(3)]
            s = statistics.median(rates)
            lines.append(f"    {name:13s} {s * 1e6:8.2f} us per call (" + ", ".join(f"{r * 1e6:.2f}" for r in rates)
                         + f")   {nbytes / s / 1e12:.2f} TB/s = {100 * nbytes / s / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
