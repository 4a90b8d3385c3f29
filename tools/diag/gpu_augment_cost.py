"""Diagnostic (GPU box): cost record of the device pianoroll loader (torch_vae_amd/data.py, vae_gather_rolls).  Three measurements in
one visit, written as text to profiles/augment_loader_cost.txt (or --out):
  1. default path unchanged - bench.py --gpus 1 --steps 200 --warmup 20 in a built checkout of the parent commit (--parent DIR) and
     in this tree, one process per run, alternating, 5 runs each; skipped when no parent tree is given;
  2. kernel time at B=256, 128x128 with device events in alternating blocks after warm-up: vae_expand_stimuli on a device-resident
     bit-plane batch (the yardstick: the same stores), vae_gather_rolls with identity parameters on the same batch, and
     vae_gather_rolls out of a resident set of 128x256 rolls with random window, time shift and transposition.  The destination
     rotates over buffers larger together than the 256 MB memory-side cache, so the stores go to HBM in every variant;
  3. end to end - train_one_epoch samples/s over the device loader (augmentation on) against a host loop of pinned bit-plane
     batches (train.pack_bits), alternating epochs."""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_loader_cost.txt"))
ap.add_argument("--parent", default=None, help="built checkout of the parent commit (its bench.py is run from there)")
ap.add_argument("--bench-runs", type=int, default=5)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--launches", type=int, default=400, help="launches per block")
ap.add_argument("--epochs", type=int, default=5, help="timed epochs per loader")
ap.add_argument("--batches", type=int, default=100, help="batches per epoch")
args = ap.parse_args()

H, W, L, B = 128, 128, 16, 256
P, T = 6, 8
COPY_TBS = 6.29   # measured float4 copy bandwidth of the MI355X, TB/s
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


# ---- 1. default path: the benchmark in the parent's tree and in this one, before this process opens the GPU
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
    say(f"Default path: python bench.py --gpus 1 --steps 200 --warmup 20, parent and this commit each in its own built tree, one process per run,")
    say(f"processes alternating; {args.bench_runs} runs each.")
    say("  run   parent ms_per_step  host_enqueue_ms   samples/s  |  new ms_per_step  host_enqueue_ms   samples/s")
    for i in range(args.bench_runs):
        a, b = res["parent"][i], res["new"][i]
        say(f"  {i + 1}     {a['ms_per_step']:<18.4f} {a['host_enqueue_ms_per_step']:<16.4f} {a['value']:<10.1f} |  {b['ms_per_step']:<16.4f} "
            f"{b['host_enqueue_ms_per_step']:<16.4f} {b['value']:.1f}")
    pm, nm = med([r["ms_per_step"] for r in res["parent"]]), med([r["ms_per_step"] for r in res["new"]])
    spread = max(r["ms_per_step"] for r in res["parent"]) - min(r["ms_per_step"] for r in res["parent"])
    say(f"  median  {pm:<18.4f}                             |  {nm:.4f}")
    say(f"  parent's own spread (max - min): ms_per_step {spread:.4f} ({100 * spread / pm:.2f} % of its median)")
    say(f"  new median - parent median: ms_per_step {nm - pm:+.4f} (band +-{spread:.4f}): {'inside' if abs(nm - pm) <= spread else 'OUTSIDE'}")
    say()
else:
    say("Default path: not measured in this run (no parent tree given).")
    say()

import torch  # noqa: E402

from torch_vae_amd import _lib, data  # noqa: E402
from torch_vae_amd.models import VanillaVAE  # noqa: E402
from torch_vae_amd.train import build_optimizer, train_one_epoch  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
lib = _lib.lib()
stream = torch.cuda.current_stream().cuda_stream
g = torch.Generator().manual_seed(0)

# ---- 2. kernel time
n_dst = 28                                                       # 28 x 16.8 MB = 470 MB of destinations
dst = [torch.empty(B, 1, H, W, device="cuda") for _ in range(n_dst)]
torch.manual_seed(0)


def random_planes(n, w):
    """[n, H, w/8] bit planes of density 1/16, made on the device (the AND of four random bytes)"""
    r = lambda: torch.randint(0, 256, (n, H, w // 8), device="cuda", dtype=torch.uint8)
    return r() & r() & r() & r()


batch_bits = random_planes(B, W)
n_long = args.batches * B
long_bits = random_planes(n_long, 2 * W)                          # the resident set
perm = torch.randperm(n_long, generator=g).cuda()
stall_a = torch.randn(8192, 8192, device="cuda")


def k_expand(i):
    _lib.check(lib.vae_expand_stimuli(batch_bits.data_ptr(), 1, dst[i % n_dst].data_ptr(), B * H * W, stream), "expand")


def k_identity(i):
    data.gather_rolls(batch_bits, "bits", W, batch=B, out=dst[i % n_dst])


def k_augment(i):
    lo = (i * B) % n_long
    data.gather_rolls(long_bits, "bits", W, index=perm[lo:lo + B], seed=1, counter0=i * B, max_pitch_shift=P, max_time_shift=T,
                      crop_mode=_lib.CROP_RANDOM, out=dst[i % n_dst])


KERNELS = {"expand_stimuli": k_expand, "gather identity": k_identity, "gather 2w crop+shifts": k_augment}


late = 0


def block(fn, n):
    """us per launch.  The kernels take a few us, less than the host needs to enqueue one, so the stream is first kept busy with
    matrix products (some 20 ms) while the host queues the whole block: the device then runs the launches back to back."""
    global late
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        torch.mm(stall_a, stall_a)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    late += int(e0.query())      # the timed window had begun before the last launch was queued: the figure includes host time
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


for fn in KERNELS.values():
    block(fn, 100)
kt = {k: [] for k in KERNELS}
order = list(KERNELS)
for i in range(args.blocks):
    for k in (order if i % 2 == 0 else order[::-1]):
        kt[k].append(block(KERNELS[k], args.launches))
want = torch.empty_like(dst[0])
_lib.check(lib.vae_expand_stimuli(batch_bits.data_ptr(), 1, want.data_ptr(), B * H * W, stream), "expand")
assert torch.equal(data.gather_rolls(batch_bits, "bits", W, batch=B), want), "identity gather differs from vae_expand_stimuli"
say(f"Kernel time, B={B}, {H}x{W}, bit planes on the device; device events around {args.launches} launches per block, queued while the stream is")
say(f"held busy so that the device runs them back to back ({late} of {3 * args.blocks + 3} blocks began before their last launch was queued);")
say(f"{args.blocks} alternating blocks after 100 warm-up launches; destinations rotate over {n_dst} buffers ({n_dst * B * H * W * 4 / 1e6:.0f} MB).  us per launch:")
say("  block   " + "   ".join(f"{k:<22s}" for k in KERNELS))
for i in range(args.blocks):
    say(f"  {i + 1:<7d} " + "   ".join(f"{kt[k][i]:<22.3f}" for k in KERNELS))
say("  median  " + "   ".join(f"{med(kt[k]):<22.3f}" for k in KERNELS))
say("  spread  " + "   ".join(f"{max(kt[k]) - min(kt[k]):<22.3f}" for k in KERNELS) + "  (max - min over the blocks)")
wbytes = B * H * W * 4
for k in KERNELS:
    tbs = wbytes / (med(kt[k]) * 1e-6) / 1e12
    say(f"  {k}: {wbytes / 1e6:.1f} MB written per launch -> {tbs:.2f} TB/s of stores, {100 * tbs / COPY_TBS:.0f} % of the {COPY_TBS} TB/s copy figure"
        f" (a copy moves each byte twice; these kernels read 1/32 as much as they write)")
d_id = med(kt["gather identity"]) - med(kt["expand_stimuli"])
sp = max(kt["expand_stimuli"]) - min(kt["expand_stimuli"])
say(f"  identity gather - expansion: {d_id:+.3f} us per launch; the expansion's own block-to-block spread is {sp:.3f} us: "
    f"{'inside' if d_id <= sp else 'OUTSIDE'}")
say()

# ---- 3. end to end
cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle", epochs=1,
                log_wandb=False, print_interval=100000, log_interval=100000, freeze_encoder=False, global_rank=0, seed=0,
                aug_pitch_shift=P, aug_time_shift=T, img_size=W)
model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).cuda()
opt, sched = build_optimizer(cfg, model, steps_per_epoch=1000000)
ds = data.PianorollDataset.from_stored(long_bits, "bits")       # the resident set above, as it is
device_loader = data.DevicePianorollLoader.from_config(cfg, ds, True, rank=0, world=1)
labels = torch.zeros(B, dtype=torch.long)
centre = long_bits[:, :, W // 16: W // 16 + W // 8].cpu()      # the same rolls' centre windows as host bit-plane batches
host_loader = [(centre[k * B:(k + 1) * B].unsqueeze(1).contiguous().pin_memory(), labels) for k in range(args.batches)]
LOADERS = {"host loop, pinned bit planes": host_loader, "device loader, augmented": device_loader}


def epoch(loader, e):
    with contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train_one_epoch(cfg, model, opt, sched, model.loss, loader, device="cuda", epoch=e)
        torch.cuda.synchronize()
    return len(loader) * B / (time.perf_counter() - t0)


for ld in LOADERS.values():
    epoch(ld, 0)
rate = {k: [] for k in LOADERS}
order = list(LOADERS)
for i in range(args.epochs):
    for k in (order if i % 2 == 0 else order[::-1]):
        rate[k].append(epoch(LOADERS[k], 1 + i))
say(f"End to end: train_one_epoch over {args.batches} batches of {B} (bf16, latent {L}), samples/s from a host clock around the epoch (it ends in a")
say(f"synchronise); {args.epochs} alternating epochs per loader after one warm-up epoch each.  Device loader: {n_long} resident rolls of {H}x{2 * W},")
say(f"random window, time shift up to {T}, transposition up to {P}.")
say("  epoch   " + "   ".join(f"{k:<30s}" for k in LOADERS))
for i in range(args.epochs):
    say(f"  {i + 1:<7d} " + "   ".join(f"{rate[k][i]:<30.0f}" for k in LOADERS))
say("  median  " + "   ".join(f"{med(rate[k]):<30.0f}" for k in LOADERS))
say("  spread  " + "   ".join(f"{max(rate[k]) - min(rate[k]):<30.0f}" for k in LOADERS))
hk, dk = order
floor = med(rate[hk]) - (max(rate[hk]) - min(rate[hk]))
say(f"  device loader median {med(rate[dk]):.0f} against the host loop's median minus its spread {floor:.0f}: "
    f"{'not slower' if med(rate[dk]) >= floor else 'SLOWER'}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
