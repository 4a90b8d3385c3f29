"""Diagnostic (GPU box): times of the differentiable paths outside the training step at the bench configuration (128x128, L=16,
B=256, bf16).  Device events around whole calls after warm-up:
  * encode(x) alone against the whole forward (train mode, no_grad);
  * decode(z) forward + backward (train mode, z.requires_grad, upstream gradient on xhat) against the fused training step;
  * the input-gradient kernel of encoder.0 (conv1_dgrad_kernel) from the library's per-kernel profile of a train-mode
    forward + backward with x.requires_grad: microseconds and achieved bytes/s of its algorithmic traffic (reads dz0 and y0,
    writes dx).
Prints one JSON line."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from torch_vae_amd import _lib
from torch_vae_amd.models import VanillaVAE
from torch_vae_amd.optim import FusedAdamW
from torch_vae_amd.train import SyntheticPianorollLoader

H, L, B = 128, 16, 256
REPS = int(os.environ.get("GRAD_PATHS_REPS", "20"))

model = VanillaVAE(1, L, H, generalised=True, compute_dtype="bf16", max_batch=B).cuda()
opt = FusedAdamW([{"params": model.encoder.parameters()}, {"params": model.decoder.parameters()}], lr=1e-4, weight_decay=0.0)
x = SyntheticPianorollLoader(B, H, 1, seed=3, device="cuda").batch(0)[0]
z = torch.randn(B, L, device="cuda")
g = torch.rand(B, 1, H, H, device="cuda") / (B * H * H)


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def encode():
    with torch.no_grad():
        model.encode(x)


def forward():
    with torch.no_grad():
        model(x)


def decode_fwd_bwd():
    zg = z.clone().requires_grad_(True)
    model.decode(zg).backward(g)


def step():
    model.fused_train_step(opt, x)


model.train()
res = {"config": f"{H}x{H} L={L} B={B} bf16", "reps": REPS,
       "encode_ms": timed(encode, REPS), "forward_ms": timed(forward, REPS),
       "decode_fwd_bwd_ms": timed(decode_fwd_bwd, REPS), "fused_step_ms": timed(step, REPS)}

# the input-gradient kernel, from the library's profile (ProfScope "conv1_dgrad": algorithmic bytes = 2*B*(H/2)^2*32*2 + 4*B*H*H)
L_ = _lib.lib()
h = model._ctx.handle
xg = x.clone().requires_grad_(True)
for i in range(REPS + 1):
    if i == 1:
        _lib.check(L_.vae_profile(h, 1), "vae_profile")
    model.zero_grad(set_to_none=True)
    model.loss(model(xg))["loss"].backward()
torch.cuda.synchronize()
buf = ctypes.create_string_buffer(1 << 16)
_lib.check(L_.vae_profile_report(h, buf, len(buf)), "vae_profile_report")
L_.vae_profile(h, 0)
rep = [r for r in json.loads(buf.value.decode()) if r["name"].startswith("conv1_dgrad")]
assert rep, "conv1_dgrad was not profiled"
r = rep[0]
us = 1e3 * r["ms"] / r["calls"]
res.update(conv1_dgrad_us=us, conv1_dgrad_bytes=r["bytes"] / r["calls"], conv1_dgrad_GBps=(r["bytes"] / r["calls"]) / (us * 1e-6) / 1e9)
print(json.dumps(res), flush=True)
