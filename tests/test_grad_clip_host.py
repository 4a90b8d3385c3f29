"""Gradient-norm clipping and non-finite step skipping, host side (no GPU): the C-ABI entry points are declared, exported and
refuse bad arguments before anything is enqueued; FusedAdamW validates its options; build_optimizer passes them through and,
without them, builds exactly today's optimiser."""
import ctypes as C
import os
import re
from argparse import Namespace

import pytest
import torch

from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_step.h")
NEW = ("vae_grad_norm", "vae_adamw_step_clipped", "vae_train_step_fused_clipped")


def declared_params(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", open(HEADER).read())
    assert m, f"{name} is not declared in include/vae_step.h"
    return [re.sub(r"\s*\b\w+$", "", " ".join(p.split())).replace(" *", "*") for p in m.group(1).split(",")]


def test_new_symbols_declared_and_exported():
    L = _lib.lib()
    for name in NEW:
        declared_params(name)
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.vae_abi_version() == 1
    hdr = open(HEADER).read()
    assert re.search(r"#define VAE_GRAD_CLIP_SCRATCH_BYTES (\d+)", hdr).group(1) == str(_lib.GRAD_CLIP_SCRATCH_BYTES)
    # the clipped update takes vae_adamw_step's arguments, the host step replaced by the clip arguments and device counters
    plain, clipped = declared_params("vae_adamw_step"), declared_params("vae_adamw_step_clipped")
    assert clipped[:13] == plain[:13] and clipped[-1] == plain[-1] == "vae_stream_t"
    assert clipped[13:-1] == ["double", "int", "int64_t*", "double*", "int64_t*", "void*"]
    fused, fclip = declared_params("vae_train_step_fused"), declared_params("vae_train_step_fused_clipped")
    i = fused.index("int", 21)              # the host step of vae_train_step_fused
    assert fclip[:i] == fused[:i] and fclip[i:i + 6] == clipped[13:-1] and fclip[i + 6:] == fused[i + 1:]


def _arrays():
    return ((C.c_int64 * 2)(0, 1024), (C.c_int64 * 2)(1000, 1000), (C.c_double * 2)(1e-3, 1e-3), (C.c_double * 2)(0.9, 0.9))


@pytest.mark.parametrize("case", ["ngroups0", "ngroups3", "nan_norm", "null_step", "null_norm", "null_skipped", "null_scratch",
                                  "unaligned_scratch", "null_params"])
def test_adamw_step_clipped_refuses_bad_arguments(case):
    L = _lib.lib()
    offs, sizes, lrs, b1s = _arrays()
    # fake, never dereferenced device addresses: every call below must fail on the host, before any launch
    a = dict(params=4096, grads=4096, m=4096, v=4096, n=2, mx=1.0, step=256, norm=256, skipped=256, scratch=4096)
    a.update({"ngroups0": {"n": 0}, "ngroups3": {"n": 3}, "nan_norm": {"mx": float("nan")}, "null_step": {"step": 0},
              "null_norm": {"norm": 0}, "null_skipped": {"skipped": 0}, "null_scratch": {"scratch": 0},
              "unaligned_scratch": {"scratch": 4100}, "null_params": {"params": 0}}[case])
    rc = L.vae_adamw_step_clipped(a["params"], a["grads"], a["m"], a["v"], a["n"], offs, sizes, lrs, b1s, 0.999, 1e-8, 0.0, 1.0,
                                  a["mx"], 1, a["step"], a["norm"], a["skipped"], a["scratch"], None)
    assert rc == -1
    msg = L.vae_last_error().decode()
    assert msg.startswith("vae_adamw_step_clipped: ") and len(msg) > len("vae_adamw_step_clipped: "), msg


def test_fused_clipped_and_grad_norm_refuse_bad_arguments():
    L = _lib.lib()
    offs, sizes, lrs, b1s = _arrays()

    def fused(n=2, mx=1.0, step=256, ctx=None):
        return L.vae_train_step_fused_clipped(ctx, 4096, 4, 4096, 4096, 4096, 4096, 4096, 4096, None, 0, 1.0, n, offs, sizes, lrs,
                                              b1s, 0.999, 1e-8, 0.0, 1.0, mx, 1, step, 256, 256, 4096, 0, 4096, 4096, 4096, 4096,
                                              4096, None)
    # the clip arguments are checked before the context (and so before the forward is enqueued)
    for kw, why in (({"n": 0}, "1 or 2 groups"), ({"mx": float("nan")}, "NaN"), ({"step": 0}, "null device pointer"),
                    ({}, "null ctx")):
        assert fused(**kw) == -1
        msg = L.vae_last_error().decode()
        assert msg.startswith("vae_train_step_fused_clipped: ") and why in msg, (kw, msg)
    assert L.vae_grad_norm(4096, 3, offs, sizes, 1.0, 256, 4096, None) == -1
    assert b"1 or 2 groups" in L.vae_last_error()
    assert L.vae_grad_norm(4096, 2, offs, sizes, 1.0, 0, 4096, None) == -1
    assert b"null device pointer" in L.vae_last_error()
    assert L.vae_grad_norm(0, 2, offs, sizes, 1.0, 256, 4096, None) == -1
    assert b"vae_grad_norm" in L.vae_last_error()


def _model():
    from torch_vae_amd.models import VanillaVAE
    return VanillaVAE(1, 16, 32)


def test_fused_adamw_validates_options():
    from torch_vae_amd.optim import FusedAdamW
    m = _model()
    for bad in (-1.0, -1, 0.0, float("nan"), "1.0", [1.0], True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW(m.parameters(), max_grad_norm=bad)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        FusedAdamW(m.parameters(), skip_nonfinite=1)
    opt = FusedAdamW(m.parameters(), max_grad_norm=2, skip_nonfinite=True)
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float) and opt.skip_nonfinite is True
    assert opt.last_grad_norm is None
    opt.max_grad_norm = None                       # reassignable between steps
    assert opt.max_grad_norm is None
    with pytest.raises(ValueError):
        opt.max_grad_norm = float("nan")
    opt.max_grad_norm = float("inf")               # a clip that never triggers
    # the options are attributes, not param_group keys: torch AdamW's keys, unchanged
    ref = torch.optim.AdamW(_model().parameters())
    assert set(opt.param_groups[0]) == set(ref.param_groups[0])
    assert set(opt.defaults) == set(ref.defaults)


def _cfg(**kw):
    base = dict(batch_size_per_gpu=8, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                epochs=1, freeze_encoder=False)
    return Namespace(**{**base, **kw})


def test_build_optimizer_passes_options_and_refuses_skip_with_torch_optimiser():
    from torch_vae_amd.train import build_optimizer
    opt, _ = build_optimizer(_cfg(max_grad_norm=0.5, skip_nonfinite=True), _model(), steps_per_epoch=10)
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is True and opt._clip_on
    with pytest.raises(NotImplementedError, match="skip_nonfinite"):
        build_optimizer(_cfg(optimizer="Adam", skip_nonfinite=True), _model(), steps_per_epoch=10)
    # clipping alone with a torch optimiser is fine (train_one_epoch calls torch's clip_grad_norm_)
    opt, _ = build_optimizer(_cfg(optimizer="Adam", max_grad_norm=1.0), _model(), steps_per_epoch=10)
    assert isinstance(opt, torch.optim.Adam) and "max_grad_norm" not in opt.defaults


def test_build_optimizer_without_options_is_unchanged():
    from torch_vae_amd.train import build_optimizer
    opt, _ = build_optimizer(_cfg(), _model(), steps_per_epoch=10)
    ref = torch.optim.AdamW(_model().parameters(), lr=1e-3)
    assert [set(g) for g in opt.param_groups] == [set(ref.param_groups[0]) | {"name", "initial_lr", "max_lr", "min_lr", "base_momentum",
                                                                              "max_momentum"}] * 2
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    assert not opt._clip_on and opt._clip is None and opt.skipped_steps is None and opt.last_grad_norm is None
    assert opt._clip_args() is None                # the unclipped entry points, byte for byte today's path
    assert opt.grad_scale == 1.0 and opt._step == 0
