"""Musical attributes of pianorolls and what ties a latent dimension to one (include/vae_attributes.h; Pati & Lerch 2020,
"Attribute-based Regularization of Latent Spaces for VAEs").

``roll_attributes`` counts, ``attribute_values`` turns the counters into the seven attributes, ``attribute_regularizer`` is the
in-batch loss ``mean_ij |tanh(delta (z_i - z_j)) - sgn(a_i - a_j)|`` with its gradient on z, ``attribute_correlation`` the Kendall
tau-b of every latent dimension with every attribute over a set.  Everything that touches rolls or latents runs on the HIP kernels;
only ``attribute_correlation`` reads back (once)."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib

ATTRIBUTE_NAMES = tuple(_lib.ATTRIBUTES)
COUNTER_COLUMNS = {name: i for i, name in enumerate(_lib.ATTR_COUNTERS)}


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _finite_number(v, name, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"{name} must be a finite number" + (" > 0" if positive else "") + f", got {v!r}")
    return float(v)


def attribute_ids(names) -> list[int]:
    """VAE_ATTR_* numbers of attribute names; ValueError on an unknown one."""
    ids = []
    for name in names:
        if not isinstance(name, str) or name not in _lib.ATTRIBUTES:
            raise ValueError(f"unknown attribute {name!r}: the attributes are {', '.join(ATTRIBUTE_NAMES)}")
        ids.append(_lib.ATTRIBUTES[name])
    return ids


def checked_attr_reg(attr_reg, latent_dim, weight=1.0, delta=10.0, threshold=0.5, batch=None):
    """(attribute numbers, dimensions, weight, delta, threshold) of a model's attr_reg / attr_weight / attr_delta / attr_threshold,
    or None when attr_reg is None; ValueError on anything the library would refuse."""
    if attr_reg is None:
        return None
    if not isinstance(attr_reg, dict) or not attr_reg:
        raise ValueError(f"attr_reg must be None or a dict of attribute name -> latent dimension, got {attr_reg!r}")
    if len(attr_reg) > _lib.ATTR_MAX_PAIRS:
        raise ValueError(f"attr_reg names {len(attr_reg)} pairs, more than the {_lib.ATTR_MAX_PAIRS} one step takes")
    ids = attribute_ids(attr_reg)
    dims = []
    for name, d in attr_reg.items():
        if isinstance(d, bool) or not isinstance(d, int) or not 0 <= d < latent_dim:
            raise ValueError(f"attr_reg[{name!r}] must be a latent dimension in 0..{latent_dim - 1}, got {d!r}")
        if d in dims:
            raise ValueError(f"attr_reg names latent dimension {d} twice: one attribute per dimension")
        dims.append(d)
    w = _finite_number(weight, "attr_weight")
    dl = _finite_number(delta, "attr_delta", positive=True)
    th = _finite_number(threshold, "attr_threshold")
    if batch is not None and batch > _lib.ATTR_MAX_BATCH:
        raise ValueError(f"attr_reg takes batches of at most {_lib.ATTR_MAX_BATCH}, got {batch}")
    return ids, dims, w, dl, th


def _checked_rolls(x):
    if not isinstance(x, torch.Tensor):
        raise TypeError("rolls must be a tensor")
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3:
        raise ValueError(f"rolls must be [n, h, w] or [n, 1, h, w], got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"rolls must be float32, got {x.dtype}")
    n, h, w = (int(v) for v in x.shape)
    if not 1 <= h <= _lib.ATTR_MAX_ROWS or w < 1 or h * w > _lib.ATTR_MAX_CELLS:
        raise ValueError(f"need 1..{_lib.ATTR_MAX_ROWS} pitch rows, at least one time step and at most 2^20 cells a roll, got {h}x{w}")
    if x.device.type != "cuda":
        raise ValueError("rolls must be on the GPU: the counters run on the HIP kernels only")
    return x.detach().contiguous(), n, h, w


def roll_attributes(x, threshold=0.5) -> torch.Tensor:
    """The integer counters of float32 rolls ([n,h,w] or [n,1,h,w] on the GPU; a cell is set iff ``value >= threshold``) in one HIP
    pass: int32 [n, 8] on the device, columns ``COUNTER_COLUMNS`` - cells, notes, used_pitches, lowest, highest, sounding_steps,
    onset_steps (as ``music_statistics`` defines them; any width, not only multiples of 32) and pitch_sum.  Nothing is read back."""
    th = _finite_number(threshold, "threshold")
    x, n, h, w = _checked_rolls(x)
    out = torch.empty(n, len(_lib.ATTR_COUNTERS), dtype=torch.int32, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().vae_attr_roll_counters(x.data_ptr(), n, h, w, th, out.data_ptr(), _stream(x.device)), "vae_attr_roll_counters")
    return out


def attribute_values(counters, names) -> torch.Tensor:
    """float64 [n, len(names)] attribute values from int32 counters [n, 8] (any device), each one IEEE operation on the integers -
    the values the kernels compare: note_density = cells, note_count = notes, pitch_range = highest - lowest + 1 (0 if empty),
    mean_pitch = pitch_sum / cells (-1 if empty), polyphony = cells / sounding_steps (0 if empty), onset_steps, used_pitches."""
    ids = attribute_ids(names)
    if counters.dim() != 2 or counters.shape[1] != len(_lib.ATTR_COUNTERS):
        raise ValueError(f"counters must be [n, {len(_lib.ATTR_COUNTERS)}], got {tuple(counters.shape)}")
    c = counters.to(torch.int64)
    cells, f = c[:, 0], c.double()
    some = cells > 0
    one = torch.ones_like(f[:, 0])
    cols = {0: lambda: f[:, 0], 1: lambda: f[:, 1],
            2: lambda: torch.where(some, (c[:, 4] - c[:, 3] + 1).double(), 0 * one),
            3: lambda: torch.where(some, f[:, 7] / torch.where(some, f[:, 0], one), -one),
            4: lambda: torch.where(some, f[:, 0] / torch.where(some, f[:, 5], one), 0 * one),
            5: lambda: f[:, 6], 6: lambda: f[:, 2]}
    return torch.stack([cols[i]() for i in ids], dim=1) if ids else f[:, :0]


def _checked_latents(z, counters, what):
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float32:
        raise ValueError(f"{what}: z must be a float32 tensor [n, latent_dim]")
    if not isinstance(counters, torch.Tensor) or counters.dtype != torch.int32 or tuple(counters.shape) != (z.shape[0], len(_lib.ATTR_COUNTERS)):
        raise ValueError(f"{what}: counters must be int32 [{z.shape[0]}, {len(_lib.ATTR_COUNTERS)}] (roll_attributes of the same rolls)")
    if z.device.type != "cuda" or counters.device != z.device:
        raise ValueError(f"{what}: z and counters must be on the same GPU")
    if not 1 <= z.shape[1] <= _lib.ATTR_MAX_DIM:
        raise ValueError(f"{what}: latent_dim must be in 1..{_lib.ATTR_MAX_DIM}, got {z.shape[1]}")
    return z.detach().contiguous(), counters.contiguous()


def _i32_array(values):
    return (ctypes.c_int32 * len(values))(*values)


def attribute_regularizer(z, counters, ids, dims, delta, weight, want_grad=True):
    """vae_attr_regularizer on z [B, L] and the counters of the same rolls: (loss float64 [1 + pairs], g_z [B, L] or None), on the
    device, g_z = weight * d loss[0] / dz.  ``ids`` / ``dims``: what ``checked_attr_reg`` returns."""
    z, counters = _checked_latents(z, counters, "attribute_regularizer")
    B, L = z.shape
    if not 1 <= B <= _lib.ATTR_MAX_BATCH:
        raise ValueError(f"attribute_regularizer takes batches of 1..{_lib.ATTR_MAX_BATCH}, got {B}")
    loss = torch.empty(1 + len(ids), dtype=torch.float64, device=z.device)
    g = torch.empty(B, L, dtype=torch.float32, device=z.device) if want_grad else None
    with torch.cuda.device(z.device):
        _lib.check(_lib.lib().vae_attr_regularizer(z.data_ptr(), L, L, counters.data_ptr(), B, len(ids), _i32_array(ids), _i32_array(dims),
                                                   float(delta), float(weight), loss.data_ptr(), _lib.ptr(g), _stream(z.device)),
                   "vae_attr_regularizer")
    return loss, g


def tau_b(S, ties_z, ties_a, n) -> torch.Tensor:
    """Kendall tau-b [A, L] (float64) from the concordance sums of n points: S / sqrt((n0 - ties_z)(n0 - ties_a)), n0 = n (n - 1) / 2;
    NaN where the denominator is zero (a constant dimension or attribute, or n < 2)."""
    n0 = n * (n - 1) // 2
    den = ((n0 - ties_a).double()[:, None] * (n0 - ties_z).double()[None, :]).sqrt()
    return torch.where(den > 0, S.double() / torch.where(den > 0, den, torch.ones_like(den)), torch.full_like(den, float("nan")))


def attribute_correlation(z, counters, names) -> torch.Tensor:
    """Kendall tau-b of every latent dimension with every named attribute over a set of up to 65536 points: z [N, L] float32 and
    counters int32 [N, 8] on the GPU -> float64 [len(names), L] on the host.  The exact int64 concordance sums and tie counts of all
    N (N - 1) / 2 pairs come from one HIP pass (vae_attr_concordance) and are read back once."""
    ids = attribute_ids(names)
    if not 1 <= len(ids) <= len(ATTRIBUTE_NAMES):
        raise ValueError(f"attribute_correlation takes 1..{len(ATTRIBUTE_NAMES)} attribute names, got {len(ids)}")
    z, counters = _checked_latents(z, counters, "attribute_correlation")
    N, L = z.shape
    if N > _lib.ATTR_MAX_POINTS:
        raise ValueError(f"attribute_correlation takes at most {_lib.ATTR_MAX_POINTS} points, got {N}")
    A = len(ids)
    buf = torch.empty(A * L + L + A, dtype=torch.int64, device=z.device)
    S, tz, ta = buf[:A * L], buf[A * L:A * L + L], buf[A * L + L:]
    if N == 0:      # (an empty tensor has no address to hand over)
        buf.zero_()
    else:
        with torch.cuda.device(z.device):
            _lib.check(_lib.lib().vae_attr_concordance(z.data_ptr(), L, L, counters.data_ptr(), N, A, _i32_array(ids), S.data_ptr(), tz.data_ptr(),
                                                       ta.data_ptr(), _stream(z.device)), "vae_attr_concordance")
    host = buf.cpu()
    return tau_b(host[:A * L].view(A, L), host[A * L:A * L + L], host[A * L + L:], N)


class AttributeTerm(torch.autograd.Function):
    """weight * loss[0] of the regulariser as a differentiable function of the latents (the autograd path of VanillaVAE.loss): the
    backward returns the kernel's own g_z times the upstream gradient."""

    @staticmethod
    def forward(ctx, z, counters, model, setting):
        ids, dims, w, delta, _ = setting
        loss, g = attribute_regularizer(z, counters, ids, dims, delta, w, want_grad=True)
        model._attr_loss = loss
        ctx.save_for_backward(g)
        return (loss[0] * w).float()

    @staticmethod
    def backward(ctx, g_out):
        (g,) = ctx.saved_tensors
        return g * g_out, None, None, None
