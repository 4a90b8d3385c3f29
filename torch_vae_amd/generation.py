"""Music out of the model: note events from decoded pianorolls, on the device (include/vae_step.h: vae_extract_notes).

``sample()`` and ``decode()`` return a float32 probability image [B,1,H,W], pitch rows by time columns.  ``extract_notes`` turns it
into notes - hysteresis thresholding, gap bridging and a minimum duration per pitch row - without copying the image to the host, and
into cleaned bit planes in ``numpy.packbits`` order, the layout ``PianorollDataset.from_stored(..., "bits")`` reads, so generated or
denoised rolls can go straight back into a resident dataset.  ``VanillaVAE.sample_notes`` and ``VanillaVAE.interpolate`` are the
model-level entries; ``evaluation.note_event_metrics`` scores two event lists against each other."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from .types_helpers import NoteEvents


def _f32(v: float) -> float:
    return ctypes.c_float(float(v)).value


def _checked_note_rolls(rolls):
    if not isinstance(rolls, torch.Tensor):
        raise TypeError("rolls must be a tensor")
    if rolls.dim() == 4 and rolls.shape[1] == 1:
        rolls = rolls[:, 0]
    if rolls.dim() != 3:
        raise ValueError(f"rolls must be [n, h, w] or [n, 1, h, w], got {tuple(rolls.shape)}")
    if rolls.dtype != torch.float32:
        raise TypeError(f"rolls must be float32, got {rolls.dtype}")
    if rolls.device.type != "cuda":
        raise ValueError("rolls must be on the GPU: note extraction runs on the HIP kernels only")
    if not rolls.is_contiguous():
        raise ValueError("rolls must be contiguous")
    n, h, w = rolls.shape
    if h < 1 or w < 8 or w % 8 or w > 65536:
        raise ValueError(f"need h >= 1 and w a multiple of 8 in 8..65536, got h={h}, w={w}")
    return rolls.detach(), n, h, w


def _extract_call(rolls, n, h, w, on, off, D, G, events, peaks, capacity, offsets, cleaned):
    dev = rolls.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_extract_notes(
            rolls.data_ptr(), n, h, w, on, off, D, G, _lib.ptr(events), _lib.ptr(peaks), capacity, offsets.data_ptr(), _lib.ptr(cleaned),
            torch.cuda.current_stream(dev).cuda_stream), "vae_extract_notes")


def extract_notes(rolls, *, onset_threshold=0.5, sustain_threshold=None, min_duration=1, max_gap=0, max_notes=None,
                  cleaned=False) -> NoteEvents:
    """Note events of ``rolls`` ([n,h,w] or [n,1,h,w] float32, contiguous, on the GPU; w a multiple of 8).  Per pitch row: a cell
    switches the note on at ``x >= onset_threshold``, off at ``not (x >= sustain_threshold)`` (a NaN is off) and otherwise keeps the
    state (``sustain_threshold=None``: the onset threshold, plain thresholding); silent gaps of at most ``max_gap`` steps between
    two sounding cells are bridged; runs shorter than ``min_duration`` are dropped.  Returns device tensors: ``events`` int32 [N,4]
    rows (roll, pitch, onset, duration) ascending by (roll, pitch, onset), ``peaks`` float32 [N] (the largest input value of the
    note, exact), ``offsets`` int64 [n+1] (roll r's events are ``events[offsets[r]:offsets[r+1]]``), ``total`` (a view of
    ``offsets[n]``) and ``cleaned`` (uint8 [n,h,w/8], the kept cells as bit planes, most significant bit first) or None.
    ``max_notes=None`` counts first, reads the total once and allocates exactly; with ``max_notes`` given nothing is read back, the
    tensors hold ``max_notes`` slots, events past them are not written and the caller compares ``total`` with it.  Repeated
    calls give the same bits.  Not differentiable."""
    rolls, n, h, w = _checked_note_rolls(rolls)
    on = _f32(onset_threshold)
    off = on if sustain_threshold is None else _f32(sustain_threshold)
    if not (math.isfinite(on) and math.isfinite(off)) or off > on:
        raise ValueError(f"need finite thresholds with sustain <= onset, got onset={onset_threshold}, sustain={sustain_threshold}")
    for name, v, lo in (("min_duration", min_duration, 1), ("max_gap", max_gap, 0)):
        if isinstance(v, bool) or int(v) != v or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}, got {v}")
    D, G = min(int(min_duration), 2 ** 31 - 1), min(int(max_gap), 2 ** 31 - 1)
    if max_notes is not None and (isinstance(max_notes, bool) or int(max_notes) != max_notes or max_notes < 0):
        raise ValueError(f"max_notes must be None or an integer >= 0, got {max_notes}")
    dev = rolls.device
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    planes = torch.empty(n, h, w // 8, dtype=torch.uint8, device=dev) if cleaned else None
    if n == 0:      # (an empty tensor has no address to hand over)
        offsets.zero_()
        cap = int(max_notes or 0)
        return NoteEvents(events=torch.empty(cap, 4, dtype=torch.int32, device=dev), peaks=torch.empty(cap, dtype=torch.float32, device=dev),
                          offsets=offsets, cleaned=planes, total=offsets[0])
    if max_notes is None:
        _extract_call(rolls, n, h, w, on, off, D, G, None, None, 0, offsets, None)
        capacity = int(offsets[n])
    else:
        capacity = int(max_notes)
    events = torch.empty(capacity, 4, dtype=torch.int32, device=dev)
    peaks = torch.empty(capacity, dtype=torch.float32, device=dev)
    if capacity or planes is not None or max_notes is not None:
        # (no slot to write: the count-only form of the call, which still writes offsets and the planes)
        _extract_call(rolls, n, h, w, on, off, D, G, events if capacity else None, peaks if capacity else None, capacity, offsets, planes)
    return NoteEvents(events=events, peaks=peaks, offsets=offsets, cleaned=planes, total=offsets[n])


def binarize_rolls(rolls, threshold=0.5) -> torch.Tensor:
    """``rolls >= threshold`` as bit planes uint8 [n,h,w/8], most significant bit first: ``numpy.packbits(x >= t, axis=-1)`` in one
    launch chain on the device (the cleaned planes of vae_extract_notes with both thresholds equal, min_duration 1, max_gap 0)."""
    rolls, n, h, w = _checked_note_rolls(rolls)
    t = _f32(threshold)
    if not math.isfinite(t):
        raise ValueError(f"threshold must be finite, got {threshold}")
    offsets = torch.empty(n + 1, dtype=torch.int64, device=rolls.device)
    planes = torch.empty(n, h, w // 8, dtype=torch.uint8, device=rolls.device)
    if n:
        _extract_call(rolls, n, h, w, t, t, 1, 0, None, None, 0, offsets, planes)
    return planes


def events_to_lists(result, *, pitch_offset=0, step_seconds=None):
    """Host lists out of an ``extract_notes`` result, with one read-back: per roll a list of ``(pitch, onset, duration, velocity)``,
    ``pitch`` shifted by ``pitch_offset`` (the MIDI number of row 0), ``velocity = round(127 * clamp(peak, 0, 1))``, onset and
    duration in steps, or in seconds when ``step_seconds`` is given.  Only events that were written count (``max_notes``)."""
    events, peaks, offsets = result["events"], result["peaks"], result["offsets"]
    n = offsets.numel() - 1
    cap = events.shape[0]
    # one buffer, one copy: offsets, then the events and the peaks' bit patterns as int64
    host = torch.cat([offsets.reshape(-1), events.reshape(-1).to(torch.int64), peaks.view(torch.int32).to(torch.int64)]).cpu()
    off = host[:n + 1].tolist()
    ev = host[n + 1:n + 1 + 4 * cap].reshape(cap, 4).tolist()
    pk = host[n + 1 + 4 * cap:].to(torch.int32).view(torch.float32).tolist()
    out = []
    for r in range(n):
        notes = []
        for i in range(min(off[r], cap), min(off[r + 1], cap)):
            _, p, t0, d = ev[i]
            vel = int(round(127.0 * min(max(pk[i], 0.0), 1.0)))
            if step_seconds is None:
                notes.append((p + pitch_offset, t0, d, vel))
            else:
                notes.append((p + pitch_offset, t0 * step_seconds, d * step_seconds, vel))
        out.append(notes)
    return out


def interpolate_latents(z_a: torch.Tensor, z_b: torch.Tensor, steps: int, mode: str = "slerp") -> torch.Tensor:
    """[pairs, steps, L]: the path from z_a[i] to z_b[i] at t = 0, 1/(steps-1), ..., 1 (steps = 1: t = 0).  "lerp": (1-t) a + t b.
    "slerp": sin((1-t) w)/sin(w) a + sin(t w)/sin(w) b with w the angle between a and b; where w < 1e-6 (or a vector is zero) the
    row falls back to lerp.  Plain torch."""
    if mode not in ("slerp", "lerp"):
        raise ValueError(f"mode must be 'slerp' or 'lerp', got {mode!r}")
    if isinstance(steps, bool) or int(steps) != steps or steps < 1:
        raise ValueError(f"steps must be an integer >= 1, got {steps}")
    if z_a.dim() != 2 or z_a.shape != z_b.shape:
        raise ValueError(f"need two [pairs, L] tensors, got {tuple(z_a.shape)} and {tuple(z_b.shape)}")
    f64 = dict(device=z_a.device, dtype=torch.float64)   # (float64 inside: acos is ill-conditioned near parallel vectors)
    t = (torch.linspace(0.0, 1.0, int(steps), **f64) if steps > 1 else torch.zeros(1, **f64)).view(1, -1, 1)
    a, b = z_a.double().unsqueeze(1), z_b.double().unsqueeze(1)
    lerp = (1.0 - t) * a + t * b
    if mode == "lerp":
        return lerp.to(z_a.dtype)
    na, nb = a.norm(dim=-1, keepdim=True), b.norm(dim=-1, keepdim=True)
    cos = ((a * b).sum(-1, keepdim=True) / (na * nb).clamp_min(1e-300)).clamp(-1.0, 1.0)
    omega = torch.acos(cos)
    flat = (omega < 1e-6) | (na == 0) | (nb == 0)
    so = torch.sin(torch.where(flat, torch.ones_like(omega), omega))
    slerp = torch.sin((1.0 - t) * omega) / so * a + torch.sin(t * omega) / so * b
    return torch.where(flat, lerp, slerp).to(z_a.dtype)


def traverse(model, z, dim, values, threshold=0.5):
    """Decode ``z`` [n, latent_dim] with latent dimension ``dim`` replaced by each of ``values`` (a sequence or 1-D tensor of
    ``steps`` numbers) - with a model trained under ``attr_reg={attribute: dim}`` this turns the attribute up and down while the rest
    of the phrase stays.  Decoded with running statistics (eval mode, the model untouched).  Returns
    ``(rolls [n, steps, 1, H, W], counters [n, steps, 8])`` on the device, the counters ``attributes.roll_attributes`` of the rolls
    cut at ``threshold``; nothing is read back."""
    from .attributes import roll_attributes
    model._require_device()
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[1] != model.latent_dim:
        raise ValueError(f"z must be a tensor [n, {model.latent_dim}], got {tuple(z.shape) if isinstance(z, torch.Tensor) else type(z)}")
    if isinstance(dim, bool) or not isinstance(dim, int) or not 0 <= dim < model.latent_dim:
        raise ValueError(f"dim must be a latent dimension in 0..{model.latent_dim - 1}, got {dim!r}")
    dev = model._flat.device
    on_device = isinstance(values, torch.Tensor) and values.is_cuda
    values = values.detach().to(dev, torch.float32).reshape(-1) if on_device else [float(v) for v in torch.as_tensor(values).reshape(-1).tolist()]
    n, steps = z.shape[0], len(values)
    if steps < 1:
        raise ValueError("values must hold at least one number")
    zz = z.detach().to(dev, torch.float32)[:, None, :].repeat(1, steps, 1)
    if on_device:
        zz[:, :, dim] = values
    else:       # host numbers go in as kernel arguments: a copy from pageable host memory would wait for the stream
        for s, v in enumerate(values):
            zz[:, s, dim].fill_(v)
    with torch.no_grad():
        rolls = model._run_decode(zz.view(n * steps, model.latent_dim), train=False)
    counters = roll_attributes(rolls, threshold)
    return rolls.view(n, steps, *rolls.shape[1:]), counters.view(n, steps, -1)


def checked_time_span(t0, t1, width: int) -> tuple[int, int]:
    """(t0, t1) as integers with 0 <= t0 < t1 <= width; ValueError otherwise."""
    for name, v in (("t0", t0), ("t1", t1)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer time step, got {v!r}")
    if not 0 <= t0 < t1 <= width:
        raise ValueError(f"need 0 <= t0 < t1 <= {width}, got [{t0}, {t1})")
    return t0, t1


def infill(model, x, t0, t1, *, threshold=None):
    """Fill the time span ``[t0, t1)`` of the rolls ``x`` [n,1,H,W]: the model encodes x with those columns zeroed - what a model
    trained on ``denoise_span`` corruptions saw - and decodes the posterior mean (running statistics, eval mode, the model
    untouched, no noise drawn).  Returns ``(filled, xhat)``: ``filled`` is x outside the span, bit for bit, and inside it the
    reconstruction - binarised to 0/1 at ``threshold`` when one is given - and ``xhat`` the raw reconstruction of the whole roll.
    Nothing is read back."""
    model._check_input(x)
    t0, t1 = checked_time_span(t0, t1, x.shape[-1])
    if threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not math.isfinite(threshold)):
        raise ValueError(f"threshold must be None or a finite number, got {threshold!r}")
    x = x.detach().contiguous().float()
    masked = x.clone()
    masked[..., t0:t1] = 0.0
    with torch.no_grad():
        mu, _, _ = model._run_encode(masked, train=False)
        xhat = model._run_decode(mu, train=False)
    inside = xhat[..., t0:t1]
    filled = x.clone()
    filled[..., t0:t1] = inside if threshold is None else (inside >= _f32(threshold)).to(torch.float32)
    return filled, xhat
