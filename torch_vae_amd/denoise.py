"""Corruption of pianorolls for the denoising / infilling objective (include/vae_denoise.h; Vincent et al. 2008; Im et al. 2017): the
encoder sees ``corrupt_rolls(x)``, the reconstruction term is taken against ``x`` (``model(x_corrupt, target=x)``,
``fused_step(..., target=x)``).

``corrupt_rolls`` drops whole notes, zeroes a time span and adds spurious cells in one HIP launch, ``corruption_spans`` gives the
spans it draws, ``Corruption`` holds the settings of a training run.  Every draw is a function of (seed, counter), so a resumed run
continues them; nothing is read back."""
from __future__ import annotations

import math

import torch

from . import _lib

_U64 = (1 << 64) - 1


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _probability(v, name) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not 0.0 <= v <= 1.0:
        raise ValueError(f"{name} must be a probability in [0, 1], got {v!r}")
    return float(v)


def _finite(v, name) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def _counter(v, name) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return v & _U64        # (counters live modulo 2^64, as in the library)


def _checked_span(span, w: int) -> tuple[int, int]:
    """(span_min, span_max) of ``span``: None or 0 = no span, an int = that length, a pair = a length drawn from min..max."""
    if span is None:
        return 0, 0
    if isinstance(span, int) and not isinstance(span, bool):
        span = (span, span)
    if (not isinstance(span, (tuple, list)) or len(span) != 2
            or any(isinstance(v, bool) or not isinstance(v, int) for v in span)):
        raise ValueError(f"span must be None, a length or a pair (min, max) of lengths, got {span!r}")
    lo, hi = int(span[0]), int(span[1])
    if not 0 <= lo <= hi <= w:
        raise ValueError(f"span needs 0 <= min <= max <= {w} time steps, got {span!r}")
    return lo, hi


def _checked_rolls(x):
    if not isinstance(x, torch.Tensor):
        raise TypeError("rolls must be a tensor")
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError(f"rolls must be [n, h, w] or [n, 1, h, w], got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"rolls must be float32, got {x.dtype}")
    n, h, w = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
    if not 1 <= h <= _lib.DENOISE_MAX_ROWS or not 8 <= w <= _lib.DENOISE_MAX_COLS or w % 8:
        raise ValueError(f"need 1..2^20 pitch rows and a multiple of 8 in 8..2^20 time steps, got {h}x{w}")
    if x.device.type != "cuda":
        raise ValueError("rolls must be on the GPU: the corruption runs on the HIP kernel only")
    return x.detach().contiguous(), n, h, w


def _checked_spans(spans, n: int, dev):
    if spans is None:
        return None
    if not isinstance(spans, torch.Tensor):
        spans = torch.as_tensor(spans)
    if spans.shape != (n, 2) or spans.dtype.is_floating_point or spans.dtype == torch.bool:
        raise ValueError(f"spans must be integers [{n}, 2] - (first column, length) per roll - got {tuple(spans.shape)} {spans.dtype}")
    return spans.detach().to(dev, torch.int32).contiguous()


def corrupt_rolls(x, *, note_dropout=0.0, span=None, add_noise=0.0, threshold=0.5, add_value=1.0, seed=0, counter0=0,
                  counter_stride=1, spans=None, return_hidden=False):
    """The corruption of float32 rolls ([n,h,w] or [n,1,h,w] on the GPU, w a multiple of 8) in one HIP launch, as a new tensor of x's
    shape; x is not touched.  In this order (roll b has the counter ``counter0 + b * counter_stride``, modulo 2^64):
      * ``note_dropout``: every note - a maximal run along time of cells ``>= threshold`` within one pitch row - is removed whole
        with this probability (its cells become 0; every other cell keeps its value, so velocity rolls stay velocity rolls);
      * ``span``: None, a length, or ``(min, max)``: a time span of a length drawn from min..max at a drawn position is zeroed in
        every row; ``spans`` (integers [n, 2]: first column and length per roll, clipped to the roll) gives them instead;
      * ``add_noise``: every cell that is off in x and outside the span becomes ``add_value`` with this probability.
    With ``return_hidden`` also the mask of what was hidden, uint8 [n,(1,)h,w/8] in numpy.packbits order: a bit is set where the
    result differs from x in on/off state or lies inside the span.  The same arguments give the same bits; nothing is read back."""
    p_drop, p_add = _probability(note_dropout, "note_dropout"), _probability(add_noise, "add_noise")
    th, av = _finite(threshold, "threshold"), _finite(add_value, "add_value")
    seed, c0, cs = _counter(seed, "seed"), _counter(counter0, "counter0"), _counter(counter_stride, "counter_stride")
    xc, n, h, w = _checked_rolls(x)
    smin, smax = _checked_span(span, w)
    spans = _checked_spans(spans, n, xc.device)
    out = torch.empty_like(xc)
    hidden = torch.empty(*xc.shape[:-1], w // 8, dtype=torch.uint8, device=xc.device) if return_hidden else None
    if n:
        with torch.cuda.device(xc.device):
            _lib.check(_lib.lib().vae_denoise_corrupt(xc.data_ptr(), out.data_ptr(), _lib.ptr(hidden), n, h, w, th, p_drop, smin, smax,
                                                      p_add, av, _lib.ptr(spans), seed, c0, cs, _stream(xc.device)), "vae_denoise_corrupt")
    return (out, hidden) if return_hidden else out


def corruption_spans(n, w, span, *, seed=0, counter0=0, counter_stride=1, device="cuda") -> torch.Tensor:
    """int32 [n, 2] on the device: (first column, length) of the time span ``corrupt_rolls`` draws for each of n rolls of w time steps
    with these arguments ((0, 0) without a span)."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"n must be an integer >= 0, got {n!r}")
    if isinstance(w, bool) or not isinstance(w, int) or not 8 <= w <= _lib.DENOISE_MAX_COLS or w % 8:
        raise ValueError(f"w must be a multiple of 8 in 8..2^20, got {w!r}")
    smin, smax = _checked_span(span, w)
    seed, c0, cs = _counter(seed, "seed"), _counter(counter0, "counter0"), _counter(counter_stride, "counter_stride")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("corruption_spans runs on the GPU only")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(n, 2, dtype=torch.int32, device=dev)
    if n:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().vae_denoise_params(out.data_ptr(), n, w, smin, smax, seed, c0, cs, _stream(dev)), "vae_denoise_params")
    return out


class Corruption:
    """The corruption settings of a training run: ``corruption(x, counter0)`` is ``corrupt_rolls`` with them."""

    def __init__(self, note_dropout=0.0, span=None, add_noise=0.0, seed=0, threshold=0.5, add_value=1.0):
        self.note_dropout, self.add_noise = _probability(note_dropout, "denoise_note_dropout"), _probability(add_noise, "denoise_add_noise")
        if span is not None and not isinstance(span, int):
            span = tuple(span)
        _checked_span(span, _lib.DENOISE_MAX_COLS)      # (against the roll's width: at the call)
        self.span = span
        self.seed = _counter(seed, "denoise_seed")
        self.threshold, self.add_value = _finite(threshold, "threshold"), _finite(add_value, "add_value")

    def __call__(self, x, counter0=0, counter_stride=1, return_hidden=False):
        return corrupt_rolls(x, note_dropout=self.note_dropout, span=self.span, add_noise=self.add_noise, threshold=self.threshold,
                             add_value=self.add_value, seed=self.seed, counter0=counter0, counter_stride=counter_stride,
                             return_hidden=return_hidden)

    @classmethod
    def from_config(cls, config) -> "Corruption | None":
        """The corruption ``config`` asks for (``denoise_note_dropout``, ``denoise_span``, ``denoise_add_noise``, ``denoise_seed``),
        or None when it sets none of the first three: the training loop is then the one without the option."""
        drop, span, add = (getattr(config, k, None) for k in ("denoise_note_dropout", "denoise_span", "denoise_add_noise"))
        if drop is None and span is None and add is None:
            return None
        seed = getattr(config, "denoise_seed", None)
        return cls(drop or 0.0, span, add or 0.0, 0 if seed is None else seed)
