"""Weight averaging beside the fused step (include/vae_average.h): an exponential moving average (EMA) or an equal average over
the tail of the run (SWA, Izmailov et al. 2018) of a ``VanillaVAE``'s flat parameter buffer and BatchNorm buffer, kept in a second
pair of buffers and updated by one HIP launch (plus the single-thread commit of its device state).

``WeightAverage.update(optimizer)`` hands the kernel the device step count of a ``FusedAdamW`` that clips or skips: a step the
optimiser skipped on the device leaves the average untouched, with no host read.  ``with avg.applied():`` swaps the average into
the model in place, so ``evaluate``, ``sample``, ``sample_notes``, ``sample_fidelity`` and the rest run on it unchanged.

Differences from ``torch.optim.swa_utils.AveragedModel``, all deliberate: the average starts as a copy at the first update (as
torch's does) but lives in flat buffers, not in a second module; ``num_batches_tracked`` is never averaged (torch's integer branch
truncates): the averaged model carries the model's own counters; parameters no optimiser touches (``fc_mu``, ``fc_var``,
``decoder_input``, ``final_layer``) average to themselves bit for bit."""
from __future__ import annotations

import contextlib
import math

import torch

from . import _lib

KINDS = {"ema": _lib.AVG_EMA, "swa": _lib.AVG_EQUAL}
BN_RECOVER = 10.0      # 1 / kBnMom: a train-mode forward from zeroed buffers leaves fl(0.1f * stat) in them (update_bn)


def _number(v, name, lo=0.0, hi=math.inf) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or not lo <= v <= hi or math.isinf(v):
        raise ValueError(f"{name} must be a finite number in [{lo:g}, {hi:g}], got {v!r}")
    return float(v)


def _count(v, name, lo=0) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return v


def schedule_due(total_step: int, start_step: int = 0, every: int = 1) -> bool:
    """Whether the step that made ``total_step`` the count of steps taken is followed by an update: a function of ``total_step``
    alone, so a resumed run continues the schedule."""
    return total_step >= start_step and (total_step - start_step) % every == 0


class WeightAverage:
    """The average of ``model`` (a ``VanillaVAE`` on the GPU): ``kind`` "ema" with ``decay`` (and, with ``warmup`` > 0, the decay
    ``min(decay, (1 + n) / (warmup + n))`` at the n-th update) or "swa", the equal average of every update.  ``use_buffers``: the
    BatchNorm running means and variances are averaged with the parameters; without it the averaged model keeps the buffers the
    model had when the average was built, until ``update_bn`` recomputes them (torch's semantics).

    ``start_step`` / ``every`` (``from_config``: ``avg_start_step``, ``avg_every``) are the training loop's schedule: it updates
    after the steps for which ``due(total_step)``."""

    def __init__(self, model, kind="ema", decay=0.999, warmup=0.0, use_buffers=True):
        from .models import VanillaVAE
        if not isinstance(model, VanillaVAE):
            raise TypeError("WeightAverage averages the flat buffers of a torch_vae_amd VanillaVAE")
        if not isinstance(kind, str) or kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        self.kind = kind
        self.decay = _number(decay, "decay", 0.0, 1.0)
        self.warmup = _number(warmup, "warmup")
        if not isinstance(use_buffers, bool):
            raise ValueError(f"use_buffers must be a bool, got {use_buffers!r}")
        self.use_buffers = use_buffers
        self.start_step, self.every = 0, 1
        model._require_device()
        self._model = model
        self._params = model._flat.detach().clone()
        self._buffers = model._bnflat.detach().clone()
        self._state = torch.zeros(_lib.AVG_STATE_BYTES // 8, dtype=torch.int64, device=self._params.device)
        self._applied = False
        self.reset()

    # -- construction from a run's configuration ----------------------------------------------------------------------
    @classmethod
    def from_config(cls, config, model) -> "WeightAverage | None":
        """The average ``config`` asks for (``weight_average``: "ema", "swa" or None; ``ema_decay``, ``ema_warmup``,
        ``avg_start_step``, ``avg_every``), or None when ``weight_average`` is None or absent."""
        kind = getattr(config, "weight_average", None)
        if kind is None:
            return None
        decay, warmup = getattr(config, "ema_decay", None), getattr(config, "ema_warmup", None)
        start, every = getattr(config, "avg_start_step", None), getattr(config, "avg_every", None)
        start, every = _count(0 if start is None else start, "avg_start_step"), _count(1 if every is None else every, "avg_every", 1)
        out = cls(model, kind=kind, decay=0.999 if decay is None else decay, warmup=0.0 if warmup is None else warmup)
        out.start_step, out.every = start, every
        return out

    def due(self, total_step: int) -> bool:
        return schedule_due(total_step, self.start_step, self.every)

    # -- the library calls ----------------------------------------------------------------------------------------------
    def _live(self):
        """The model's flat buffers as they are now: the average follows a model that stays on its device."""
        m = self._model
        m._require_device()
        if m._flat.device != self._params.device or m._flat.shape != self._params.shape:
            raise RuntimeError("the model's flat buffers changed device or size since the average was built: build a new WeightAverage")
        return m._flat, m._bnflat

    def _stream(self):
        return torch.cuda.current_stream(self._params.device).cuda_stream

    @staticmethod
    def _step_counter(optimizer):
        """The device step count of a FusedAdamW that keeps one (max_grad_norm / skip_nonfinite), else None."""
        from .optim import FusedAdamW
        if isinstance(optimizer, FusedAdamW) and optimizer._clip_on:
            return optimizer._clip_state()[0]
        return None

    def reset(self, optimizer=None, n_averaged: int = 0):
        """Start over (or from ``n_averaged`` updates): the next update copies when ``n_averaged`` is 0.  With an optimiser that keeps
        its step count on the device that count is marked as seen, on the device: the next update applies only once a step has."""
        step = self._step_counter(optimizer)
        if step is not None and step.device != self._state.device:
            raise RuntimeError("the optimiser's step count and the average are on different devices")
        with torch.cuda.device(self._params.device):
            _lib.check(_lib.lib().vae_average_state_init(self._state.data_ptr(), _lib.ptr(step), _count(n_averaged, "n_averaged"),
                                                         self._stream()), "vae_average_state_init")

    @torch.no_grad()
    def update(self, optimizer=None):
        """One averaging update from the model's current parameters (and buffers), on the model's device and the current stream.
        ``optimizer``: a ``FusedAdamW`` with ``max_grad_norm`` or ``skip_nonfinite`` passes its device step count, and the update
        applies only if that count moved since the last applied update; any other optimiser (or None): it always applies."""
        if self._applied:
            raise RuntimeError("update() inside applied(): the model holds the average, not the weights being trained")
        flat, bnflat = self._live()
        step = self._step_counter(optimizer)
        nb = bnflat.numel() if self.use_buffers else 0
        with torch.cuda.device(flat.device):
            _lib.check(_lib.lib().vae_average_update(
                self._params.data_ptr(), flat.data_ptr(), flat.numel(), 1.0, self._buffers.data_ptr() if nb else 0,
                bnflat.data_ptr() if nb else 0, nb, 1.0, KINDS[self.kind], self.decay, self.warmup, _lib.ptr(step),
                self._state.data_ptr(), self._stream()), "vae_average_update")

    @property
    def n_averaged(self) -> torch.Tensor:
        """Updates applied so far: a 0-d int64 device tensor (a view of the device state; no synchronisation)."""
        return self._state[1]

    @property
    def last_weight(self) -> torch.Tensor:
        """The weight of the last applied update (1 for the copy): a 0-d float64 device tensor, no synchronisation."""
        return self._state.view(torch.float64)[2]

    def _swap(self):
        flat, bnflat = self._live()
        with torch.cuda.device(flat.device):
            _lib.check(_lib.lib().vae_average_swap(flat.data_ptr(), self._params.data_ptr(), flat.numel(), bnflat.data_ptr(),
                                                   self._buffers.data_ptr(), bnflat.numel(), self._stream()), "vae_average_swap")

    @contextlib.contextmanager
    def applied(self):
        """The model runs on the average inside the block: parameters and BatchNorm buffers are exchanged with the averaged ones in
        place (one launch, no copy of either) and exchanged back on exit, exception or not.  The model's last-forward record is
        dropped on entry and on exit: nothing differentiates through the change.  Does not nest."""
        if self._applied:
            raise RuntimeError("applied() does not nest: the model already holds the average")
        self._swap()
        self._applied = True
        self._model._last = None
        try:
            yield self._model
        finally:
            self._swap()
            self._applied = False
            self._model._last = None

    @torch.no_grad()
    def copy_to(self, model=None):
        """Write the average into ``model`` (default: the averaged model itself) for good."""
        if self._applied:
            raise RuntimeError("copy_to() inside applied()")
        model = self._model if model is None else model
        model._require_device()
        if model._flat.shape != self._params.shape or model._bnflat.shape != self._buffers.shape:
            raise ValueError("copy_to needs a VanillaVAE of the averaged model's geometry")
        model._flat.copy_(self._params)
        model._bnflat.copy_(self._buffers)
        model._last = None

    def module_state_dict(self) -> dict:
        """The average under ``model.state_dict()``'s keys (new tensors): loads into a ``VanillaVAE`` and into the reference's model.
        ``num_batches_tracked`` is the model's own."""
        if self._applied:
            raise RuntimeError("module_state_dict() inside applied()")
        m = self._model
        self._live()
        out = {}
        where = {}
        for i, name in enumerate(_lib.PARAM_NAMES):
            where[name] = (self._params, m._offs[i], m._sizes[i])
        for i, name in enumerate(_lib.BN_NAMES):
            c, o = m._bn_ch[i], m._bn_offs[i]
            where[name + ".running_mean"] = (self._buffers, o, c)
            where[name + ".running_var"] = (self._buffers, o + c, c)
        for key, value in m.state_dict().items():
            if key in where:
                buf, o, n = where[key]
                out[key] = buf[o:o + n].view(value.shape).clone()
            else:
                out[key] = value.detach().clone()
        return out

    # -- checkpoints ------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Everything a resumed run needs (one synchronisation, at checkpoint time, for the three numbers of the device state)."""
        if self._applied:
            raise RuntimeError("state_dict() inside applied()")
        raw = self._state.cpu()
        return {"kind": self.kind, "decay": self.decay, "warmup": self.warmup, "use_buffers": self.use_buffers,
                "start_step": self.start_step, "every": self.every, "params": self._params.clone(), "buffers": self._buffers.clone(),
                "n_averaged": int(raw[1]), "seen_step": int(raw[0]), "last_weight": float(raw.view(torch.float64)[2])}

    @torch.no_grad()
    def load_state_dict(self, state: dict, optimizer=None):
        """Restore ``state_dict()``'s result.  With the (already restored) optimiser its device step count is marked as seen, on the
        device; without one the checkpoint's own ``seen_step`` is."""
        if self._applied:
            raise RuntimeError("load_state_dict() inside applied()")
        if state["kind"] not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {state['kind']!r}")
        if state["params"].shape != self._params.shape or state["buffers"].shape != self._buffers.shape:
            raise ValueError("the checkpoint's average belongs to a model of another geometry")
        self.kind, self.decay, self.warmup = state["kind"], _number(state["decay"], "decay", 0.0, 1.0), _number(state["warmup"], "warmup")
        self.use_buffers = bool(state["use_buffers"])
        self.start_step, self.every = _count(state.get("start_step", 0), "start_step"), _count(state.get("every", 1), "every", 1)
        self._params.copy_(state["params"])
        self._buffers.copy_(state["buffers"])
        self.reset(optimizer, int(state["n_averaged"]))
        if self._step_counter(optimizer) is None:
            self._state[0].fill_(int(state.get("seen_step", -1)))
        self.last_weight.fill_(float(state.get("last_weight", 0.0)))

    # -- BatchNorm statistics of the averaged weights ---------------------------------------------------------------------
    @torch.no_grad()
    def update_bn(self, loader, device=None, *, eps=None):
        """``torch.optim.swa_utils.update_bn`` for the averaged weights: one pass over ``loader`` (batches, or tuples whose first
        entry is the batch) and the averaged model's running means and variances become the cumulative mean (momentum ``None``) of
        the per-batch statistics.  No forward kernel changes for it: inside ``applied()`` the model's buffer is zeroed before each
        batch, the train-mode forward leaves ``fl(0.1f * stat)`` there, and one ``vae_average_update`` (equal average, source scaled
        by 10) folds it into the cumulative mean.  The model's own buffers, counters and mode are as before afterwards.
        ``eps``: an iterable of [batch, latent_dim] tensors replacing the forward's draws, one per batch (parity runs)."""
        model = self._model
        dev = self._params.device if device is None else torch.device(device)
        acc = torch.zeros_like(self._buffers)
        state = torch.zeros_like(self._state)
        L, st = _lib.lib(), self._stream()
        with torch.cuda.device(self._params.device):
            _lib.check(L.vae_average_state_init(state.data_ptr(), 0, 0, st), "vae_average_state_init")
        eps = None if eps is None else iter(eps)
        was_training = model.training
        seen = False
        with self.applied():
            kept, kept_nbt = model._bnflat.clone(), model._nbt.clone()     # (the averaged buffers, should the pass fail)
            try:
                model.train()
                for batch in loader:
                    x = batch[0] if isinstance(batch, (tuple, list)) else batch
                    x = x.to(dev)
                    model._bnflat.zero_()
                    model._run_forward(x, None if eps is None else next(eps), train=True, want_pre=False)
                    with torch.cuda.device(self._params.device):
                        _lib.check(L.vae_average_update(acc.data_ptr(), model._bnflat.data_ptr(), acc.numel(), BN_RECOVER, 0, 0, 0, 1.0,
                                                        _lib.AVG_EQUAL, 0.0, 0.0, 0, state.data_ptr(), self._stream()), "vae_average_update")
                    seen = True
                model._bnflat.copy_(acc if seen else kept)     # (exchanged into the average on exit)
            except BaseException:
                model._bnflat.copy_(kept)
                raise
            finally:
                model._nbt.copy_(kept_nbt)
                model.train(was_training)
