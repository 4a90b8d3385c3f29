"""Fused AdamW over the model's flat parameter buffer.

Behaves as ``torch.optim.AdamW`` (train.py:228): same ``param_groups`` keys, so
``torch.optim.lr_scheduler.OneCycleLR`` (train.py:233-238) drives ``lr`` and
``betas[0]`` exactly as it does for the reference.  ``step()`` is one kernel launch
for all groups (include/vae_step.h: vae_adamw_step).

Gradient-norm clipping and non-finite step skipping (``max_grad_norm``, ``skip_nonfinite``) run on the device, inside the
update (include/vae_step.h: vae_adamw_step_clipped / vae_train_step_fused_clipped): no host synchronisation per step.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import _lib


def _check_max_grad_norm(v):
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(float(v)) or float(v) <= 0:
        raise ValueError(f"max_grad_norm must be a positive number or None, got {v!r}")
    return float(v)


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW over the flat buffers of one VanillaVAE (at most two groups: encoder, decoder).

    ``max_grad_norm``: the update uses ``g * grad_scale * coef`` with torch.nn.utils.clip_grad_norm_'s
    ``coef = min(1, max_grad_norm / (total_norm + 1e-6))``, where ``total_norm`` is the L2 norm of ``g * grad_scale`` over
    every range this optimiser updates, all groups together (taken in f64; coef rounded once to f32).  The one difference
    from calling torch's in-place ``clip_grad_norm_`` before ``step()``: ``p.grad`` / ``flat_grads()`` keep the UNCLIPPED
    gradient, the clipping happens inside the update.  None: no clipping; the norm is still reported.

    ``skip_nonfinite``: when the total norm is inf or NaN the update is skipped on the device - parameters, ``exp_avg`` and
    ``exp_avg_sq`` stay bit-unchanged, the AdamW step count does not advance (as with torch's GradScaler) and
    ``skipped_steps`` grows by one.  BatchNorm running statistics were already updated by the forward, as in torch.
    Without it, non-finite gradients propagate as with ``clip_grad_norm_(error_if_nonfinite=False)``.

    ``last_grad_norm`` (0-d float64 device tensor, pre-clip norm of the last step, overwritten in place by the next one; None
    before the first) and
    ``skipped_steps`` (0-d int64 device tensor) are read without a host synchronisation.  Once either option is set the
    step count lives on the device for the optimiser's life; ``state_dict()`` reads it back (one synchronisation).  Both
    options are attributes, not ``param_groups`` keys, and may be reassigned between steps.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None,
                 skip_nonfinite=False):
        # (the inert keys are torch.optim.AdamW's: checkpoints written by either optimiser then carry the same param_group
        #  keys and load into the other, reference train.py:320-329)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._model = None
        self._m = self._v = None
        self._step = 0
        self.grad_scale = 1.0
        if len(self.param_groups) > 2:
            raise ValueError("FusedAdamW supports at most two parameter groups (encoder, decoder)")
        self._clip_on = False    # set for good by either option: the step count then lives on the device
        self._clip = None        # (step int64, skipped int64, norm f64, scratch uint8) on the model's device
        self._clip_stepped = False
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite

    @property
    def max_grad_norm(self):
        return self.__dict__.get("_max_grad_norm")

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        self.__dict__["_max_grad_norm"] = _check_max_grad_norm(v)
        self._clip_on = self._clip_on or v is not None

    @property
    def skip_nonfinite(self):
        return self.__dict__.get("_skip_nonfinite", False)

    @skip_nonfinite.setter
    def skip_nonfinite(self, v):
        if not isinstance(v, bool):
            raise ValueError(f"skip_nonfinite must be a bool, got {v!r}")
        self.__dict__["_skip_nonfinite"] = v
        self._clip_on = self._clip_on or v

    @property
    def last_grad_norm(self):
        return self._clip[2] if self._clip_stepped else None

    @property
    def skipped_steps(self):
        return self._clip_state()[1] if self._clip_on and self._model_ready() else None

    def _model_ready(self):
        try:
            self._bind()
        except ValueError:
            return False
        return True

    def _clip_state(self):
        """The device state of the clipped update, created on first use (the step count so far carried over)."""
        if self._clip is None:
            self._bind()
            dev = self._m.device
            self._clip = (torch.full((), self._step, dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.int64, device=dev),
                          torch.full((), float("nan"), dtype=torch.float64, device=dev),
                          torch.empty(_lib.GRAD_CLIP_SCRATCH_BYTES, dtype=torch.uint8, device=dev))
        return self._clip

    def _clip_args(self):
        """(max_grad_norm, skip_nonfinite, step, norm_out, skipped, scratch) of the clipped entry points, or None."""
        if not self._clip_on:
            return None
        step, skipped, norm, scratch = self._clip_state()
        return (float(self.max_grad_norm or 0.0), int(self.skip_nonfinite), step.data_ptr(), norm.data_ptr(), skipped.data_ptr(),
                scratch.data_ptr())

    def state_dict(self):
        if self._clip is not None:     # the device step count (one synchronisation, at checkpoint time)
            self._step = int(self._clip[0])
            self._step_t.fill_(float(self._step))
        return super().state_dict()

    def _bind(self):
        if self._model is not None:
            return
        owners = {getattr(p, "_vae_owner", None) for g in self.param_groups for p in g["params"]}
        if len(owners) != 1 or None in owners:
            raise ValueError("FusedAdamW needs parameters of one torch_vae_amd VanillaVAE that is already on the GPU "
                             "(move the model with .to('cuda') before building the optimiser)")
        self._model = next(iter(owners))()
        model = self._model
        self._ranges = []
        for g in self.param_groups:
            idx = sorted(p._vae_index for p in g["params"])
            if idx != list(range(idx[0], idx[-1] + 1)):
                raise ValueError("each FusedAdamW group must be a contiguous run of model parameters")
            start = model._offs[idx[0]]
            self._ranges.append((start, model._offs[idx[-1]] + model._sizes[idx[-1]] - start))
        flat = model.flat_parameters()
        self._m = torch.zeros_like(flat)
        self._v = torch.zeros_like(flat)
        # one step counter tensor shared by every parameter's state (torch keeps one per parameter and bumps each: 16 host
        # tensor ops per step); state_dict() shows the same values either way
        self._step_t = torch.tensor(0.0)
        for g in self.param_groups:
            for p in g["params"]:
                o, n = model._offs[p._vae_index], model._sizes[p._vae_index]
                self.state[p] = {"step": self._step_t, "exp_avg": self._m[o:o + n].view(p.shape),
                                 "exp_avg_sq": self._v[o:o + n].view(p.shape)}

    def load_state_dict(self, state_dict):
        """torch's loader replaces the state tensors; copy them back into the flat moment buffers."""
        self._bind()
        super().load_state_dict(state_dict)
        model = self._model
        step = 0
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state.get(p, {})
                o, n = model._offs[p._vae_index], model._sizes[p._vae_index]
                for key, flat in (("exp_avg", self._m), ("exp_avg_sq", self._v)):
                    view = flat[o:o + n].view(p.shape)
                    if key in st:
                        view.copy_(st[key])
                    st[key] = view
                step = max(step, int(st.get("step", 0)))
                self.state[p] = st
        self._step = step
        self._step_t = torch.tensor(float(step))
        if self._clip is not None:
            self._clip[0].fill_(step)
        for g in self.param_groups:
            for p in g["params"]:
                self.state[p]["step"] = self._step_t

    def _step_args(self):
        """(ngroups, offsets, sizes, lrs, beta1s, beta2, eps, weight_decay) of the next update as the C ABI wants them, for
        the one-call fused step (VanillaVAE.fused_train_step): every group is active there, the gradients being the flat
        buffer's.  The ctypes arrays are cached; only the two scheduler-driven values per group are refreshed."""
        self._bind()
        cache = self.__dict__.get("_arg_cache")
        n = len(self.param_groups)
        if cache is None:
            cache = ((C.c_int64 * n)(*[r[0] for r in self._ranges]), (C.c_int64 * n)(*[r[1] for r in self._ranges]),
                     (C.c_double * n)(), (C.c_double * n)())
            self.__dict__["_arg_cache"] = cache
        offs, sizes, lrs, b1s = cache
        g0 = self.param_groups[0]
        for i, g in enumerate(self.param_groups):
            lrs[i] = g["lr"]; b1s[i] = g["betas"][0]
            if (g["betas"][1], g["eps"], g["weight_decay"]) != (g0["betas"][1], g0["eps"], g0["weight_decay"]):
                raise NotImplementedError("groups must share beta2, eps and weight_decay")
        return n, offs, sizes, lrs, b1s, float(g0["betas"][1]), float(g0["eps"]), float(g0["weight_decay"])

    def _stepped(self):
        """Bookkeeping of an update the library performed inside vae_train_step_fused."""
        if self._clip_on:
            self._clip_stepped = True     # (the count is on the device)
        else:
            self._step += 1
            self._step_t += 1
        self._opt_called = True   # (torch's schedulers check that the optimiser stepped before them)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._bind()
        model = self._model
        gflat = model.flat_grads()
        views = model._param_grad_views()[1]
        active = []
        for g, rng in zip(self.param_groups, self._ranges):
            grads = [p.grad for p in g["params"]]
            if all(gr is None for gr in grads):
                continue  # torch skips parameters without gradients
            for p, gr in zip(g["params"], grads):
                if gr is views[p._vae_index]:
                    continue              # the fused path's own view of the flat gradient buffer
                o, n = model._offs[p._vae_index], model._sizes[p._vae_index]
                if gr is None:
                    raise NotImplementedError("a FusedAdamW group with only some gradients set")
                if gr.data_ptr() != gflat.data_ptr() + 4 * o:
                    gflat[o:o + n].view(p.shape).copy_(gr)  # foreign gradient tensor: stage it
            active.append((g, rng))
        if not active:
            return loss
        clip = self._clip_args()
        if clip is None:
            self._step += 1
        n = len(active)
        offs = (C.c_int64 * n)(*[r[0] for _, r in active])
        sizes = (C.c_int64 * n)(*[r[1] for _, r in active])
        lrs = (C.c_double * n)(*[float(g["lr"]) for g, _ in active])
        b1s = (C.c_double * n)(*[float(g["betas"][0]) for g, _ in active])
        g0 = active[0][0]
        for g, _ in active:
            if (g["betas"][1], g["eps"], g["weight_decay"]) != (g0["betas"][1], g0["eps"], g0["weight_decay"]):
                raise NotImplementedError("groups must share beta2, eps and weight_decay")
        dev = gflat.device
        with model._device_guard():    # launch on the model's device, whatever the caller's current device is
            if clip is not None:
                _lib.check(_lib.lib().vae_adamw_step_clipped(
                    model.flat_parameters().data_ptr(), gflat.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), n, offs, sizes,
                    lrs, b1s, float(g0["betas"][1]), float(g0["eps"]), float(g0["weight_decay"]), float(self.grad_scale),
                    *clip, torch.cuda.current_stream(dev).cuda_stream), "vae_adamw_step_clipped")
                self._clip_stepped = True
                return loss
            _lib.check(_lib.lib().vae_adamw_step(
                model.flat_parameters().data_ptr(), gflat.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), n, offs, sizes,
                lrs, b1s, float(g0["betas"][1]), float(g0["eps"]), float(g0["weight_decay"]), float(self.grad_scale),
                self._step, torch.cuda.current_stream(dev).cuda_stream), "vae_adamw_step")
        self._step_t += 1
        return loss
