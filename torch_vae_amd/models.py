"""MI355X-native mirror of the reference's ``models.VanillaVAE`` (models.py:7-272).

Same class name, constructor signature, attributes (``encoder``, ``decoder``,
``fc_mu``, ``fc_var``, ``decoder_input``, ``final_layer``, ``kld_weight``,
``latent_dim``), ``state_dict`` keys and output dict shapes, so code written
against the reference (``train.run``, ``evaluation.evaluate``) can use it
unchanged.  The arithmetic is not PyTorch's: ``forward``/``loss``/``backward``
call the hand-written gfx950 kernels behind ``include/vae_step.h``.

The torch sub-modules below are parameter CONTAINERS only (they give the
reference's names, shapes and initialisation); they are never called.  All
parameters are views into one flat f32 HBM buffer so the kernels, the fused
AdamW and the gradient all-reduce see single contiguous ranges.

Deviations from the reference, all explicit:
  * ``in_channels`` must be 1 and ``hidden_dims`` None/[32,64,128,256] (the only
    configuration the hot path in BASELINE.json names).
  * ``generalised=True`` (or ``input_dim != 32``) sizes the bottleneck as
    256*(input_dim/16)^2 instead of the hard-wired 1024 (models.py:33,166).
  * gradients are written to ``param.grad`` by the backward kernel directly
    (no AccumulateGrad hooks fire).
  * ``decode(z)`` records an autograd graph only when ``z`` requires grad (the reference's does whenever a decoder
    parameter requires grad); ``sample()`` runs under ``torch.no_grad()``.
  * ``recon_loss="mse"`` (keyword-only; default ``"bce"``, the reference's
    models.py:208) replaces the reconstruction term of the ELBO by
    ``F.mse_loss(xhat, x)`` - a Gaussian likelihood for velocity-valued rolls
    with targets anywhere in [0, 1].  ``model.recon_loss`` may be reassigned; it
    is read at every forward and fused step.  ``loss()`` keys are unchanged.
  * ``pos_weight=w`` (keyword-only; default ``None`` = off) weights the BCE
    term against the sparsity of pianorolls:
    ``F.binary_cross_entropy(xhat, x, weight=1 + (w - 1) * x)``, the mean still
    over B*H*W.  For 0/1 rolls this is ``BCEWithLogitsLoss(pos_weight=w)``.
    For velocity rolls the weight grows with how much of a note the cell is
    and the per-cell optimum stays ``xhat = x`` (weighting only the positive
    log term would move it).  A finite number in (0, 1024], not with
    ``recon_loss="mse"``; ``evaluation.balanced_pos_weight`` derives one from
    a note density.  Read at every forward and fused step like ``recon_loss``;
    a forward's ``loss()`` and backward use the weight it ran with.
    ``log_likelihood`` ignores it (a weighted BCE is not a likelihood) and
    ``evaluate()``'s ``bce`` stays unweighted.  ``pos_weight=1`` gives the bits
    of plain BCE.  f16 storage: the power-of-two gradient scale is lowered
    by ``2**ceil(log2 w)`` for ``w > 1`` (csrc/vae_ctx.h: set_grad_scale).
  * ``kl_free_bits`` / ``kl_capacity`` (keyword-only; default off, the
    reference's plain KL) replace the KL term of the ELBO by
    ``sum_d max(kl_d, kl_free_bits)`` (Kingma et al. 2016; ``kl_d`` the batch
    mean of dimension d's KL, nats) or ``|KL - kl_capacity|`` (Burgess et al.
    2018; ``kld_weight`` plays gamma).  Both are attributes read at every forward
    and fused step; ``kld_loss`` stays the raw KL.  The reduction and the mask
    / sign decision run on the device in f64, in a fixed order.  Data parallel:
    ``kl_d`` and ``KL`` are the replica's OWN batch means (as BatchNorm
    statistics are per replica), so replicas may mask different dimensions in
    a step; the all-reduce averages the resulting gradients.
  * ``tc_weight`` (keyword-only; default ``None`` = off) is the beta-TCVAE
    objective (Chen et al. 2018) in the form ``KL + (tc_weight - 1) * TC``:
    ``TC = mean_i [log q(z_i) - sum_d log q(z_id)]`` over the in-batch
    mixture ``q``, the query's own component included, at the forward's own
    ``z`` - what ``latent_statistics(mu, log_var, eps=eps[None]).tc`` reports.
    An alternative to ``kl_free_bits`` / ``kl_capacity``; read at every
    forward and fused step; batches of at most 4096.  ``total_correlation()``
    returns the value of the last forward.  Data parallel: TC is over the
    replica's OWN batch, as ``kl_d`` and the BatchNorm statistics are.
  * ``attr_reg`` (keyword-only; default ``None`` = off) ties latent
    dimensions to musical attributes of the input roll (Pati & Lerch 2020):
    a dict ``{attribute: dimension}`` of up to 8 pairs, attributes
    ``note_density``, ``note_count``, ``pitch_range``, ``mean_pitch``,
    ``polyphony``, ``onset_steps``, ``used_pitches``, one attribute per
    dimension.  The loss gains ``attr_weight * sum_r L_r`` with
    ``L_r = mean_ij |tanh(attr_delta (z_i^r - z_j^r)) - sgn(a_i - a_j)|``
    over the batch, the attributes counted from ``x >= attr_threshold`` on the
    device (include/vae_attributes.h).  All four are attributes read at every
    forward and fused step; batches of at most 4096; combines with every
    reconstruction term, KL option and storage type.  ``attribute_loss()``
    returns ``[sum_r L_r, L_1, ...]`` of the last step.  ``kld_loss`` and
    ``reconstruction_loss`` are unchanged.  Data parallel: the replica's OWN
    batch.  f16 storage: the gradient on z rides on the backward's
    power-of-two scale; its entries are at most
    ``attr_weight * 2 * attr_delta / B``.

  Reconstruction term of ``loss = reconstruction + kld_weight * T`` (mean over B*H*W):

    ====================  ===============================
    option                reconstruction
    ====================  ===============================
    (none)                bce(xhat, x)
    ``recon_loss="mse"``  (xhat - x)^2
    ``pos_weight=w``      (1 + (w - 1) x) * bce(xhat, x)
    ====================  ===============================

  KL term ``T`` of ``loss = reconstruction + kld_weight * T``:

    ===================  =============================  ==================
    option               T                              KL gradient
    ===================  =============================  ==================
    (none)               KL                             plain
    ``kl_free_bits=l``   sum_d max(kl_d, l)             0 where kl_d <= l
    ``kl_capacity=C``    |KL - C|                       times sign(KL - C)
    ``tc_weight=b``      KL + (b - 1) TC                plain + (b - 1) dTC
    ===================  =============================  ==================
"""
from __future__ import annotations

import math
import contextlib
import weakref

import torch
from torch import Tensor, nn

from . import _lib
from .attributes import AttributeTerm, attribute_regularizer, checked_attr_reg, roll_attributes
from .types_helpers import EncoderOutput, LikelihoodOutput, LossOutput, ModelOutput

_DTYPES = {"f32": _lib.DTYPE_F32, "fp32": _lib.DTYPE_F32, "float32": _lib.DTYPE_F32,
           "bf16": _lib.DTYPE_BF16, "bfloat16": _lib.DTYPE_BF16,
           "f16": _lib.DTYPE_F16, "fp16": _lib.DTYPE_F16, "float16": _lib.DTYPE_F16, "half": _lib.DTYPE_F16}


_RECON = {"bce": _lib.RECON_BCE, "mse": _lib.RECON_MSE}


def _recon_kind(name) -> int:
    kind = _RECON.get(name) if isinstance(name, str) else None
    if kind is None:
        raise ValueError(f"recon_loss must be one of {sorted(_RECON)}, got {name!r}")
    return kind


def _recon_setting(recon_loss, pos_weight=None) -> tuple[int, float]:
    """(VAE_RECON_* kind, parameter) of the recon_loss / pos_weight pair; ValueError on anything the library would refuse."""
    kind = _recon_kind(recon_loss)
    if pos_weight is None:
        return kind, 0.0
    w = pos_weight
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or not 0 < w <= _lib.POS_WEIGHT_MAX:
        raise ValueError(f"pos_weight must be None or a finite number in (0, {_lib.POS_WEIGHT_MAX:g}], got {pos_weight!r}")
    if kind != _lib.RECON_BCE:
        raise ValueError('pos_weight weights the BCE term: it cannot be combined with recon_loss="mse"')
    return _lib.RECON_WBCE, float(w)


def _kl_objective(free_bits, capacity, tc_weight=None) -> tuple[int, float]:
    """(VAE_KL_* kind, parameter) of the kl_free_bits / kl_capacity / tc_weight triple; ValueError on anything the library would refuse."""
    def number(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        return float(v)
    fb = number(free_bits, "kl_free_bits")
    if tc_weight is not None:
        tcw = number(tc_weight, "tc_weight")
        if fb > 0.0 or capacity is not None:
            raise ValueError("tc_weight, kl_free_bits and kl_capacity are alternatives: set one of them")
        return _lib.KL_TC, tcw
    if capacity is None:
        return (_lib.KL_FREE_BITS, fb) if fb > 0.0 else (_lib.KL_PLAIN, 0.0)
    cap = number(capacity, "kl_capacity")
    if fb > 0.0:
        raise ValueError("kl_free_bits and kl_capacity are alternatives: set one of them")
    return _lib.KL_CAPACITY, cap


_NULL_GUARD = contextlib.nullcontext()


def _stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def _rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class _Context:
    """Owns one vae_ctx (scratch sized for max_batch)."""

    def __init__(self, img_size, latent_dim, max_batch, dtype, generalised):
        self.key = (img_size, latent_dim, max_batch, dtype, generalised)
        self.handle = _lib.lib().vae_create(img_size, latent_dim, max_batch, dtype, int(generalised))
        if not self.handle:
            raise _lib.VaeLibError("vae_create: " + _lib.lib().vae_last_error().decode())
        self.recon = (_lib.RECON_BCE, 0.0)   # the library's default (vae_set_recon_loss_ex): kind, parameter
        self.kl = (_lib.KL_PLAIN, 0.0)  # the library's default (vae_set_kl_objective)

    def set_recon(self, recon: tuple[int, float]):
        if recon != self.recon:         # (kind or weight changed; never for a model that stays with the default)
            _lib.check(_lib.lib().vae_set_recon_loss_ex(self.handle, recon[0], recon[1]), "vae_set_recon_loss_ex")
            self.recon = recon

    def set_kl(self, kl: tuple[int, float]):
        if kl != self.kl:               # (never for a model that leaves both options off: no call beyond the library's default)
            _lib.check(_lib.lib().vae_set_kl_objective(self.handle, kl[0], kl[1]), "vae_set_kl_objective")
            self.kl = kl

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().vae_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class _VAEForward(torch.autograd.Function):
    """forward (models.py:185-188) + backward (train.py:650) through the C ABI."""

    @staticmethod
    def forward(ctx, x, anchor, model, eps, target=None):
        ctx.set_materialize_grads(False)
        ctx.model_ref = weakref.ref(model)      # no model -> _last -> grad_fn -> model reference cycle
        out = model._run_forward(x, eps, train=model.training, target=target)
        ctx.generation = model._fwd_count       # the activations saved for backward live in the context, not in the graph
        handle = torch.zeros((), device=x.device, dtype=torch.float32)
        return (*out, handle)

    @staticmethod
    def backward(ctx, g_xhat, g_mu, g_lv, g_z, g_pre, g_handle):
        model = _graph_model(ctx)
        if model._last["train"] and not ctx.needs_input_grad[0]:
            model._run_backward(g_xhat, g_mu, g_lv, g_z, g_pre, g_handle)     # the training path: vae_backward, as always
            return None, None, None, None, None
        dx, _ = model._run_backward_ex(g_xhat, g_mu, g_lv, g_z, g_pre, g_handle, want_dx=ctx.needs_input_grad[0])
        return dx, None, None, None, None     # (the reconstruction target is data: no gradient flows to it)


def _graph_model(ctx):
    """The model of an autograd node of this module, if the context still holds the activations of that node's forward."""
    model = ctx.model_ref()
    if model is None:
        raise RuntimeError("the VanillaVAE of this graph no longer exists")
    if model._fwd_count != ctx.generation:
        raise RuntimeError("backward through a forward that is no longer the model's last one: the context keeps the "
                           "activations of one forward only (run backward before the next forward, or one model per graph)")
    return model


class _VAEEncode(torch.autograd.Function):
    """VanillaVAE.encode (models.py:107-145): the encoder and fc heads only (vae_encode / vae_backward_ex)."""

    @staticmethod
    def forward(ctx, x, anchor, model):
        ctx.set_materialize_grads(False)
        ctx.model_ref = weakref.ref(model)
        out = model._run_encode(x, train=model.training)
        ctx.generation = model._fwd_count
        return out

    @staticmethod
    def backward(ctx, g_mu, g_lv, g_pre):
        model = _graph_model(ctx)
        dx, _ = model._run_backward_ex(None, g_mu, g_lv, None, g_pre, None, want_dx=ctx.needs_input_grad[0])
        return dx, None, None


class _VAEDecode(torch.autograd.Function):
    """VanillaVAE.decode (models.py:147-175): decoder_input, decoder and final_layer only (vae_decode / vae_backward_ex)."""

    @staticmethod
    def forward(ctx, z, anchor, model):
        ctx.set_materialize_grads(False)
        ctx.model_ref = weakref.ref(model)
        out = model._run_decode(z, train=model.training)
        ctx.generation = model._fwd_count
        return out

    @staticmethod
    def backward(ctx, g_xhat):
        model = _graph_model(ctx)
        _, dz = model._run_backward_ex(g_xhat, None, None, None, None, None, want_dz=ctx.needs_input_grad[0])
        return dz, None, None


class _FusedELBO(torch.autograd.Function):
    """VanillaVAE.loss (models.py:190-225) of the model's last forward."""

    @staticmethod
    def forward(ctx, handle, model, kld_weight):
        out3 = torch.empty(3, device=handle.device, dtype=torch.float32)
        with torch.cuda.device(handle.device):
            _lib.check(_lib.lib().vae_loss(model._ctx.handle, float(kld_weight), out3.data_ptr(), _stream_ptr(handle.device)), "vae_loss")
        model._bwd_kld_weight = float(kld_weight)
        ctx.mark_non_differentiable(out3)
        return out3[0].clone(), out3

    @staticmethod
    def backward(ctx, g_loss, _g_out3):
        return g_loss, None, None


class _GenericELBO(torch.autograd.Function):
    """VanillaVAE.loss on tensors that are not the model's own last forward."""

    @staticmethod
    def forward(ctx, xhat, target, mu, lv, kld_weight, recon, kl=(_lib.KL_PLAIN, 0.0)):
        kind, param = recon if isinstance(recon, tuple) else (recon, 0.0)   # (VAE_RECON_* kind, its parameter)
        xhat, target, mu, lv = (t.contiguous().float() for t in (xhat, target, mu, lv))
        out3 = torch.empty(3, device=xhat.device, dtype=torch.float32)
        gx, gm, gl = torch.empty_like(xhat), torch.empty_like(mu), torch.empty_like(lv)
        with torch.cuda.device(xhat.device):
            _lib.check(_lib.lib().vae_elbo_generic_w(xhat.data_ptr(), target.data_ptr(), mu.data_ptr(), lv.data_ptr(),
                                                    xhat.numel(), mu.shape[0], mu.shape[1], float(kld_weight), int(kind), float(param),
                                                    int(kl[0]), float(kl[1]), out3.data_ptr(), gx.data_ptr(), gm.data_ptr(),
                                                    gl.data_ptr(), _stream_ptr(xhat.device)), "vae_elbo_generic_w")
        ctx.save_for_backward(gx, gm, gl)
        ctx.mark_non_differentiable(out3)
        return out3[0].clone(), out3

    @staticmethod
    def backward(ctx, g_loss, _g_out3):
        gx, gm, gl = ctx.saved_tensors
        return gx * g_loss, None, gm * g_loss, gl * g_loss, None, None, None


class VanillaVAE(nn.Module):
    name = "VanillaVAE"

    def __init__(
        self,
        in_channels: int,
        embed_dim: int,
        input_dim: int,
        hidden_dims: list[int] = None,
        kld_weight: float = 1.0,
        verbose: bool = False,
        *,
        generalised: bool | None = None,
        compute_dtype: str = "bf16",
        recon_loss: str = "bce",
        max_batch: int | None = None,
        kl_free_bits: float = 0.0,
        kl_capacity: float | None = None,
        tc_weight: float | None = None,
        pos_weight: float | None = None,
        attr_reg: dict | None = None,
        attr_weight: float = 1.0,
        attr_delta: float = 10.0,
        attr_threshold: float = 0.5,
    ):
        super().__init__()
        if in_channels != 1:
            raise NotImplementedError("the MI355X VAE step is built for 1-channel pianoroll input (in_channels=1)")
        self.latent_dim = embed_dim
        self.input_dim = input_dim
        self.in_channels = in_channels
        self.verbose = verbose
        self.kld_weight = kld_weight
        if hidden_dims is None:
            hidden_dims = [32, 64, 128, 256]
        if list(hidden_dims) != [32, 64, 128, 256]:
            raise NotImplementedError("hidden_dims must be the reference default [32, 64, 128, 256]")
        self.hidden_dims = hidden_dims
        if generalised is None:
            generalised = input_dim != 32
        self.generalised = bool(generalised)
        self.img_size = int(input_dim) if self.generalised else 32
        if compute_dtype not in _DTYPES:
            raise ValueError(f"compute_dtype must be one of {sorted(_DTYPES)}")
        self.compute_dtype = compute_dtype
        _recon_setting(recon_loss, pos_weight)
        self.recon_loss = recon_loss
        self.pos_weight = pos_weight
        _kl_objective(kl_free_bits, kl_capacity, tc_weight)
        self.kl_free_bits = kl_free_bits
        self.kl_capacity = kl_capacity
        self.tc_weight = tc_weight
        checked_attr_reg(attr_reg, embed_dim, attr_weight, attr_delta, attr_threshold)
        self.attr_reg = attr_reg
        self.attr_weight = attr_weight
        self.attr_delta = attr_delta
        self.attr_threshold = attr_threshold
        self._attr_loss = None
        s = self.img_size // 16 if self.generalised else 2
        self.last_conv_size = s * s  # models.py:33 hard-wires 4
        self.flattened_size = self.last_conv_size * hidden_dims[-1]
        self._offs, self._sizes, self._total = _lib.param_layout(self.img_size, embed_dim, self.generalised)
        self._bn_offs, self._bn_ch, self._bn_total = _lib.bn_layout()

        # parameter containers, built and initialised in the reference's order (models.py:41-83)
        modules = []
        cin = in_channels
        for h_dim in hidden_dims:
            modules.append(nn.Sequential(nn.Conv2d(cin, h_dim, kernel_size=3, stride=2, padding=1),
                                         nn.BatchNorm2d(h_dim), nn.LeakyReLU()))
            cin = h_dim
        self.encoder = nn.Sequential(*modules)
        self._init_weights(self.encoder, "encoder")
        self.fc_mu = nn.Linear(self.flattened_size, self.latent_dim)
        self.fc_var = nn.Linear(self.flattened_size, self.latent_dim)
        self.decoder_input = nn.Linear(self.latent_dim, self.flattened_size)
        hidden_dims.reverse()  # models.py:60 mutates the caller's list; kept
        modules = []
        for i in range(len(hidden_dims) - 1):
            modules.append(nn.Sequential(
                nn.ConvTranspose2d(hidden_dims[i], hidden_dims[i + 1], kernel_size=3, stride=2, padding=1, output_padding=1),
                nn.BatchNorm2d(hidden_dims[i + 1]), nn.LeakyReLU()))
        self.decoder = nn.Sequential(*modules)
        self._init_weights(self.decoder, "decoder")
        self.final_layer = nn.Sequential(
            nn.ConvTranspose2d(hidden_dims[-1], hidden_dims[-1], kernel_size=3, stride=2, padding=1, output_padding=1),
            nn.BatchNorm2d(hidden_dims[-1]), nn.LeakyReLU(),
            nn.Conv2d(hidden_dims[-1], 1, kernel_size=3, stride=1, padding=1), nn.Sigmoid())
        self._init_weights(self.final_layer, "final layer")

        self._flat = self._gflat = self._gnew = self._bnflat = self._nbt = None
        self._ctx = None
        self._max_batch = max_batch
        self._next_eps = None
        self._last = None
        self._bwd_kld_weight = float(kld_weight)
        self.materialize_pre_latents = True
        self.eps_seed = 0
        self._fwd_count = 0
        self._ll_count = 0      # calls of log_likelihood() that drew their noise on the device (its seeds; see there)

    # -- reference helpers --------------------------------------------------
    def _init_weights(self, module: nn.Sequential, name: str):
        """models.py:227-236: xavier for nn.Linear/nn.Conv2d inside `module`, BN weight 1 / bias 0.
        nn.ConvTranspose2d is not an nn.Conv2d subclass and keeps its default init."""
        for m in module.modules():
            if isinstance(m, nn.Linear) or isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.verbose:
            print(f"{name} layer weight initialization complete")

    def _compute_conv_output_size(self, dim: int, num_layers: int, kernel: int = 3, stride: int = 2, padding: int = 1):
        for _ in range(num_layers):
            dim = (dim - kernel + stride * padding) // stride + 1
        return dim

    # -- flat storage -------------------------------------------------------
    def _named_param_list(self):
        sd = dict(self.named_parameters())
        return [sd[n] for n in _lib.PARAM_NAMES]

    def _param_grad_views(self):
        """(parameters, their slices of the flat gradient buffer), cached: walking named_parameters() and re-slicing on
        every step cost ~0.1 ms of host time, more than the launches of a 32x32 step.  Rebuilt with the flat buffers."""
        cache = self.__dict__.get("_gview_cache")
        if cache is None or cache[0] is not self._gflat:
            params = self._named_param_list()
            views = [self._gflat[self._offs[i]:self._offs[i] + self._sizes[i]].view(p.shape) for i, p in enumerate(params)]
            cache = (self._gflat, params, views)
            self.__dict__["_gview_cache"] = cache
        return cache[1], cache[2]

    def _bn_modules(self):
        return [self.get_submodule(n) for n in _lib.BN_NAMES]

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._rebuild_flat()
        return out

    def _rebuild_flat(self):
        params = self._named_param_list()
        dev = params[0].device
        if dev.type != "cuda":
            self._flat = None
            return
        if any(p.dtype != torch.float32 for p in params):
            raise TypeError("VanillaVAE parameters must stay float32 (master weights); pick compute_dtype instead")
        flat = torch.zeros(self._total, device=dev, dtype=torch.float32)
        for i, p in enumerate(params):
            view = flat[self._offs[i]:self._offs[i] + self._sizes[i]].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p._vae_owner = weakref.ref(self)
            p._vae_index = i
            p.grad = None
        bnflat = torch.zeros(self._bn_total, device=dev, dtype=torch.float32)
        nbt = torch.zeros(_lib.NUM_BN, device=dev, dtype=torch.int64)
        for i, bn in enumerate(self._bn_modules()):
            c, o = self._bn_ch[i], self._bn_offs[i]
            bnflat[o:o + c].copy_(bn.running_mean)
            bnflat[o + c:o + 2 * c].copy_(bn.running_var)
            nbt[i].copy_(bn.num_batches_tracked)
            bn.running_mean = bnflat[o:o + c]
            bn.running_var = bnflat[o + c:o + 2 * c]
            bn.num_batches_tracked = nbt[i]
        self._flat, self._bnflat, self._nbt = flat, bnflat, nbt
        self._gflat = torch.zeros_like(flat)
        self._gnew = torch.zeros_like(flat)
        self._ctx = None
        self._last = None

    def flat_parameters(self) -> Tensor:
        self._require_device()
        return self._flat

    def flat_grads(self) -> Tensor:
        self._require_device()
        return self._gflat

    def group_range(self, prefix: str) -> tuple[int, int]:
        """(offset, length) in the flat buffer of all parameters whose name starts with `prefix`."""
        idx = [i for i, n in enumerate(_lib.PARAM_NAMES) if n.startswith(prefix + ".")]
        if not idx or idx != list(range(idx[0], idx[-1] + 1)):
            raise ValueError(f"{prefix!r} is not a contiguous parameter range")
        start = self._offs[idx[0]]
        return start, self._offs[idx[-1]] + self._sizes[idx[-1]] - start

    def comm_stream(self) -> "torch.cuda.Stream":
        """The context's communication stream, ordered after the work enqueued so far on the current stream; joined
        back at the end of the backward's second half (include/vae_step.h: vae_comm_stream)."""
        import ctypes as C
        out = C.c_void_p()
        with self._device_guard():
            _lib.check(_lib.lib().vae_comm_stream(self._ctx.handle, self._stream(), C.byref(out)), "vae_comm_stream")
        return torch.cuda.ExternalStream(out.value, device=self._flat.device)

    def _require_device(self):
        if self._flat is None:
            raise RuntimeError("VanillaVAE (MI355X) runs only on a HIP device: call model.to('cuda') first; "
                               "there is no CPU path.")

    def _device_guard(self):
        """Every library call runs with the MODEL's device current: vae_create allocates its workspace on the current
        HIP device and kernels launch on the stream passed in, which must belong to the device that owns the tensors."""
        dev = self._flat.device
        if torch.cuda.current_device() == dev.index:
            return _NULL_GUARD          # (the usual case: entering torch.cuda.device costs two HIP calls per library call)
        return torch.cuda.device(dev)

    def _stream(self):
        return _stream_ptr(self._flat.device)

    def _context(self, batch: int) -> _Context:
        need = max(batch, self._max_batch or 0)
        if self._ctx is None or self._ctx.key[2] < batch:
            self._ctx = None
            with self._device_guard():
                self._ctx = _Context(self.img_size, self.latent_dim, need, _DTYPES[self.compute_dtype], self.generalised)
                if getattr(self, "_want_lib_comm", False):
                    self._init_library_comm()
            self._max_batch = need
        self._ctx.set_recon(_recon_setting(self.recon_loss, getattr(self, "pos_weight", None)))
        tcw = getattr(self, "tc_weight", None)
        if self.kl_capacity is not None or self.kl_free_bits != 0.0 or tcw is not None or self._ctx.kl[0] != _lib.KL_PLAIN:
            self._ctx.set_kl(_kl_objective(self.kl_free_bits, self.kl_capacity, tcw))
        return self._ctx

    # -- data parallel: the step library's own RCCL communicator (include/vae_step.h: vae_comm_*) ----------------------
    def _init_library_comm(self):
        """COLLECTIVE over torch.distributed's default group: rank 0 draws the RCCL unique id, the process group carries it
        to the other ranks, every rank creates its communicator.  On failure the model falls back to torch.distributed's
        collectives (and says so once)."""
        import ctypes as C
        import warnings
        import torch.distributed as dist
        L = _lib.lib()
        rank, world = dist.get_rank(), dist.get_world_size()
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        ok = True
        if rank == 0:
            ok = L.vae_comm_unique_id(buf) == 0
        box = [bytes(buf.raw) if ok else None]
        dist.broadcast_object_list(box, src=0)
        if box[0] is None or L.vae_comm_init(self._ctx.handle, rank, world, C.create_string_buffer(box[0], _lib.COMM_ID_BYTES)) != 0:
            warnings.warn("torch_vae_amd: RCCL communicator of the step library unavailable ("
                          + L.vae_last_error().decode() + "); gradients go through torch.distributed instead")
            self._want_lib_comm = False

    def library_comm_world(self) -> int:
        """World size of the context's own RCCL communicator (0: none, gradients go through torch.distributed)."""
        if self._ctx is None or not self._ctx.handle:
            return 0
        return int(_lib.lib().vae_comm_world(self._ctx.handle))

    def allreduce_ranges(self, prefixes, on_comm_stream: bool = False, average: bool = True):
        """Mean (or sum) all-reduce of the flat-gradient ranges of the named parameter groups through the library's
        communicator, as ONE RCCL group, on the current stream or on the context's communication stream (which is ordered
        after everything enqueued so far and joined back by the second half of the backward)."""
        import ctypes as C
        L = _lib.lib()
        rngs = [self.group_range(p) for p in prefixes]
        offs = (C.c_int64 * len(rngs))(*[r[0] for r in rngs])
        sizes = (C.c_int64 * len(rngs))(*[r[1] for r in rngs])
        with self._device_guard():
            st = self._stream()
            if on_comm_stream:
                out = C.c_void_p()
                _lib.check(L.vae_comm_stream(self._ctx.handle, st, C.byref(out)), "vae_comm_stream")
                st = out.value
            _lib.check(L.vae_allreduce_grads(self._ctx.handle, self._gflat.data_ptr(), len(rngs), offs, sizes, int(average), st),
                       "vae_allreduce_grads")

    # -- kernels ------------------------------------------------------------
    def set_next_eps(self, eps: Tensor | None):
        """Supply the N(0,1) draw models.py:182 takes from torch.randn_like (parity runs)."""
        self._next_eps = eps

    def _check_input(self, x: Tensor):
        self._require_device()
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.img_size or x.shape[3] != self.img_size:
            # the reference fails inside ATen with a shape RuntimeError; same exception type
            raise RuntimeError(f"expected input [B,1,{self.img_size},{self.img_size}], got {tuple(x.shape)}")
        if x.device != self._flat.device:
            raise RuntimeError("input and model are on different devices")

    def _checked_target(self, target: Tensor | None, x: Tensor):
        """The reconstruction target of a step whose input is x (denoising: x is the corruption, target the clean roll): checked
        like x, and as the float32 contiguous tensor the library reads.  None stays None - the target is then x itself."""
        if target is None:
            return None
        self._check_input(target)
        if target.shape != x.shape or target.device != x.device:
            raise RuntimeError(f"target must have the input's shape and device: {tuple(target.shape)} on {target.device} against "
                               f"{tuple(x.shape)} on {x.device}")
        return target.detach().contiguous().float()

    def _set_recon_target(self, ctx, target: Tensor | None):
        """vae_set_recon_target for the forward that follows (one-shot in the library).  Inside the device guard.  Nothing without one."""
        if target is not None:
            _lib.check(_lib.lib().vae_set_recon_target(ctx.handle, target.data_ptr()), "vae_set_recon_target")

    def _noise_seed(self, counter: int) -> int:
        """Seed of the device-side noise (used when no eps is given): distinct per call AND per rank, so data-parallel
        replicas draw independent noise like the reference's per-process torch generator (models.py:182)."""
        return (int(self.eps_seed) + counter + _rank() * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF

    def _checked_eps(self, eps: Tensor | None, B: int, dev):
        if eps is None:
            return None
        eps = eps.detach().to(dev, torch.float32).contiguous()
        if eps.shape != (B, self.latent_dim):
            raise RuntimeError(f"eps must be [{B},{self.latent_dim}]")
        return eps

    def _pre_latents(self, ctx, B: int, dev, want: bool) -> Tensor:
        """EncoderOutput.pre_latents of the forward the context holds ([B, 0] when not wanted).  Inside the device guard."""
        if not want:
            return torch.empty(B, 0, device=dev)
        pre = torch.empty(B, self.flattened_size, device=dev)
        _lib.check(_lib.lib().vae_pre_latents(ctx.handle, pre.data_ptr(), self._stream()), "vae_pre_latents")
        return pre

    def _run_forward(self, x: Tensor, eps: Tensor | None, train: bool, want_pre: bool | None = None, defer_output: bool = False,
                     target: Tensor | None = None):
        self._check_input(x)
        target = self._checked_target(target, x)
        x = x.detach().contiguous().float()
        B, L, dev = x.shape[0], self.latent_dim, x.device
        ctx = self._context(B)
        xhat = torch.empty_like(x)
        mu = torch.empty(B, L, device=dev)
        lv = torch.empty(B, L, device=dev)
        z = torch.empty(B, L, device=dev)
        eps = self._checked_eps(eps, B, dev)
        self._fwd_count += 1
        seed = self._noise_seed(self._fwd_count)
        with self._device_guard():
            self._set_recon_target(ctx, target)
            _lib.check(_lib.lib().vae_forward(
                ctx.handle, x.data_ptr(), B, self._flat.data_ptr(), self._bnflat.data_ptr(), self._nbt.data_ptr(),
                _lib.ptr(eps), seed, (2 if (train and defer_output) else int(train)), xhat.data_ptr(), mu.data_ptr(),
                lv.data_ptr(), z.data_ptr(), self._stream()), "vae_forward")
            pre = self._pre_latents(ctx, B, dev, self.materialize_pre_latents if want_pre is None else want_pre)
        # (target: kept alive as long as x - a deferred output conv reads it in the backward)
        self._last = dict(kind="forward", x=x, xhat=xhat, mu=mu, lv=lv, z=z, train=train, B=B, target=target)
        return xhat, mu, lv, z, pre

    def _run_encode(self, x: Tensor, train: bool):
        """vae_encode: the encoder half of _run_forward (same launches: mu / log_var bit-identical).  Returns mu, log_var, pre."""
        self._check_input(x)
        x = x.detach().contiguous().float()
        B, L, dev = x.shape[0], self.latent_dim, x.device
        ctx = self._context(B)
        mu, lv, z = (torch.empty(B, L, device=dev) for _ in range(3))
        self._fwd_count += 1
        seed = self._noise_seed(self._fwd_count)
        with self._device_guard():
            _lib.check(_lib.lib().vae_encode(
                ctx.handle, x.data_ptr(), B, self._flat.data_ptr(), self._bnflat.data_ptr(), self._nbt.data_ptr(), 0, seed,
                int(train), mu.data_ptr(), lv.data_ptr(), z.data_ptr(), self._stream()), "vae_encode")
            pre = self._pre_latents(ctx, B, dev, self.materialize_pre_latents)
        self._last = dict(kind="encode", x=x, mu=mu, lv=lv, z=z, train=train, B=B)
        return mu, lv, pre

    def _run_decode(self, z: Tensor, train: bool):
        """vae_decode: z [B, latent_dim] -> xhat [B,1,H,W]."""
        self._require_device()
        z = z.detach().to(self._flat.device, torch.float32).contiguous()
        if z.dim() != 2 or z.shape[1] != self.latent_dim:
            raise RuntimeError(f"expected z [B,{self.latent_dim}], got {tuple(z.shape)}")
        B = z.shape[0]
        ctx = self._context(B)
        xhat = torch.empty(B, 1, self.img_size, self.img_size, device=z.device, dtype=torch.float32)
        self._fwd_count += 1
        with self._device_guard():
            _lib.check(_lib.lib().vae_decode(ctx.handle, z.data_ptr(), B, self._flat.data_ptr(), self._bnflat.data_ptr(),
                                            self._nbt.data_ptr(), int(train), xhat.data_ptr(), self._stream()), "vae_decode")
        self._last = dict(kind="decode", z=z, xhat=xhat, train=train, B=B)   # (z and xhat stay alive for the backward)
        return xhat

    def _needs_graph(self, inp: Tensor) -> bool:
        """Record an autograd node for a call on `inp`: grad mode on and something to differentiate (the reference's modules
        build a graph whenever a parameter requires grad)."""
        if not torch.is_grad_enabled():
            return False
        return inp.requires_grad or any(p.requires_grad for p in self._named_param_list())

    def _run_backward(self, g_xhat, g_mu, g_lv, g_z, g_pre, g_handle, into_gflat: bool = False):
        last = self._last
        if last is None or not last["train"] or last["kind"] != "forward":
            raise RuntimeError("backward needs a train-mode forward of this model")
        c = lambda t: None if t is None else t.contiguous().float()  # noqa: E731
        g_xhat, g_mu, g_lv, g_z, g_pre, g_handle = map(c, (g_xhat, g_mu, g_lv, g_z, g_pre, g_handle))
        target = self._gflat if into_gflat else self._gnew
        with self._device_guard():
            _lib.check(_lib.lib().vae_backward(
                self._ctx.handle, last["x"].data_ptr(), self._flat.data_ptr(), target.data_ptr(), _lib.ptr(g_xhat),
                _lib.ptr(g_handle), _lib.ptr(g_mu), _lib.ptr(g_lv), _lib.ptr(g_z), _lib.ptr(g_pre),
                float(self._bwd_kld_weight), int(g_handle is not None), self._stream()), "vae_backward")
        if not into_gflat:
            self._commit_grads()

    # parameters a decode-only / encode-only backward writes (indices into _lib.PARAM_NAMES)
    _DECODER_PARAMS = frozenset(i for i, n in enumerate(_lib.PARAM_NAMES) if n.split(".")[0] in ("decoder_input", "decoder", "final_layer"))
    _ENCODER_PARAMS = frozenset(range(len(_lib.PARAM_NAMES))) - _DECODER_PARAMS

    def _run_backward_ex(self, g_xhat, g_mu, g_lv, g_z, g_pre, g_handle, want_dx: bool = False, want_dz: bool = False):
        """vae_backward_ex: the backward of whichever forward ran last (forward / encode / decode, train or eval mode).
        Commits the parameter gradients that forward has and returns (dx or None, dz or None).

        f16 storage: the library scales the backward's gradients by a power of two chosen for the mean-reduced ELBO
        (vae_ctx.h: set_grad_scale).  An arbitrary upstream gradient (a sum-reduced loss, a masked loss on decode(z)) can be
        far larger, and its scaled products would overflow f16.  So the upstream gradients are first multiplied by a second
        power of two s, formed on the device (no host sync) from their largest magnitude relative to that of the standard ELBO
        (1/(B*H*W) on the reconstruction, 1/B on the latent), and every result is multiplied by 1/s afterwards.  Powers of two
        are exact: the f32 arithmetic is unchanged wherever nothing overflows or underflows."""
        last = self._last
        if last is None:
            raise RuntimeError("backward needs a forward of this model")
        kind = last["kind"]
        c = lambda t: None if t is None else t.contiguous().float()  # noqa: E731
        g_xhat, g_mu, g_lv, g_z, g_pre, g_handle = map(c, (g_xhat, g_mu, g_lv, g_z, g_pre, g_handle))
        B = last["B"]
        inv_s = None
        if self.compute_dtype in ("f16", "fp16", "float16", "half"):
            npix = float(B * self.img_size * self.img_size)
            mags = [g.abs().amax() * f for g, f in ((g_xhat, npix), (g_mu, B), (g_lv, B), (g_z, B), (g_pre, B), (g_handle, 1.0))
                    if g is not None and g.numel()]
            if mags:
                m = torch.stack(mags).amax()
                e = torch.where(torch.isfinite(m) & (m > 0), torch.ceil(torch.log2(m)), torch.zeros_like(m)).clamp(-100, 100)
                s, inv_s = torch.exp2(-e), torch.exp2(e)
                g_xhat, g_mu, g_lv, g_z, g_pre, g_handle = (None if g is None else g * s
                                                            for g in (g_xhat, g_mu, g_lv, g_z, g_pre, g_handle))
        dev = self._flat.device
        dx = torch.empty(B, 1, self.img_size, self.img_size, device=dev) if want_dx and kind != "decode" else None
        dz = torch.empty(B, self.latent_dim, device=dev) if want_dz and kind == "decode" else None
        with self._device_guard():
            _lib.check(_lib.lib().vae_backward_ex(
                self._ctx.handle, _lib.ptr(last.get("x")), self._flat.data_ptr(), self._gnew.data_ptr(), _lib.ptr(g_xhat),
                _lib.ptr(g_handle), _lib.ptr(g_mu), _lib.ptr(g_lv), _lib.ptr(g_z), _lib.ptr(g_pre),
                float(self._bwd_kld_weight), int(g_handle is not None), _lib.ptr(dx), _lib.ptr(dz), self._stream()), "vae_backward_ex")
        which = self._DECODER_PARAMS if kind == "decode" else self._ENCODER_PARAMS if kind == "encode" else None
        if inv_s is not None:
            for i in (range(len(self._offs)) if which is None else which):
                self._gnew[self._offs[i]:self._offs[i] + self._sizes[i]].mul_(inv_s)
            for t in (dx, dz):
                if t is not None:
                    t.mul_(inv_s)
        self._commit_grads(which)
        return dx, dz

    def _commit_grads(self, which=None):
        """param.grad semantics of autograd: assign where grad is None, accumulate otherwise.  ``which``: indices of the
        parameters the backward produced (None: all)."""
        params = self._named_param_list()
        runs, cur = [], None
        for i, p in enumerate(params):
            if not p.requires_grad or (which is not None and i not in which):
                kind = "skip"
            elif p.grad is None:
                kind = "assign"
            elif p.grad.data_ptr() == self._gflat.data_ptr() + 4 * self._offs[i]:
                kind = "add"
            else:
                kind = "foreign"
            if kind == "foreign":
                p.grad.add_(self._gnew[self._offs[i]:self._offs[i] + self._sizes[i]].view(p.shape))
                cur = None
                continue
            if cur is not None and cur[0] == kind:
                cur[2] = self._offs[i] + self._sizes[i]
            else:
                cur = [kind, self._offs[i], self._offs[i] + self._sizes[i]]
                runs.append(cur)
        for kind, a, b in runs:
            if kind == "assign":
                self._gflat[a:b].copy_(self._gnew[a:b])
            elif kind == "add":
                self._gflat[a:b].add_(self._gnew[a:b])
        for i, p in enumerate(params):
            if p.requires_grad and p.grad is None and (which is None or i in which):
                p.grad = self._gflat[self._offs[i]:self._offs[i] + self._sizes[i]].view(p.shape)

    def bind_flat_grads(self):
        """Point every param.grad at its slice of the flat gradient buffer (fused step path)."""
        params, views = self._param_grad_views()
        for p, g in zip(params, views):
            if p.grad is not g and p.requires_grad:
                if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                    p.grad = g

    # -- reference API ------------------------------------------------------
    def encode(self, x: Tensor) -> EncoderOutput:
        """models.py:107-145: the encoder and the fc heads only (vae_encode; no decoder launch).  mu / log_var are
        bit-identical to forward()'s.  Differentiable w.r.t. the encoder / fc parameters and x, in train and eval mode."""
        self._require_device()
        if self._needs_graph(x):
            mu, lv, pre = _VAEEncode.apply(x, self._anchor_tensor(x.device), self)
        else:
            mu, lv, pre = self._run_encode(x, train=self.training)
        return EncoderOutput(mu=mu, log_var=lv, pre_latents=pre)

    def decode(self, z: Tensor) -> Tensor:
        """models.py:147-175: latent [B, latent_dim] -> reconstruction [B,1,H,W] (vae_decode: the decoder kernels only).
        Differentiable w.r.t. z and the decoder_input / decoder / final_layer parameters, in train mode (batch statistics,
        running statistics updated once) and eval mode (running statistics), when z requires grad; a z that does not
        decodes for inference, as sample() does (no graph, whatever the parameters' requires_grad)."""
        self._require_device()
        if torch.is_grad_enabled() and z.requires_grad:
            return _VAEDecode.apply(z, self._anchor_tensor(self._flat.device), self)
        return self._run_decode(z, train=self.training)

    def log_likelihood(self, x: Tensor, num_samples: int = 64, *, eps: Tensor | None = None, chunk: int | None = None,
                       seed: int | None = None) -> LikelihoodOutput:
        """Importance-weighted estimate of log p(x) (Burda et al., IWAE with K = num_samples draws from q(z|x)) and the
        per-sample ELBO, in nats, through the HIP kernels (include/vae_step.h: vae_log_likelihood):
            log_weights[k, b]  = log p(x_b|z_kb) + log p(z_kb) - log q(z_kb|x_b),   z_kb ~ q(z|x_b)
            log_likelihood[b]  = logsumexp_k log_weights[k, b] - log K
            elbo[b]            = mean_k log p(x_b|z_kb) - KL(q(z|x_b) || N(0, I))
        p(x|z) follows ``recon_loss``: "bce" - Bernoulli (normalised only for 0/1 targets), "mse" - Gaussian with variance
        1/2, whose negative log-likelihood is the summed squared error plus (H*W/2) log(pi).  ``pos_weight`` is ignored: a
        weighted BCE is not a likelihood, the estimate stays the unweighted Bernoulli.

        Always in eval semantics (BatchNorm on the running statistics, which are read and never written), whatever
        ``self.training`` is; not differentiable.  The training noise seeds are untouched.  ``eps`` [K, B, latent_dim]
        replaces the draws; by default they come from the device generator with ``seed`` (None: derived from ``eps_seed``
        and a call counter of this method).  ``chunk`` draws of the whole batch are decoded per pass (default: as many as
        the model's max_batch allows)."""
        K = int(num_samples)
        if K < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        B, L = (x.shape[0] if x.dim() else 0), self.latent_dim
        if eps is not None and tuple(eps.shape) != (K, B, L):
            raise ValueError(f"eps must be [{K},{B},{L}] (num_samples, batch, latent_dim), got {tuple(eps.shape)}")
        self._check_input(x)
        x = x.detach().contiguous().float()
        dev = x.device
        ctx = self._context(B)
        if chunk is None:
            chunk = max(1, min(K, ctx.key[2] // B))
        else:
            chunk = min(int(chunk), K)
            if chunk * B > ctx.key[2]:
                ctx = self._context(chunk * B)
        if eps is not None:
            eps = eps.detach().to(dev, torch.float32).contiguous()
        if seed is None:
            self._ll_count = getattr(self, "_ll_count", 0) + 1
            seed = self._noise_seed(self._ll_count)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        log_w = torch.empty(K, B, device=dev, dtype=torch.float64)
        ll = torch.empty(B, device=dev, dtype=torch.float64)
        elbo = torch.empty(B, device=dev, dtype=torch.float64)
        with self._device_guard():
            _lib.check(_lib.lib().vae_log_likelihood(
                ctx.handle, x.data_ptr(), B, self._flat.data_ptr(), self._bnflat.data_ptr(), K, chunk, _lib.ptr(eps), seed,
                log_w.data_ptr(), ll.data_ptr(), elbo.data_ptr(), self._stream()), "vae_log_likelihood")
        self._last = None
        return LikelihoodOutput(log_likelihood=ll, elbo=elbo, log_weights=log_w)

    def reparameterize(self, mu: Tensor, log_var: Tensor) -> Tensor:
        """models.py:177-183 (plumbing-level torch ops; the hot path fuses this into the latent kernel)."""
        std = torch.exp(0.5 * log_var)
        return torch.randn_like(std) * std + mu

    def forward(self, x: Tensor, target: Tensor | None = None) -> ModelOutput:
        """models.py:185-188.  ``target`` (default: x itself): what the reconstruction term is taken against - the clean roll of a
        denoising step whose input x is its corruption (denoise.corrupt_rolls).  It becomes ``ModelOutput["input"]``, so loss() on
        the output scores the reconstruction against it, on the same HIP path as without one."""
        self._require_device()
        eps, self._next_eps = self._next_eps, None
        if eps is None:
            # torch.randn_like(std) of models.py:182: drawn from torch's device generator
            eps = torch.randn(x.shape[0], self.latent_dim, device=x.device, dtype=torch.float32)
        if torch.is_grad_enabled() and (self.training or self._needs_graph(x)):
            anchor = self._anchor_tensor(x.device)
            xhat, mu, lv, z, pre, handle = _VAEForward.apply(x, anchor, self, eps, target)
        else:
            xhat, mu, lv, z, pre = self._run_forward(x, eps, train=self.training, target=target)
            handle = None
        self._last.update(handle=handle, out_ref=xhat, mu=mu, lv=lv, z=z, target_ref=target)
        encoding = EncoderOutput(mu=mu, log_var=lv, pre_latents=pre)
        return ModelOutput(output=xhat, input=x if target is None else target, encoded=encoding, latents=z)

    def _anchor_tensor(self, dev):
        a = getattr(self, "_anchor", None)
        if a is None or a.device != dev:
            a = torch.zeros((), device=dev, requires_grad=True)
            self._anchor = a
        return a

    def loss(self, output: ModelOutput):
        """models.py:190-225."""
        last = self._last
        # (a forward with a target put the target into output["input"]: the library scored the reconstruction against it)
        scored = None if last is None else (last.get("target_ref") if last.get("target_ref") is not None else last.get("x"))
        own = (last is not None and output["output"] is last.get("out_ref") and last.get("handle") is not None
               and output["encoded"]["mu"] is last["mu"] and (output["input"] is scored or
                                                            output["input"].data_ptr() == scored.data_ptr()))
        if own:
            loss, out3 = _FusedELBO.apply(last["handle"], self, self.kld_weight)
        elif last is not None and output["output"] is last.get("out_ref") and last.get("handle") is None:
            out3 = torch.empty(3, device=last["xhat"].device)
            with self._device_guard():
                _lib.check(_lib.lib().vae_loss(self._ctx.handle, float(self.kld_weight), out3.data_ptr(), self._stream()), "vae_loss")
            loss = out3[0].clone()
        else:
            if getattr(self, "tc_weight", None) is not None:
                raise ValueError("loss() on tensors that are not this model's last forward cannot take tc_weight: the total correlation "
                                 "is evaluated at z = mu + eps * exp(log_var / 2) and only the model's own forward holds its eps "
                                 "(pass the forward's own output, or use vae_total_correlation with the eps)")
            loss, out3 = _GenericELBO.apply(output["output"], output["input"], output["encoded"]["mu"],
                                            output["encoded"]["log_var"], self.kld_weight,
                                            _recon_setting(self.recon_loss, getattr(self, "pos_weight", None)),
                                            _kl_objective(self.kl_free_bits, self.kl_capacity))
        if getattr(self, "attr_reg", None) is not None:     # (off: the output is not looked at any further, as before)
            z = output.get("latents") if hasattr(output, "get") else None
            if z is None:
                raise ValueError("loss() with attr_reg set needs output['latents']: the regulariser is a function of z")
            attr = self._attr_setting(z.shape[0])
            counters = roll_attributes(output["input"].detach().float(), attr[4])
            loss = loss + AttributeTerm.apply(z if z.dtype == torch.float32 else z.float(), counters, self, attr)
        return LossOutput(loss=loss, reconstruction_loss=out3[1].detach(), kld_loss=out3[2].detach())

    def kl_per_dim(self) -> Tensor:
        """Batch-mean KL of every latent dimension (nats) for the model's last forward / fused step / encode: a float64
        [latent_dim] device tensor, reduced in a fixed order, with no host synchronisation - a per-step collapse monitor that can
        stay on the device.  With kl_free_bits / kl_capacity set it is the very reduction the step's mask was decided on.  Data
        parallel: the replica's own batch."""
        self._require_device()
        if self._last is None or self._last["kind"] == "decode" or self._ctx is None:
            raise RuntimeError("kl_per_dim needs a forward, fused step or encode of this model")
        out = torch.empty(self.latent_dim, device=self._flat.device, dtype=torch.float64)
        with self._device_guard():
            _lib.check(_lib.lib().vae_kl_per_dim(self._ctx.handle, out.data_ptr(), self._stream()), "vae_kl_per_dim")
        return out

    def total_correlation(self) -> Tensor:
        """Total correlation (nats) of the model's last forward / fused step / encode over the in-batch mixture, at that forward's own
        z: a float64 device scalar with no host synchronisation.  With tc_weight set it is the very value the step's loss used;
        otherwise it is computed on demand by the same kernels.  Data parallel: the replica's own batch."""
        self._require_device()
        if self._last is None or self._last["kind"] == "decode" or self._ctx is None:
            raise RuntimeError("total_correlation needs a forward, fused step or encode of this model")
        out = torch.empty((), device=self._flat.device, dtype=torch.float64)
        with self._device_guard():
            _lib.check(_lib.lib().vae_last_total_correlation(self._ctx.handle, out.data_ptr(), self._stream()), "vae_last_total_correlation")
        return out

    def sample(self, num_samples: int, current_device: int, *, prior=None, temperature: float = 1.0, seed: int = 0, **kwargs) -> Tensor:
        """models.py:250-263: z ~ N(0, I) on the host generator, moved to the device, decoded.  With ``prior`` (a
        ``mixture.LatentMixture`` on the model's device) z = prior.sample(num_samples, temperature=..., seed=...) instead;
        ``temperature`` and ``seed`` are read only then."""
        if prior is not None:
            z = prior.sample(int(num_samples), temperature=temperature, seed=seed)
            with torch.no_grad():
                return self.decode(z)
        z = torch.randn(num_samples, self.latent_dim)
        z = z.to(current_device)
        with torch.no_grad():
            return self.decode(z)

    def sample_notes(self, num_samples: int, *, temperature: float = 1.0, seed: int | None = None, return_rolls: bool = False,
                     prior=None, **extract_kwargs):
        """Generated music as notes: z = temperature * N(0, I) from a ``torch.Generator`` on the model's device (seeded with
        ``seed`` when given), decoded with running statistics (eval mode, whatever mode the model is in; it is left in that
        mode and nothing of it changes), then ``generation.extract_notes(rolls, **extract_kwargs)``.  Returns the NoteEvents,
        with the decoded ``rolls`` [num_samples,1,H,W] added under that key when ``return_rolls``.  With ``prior`` (a
        ``mixture.LatentMixture`` fitted to the encodings) z = prior.sample(num_samples, temperature=..., seed=...) instead
        (``seed`` None: one drawn from torch's host generator)."""
        from .generation import extract_notes
        self._require_device()
        dev = self._flat.device
        if prior is not None:
            z = prior.sample(int(num_samples), temperature=temperature,
                             seed=int(torch.randint(0, 2 ** 62, (1,))) if seed is None else int(seed))
        else:
            g = torch.Generator(device=dev)
            if seed is None:
                g.seed()
            else:
                g.manual_seed(int(seed))
            z = float(temperature) * torch.randn(int(num_samples), self.latent_dim, generator=g, device=dev, dtype=torch.float32)
        with torch.no_grad():
            rolls = self._run_decode(z, train=False)
        out = extract_notes(rolls, **extract_kwargs)
        if return_rolls:
            out["rolls"] = rolls
        return out

    def interpolate(self, x_a: Tensor, x_b: Tensor, steps: int, mode: str = "slerp"):
        """Paths between pairs of rolls in latent space: both batches [pairs,1,H,W] are encoded with running statistics (eval
        mode, the model untouched), their posterior means interpolated over ``steps`` points (``generation.interpolate_latents``:
        "slerp" spherical, falling back to linear where the angle is below 1e-6, or "lerp"; plain torch) and every point decoded.
        Returns ``(rolls [pairs, steps, 1, H, W], z [pairs, steps, L])``."""
        from .generation import interpolate_latents
        self._require_device()
        if x_a.shape != x_b.shape:
            raise ValueError(f"x_a and x_b must have the same shape, got {tuple(x_a.shape)} and {tuple(x_b.shape)}")
        with torch.no_grad():
            mu_a = self._run_encode(x_a, train=False)[0]
            mu_b = self._run_encode(x_b, train=False)[0]
            z = interpolate_latents(mu_a.float(), mu_b.float(), steps, mode).contiguous()
            pairs, nsteps, L = z.shape
            rolls = self._run_decode(z.view(pairs * nsteps, L), train=False)
        return rolls.view(pairs, nsteps, *rolls.shape[1:]), z

    def generate(self, x: Tensor, **kwargs) -> Tensor:
        """models.py:265-272."""
        return self.forward(x)["output"]

    # -- fused step (no autograd): forward, ELBO, backward in one call chain --
    def fused_forward_backward(self, x: Tensor, eps: Tensor | None = None, use_device_eps: bool = True,
                               on_decoder_grads=None, target: Tensor | None = None):
        """forward -> loss -> backward (train.py:634-650) with gradients written straight into the
        flat gradient buffer.  Returns a 3-element device tensor {loss, reconstruction, kld_loss}.
        ``on_decoder_grads`` (data parallel): called between the two halves of the backward, when every
        decoder / final_layer gradient is complete in stream order - the caller starts that bucket's
        all-reduce there so it overlaps the encoder half.  ``target``: the reconstruction target where it is not x (forward())."""
        self._require_device()
        if eps is None and not use_device_eps:
            eps = torch.randn(x.shape[0], self.latent_dim, device=x.device, dtype=torch.float32)
        # train = 2: the library may leave the output conv / sigmoid / BCE to the backward (one kernel for the layer's
        # forward and backward): xhat and the ELBO scalars are then written by the backward call below
        attr = self._attr_setting(x.shape[0])    # (None: not one launch or byte below differs from the step without the option)
        xhat, mu, lv, z, _ = self._run_forward(x, eps, train=True, want_pre=False, defer_output=True, target=target)
        g_z = 0
        if attr is not None:
            # the regulariser of this forward's own z, in line on the caller's stream: two small launches whose gradient the
            # backward's latent kernel needs (csrc/edge_kernels.cuh: LatentBwdArgs::gz)
            ids, dims, aw, delta, th = attr
            # (the attribute belongs to the phrase, not to its corruption: counted on the target where there is one)
            scored = self._last["x"] if self._last["target"] is None else self._last["target"]
            self._attr_loss, g = attribute_regularizer(z, roll_attributes(scored, th), ids, dims, delta, aw)
            g_z = g.data_ptr()
        out3 = torch.empty(3, device=x.device, dtype=torch.float32)
        # the ELBO scalars are only read after the step: finalised beside the backward (joined by it), not in front of it
        with self._device_guard():
            _lib.check(_lib.lib().vae_loss_deferred(self._ctx.handle, float(self.kld_weight), out3.data_ptr(), self._stream()), "vae_loss_deferred")
        self._bwd_kld_weight = float(self.kld_weight)
        last = self._last
        for part in ((0,) if on_decoder_grads is None else (1, 2)):
            with self._device_guard():
                _lib.check(_lib.lib().vae_backward_part(
                    self._ctx.handle, last["x"].data_ptr(), self._flat.data_ptr(), self._gflat.data_ptr(), 0, 0, 0, 0, g_z, 0,
                    float(self.kld_weight), 1, part, self._stream()), "vae_backward")
            if part == 1:
                self.bind_flat_grads()
                on_decoder_grads()
        self.bind_flat_grads()
        if attr is not None:
            out3[0].add_(self._attr_loss[0], alpha=attr[2])    # (behind the backward, which joins the deferred ELBO scalars)
        return out3, xhat

    # -- attribute regularisation (include/vae_attributes.h) ---------------------------------------------------------
    def _attr_setting(self, batch: int):
        """None with attr_reg off, else (attribute numbers, dimensions, weight, delta, threshold); ValueError on a bad value."""
        reg = getattr(self, "attr_reg", None)
        if reg is None:
            return None
        return checked_attr_reg(reg, self.latent_dim, getattr(self, "attr_weight", 1.0), getattr(self, "attr_delta", 10.0),
                                getattr(self, "attr_threshold", 0.5), batch)

    def attribute_loss(self) -> Tensor:
        """The attribute regulariser of the model's last step with ``attr_reg`` set (fused_forward_backward, fused_step or
        loss()): a float64 device tensor ``[1 + pairs]`` - the unweighted sum, then L_r of every pair in ``attr_reg``'s order - with
        no host synchronisation."""
        self._require_device()
        if getattr(self, "_attr_loss", None) is None:
            raise RuntimeError("attribute_loss needs a step or loss() of this model with attr_reg set")
        return self._attr_loss


    # -- the whole training step as ONE library call ------------------------------------------------------------
    def fused_train_step(self, optimizer, x: Tensor, eps: Tensor | None = None, use_device_eps: bool = True, exchange: int = 0,
                         target: Tensor | None = None):
        """forward -> ELBO -> backward -> [gradient exchange] -> AdamW (train.py:634-656) enqueued by ONE call into the library
        (include/vae_step.h: vae_train_step_fused) instead of five, with no per-step tensor allocation: the outputs live in
        buffers owned by the model for the batch size, valid until the next fused step of this model.  ``exchange``: 0 none,
        1 one RCCL group between backward and AdamW, 2 bucketed (decoder bucket under the encoder backward, each group's AdamW
        behind its own bucket) - both need the library communicator.  ``target``: the reconstruction target where it is not x
        (forward()).  Returns (out3, xhat)."""
        import ctypes as C
        self._check_input(x)
        target = self._checked_target(target, x)
        if not x.is_contiguous() or x.dtype != torch.float32:
            x = x.detach().contiguous().float()
        B, L, dev = x.shape[0], self.latent_dim, x.device
        ctx = self._context(B)
        if eps is None and not use_device_eps:
            eps = torch.randn(B, L, device=dev, dtype=torch.float32)
        eps = self._checked_eps(eps, B, dev)
        bufs = self.__dict__.get("_step_bufs")
        if bufs is None or bufs[0] != (B, dev):
            bufs = ((B, dev), torch.empty(B, 1, self.img_size, self.img_size, device=dev), torch.empty(B, L, device=dev),
                    torch.empty(B, L, device=dev), torch.empty(B, L, device=dev), torch.empty(3, device=dev))
            self.__dict__["_step_bufs"] = bufs
        _, xhat, mu, lv, z, out3 = bufs
        self._fwd_count += 1
        seed = self._noise_seed(self._fwd_count)
        n, offs, sizes, lrs, b1s, beta2, adam_eps, wd = optimizer._step_args()
        clip = optimizer._clip_args()   # (max_grad_norm / skip_nonfinite: norm, decision and step count on the device)
        self._bwd_kld_weight = float(self.kld_weight)
        with self._device_guard():
            self._set_recon_target(ctx, target)
            if clip is not None:
                _lib.check(_lib.lib().vae_train_step_fused_clipped(
                    ctx.handle, x.data_ptr(), B, self._flat.data_ptr(), self._gflat.data_ptr(), optimizer._m.data_ptr(),
                    optimizer._v.data_ptr(), self._bnflat.data_ptr(), self._nbt.data_ptr(), _lib.ptr(eps), seed, float(self.kld_weight),
                    n, offs, sizes, lrs, b1s, beta2, adam_eps, wd, float(optimizer.grad_scale), *clip, int(exchange),
                    xhat.data_ptr(), mu.data_ptr(), lv.data_ptr(), z.data_ptr(), out3.data_ptr(), self._stream()),
                    "vae_train_step_fused_clipped")
            else:
                _lib.check(_lib.lib().vae_train_step_fused(
                    ctx.handle, x.data_ptr(), B, self._flat.data_ptr(), self._gflat.data_ptr(), optimizer._m.data_ptr(),
                    optimizer._v.data_ptr(), self._bnflat.data_ptr(), self._nbt.data_ptr(), _lib.ptr(eps), seed, float(self.kld_weight),
                    n, offs, sizes, lrs, b1s, beta2, adam_eps, wd, float(optimizer.grad_scale), optimizer._step + 1, int(exchange),
                    xhat.data_ptr(), mu.data_ptr(), lv.data_ptr(), z.data_ptr(), out3.data_ptr(), self._stream()), "vae_train_step_fused")
        optimizer._stepped()
        self._last = dict(kind="forward", x=x, xhat=xhat, mu=mu, lv=lv, z=z, train=True, B=B, target=target)
        params, views = self._param_grad_views()
        if params[0].grad is not views[0] or params[-1].grad is not views[-1]:   # (bound once: the fused path never unbinds them)
            self.bind_flat_grads()
        return out3, xhat


def count_flops_per_sample(img_size: int, latent_dim: int, generalised: bool = True) -> float:
    """Algorithmic FLOPs of one training step per sample: 3 x 2 x forward MACs."""
    h = img_size
    s = h // 16 if generalised else 2
    macs = 9 * 1 * 32 * (h // 2) ** 2
    for ci, co, ho in ((32, 64, h // 4), (64, 128, h // 8), (128, 256, h // 16)):
        macs += 9 * ci * co * ho * ho
    f = 256 * s * s
    macs += 2 * f * latent_dim + f * latent_dim
    for ci, co, hi in ((256, 128, s), (128, 64, 2 * s), (64, 32, 4 * s), (32, 32, 8 * s)):
        macs += 9 * ci * co * hi * hi
    macs += 9 * 32 * (16 * s) ** 2
    return 6.0 * macs


def algorithmic_bytes_per_step(img_size: int, latent_dim: int, batch: int, elem_bytes: int, generalised: bool = True) -> float:
    """B*(2*H^2*e + 5*A*e) + P*(2e + 32)."""
    h = img_size
    s = h // 16 if generalised else 2
    f = 256 * s * s
    a = 32 * (h // 2) ** 2 + 64 * (h // 4) ** 2 + 128 * (h // 8) ** 2 + 256 * (h // 16) ** 2
    a += 3 * latent_dim + f
    a += 128 * (2 * s) ** 2 + 64 * (4 * s) ** 2 + 32 * (8 * s) ** 2 + 32 * (16 * s) ** 2 + (16 * s) ** 2
    _, sizes, _ = _lib.param_layout(img_size if generalised else 32, latent_dim, generalised)
    p = sum(sizes)
    return batch * (2 * h * h * elem_bytes + 5 * a * elem_bytes) + p * (2 * elem_bytes + 32)
