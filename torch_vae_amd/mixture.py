"""Ex-post density estimation in the latent space (Ghosh et al. 2020, "From Variational to Deterministic Autoencoders"): a mixture
of Gaussians fitted to the encodings of the training rolls and sampled from instead of N(0, I), on the HIP kernels
(include/vae_mixture.h).  A VAE trained with a small ``kld_weight``, free bits, a capacity target or ``pos_weight`` has an aggregate
posterior far from the unit Gaussian (``evaluation.latent_statistics`` measures the gap); draws from the fitted mixture decode to
rolls on the data manifold.

    mu, _ = encode_dataset(model, loader)
    mix = LatentMixture.fit(mu, components=10)
    notes = model.sample_notes(64, prior=mix, seed=1)

Everything stays on the device: the EM loop is one library call that enqueues ``iters`` x (factor, E-step, M-step) and nothing
inside it reads back."""
from __future__ import annotations

import torch

from . import _lib
from .data import epoch_indices

_KINDS = {"full": _lib.MIXTURE_FULL, "diag": _lib.MIXTURE_DIAG}
_U64 = 0xFFFFFFFFFFFFFFFF


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _integer(v, name, lo):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return v


def _checked_points(z, what="z"):
    if not isinstance(z, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if z.dim() != 2:
        raise ValueError(f"{what} must be [n, latent_dim], got {tuple(z.shape)}")
    if z.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {z.dtype}")
    if z.device.type != "cuda":
        raise ValueError(f"{what} must be on the GPU: the mixture runs on the HIP kernels only")
    return z.detach().contiguous()


def _checked_shape(K, L, covariance):
    if covariance not in _KINDS:
        raise ValueError(f"covariance must be 'full' or 'diag', got {covariance!r}")
    if not 1 <= K <= _lib.MIXTURE_MAX_COMPONENTS:
        raise ValueError(f"components must be in 1..{_lib.MIXTURE_MAX_COMPONENTS}, got {K}")
    top = _lib.MIXTURE_MAX_DIM_FULL if covariance == "full" else _lib.MIXTURE_MAX_DIM_DIAG
    if not 1 <= L <= top:
        raise ValueError(f"latent_dim must be in 1..{top} for covariance={covariance!r}, got {L}")


class LatentMixture:
    """K Gaussians in L dimensions.  Device tensors, float64 unless noted: ``weights`` [K], ``means`` [K, L], ``covariances`` and
    ``cholesky`` ([K, L, L]; for ``covariance == "diag"`` the variances and their roots, [K, L]), ``log_likelihood_history``
    [iters] (the mean log-likelihood each E-step of the fit saw; empty for a mixture that was not fitted here)."""

    def __init__(self, weights, means, covariances, covariance="full", *, log_likelihood_history=None):
        if covariance not in _KINDS:
            raise ValueError(f"covariance must be 'full' or 'diag', got {covariance!r}")
        for name, t in (("weights", weights), ("means", means), ("covariances", covariances)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device.type != "cuda":
                raise TypeError(f"{name} must be a float64 tensor on the GPU")
        if weights.dim() != 1 or means.dim() != 2 or means.shape[0] != weights.shape[0]:
            raise ValueError(f"weights must be [K] and means [K, L], got {tuple(weights.shape)} and {tuple(means.shape)}")
        K, L = means.shape
        _checked_shape(K, L, covariance)
        want = (K, L, L) if covariance == "full" else (K, L)
        if tuple(covariances.shape) != want:
            raise ValueError(f"covariances must be {list(want)} for covariance={covariance!r}, got {tuple(covariances.shape)}")
        self.covariance, self.components, self.latent_dim = covariance, K, L
        self.weights, self.means, self.covariances = weights.contiguous(), means.contiguous(), covariances.contiguous()
        dev = means.device
        self.cholesky = torch.empty_like(self.covariances)
        self._winv = torch.empty_like(self.covariances)
        self._winv32 = torch.empty(want, device=dev, dtype=torch.float32)
        self._logdet = torch.empty(K, device=dev, dtype=torch.float64)
        self._status = torch.empty(K, device=dev, dtype=torch.int32)
        self.log_likelihood_history = (torch.empty(0, device=dev, dtype=torch.float64) if log_likelihood_history is None
                                       else log_likelihood_history)

    @property
    def _kind(self):
        return _KINDS[self.covariance]

    @property
    def device(self):
        return self.means.device

    def _factor(self):
        dev = self.device
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().vae_mixture_factor(self.covariances.data_ptr(), self.components, self.latent_dim, self._kind,
                                                     self.cholesky.data_ptr(), self._winv.data_ptr(), self._winv32.data_ptr(),
                                                     self._logdet.data_ptr(), self._status.data_ptr(), _stream(dev)), "vae_mixture_factor")

    def _raise_on_failed_pivot(self):
        status = self._status.tolist()                      # the one host read
        bad = [(k, s) for k, s in enumerate(status) if s]
        if bad:
            k, s = bad[0]
            raise RuntimeError(f"component {k} of the mixture has a covariance that is not positive definite (pivot {s} of its "
                               f"Cholesky factorisation is not > 0); raise reg_covar or use fewer components")

    @classmethod
    def fit(cls, z, components=10, *, covariance="full", iters=30, reg_covar=1e-6, seed=0) -> "LatentMixture":
        """EM from ``z`` [n, L] float32 on the device.  Initial means: the points at the first K indices of
        ``data.epoch_indices(n, seed=seed, epoch=0)``; initial covariances: the data covariance + ``reg_covar`` I (one M-step
        with a single component and log_resp = 0); initial weights uniform.  Then ``iters`` EM iterations in one library call.  No
        host read inside the loop; after it one read of the factorisation status raises a RuntimeError naming the component if a
        pivot failed."""
        z = _checked_points(z)
        n, L = z.shape
        K = _integer(components, "components", 1)
        _integer(iters, "iters", 1)
        _checked_shape(K, L, covariance)
        if n < K:
            raise ValueError(f"need at least as many points as components, got n = {n} and components = {K}")
        if n > 1 << 30:
            raise ValueError(f"n must be <= 2^30, got {n}")
        reg = float(reg_covar)
        if not (reg >= 0.0 and reg < float("inf")):
            raise ValueError(f"reg_covar must be finite and >= 0, got {reg_covar!r}")
        dev, kind = z.device, _KINDS[covariance]
        f64 = dict(device=dev, dtype=torch.float64)
        first = epoch_indices(n, seed=int(seed), epoch=0)[:K].to(dev, non_blocking=True)
        means = z.index_select(0, first).double()
        weights = torch.full((K,), 1.0 / K, **f64)
        one_w, one_m = torch.empty(1, **f64), torch.empty(1, L, **f64)
        one_s = torch.empty((1, L, L) if covariance == "full" else (1, L), **f64)
        L_ = _lib.lib()
        with torch.cuda.device(dev):
            _lib.check(L_.vae_mixture_mstep(torch.zeros(n, 1, device=dev).data_ptr(), z.data_ptr(), n, L, 1, kind, reg, one_w.data_ptr(),
                                            one_m.data_ptr(), one_s.data_ptr(), _stream(dev)), "vae_mixture_mstep")
        mix = cls(weights, means, one_s.expand(K, *one_s.shape[1:]).contiguous(), covariance,
                  log_likelihood_history=torch.empty(int(iters), **f64))
        with torch.cuda.device(dev):
            _lib.check(L_.vae_mixture_em(z.data_ptr(), n, L, K, kind, int(iters), reg, mix.weights.data_ptr(), mix.means.data_ptr(),
                                         mix.covariances.data_ptr(), mix.cholesky.data_ptr(), mix._winv.data_ptr(), mix._winv32.data_ptr(),
                                         mix._logdet.data_ptr(), mix._status.data_ptr(), mix.log_likelihood_history.data_ptr(), _stream(dev)),
                       "vae_mixture_em")
        mix._raise_on_failed_pivot()
        return mix

    def _points(self, z):
        z = _checked_points(z)
        if z.shape[1] != self.latent_dim or z.device != self.device:
            raise ValueError(f"z must be [n, {self.latent_dim}] on {self.device}, got {tuple(z.shape)} on {z.device}")
        if z.shape[0] < self.components:
            raise ValueError(f"need at least as many points as components ({self.components}), got {z.shape[0]}")
        return z

    def _log_prob(self, z, want_resp):
        z = self._points(z)
        n, dev = z.shape[0], self.device
        log_prob = torch.empty(n, device=dev, dtype=torch.float64)
        log_resp = torch.empty(n, self.components, device=dev, dtype=torch.float32) if want_resp else None
        mean = torch.empty((), device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().vae_mixture_log_prob(z.data_ptr(), n, self.latent_dim, self.components, self._kind, self.weights.data_ptr(),
                                                       self.means.data_ptr(), self._winv32.data_ptr(), self._logdet.data_ptr(),
                                                       log_prob.data_ptr(), _lib.ptr(log_resp), mean.data_ptr(), _stream(dev)),
                       "vae_mixture_log_prob")
        return log_prob, log_resp

    def log_prob(self, z):
        """log p(z_n) under the mixture, [n] float64 (nats).  Needs at least as many points as components."""
        return self._log_prob(z, False)[0]

    def log_responsibilities(self, z):
        """log p(k | z_n), [n, K] float32."""
        return self._log_prob(z, True)[1]

    def sample(self, n, *, temperature=1.0, seed=0, return_components=False):
        """``n`` latents [n, L] float32: the component from the device counter generator, then mean + temperature * C eps.
        The same ``seed`` gives the same bits.  ``return_components`` adds the int32 component of every draw."""
        n = _integer(n, "n", 0)
        t = float(temperature)
        if not (abs(t) < float("inf")):
            raise ValueError(f"temperature must be finite, got {temperature!r}")
        dev = self.device
        z = torch.empty(n, self.latent_dim, device=dev, dtype=torch.float32)
        comp = torch.empty(n, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            if n:
                _lib.check(_lib.lib().vae_mixture_sample(n, self.latent_dim, self.components, self._kind, self.weights.data_ptr(),
                                                         self.means.data_ptr(), self.cholesky.data_ptr(), t, int(seed) & _U64, 0, 0,
                                                         z.data_ptr(), comp.data_ptr(), _stream(dev)), "vae_mixture_sample")
        return (z, comp) if return_components else z

    def state_dict(self) -> dict:
        """Plain tensors (and the covariance kind as a string): ``torch.save`` works on it."""
        return dict(covariance=self.covariance, weights=self.weights, means=self.means, covariances=self.covariances,
                    log_likelihood_history=self.log_likelihood_history)

    @classmethod
    def from_state_dict(cls, state, device="cuda") -> "LatentMixture":
        """The mixture of a ``state_dict()``; the factors are recomputed on the device (a failed pivot raises)."""
        t = {k: state[k].to(device) for k in ("weights", "means", "covariances", "log_likelihood_history")}
        mix = cls(t["weights"], t["means"], t["covariances"], state["covariance"], log_likelihood_history=t["log_likelihood_history"])
        mix._factor()
        mix._raise_on_failed_pivot()
        return mix


def encode_dataset(model, loader, max_rolls=None):
    """Eval-mode ``model.encode`` over ``loader`` (the model is left in eval mode, as ``evaluate`` leaves it): ``(mu, log_var)``,
    each [rolls, L] float32 on the device, in loader order.  DistributedSampler padding is trimmed as ``evaluate`` trims it;
    ``max_rolls`` stops after that many rolls.  Nothing is read back."""
    if max_rolls is not None:
        _integer(max_rolls, "max_rolls", 1)
    model.eval()
    n_samples = len(loader.dataset) if hasattr(loader, "dataset") else None
    if max_rolls is not None:
        n_samples = max_rolls if n_samples is None else min(n_samples, max_rolls)
    dev = next(model.parameters()).device
    mus, lvs, seen = [], [], 0
    for stimuli, _ in loader:
        stimuli = stimuli.to(dev)
        if n_samples is not None and seen + stimuli.shape[0] > n_samples:
            stimuli = stimuli[: n_samples - seen]
            if stimuli.shape[0] == 0:
                break
        with torch.no_grad():
            enc = model.encode(stimuli)
        mus.append(enc["mu"].detach().clone())
        lvs.append(enc["log_var"].detach().clone())
        seen += stimuli.shape[0]
        if n_samples is not None and seen >= n_samples:
            break
    if not mus:
        raise ValueError("the loader gave no rolls")
    return torch.cat(mus), torch.cat(lvs)
