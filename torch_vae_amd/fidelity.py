"""Does a set of samples cover the data distribution, and does it stay on it?  The set-level fidelity metrics between two sets of
feature vectors - here the encoder means of the training rolls and of generated rolls, decoded and encoded again - on the HIP
kernels of include/vae_fidelity.h, all of them functions of the pairwise squared distances, none of which is ever stored:

* the Frechet distance between Gaussian fits (the FID recipe of Heusel et al. 2017, on the VAE's own features),
* the unbiased kernel MMD^2 with Gaussian kernels (Gretton et al. 2012),
* k-NN precision and recall (Kynkaanniemi et al. 2019),
* density and coverage (Naeem et al. 2020).

    r = sample_fidelity(model, dataset, 10000, prior=mix, seed=1)
    r["precision"], r["recall"], r["density"], r["coverage"], r["mmd2"], r["frechet"]

Everything up to the result stays on the device; ``compare_encodings`` reads back once.  Points are float32 ``[n, D]`` with
``D <= 128``, sets of up to 2^22 points."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

DEFAULT_BANDWIDTH_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)      # gamma = 1 / (s * mean cross-set squared distance)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _points(t, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if t.dim() != 2:
        raise ValueError(f"{what} must be [n, D], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    if t.device.type != "cuda":
        raise ValueError(f"{what} must be on the GPU: the fidelity metrics run on the HIP kernels only")
    n, D = t.shape
    if not 1 <= D <= _lib.FID_MAX_DIM:
        raise ValueError(f"{what} must have 1..{_lib.FID_MAX_DIM} columns, got {D}")
    if not 1 <= n <= _lib.FID_MAX_POINTS:
        raise ValueError(f"{what} must have 1..2^22 rows, got {n}")
    return t.detach().contiguous()


def _pair(a, b, na, nb):
    a, b = _points(a, na), _points(b, nb)
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"{na} and {nb} must have the same number of columns, got {a.shape[1]} and {b.shape[1]}")
    if a.device != b.device:
        raise ValueError(f"{na} and {nb} must be on the same device, got {a.device} and {b.device}")
    return a, b


def _k(k, n):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.FID_MAX_K:
        raise ValueError(f"k must be an integer in 1..{_lib.FID_MAX_K}, got {k!r}")
    if k >= n:
        raise ValueError(f"k must be below the number of points, got k = {k} and {n} points")
    return k


def _splits(splits):
    if isinstance(splits, bool) or not isinstance(splits, int) or not 0 <= splits <= _lib.FID_MAX_SPLITS:
        raise ValueError(f"splits must be an integer in 0..{_lib.FID_MAX_SPLITS}, got {splits!r}")
    return splits


def knn_radii(x, k=5, *, splits=0):
    """``[n]`` float32: the squared distance from every point of ``x`` to its k-th nearest other point (vae_fidelity_knn_radii)."""
    x = _points(x, "x")
    n, D = x.shape
    _k(k, n)
    splits = _splits(splits)
    out = torch.empty(n, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vae_fidelity_knn_radii(x.data_ptr(), n, D, k, splits, out.data_ptr(), _stream(x.device)),
                   "vae_fidelity_knn_radii")
    return out


def ball_membership(queries, refs, radii2=None, exclude_self=False, *, splits=0):
    """vae_fidelity_balls: ``(counts, nearest, nearest_d2)``, each ``[m]`` - in how many balls ``d2(q_i, r_j) <= radii2[j]`` a query
    lies (int32; None without ``radii2``), the index of its nearest reference (int32; the lowest on a tie, -1 if no distance is
    finite) and the squared distance to it (float32).  ``exclude_self`` leaves the pairs i == j out."""
    q, r = _pair(queries, refs, "queries", "refs")
    m, n, D, dev = q.shape[0], r.shape[0], q.shape[1], q.device
    splits = _splits(splits)
    if radii2 is not None:
        if not isinstance(radii2, torch.Tensor) or radii2.dtype != torch.float32 or tuple(radii2.shape) != (n,) or radii2.device != dev:
            raise ValueError(f"radii2 must be a float32 tensor [{n}] on {dev}")
        radii2 = radii2.detach().contiguous()
    counts = torch.empty(m, device=dev, dtype=torch.int32) if radii2 is not None else None
    nearest = torch.empty(m, device=dev, dtype=torch.int32)
    nearest_d2 = torch.empty(m, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_fidelity_balls(q.data_ptr(), m, r.data_ptr(), n, D, _lib.ptr(radii2), int(bool(exclude_self)), splits,
                                                 _lib.ptr(counts), nearest.data_ptr(), nearest_d2.data_ptr(), _stream(dev)), "vae_fidelity_balls")
    return counts, nearest, nearest_d2


def kernel_sums(a, b, gammas, exclude_self=False, *, splits=0):
    """vae_fidelity_kernel_sums: ``[G + 1]`` float64 on the device - ``sum_ij exp(-gammas[g] d2(a_i, b_j))`` per bandwidth, then
    ``sum_ij d2(a_i, b_j)``.  ``gammas``: up to 8 numbers, or a float64 device tensor (nothing of it is read on the host); None or
    empty gives the distance sum alone."""
    a, b = _pair(a, b, "a", "b")
    dev = a.device
    splits = _splits(splits)
    if gammas is None:
        g = torch.empty(0, device=dev, dtype=torch.float64)
    elif isinstance(gammas, torch.Tensor):
        if gammas.dtype != torch.float64 or gammas.dim() != 1 or gammas.device != dev:
            raise ValueError(f"a gammas tensor must be float64 [G] on {dev}")
        g = gammas.detach().contiguous()
    else:
        vals = [float(v) for v in gammas]
        if not all(v >= 0.0 and v < float("inf") for v in vals):
            raise ValueError(f"gammas must be finite and >= 0, got {vals}")
        g = torch.tensor(vals, device=dev, dtype=torch.float64)
    G = g.shape[0]
    if G > _lib.FID_MAX_BANDWIDTHS:
        raise ValueError(f"at most {_lib.FID_MAX_BANDWIDTHS} bandwidths, got {G}")
    sums = torch.empty(G + 1, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_fidelity_kernel_sums(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], g.data_ptr() if G else 0, G,
                                                       int(bool(exclude_self)), splits, sums.data_ptr(), _stream(dev)),
                   "vae_fidelity_kernel_sums")
    return sums


def _gammas(x, y, bandwidths):
    """The float64 device tensor of gammas: ``bandwidths`` as given, or 1 / (s * mean cross-set d2) formed on the device."""
    if bandwidths is not None:
        if isinstance(bandwidths, torch.Tensor):
            return bandwidths
        vals = [float(v) for v in bandwidths]
        if not vals or len(vals) > _lib.FID_MAX_BANDWIDTHS or not all(v > 0.0 and v < float("inf") for v in vals):
            raise ValueError(f"bandwidths must be 1..{_lib.FID_MAX_BANDWIDTHS} finite positive gammas, got {bandwidths!r}")
        return torch.tensor(vals, device=x.device, dtype=torch.float64)
    mean_d2 = kernel_sums(x, y, None)[0] / (x.shape[0] * y.shape[0])
    return 1.0 / torch.stack([mean_d2 * s for s in DEFAULT_BANDWIDTH_SCALES])      # (device arithmetic only: no host-to-device copy)


def _mmd2(x, y, gammas):
    n, m, G = x.shape[0], y.shape[0], gammas.shape[0]
    xx, yy, xy = kernel_sums(x, x, gammas, True)[:G], kernel_sums(y, y, gammas, True)[:G], kernel_sums(x, y, gammas)[:G]
    return xx / (n * (n - 1)) + yy / (m * (m - 1)) - 2.0 * xy / (n * m)


def mmd2(x, y, bandwidths=None):
    """The unbiased estimate of the squared maximum mean discrepancy per Gaussian kernel ``exp(-gamma d2)``:
    ``sum' K_xx / (n (n-1)) + sum' K_yy / (m (m-1)) - 2 sum K_xy / (n m)``, ``sum'`` without the diagonal.  ``bandwidths``: the
    gammas (numbers or a float64 device tensor); None takes ``1 / (s * mean cross-set d2)`` for s in DEFAULT_BANDWIDTH_SCALES,
    formed on the device.  Returns ``(values [G], their mean)``, float64 on the device; nothing is read back."""
    x, y = _pair(x, y, "x", "y")
    if x.shape[0] < 2 or y.shape[0] < 2:
        raise ValueError(f"the unbiased estimator needs at least 2 points a side, got {x.shape[0]} and {y.shape[0]}")
    values = _mmd2(x, y, _gammas(x, y, bandwidths))
    return values, values.mean()


def precision_recall(real, fake, k=5):
    """``dict(precision, recall, density, coverage)`` of float64 device scalars, the balls being those of the k-th nearest
    neighbour within a set: precision - the share of fakes inside some real ball; recall - the share of reals inside some fake
    ball; density - the number of real balls a fake lies in, over k, averaged; coverage - the share of reals whose nearest fake
    lies within the real's own radius."""
    real, fake = _pair(real, fake, "real", "fake")
    _k(k, real.shape[0]), _k(k, fake.shape[0])
    r_real, r_fake = knn_radii(real, k), knn_radii(fake, k)
    in_real, _, _ = ball_membership(fake, real, r_real)
    in_fake, _, to_fake = ball_membership(real, fake, r_fake)
    return dict(precision=(in_real > 0).double().mean(), recall=(in_fake > 0).double().mean(),
                density=in_real.double().sum() / (k * fake.shape[0]), coverage=(to_fake <= r_real).double().mean())


def _moments(x):
    """(mean [D], covariance about it [D, D]), float64 on the device: one M-step of a one-component mixture with zero
    log-responsibilities and no regulariser (include/vae_mixture.h; the covariance divides by n)."""
    n, D = x.shape
    if n < 2:
        raise ValueError(f"the moments need at least 2 points, got {n}")
    dev = x.device
    w = torch.empty(1, device=dev, dtype=torch.float64)
    mean = torch.empty(1, D, device=dev, dtype=torch.float64)
    cov = torch.empty(1, D, D, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_mixture_mstep(torch.zeros(n, 1, device=dev).data_ptr(), x.data_ptr(), n, D, 1, _lib.MIXTURE_FULL, 0.0,
                                                w.data_ptr(), mean.data_ptr(), cov.data_ptr(), _stream(dev)), "vae_mixture_mstep")
    return mean[0], cov[0]


def _sqrt_psd(s):
    w, v = np.linalg.eigh((s + s.T) / 2)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet_from_moments(m1, s1, m2, s2) -> float:
    """``|m1 - m2|^2 + tr(S1 + S2 - 2 (S1^1/2 S2 S1^1/2)^1/2)`` in host float64 (numpy arrays), the roots through
    ``numpy.linalg.eigh`` with eigenvalues below 0 taken as 0."""
    m1, s1, m2, s2 = (np.asarray(t, dtype=np.float64) for t in (m1, s1, m2, s2))
    h = _sqrt_psd(s1)
    inner = h @ s2 @ h
    w = np.linalg.eigvalsh((inner + inner.T) / 2)
    dm = m1 - m2
    return float(dm @ dm + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(w, 0.0, None)).sum())


def frechet_distance(x, y) -> float:
    """The Frechet distance between the Gaussian fits of two sets: the moments on the device, one read-back of the two means and
    covariances, the rest in host float64 (frechet_from_moments)."""
    x, y = _pair(x, y, "x", "y")
    D = x.shape[1]
    flat = torch.cat([t.reshape(-1) for t in (*_moments(x), *_moments(y))]).cpu().numpy()      # the one read-back
    m1, s1, m2, s2 = flat[:D], flat[D:D + D * D], flat[D + D * D:2 * D + D * D], flat[2 * D + D * D:]
    return frechet_from_moments(m1, s1.reshape(D, D), m2, s2.reshape(D, D))


def compare_encodings(real, fake, k=5, bandwidths=None) -> dict:
    """Everything above between two sets of encodings as one dict of Python floats after a single read-back: ``precision``,
    ``recall``, ``density``, ``coverage``, ``mmd2`` (the mean over the bandwidths), ``mmd2_per_bandwidth`` and ``gammas`` (lists),
    ``frechet``, and the set sizes ``real`` / ``fake``."""
    real, fake = _pair(real, fake, "real", "fake")
    if real.shape[0] < 2 or fake.shape[0] < 2:
        raise ValueError(f"need at least 2 points a side, got {real.shape[0]} and {fake.shape[0]}")
    D = real.shape[1]
    prdc = precision_recall(real, fake, k)
    gammas = _gammas(real, fake, bandwidths)
    values = _mmd2(real, fake, gammas.to(torch.float64))
    G = values.shape[0]
    parts = [torch.stack([prdc[n] for n in ("precision", "recall", "density", "coverage")]), values, gammas.double(),
             *(t.reshape(-1) for t in (*_moments(real), *_moments(fake)))]
    flat = torch.cat(parts).cpu().numpy()                                                        # the one read-back
    out = dict(zip(("precision", "recall", "density", "coverage"), (float(v) for v in flat[:4])))
    per = [float(v) for v in flat[4:4 + G]]
    out.update(mmd2=float(np.mean(flat[4:4 + G])), mmd2_per_bandwidth=per, gammas=[float(v) for v in flat[4 + G:4 + 2 * G]])
    mo = flat[4 + 2 * G:]
    m1, s1, m2, s2 = mo[:D], mo[D:D + D * D], mo[D + D * D:2 * D + D * D], mo[2 * D + D * D:]
    out.update(frechet=frechet_from_moments(m1, s1.reshape(D, D), m2, s2.reshape(D, D)), real=int(real.shape[0]), fake=int(fake.shape[0]))
    return out


def sample_fidelity(model, dataset, num_samples, *, prior=None, temperature=1.0, seed=None, k=5, batch_size=256, max_rolls=None,
                    bandwidths=None) -> dict:
    """Do the model's samples cover the training set in its own latent space, and stay on it?  Real features: the encoder means of
    ``dataset`` (a ``PianorollDataset``; the centre window of the model's width, ``mixture.encode_dataset`` over batches of
    ``batch_size``, the first ``max_rolls`` rolls when given).  Fake features: ``num_samples`` latents - with ``prior`` (a
    ``mixture.LatentMixture``) through ``model.sample(..., prior=prior, temperature=..., seed=...)``, else
    ``temperature * N(0, I)`` from a ``torch.Generator`` on the model's device seeded with ``seed``, as ``sample_notes`` draws them
    (``seed`` None: a fresh one either way) - decoded and encoded again by the eval-mode model, which is left in eval mode.
    Returns ``compare_encodings(real, fake, k, bandwidths)``."""
    from .data import DevicePianorollLoader, PianorollDataset
    from .mixture import encode_dataset
    if not isinstance(dataset, PianorollDataset):
        raise TypeError("dataset must be a PianorollDataset")
    for name, v in (("num_samples", num_samples), ("batch_size", batch_size)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v}")
    size = int(model.img_size)
    if dataset.height != size or dataset.width < size:
        raise ValueError(f"the dataset's rolls are {dataset.height}x{dataset.width}, the model's {size}x{size}")
    real, _ = encode_dataset(model, DevicePianorollLoader(dataset, int(batch_size), width=size, train=False, rank=0, world=1), max_rolls)
    dev = real.device
    num = int(num_samples)
    if prior is not None:
        rolls = model.sample(num, dev, prior=prior, temperature=temperature,
                             seed=int(torch.randint(0, 2 ** 62, (1,))) if seed is None else int(seed))
    else:
        g = torch.Generator(device=dev)
        if seed is None:
            g.seed()
        else:
            g.manual_seed(int(seed))
        z = float(temperature) * torch.randn(num, model.latent_dim, generator=g, device=dev, dtype=torch.float32)
        with torch.no_grad():
            rolls = model.decode(z)
    fakes = []
    with torch.no_grad():
        for first in range(0, num, int(batch_size)):
            fakes.append(model.encode(rolls[first:first + int(batch_size)].contiguous())["mu"].detach().clone())
    return compare_encodings(real, torch.cat(fakes).float(), k, bandwidths)
