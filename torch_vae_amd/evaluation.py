"""Forward-only consumer of the hot path: mirror of the reference's ``evaluation.evaluate``
(evaluation.py:12-113).  Same signature and result keys; the model runs in eval mode (BatchNorm with
running statistics) through the HIP kernels; MSE / MAE are reduced on the device instead of with
sklearn on the host (same definitions, converted to percentages as the reference does)."""
from __future__ import annotations

import torch

from . import _lib
from .types_helpers import LatentStatsOutput

MAX_LATENT_DIM = 4096


def latent_statistics(mu, log_var, *, draws=1, eps=None, seed=0, active_threshold=0.01) -> LatentStatsOutput:
    """How a VAE uses its latent space, from the posteriors q(z|x_i) = N(mu_i, diag exp(log_var_i)) of N rolls (the eval-mode
    ``encode`` outputs, [N, L] float32 on the GPU), through the HIP kernels (include/vae_step.h: vae_latent_stats).

    With the aggregate posterior q(z) = 1/N sum_j q(z|x_j) over the N rolls given (each roll's own component included),
    evaluated at ``draws`` = S samples z ~ q(z|x_i) per roll (queries q = (s, i)):
        kl           mean_i KL(q(z|x_i) || N(0, I))
        mi           I(x;z) = mean_i E log q(z|x_i) - mean_q log q(z_q)                    (He et al. 2019)
        tc           mean_q log q(z_q) - mean_q sum_d log q(z_qd)       total correlation  (Chen et al. 2018)
        dwkl         mean_q sum_d log q(z_qd) - mean_i E log p(z)       dimension-wise KL;  kl = mi + tc + dwkl
        active_units #{d : var_mu[d] > active_threshold}, var_mu the population variance of mu_d over the rolls (Burda et al. 2016)
    plus kl_per_dim, var_mu and dwkl_per_dim [L], log_qz [S, N] and log_qz_dims [S, N, L].  All float64, nats.

    The draws come from ``eps`` [S, N, L] when given, else from stream 7 of the device counter generator with ``seed``: the fixed
    default makes numbers from one epoch to the next differ only by the model.  Not differentiable.  Under torch.distributed
    each rank reports the statistics of its own rolls; nothing is gathered across ranks."""
    if not isinstance(mu, torch.Tensor) or not isinstance(log_var, torch.Tensor):
        raise TypeError("mu and log_var must be tensors")
    if mu.dim() != 2 or tuple(log_var.shape) != tuple(mu.shape):
        raise ValueError(f"mu and log_var must both be [N, L], got {tuple(mu.shape)} and {tuple(log_var.shape)}")
    N, L = mu.shape
    if N < 1 or not 1 <= L <= MAX_LATENT_DIM:
        raise ValueError(f"need N >= 1 and 1 <= L <= {MAX_LATENT_DIM}, got [N, L] = [{N}, {L}]")
    if mu.dtype != torch.float32 or log_var.dtype != torch.float32:
        raise TypeError(f"mu and log_var must be float32, got {mu.dtype} and {log_var.dtype}")
    if isinstance(draws, bool) or int(draws) != draws or draws < 1:
        raise ValueError(f"draws must be an integer >= 1, got {draws}")
    S = int(draws)
    if eps is not None:
        if tuple(eps.shape) != (S, N, L):
            raise ValueError(f"eps must be [{S},{N},{L}] (draws, N, latent_dim), got {tuple(eps.shape)}")
        if eps.dtype != torch.float32:
            raise TypeError(f"eps must be float32, got {eps.dtype}")
    if mu.device.type != "cuda" or log_var.device != mu.device or (eps is not None and eps.device != mu.device):
        raise ValueError("mu, log_var (and eps) must be on the same GPU: the statistics run on the HIP kernels only")
    dev = mu.device
    mu = mu.detach().contiguous()
    log_var = log_var.detach().contiguous()
    if eps is not None:
        eps = eps.detach().contiguous()
    f64 = dict(device=dev, dtype=torch.float64)
    log_qz = torch.empty(S, N, **f64)
    log_qz_dims = torch.empty(S, N, L, **f64)
    per_dim = torch.empty(3, L, **f64)
    scalars = torch.empty(4, **f64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_latent_stats(
            mu.data_ptr(), log_var.data_ptr(), N, L, S, _lib.ptr(eps), int(seed) & 0xFFFFFFFFFFFFFFFF, log_qz.data_ptr(),
            log_qz_dims.data_ptr(), per_dim.data_ptr(), scalars.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "vae_latent_stats")
    var_mu = per_dim[1]
    return LatentStatsOutput(kl=scalars[0], mi=scalars[1], tc=scalars[2], dwkl=scalars[3],
                             active_units=int((var_mu > active_threshold).sum()), kl_per_dim=per_dim[0], var_mu=var_mu,
                             dwkl_per_dim=per_dim[2], log_qz=log_qz, log_qz_dims=log_qz_dims)


def evaluate(dataloader, model, device, partition_name="Val", verbosity=1, *, nll_samples=0, latent_rolls=0):
    """nll_samples = K > 0 adds ``nll`` (mean over the samples of -log p(x), importance-weighted with K draws) and ``elbo``
    (mean per-sample ELBO), both in nats per roll (VanillaVAE.log_likelihood); 0 leaves keys, values and printout as the
    reference has them.  latent_rolls = R > 0 keeps the eval forward's own mu / log_var of the first R rolls (loader order)
    and adds ``kl``, ``mi``, ``tc``, ``dwkl`` (nats) and ``active_units`` from latent_statistics on them (default draws and
    seed); 0 leaves everything as it is.  Under torch.distributed each rank reports its own shard."""
    if isinstance(latent_rolls, bool) or int(latent_rolls) != latent_rolls or latent_rolls < 0:
        raise ValueError(f"latent_rolls must be an integer >= 0, got {latent_rolls}")
    model.eval()
    lat_mu, lat_lv, lat_n = [], [], 0
    nll_sum = torch.zeros((), device=device, dtype=torch.float64)
    elbo_sum = torch.zeros((), device=device, dtype=torch.float64)
    n_seen = 0
    se = torch.zeros((), device=device, dtype=torch.float64)
    ae = torch.zeros((), device=device, dtype=torch.float64)
    n_elem = 0
    stim_min, stim_max, rec_min, rec_max = float("inf"), float("-inf"), float("inf"), float("-inf")
    n_samples = len(dataloader.dataset) if hasattr(dataloader, "dataset") else None
    for stimuli, _ in dataloader:
        stimuli = stimuli.to(device)
        if n_samples is not None and n_seen + stimuli.shape[0] > n_samples:
            stimuli = stimuli[: n_samples - n_seen]      # trim DistributedSampler padding (evaluation.py:88-95)
            if stimuli.shape[0] == 0:
                break
        with torch.no_grad():
            output = model(stimuli)
        if lat_n < latent_rolls:
            k = min(latent_rolls - lat_n, stimuli.shape[0])
            lat_mu.append(output["encoded"]["mu"][:k].detach().clone())
            lat_lv.append(output["encoded"]["log_var"][:k].detach().clone())
            lat_n += k
        if nll_samples:
            lk = model.log_likelihood(stimuli, nll_samples)
            nll_sum -= lk["log_likelihood"].sum()
            elbo_sum += lk["elbo"].sum()
        rec = output["output"]
        d = (rec - stimuli).double()
        se += (d * d).sum()
        ae += d.abs().sum()
        n_elem += d.numel()
        n_seen += stimuli.shape[0]
        stim_min, stim_max = min(stim_min, float(stimuli.min())), max(stim_max, float(stimuli.max()))
        rec_min, rec_max = min(rec_min, float(rec.min())), max(rec_max, float(rec.max()))
    if verbosity >= 1:
        print(f"input has range  [{stim_min:.03f}, {stim_max:.03f}]")
        print(f"output has range [{rec_min:.03f}, {rec_max:.03f}]")
    results = {"count": n_seen}
    # F.cross_entropy(reconstruction, stimuli) over the single channel C=1 is identically 0 (evaluation.py:66)
    results["cross-entropy"] = 0.0
    results["mse"] = 100.0 * float(se) / max(n_elem, 1)
    results["mae"] = 100.0 * float(ae) / max(n_elem, 1)
    if nll_samples:
        results["nll"] = float(nll_sum) / max(n_seen, 1)
        results["elbo"] = float(elbo_sum) / max(n_seen, 1)
    if latent_rolls and lat_n:
        ls = latent_statistics(torch.cat(lat_mu), torch.cat(lat_lv))
        for k in ("kl", "active_units", "mi", "tc", "dwkl"):
            results[k] = ls[k] if k == "active_units" else float(ls[k])
    if verbosity >= 1:
        print(f"\n{partition_name} evaluation results:")
        for k, v in results.items():
            if "count" in k or k == "active_units":
                print(f"  {k + ' ':.<21s}{v:7d}")
            elif "entropy" in k:
                print(f"  {k + ' ':.<24s} {v:9.5f} nat")
            elif k in ("nll", "elbo", "kl", "mi", "tc", "dwkl"):
                print(f"  {k + ' ':.<24s} {v:9.3f} nat")
            else:
                print(f"  {k + ' ':.<24s} {v:6.2f} %")
    return results
