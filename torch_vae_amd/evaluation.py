"""Forward-only consumer of the hot path: mirror of the reference's ``evaluation.evaluate``
(evaluation.py:12-113).  Same signature and result keys; the model runs in eval mode (BatchNorm with
running statistics) through the HIP kernels; MSE / MAE are reduced on the device instead of with
sklearn on the host (same definitions, converted to percentages as the reference does)."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from .attributes import ATTRIBUTE_NAMES, attribute_correlation, attribute_values, roll_attributes  # noqa: F401  (part of this module's surface)
from .types_helpers import LatentStatsOutput, MusicStats, NearestRolls, ReconMetricsOutput

MAX_LATENT_DIM = 4096
MAX_NOTE_THRESHOLDS = _lib.RECON_METRICS_MAX_THRESHOLDS


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


def _note_thresholds(thresholds, target_threshold):
    """(thresholds rounded to float32 once, as Python floats; the same for target_threshold).  A float stands for a list of one."""
    if isinstance(thresholds, (int, float)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    try:
        ts = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise ValueError(f"thresholds must be a float or a sequence of floats, got {thresholds!r}") from None
    if not 1 <= len(ts) <= MAX_NOTE_THRESHOLDS:
        raise ValueError(f"need 1 to {MAX_NOTE_THRESHOLDS} thresholds, got {len(ts)}")
    tt = float(target_threshold)
    if not all(math.isfinite(t) for t in ts) or not math.isfinite(tt):
        raise ValueError(f"thresholds and target_threshold must be finite, got {ts} and {tt}")
    f32 = lambda v: ctypes.c_float(v).value
    ts, tt = tuple(f32(t) for t in ts), f32(tt)
    if not all(math.isfinite(t) for t in ts) or not math.isfinite(tt):
        raise ValueError("thresholds and target_threshold must be finite in float32")
    return ts, tt


def _checked_rolls(xhat, target):
    """The two tensors as the kernel reads them ([N, roll_len] float32, contiguous, on one GPU) and (N, roll_len)."""
    if not isinstance(xhat, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("xhat and target must be tensors")
    if xhat.dim() < 1 or tuple(xhat.shape) != tuple(target.shape):
        raise ValueError(f"xhat and target must have the same shape [N, ...], got {tuple(xhat.shape)} and {tuple(target.shape)}")
    if xhat.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"xhat and target must be float32, got {xhat.dtype} and {target.dtype}")
    if xhat.device.type != "cuda" or target.device != xhat.device:
        raise ValueError("xhat and target must be on the same GPU: the metrics run on the HIP kernels only")
    n = xhat.shape[0]
    roll_len = 1
    for s in xhat.shape[1:]:
        roll_len *= s
    if roll_len < 1:
        raise ValueError(f"a roll must have at least one cell, got shape {tuple(xhat.shape)}")
    return xhat.detach().contiguous(), target.detach().contiguous(), n, roll_len


def _recon_metrics_call(xhat, target, n, roll_len, c_thresholds, tt, roll_sums, roll_counts, totals, total_counts, accumulate):
    dev = xhat.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_recon_metrics(
            xhat.data_ptr(), target.data_ptr(), n, roll_len, c_thresholds, len(c_thresholds), tt, roll_sums.data_ptr(),
            roll_counts.data_ptr(), totals.data_ptr(), total_counts.data_ptr(), int(accumulate),
            torch.cuda.current_stream(dev).cuda_stream), "vae_recon_metrics")


def ratios_from_counts(n_cells, positives, tp, fp):
    """Per-threshold note ratios from the counts of vae_recon_metrics (host integers; tp, fp sequences of equal length):
    precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn), accuracy = (tp + tn) / n_cells,
    pred_density = (tp + fp) / n_cells, with fn = positives - tp and tn = n_cells - positives - fp.  A ratio whose denominator
    is 0 is 0.0 (scikit-learn's zero_division=0).  Returns a dict of lists."""
    n_cells, positives = int(n_cells), int(positives)
    div = lambda a, b: a / b if b else 0.0
    out = {k: [] for k in ("precision", "recall", "f1", "accuracy", "pred_density")}
    for t, f in zip(tp, fp):
        t, f = int(t), int(f)
        fn = positives - t
        out["precision"].append(div(t, t + f))
        out["recall"].append(div(t, t + fn))
        out["f1"].append(div(2 * t, 2 * t + f + fn))
        out["accuracy"].append(div(t + (n_cells - positives - f), n_cells))
        out["pred_density"].append(div(t + f, n_cells))
    return out


def reconstruction_metrics(xhat, target, thresholds=(0.5,), *, target_threshold=0.5) -> ReconMetricsOutput:
    """Note-level reconstruction metrics of N rolls in one HIP pass (include/vae_step.h: vae_recon_metrics).  xhat, target: float32
    GPU tensors of equal shape [N, ...], dimension 0 indexing rolls.  A cell is a true note iff target >= target_threshold and a
    predicted note at threshold t iff xhat >= t (float32 comparisons; up to 8 thresholds, in any order).  Returns device tensors,
    with no host synchronisation: the sums se, ae, bce (float64; bce is the ELBO's BCE term, nats), n_cells, positives, tp / fp / fn
    [T] (int64), xhat_range and target_range (min, max), and the per-roll partials they were folded from (roll_se, roll_ae,
    roll_bce, roll_positives [N], roll_tp, roll_fp [N, T]) - rank rolls by them.  Counts are exact; every sum runs in a fixed order,
    so repeated calls are bit-identical.  Not differentiable."""
    ts, tt = _note_thresholds(thresholds, target_threshold)
    xhat, target, n, roll_len = _checked_rolls(xhat, target)
    T, dev = len(ts), xhat.device
    roll_sums = torch.empty(n, 3, device=dev, dtype=torch.float64)
    roll_counts = torch.empty(n, 1 + 2 * T, device=dev, dtype=torch.int64)
    totals = torch.empty(8, device=dev, dtype=torch.float64)
    total_counts = torch.empty(1 + 2 * T, device=dev, dtype=torch.int64)
    _recon_metrics_call(xhat, target, n, roll_len, (ctypes.c_float * T)(*ts), tt, roll_sums, roll_counts, totals, total_counts, 0)
    tp = total_counts[1::2]
    return ReconMetricsOutput(
        se=totals[0], ae=totals[1], bce=totals[2], n_cells=totals[3].to(torch.int64), positives=total_counts[0], tp=tp,
        fp=total_counts[2::2], fn=total_counts[0] - tp, xhat_range=totals[4:6], target_range=totals[6:8],
        roll_se=roll_sums[:, 0], roll_ae=roll_sums[:, 1], roll_bce=roll_sums[:, 2], roll_positives=roll_counts[:, 0],
        roll_tp=roll_counts[:, 1::2], roll_fp=roll_counts[:, 2::2])


def infill_metrics(xhat, target, t0, t1, thresholds=(0.5,), *, target_threshold=0.5) -> ReconMetricsOutput:
    """``reconstruction_metrics`` on the time span ``[t0, t1)`` only - the columns ``generation.infill`` filled: xhat and target are
    float32 GPU tensors [N, ..., W]; their last dimension is cut to the span (a strided view made contiguous: plumbing) and the
    same HIP pass scores it."""
    from .generation import checked_time_span
    if not isinstance(xhat, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("xhat and target must be tensors")
    if xhat.dim() < 2 or tuple(xhat.shape) != tuple(target.shape):
        raise ValueError(f"xhat and target must have the same shape [N, ..., W], got {tuple(xhat.shape)} and {tuple(target.shape)}")
    t0, t1 = checked_time_span(t0, t1, xhat.shape[-1])
    return reconstruction_metrics(xhat[..., t0:t1], target[..., t0:t1], thresholds, target_threshold=target_threshold)


class ReconMetricsAccumulator:
    """reconstruction_metrics over a whole pass: update() adds a batch to totals that stay on the device (one library call, no host
    synchronisation, no allocation beyond the per-roll work space, which is reused while the batch size stays the same); compute()
    reads them back once."""

    def __init__(self, thresholds=(0.5,), target_threshold=0.5, device="cuda"):
        self.thresholds, self.target_threshold = _note_thresholds(thresholds, target_threshold)
        self.device = torch.device(device)
        self._c_thresholds = (ctypes.c_float * len(self.thresholds))(*self.thresholds)
        self._state = None     # 8 float64 totals then 1 + 2T int64 counts, one buffer: one read in compute()
        self._roll = None      # (n, roll_sums, roll_counts)

    def _views(self):
        if self._state is None:
            self._state = torch.zeros(8 + 1 + 2 * len(self.thresholds), device=self.device, dtype=torch.int64)
        return self._state[:8].view(torch.float64), self._state[8:]

    def reset(self):
        if self._state is not None:
            self._state.zero_()     # all zeros is the kernels' empty state (n_cells == 0)

    def update(self, xhat, target):
        xhat, target, n, roll_len = _checked_rolls(xhat, target)
        if xhat.device != self._views()[0].device:
            raise ValueError(f"the accumulator lives on {self._state.device}, the tensors on {xhat.device}")
        totals, counts = self._views()
        if self._roll is None or self._roll[0] != n:
            self._roll = (n, torch.empty(n, 3, device=xhat.device, dtype=torch.float64),
                          torch.empty(n, counts.numel(), device=xhat.device, dtype=torch.int64))
        _recon_metrics_call(xhat, target, n, roll_len, self._c_thresholds, self.target_threshold, self._roll[1], self._roll[2],
                            totals, counts, 1)

    def totals(self) -> dict:
        """The running totals as device tensors (views of the state, no host synchronisation), under ReconMetricsOutput's keys."""
        t, c = self._views()
        tp = c[1::2]
        return dict(se=t[0], ae=t[1], bce=t[2], n_cells=t[3].to(torch.int64), positives=c[0], tp=tp, fp=c[2::2], fn=c[0] - tp,
                    xhat_range=t[4:6], target_range=t[6:8])

    def compute(self) -> dict:
        """Python numbers: count_cells, mse, mae, bce (means per cell; bce in nats), note_density, xhat_range and target_range
        (min, max), and per threshold the lists precision, recall, f1, accuracy, pred_density (ratios_from_counts)."""
        T = len(self.thresholds)
        if self._state is None:
            tot, cnt = [0.0] * 8, [0] * (1 + 2 * T)
        else:
            host = self._state.cpu()
            tot, cnt = host[:8].view(torch.float64).tolist(), host[8:].tolist()
        n = int(tot[3])
        d = max(n, 1)
        out = {"count_cells": n, "mse": tot[0] / d, "mae": tot[1] / d, "bce": tot[2] / d, "note_density": cnt[0] / d,
               "xhat_range": (tot[4], tot[5]), "target_range": (tot[6], tot[7])}
        out.update(ratios_from_counts(n, cnt[0], cnt[1::2], cnt[2::2]))
        return out


def balanced_pos_weight(note_density, max_weight=64.0) -> float:
    """The ``pos_weight`` of ``VanillaVAE`` that balances notes against silence: ``min(max_weight, (1 - d) / d)`` for a note
    density ``d`` in [0, 1] (a fraction, as ``ReconMetricsAccumulator.compute()["note_density"]`` reports it; ``evaluate()``'s key
    of the same name is a percentage).  ``d = 0`` gives ``max_weight``; a ``d`` outside [0, 1] (or NaN) raises ValueError.  A pure
    host function: nothing touches the device."""
    d, cap = float(note_density), float(max_weight)
    if not 0.0 <= d <= 1.0:
        raise ValueError(f"note_density must be a fraction in [0, 1], got {note_density!r}")
    if not (math.isfinite(cap) and cap > 0.0):
        raise ValueError(f"max_weight must be a finite number > 0, got {max_weight!r}")
    return cap if d == 0.0 else min(cap, (1.0 - d) / d)


def _count_note_matches(pred, ref, onset_tolerance):
    """(notes_pred, notes_true, matched) of two host lists of (roll, pitch, onset, duration) rows sorted by (roll, pitch, onset)."""
    i = j = matched = 0
    while i < len(pred) and j < len(ref):
        (ra, pa, ta), (rb, pb, tb) = pred[i][:3], ref[j][:3]
        if (ra, pa) != (rb, pb):     # the row that is behind catches up
            if (ra, pa) < (rb, pb):
                i += 1
            else:
                j += 1
        elif abs(ta - tb) <= onset_tolerance:
            matched += 1
            i += 1
            j += 1
        elif ta < tb:
            i += 1
        else:
            j += 1
    return len(pred), len(ref), matched


def note_event_ratios(notes_pred, notes_true, matched) -> dict:
    """The result of note_event_metrics from its three counts; a ratio with a zero denominator is 0.0."""
    div = lambda a, b: a / b if b else 0.0
    return {"notes_pred": int(notes_pred), "notes_true": int(notes_true), "matched": int(matched),
            "note_precision": div(matched, notes_pred), "note_recall": div(matched, notes_true),
            "note_f1": div(2 * matched, notes_pred + notes_true)}


def _host_events(ev):
    """An event list as host rows: a NoteEvents dict (the events written, at most ``total``), a tensor or anything array-like."""
    if isinstance(ev, dict):
        ev = ev["events"][:min(int(ev["total"]), ev["events"].shape[0])]
    if isinstance(ev, torch.Tensor):
        return ev.detach().reshape(-1, 4).cpu().tolist()
    return [[int(v) for v in row] for row in ev]


def note_event_metrics(pred, ref, *, onset_tolerance=1) -> dict:
    """Note-onset scores of predicted against reference events (``generation.extract_notes`` results, or [N,4] event arrays sorted
    by (roll, pitch, onset)): a predicted note is matched when a reference note of the same roll and pitch has its onset within
    ``onset_tolerance`` steps, every note at most once (a two-pointer sweep within each row, which finds the most matches there
    are).  Returns notes_pred, notes_true, matched, note_precision, note_recall, note_f1.  Runs on the host after one read-back
    of each event array."""
    if isinstance(onset_tolerance, bool) or int(onset_tolerance) != onset_tolerance or onset_tolerance < 0:
        raise ValueError(f"onset_tolerance must be an integer >= 0, got {onset_tolerance}")
    return note_event_ratios(*_count_note_matches(_host_events(pred), _host_events(ref), int(onset_tolerance)))


def _query_planes(queries, threshold):
    """Tensor queries of nearest_rolls as contiguous uint8 planes [Q, h, w/8] on the GPU."""
    if not isinstance(queries, torch.Tensor):
        raise TypeError("queries must be a tensor or a PianorollDataset")
    if queries.device.type != "cuda":
        raise ValueError("queries must be on the GPU: the search runs on the HIP kernels only")
    if queries.dtype == torch.float32:
        from .generation import binarize_rolls
        return binarize_rolls(queries.contiguous(), threshold)
    if queries.dtype != torch.uint8:
        raise TypeError(f"queries must be uint8 bit planes or float32 rolls, got {queries.dtype}")
    if queries.dim() != 3:
        raise ValueError(f"bit-plane queries must be [Q, h, w/8], got {tuple(queries.shape)}")
    return queries.detach().contiguous()


def nearest_rolls(queries, dataset, k=1, *, max_pitch_shift=0, max_time_shift=0, exclude=None, threshold=0.5) -> NearestRolls:
    """The ``k`` rolls of ``dataset`` nearest to each query under transposition and time shift, on the device (include/vae_step.h:
    vae_nearest_rolls has the definition).  ``queries``: uint8 bit planes [Q,h,w/8], float32 rolls [Q,h,w] or [Q,1,h,w] (cut at
    ``threshold`` by ``generation.binarize_rolls``) on the GPU, or a ``PianorollDataset`` with "bits" storage.  ``dataset``: a
    ``PianorollDataset`` with "bits" storage on the device, of the same height and width.  The distance of a pair is the smallest
    Hamming distance over transpositions of up to ``max_pitch_shift`` rows and shifts of up to ``max_time_shift`` steps of the
    dataset roll (zero-filled, as the training augmentation does it); neighbours ascend by (distance, index).  ``exclude``: None,
    an int64 [Q] GPU tensor of dataset indices to leave out per query, or "self" (needs ``queries is dataset``): the near-duplicate
    search of a dataset against itself.  ``k > len(dataset)`` leaves slots of index -1.  Returns device tensors (NearestRolls);
    nothing is read back.  Repeated calls give the same bits."""
    from .data import PianorollDataset
    if not isinstance(dataset, PianorollDataset):
        raise TypeError("dataset must be a PianorollDataset")
    if dataset.storage != "bits":
        raise ValueError(f"the dataset must have 'bits' storage, got {dataset.storage!r}")
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= _lib.NEAREST_MAX_K:
        raise ValueError(f"k must be an integer in 1..{_lib.NEAREST_MAX_K}, got {k}")
    for name, v in (("max_pitch_shift", max_pitch_shift), ("max_time_shift", max_time_shift)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError(f"{name} must be an integer >= 0, got {v}")
    if isinstance(exclude, str):
        if exclude != "self":
            raise ValueError(f"exclude must be None, 'self' or an int64 tensor, got {exclude!r}")
        if queries is not dataset:
            raise ValueError("exclude='self' needs the dataset itself as queries")
    if isinstance(queries, PianorollDataset):
        if queries.storage != "bits":
            raise ValueError(f"a dataset used as queries must have 'bits' storage, got {queries.storage!r}")
        planes = queries.data
    else:
        planes = _query_planes(queries, threshold)
    rolls = dataset.data
    Q, h, wb = (int(s) for s in planes.shape)
    if (h, wb * 8) != (dataset.height, dataset.width):
        raise ValueError(f"queries are {h}x{wb * 8}, the dataset's rolls {dataset.height}x{dataset.width}")
    if dataset.pinned or not rolls.is_cuda:
        raise ValueError("the dataset must be on the device, not in pinned host memory: the kernel reads every roll once per query "
                         "tile, which the host link cannot feed")
    if not planes.is_cuda:
        raise ValueError("a dataset used as queries must be on the device, not in pinned host memory")
    if planes.device != rolls.device:
        raise ValueError(f"queries are on {planes.device}, the dataset on {rolls.device}")
    dev = rolls.device
    if isinstance(exclude, str):
        exclude = torch.arange(Q, dtype=torch.int64, device=dev)
    elif exclude is not None:
        if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int64 or tuple(exclude.shape) != (Q,) or exclude.device != dev:
            raise ValueError(f"exclude must be an int64 [{Q}] tensor on {dev}")
        exclude = exclude.contiguous()
    k = int(k)
    index = torch.full((Q, k), -1, dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    distance, shift = torch.full((Q, k), -1, **i32), torch.zeros(Q, k, 2, **i32)
    inter, cells = torch.zeros(Q, k, **i32), torch.zeros(Q, **i32)
    if Q:      # (an empty tensor has no address to hand over)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().vae_nearest_rolls(
                planes.data_ptr(), Q, rolls.data_ptr(), len(dataset), h, wb * 8, int(max_pitch_shift), int(max_time_shift),
                _lib.ptr(exclude), k, 0, index.data_ptr(), distance.data_ptr(), shift.data_ptr(), inter.data_ptr(), cells.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream), "vae_nearest_rolls")
    return _nearest_result(index, distance, shift, inter, cells)


def _nearest_result(index, distance, shift, intersection, query_cells) -> NearestRolls:
    """The derived fields: the shifted neighbour's cells d + 2 inter - |q|, and the Jaccard index inter / (d + inter) - the union
    is the differing cells plus the common ones - as float64, 1.0 where both rolls are empty, nan in empty slots."""
    found = index >= 0
    ncells = torch.where(found, distance + 2 * intersection - query_cells[:, None], torch.zeros_like(distance))
    union = (distance + intersection).double()
    jac = torch.where(union > 0, intersection.double() / union.clamp_min(1.0), torch.ones_like(union))
    jac = torch.where(found, jac, torch.full_like(jac, float("nan")))
    return NearestRolls(index=index, distance=distance, shift=shift, intersection=intersection, query_cells=query_cells,
                        neighbour_cells=ncells, jaccard=jac)


def novelty_summary(result, copy_jaccard=0.9) -> dict:
    """What a nearest_rolls result says about novelty, with one read-back (CPU tensors work too).  Over the queries that have a
    nearest neighbour: ``count``; ``copies``, the share whose nearest neighbour has ``jaccard >= copy_jaccard``;
    ``shifted_copies``, the share that are copies found at a non-zero shift; ``median_jaccard`` and ``mean_distance`` of the nearest
    neighbour.  ``without_neighbour`` counts the others (every roll excluded, or none there).  With no query left the shares and
    means are 0.0."""
    cj = float(copy_jaccard)
    if not 0.0 <= cj <= 1.0:
        raise ValueError(f"copy_jaccard must be in [0, 1], got {copy_jaccard!r}")
    idx, jac = result["index"][:, 0], result["jaccard"][:, 0]
    host = torch.stack([idx.double(), jac.double(), result["distance"][:, 0].double(),
                        (result["shift"][:, 0] != 0).any(dim=-1).double()]).cpu()
    found = host[0] >= 0
    n = int(found.sum())
    out = {"count": n, "without_neighbour": int(idx.numel()) - n, "copies": 0.0, "shifted_copies": 0.0, "median_jaccard": 0.0,
           "mean_distance": 0.0}
    if n:
        j, d, moved = host[1][found], host[2][found], host[3][found] > 0
        copy = j >= cj
        out.update(copies=int(copy.sum()) / n, shifted_copies=int((copy & moved).sum()) / n,
                   median_jaccard=float(j.sort().values[(n - 1) // 2]) if n % 2 else float(j.sort().values[n // 2 - 1:n // 2 + 1].mean()),
                   mean_distance=float(d.mean()))
    return out


def sample_novelty(model, dataset, num_samples, *, temperature=1.0, seed=None, k=1, max_pitch_shift=0, max_time_shift=0,
                   copy_jaccard=0.9, prior=None, **extract_kwargs):
    """Is what the model generates new?  ``model.sample_notes(num_samples, temperature=..., seed=..., cleaned=True,
    **extract_kwargs)``, then nearest_rolls of the cleaned planes in ``dataset`` under the shift window.  Returns
    ``(novelty_summary, NearestRolls, NoteEvents)``.  ``prior``: a ``mixture.LatentMixture`` to draw the latents from instead of
    N(0, I) (``sample_notes(prior=...)``)."""
    if prior is not None:
        extract_kwargs = dict(extract_kwargs, prior=prior)
    notes = model.sample_notes(int(num_samples), temperature=temperature, seed=seed, cleaned=True, **extract_kwargs)
    near = nearest_rolls(notes["cleaned"], dataset, k, max_pitch_shift=max_pitch_shift, max_time_shift=max_time_shift)
    return novelty_summary(near, copy_jaccard), near, notes


# ---- musical statistics of sets of rolls (include/vae_music.h) ---------------------------------------------------------------------
MUSIC_FEATURES = _lib.MUSIC_FEATURES
MUSIC_COLUMNS = {
    "rolls": slice(0, 1), "nonempty": slice(1, 2), "cells": slice(2, 3), "notes": slice(3, 4), "used_pitches": slice(4, 5),
    "lowest": slice(5, 6), "highest": slice(6, 7), "sounding_steps": slice(7, 8), "onset_steps": slice(8, 9),
    "max_polyphony": slice(9, 10), "pc_cells": slice(10, 22), "pc_notes": slice(22, 34), "duration": slice(34, 46),
    "polyphony": slice(46, 62), "ioi": slice(62, 74),
}
# the normalised distributions of music_summary / compare_music and the columns they are made of
MUSIC_DISTRIBUTIONS = {"pitch_class": "pc_cells", "pitch_class_onsets": "pc_notes", "duration": "duration", "polyphony": "polyphony",
                       "ioi": "ioi"}
MUSIC_SCALARS = ("notes", "cells", "used_pitches", "pitch_range", "max_polyphony")     # per-roll numbers compare_music holds against each other
MAJOR_SCALE = (0, 2, 4, 5, 7, 9, 11)
_NAN = float("nan")


def _music_pitch_offset(pitch_offset):
    if isinstance(pitch_offset, bool) or int(pitch_offset) != pitch_offset or not 0 <= pitch_offset <= _lib.MUSIC_MAX_PITCH_OFFSET:
        raise ValueError(f"pitch_offset must be an integer in 0..{_lib.MUSIC_MAX_PITCH_OFFSET}, got {pitch_offset}")
    return int(pitch_offset)


def _music_checked_shape(h, w):
    if h < 1 or w < 32 or w % 32:
        raise ValueError(f"need at least one pitch row and a width (time steps) that is a positive multiple of 32, got {h}x{w}")
    if h * (w // 8) > _lib.MUSIC_MAX_ROLL_BYTES:
        raise ValueError(f"a roll of {h}x{w} cells takes {h * (w // 8)} bytes as bit planes, above the {_lib.MUSIC_MAX_ROLL_BYTES} the kernel holds")


def _music_planes(rolls, threshold):
    """The rolls of music_statistics as contiguous uint8 planes [n, h, w/8] on the GPU, with (n, h, w)."""
    from .data import PianorollDataset
    if isinstance(rolls, PianorollDataset):
        if rolls.storage != "bits":
            raise ValueError(f"a dataset must have 'bits' storage, got {rolls.storage!r}")
        if rolls.pinned or not rolls.data.is_cuda:
            raise ValueError("the dataset must be on the device, not in pinned host memory")
        planes = rolls.data
    elif not isinstance(rolls, torch.Tensor):
        raise TypeError("rolls must be a tensor or a PianorollDataset")
    elif rolls.dtype == torch.float32:
        if rolls.dim() not in (3, 4) or (rolls.dim() == 4 and rolls.shape[1] != 1):
            raise ValueError(f"float32 rolls must be [n, h, w] or [n, 1, h, w], got {tuple(rolls.shape)}")
        h, w = int(rolls.shape[-2]), int(rolls.shape[-1])
        _music_checked_shape(h, w)
        if rolls.device.type != "cuda":
            raise ValueError("rolls must be on the GPU: the statistics run on the HIP kernels only")
        from .generation import binarize_rolls
        planes = binarize_rolls(rolls.detach().contiguous(), threshold)
    elif rolls.dtype != torch.uint8:
        raise TypeError(f"rolls must be uint8 bit planes or float32 rolls, got {rolls.dtype}")
    elif rolls.dim() != 3:
        raise ValueError(f"bit-plane rolls must be [n, h, w/8], got {tuple(rolls.shape)}")
    else:
        planes = rolls.detach().contiguous()
    n, h, wb = (int(v) for v in planes.shape)
    _music_checked_shape(h, wb * 8)
    if planes.device.type != "cuda":
        raise ValueError("rolls must be on the GPU: the statistics run on the HIP kernels only")
    return planes, n, h, wb * 8


def _music_empty_totals(dev):
    """zeros, lowest -1, highest -1 (built on the device: a copy from host memory would wait for the stream)"""
    empty = torch.zeros(MUSIC_FEATURES, dtype=torch.int64, device=dev)
    empty[5:7] = -1
    return empty


def _music_call(planes, n, h, w, pitch_offset, features, totals, accumulate):
    dev = planes.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_music_roll_stats(planes.data_ptr(), n, h, w, pitch_offset, features.data_ptr(), totals.data_ptr(),
                                                   int(accumulate), torch.cuda.current_stream(dev).cuda_stream), "vae_music_roll_stats")


def music_statistics(rolls, *, pitch_offset=0, threshold=0.5) -> MusicStats:
    """What ``rolls`` are as music, counted on the device in one HIP pass over bit planes (include/vae_music.h: vae_music_roll_stats
    has the table of the 76 columns).  ``rolls``: uint8 bit planes [n,h,w/8] on the GPU, float32 rolls [n,h,w] or [n,1,h,w] (cut at
    ``threshold`` by ``generation.binarize_rolls``), or a ``PianorollDataset`` with "bits" storage on the device, whose planes are
    used as they are.  A note is a maximal run of set cells along time in one pitch row; row p has pitch class
    ``(p + pitch_offset) mod 12``.  w must be a multiple of 32 and a roll at most 8192 bytes of planes (256x256 fits).  Returns
    device tensors - ``features`` int32 [n,76], ``totals`` int64 [76] - with ``columns`` (name -> slice of the 76, so nobody
    indexes by number), ``height``, ``width`` and ``pitch_offset``; nothing is read back.  All counts are exact and repeat bit for
    bit.  ``music_summary`` and ``compare_music`` turn them into numbers."""
    off = _music_pitch_offset(pitch_offset)
    planes, n, h, w = _music_planes(rolls, threshold)
    dev = planes.device
    features = torch.empty(n, MUSIC_FEATURES, dtype=torch.int32, device=dev)
    if n:      # (an empty tensor has no address to hand over)
        totals = torch.empty(MUSIC_FEATURES, dtype=torch.int64, device=dev)
        _music_call(planes, n, h, w, off, features, totals, 0)
    else:
        totals = _music_empty_totals(dev)
    return MusicStats(features=features, totals=totals, columns=dict(MUSIC_COLUMNS), height=h, width=w, pitch_offset=off)


class MusicStatsAccumulator:
    """music_statistics over a set that arrives in batches: update() makes one library call that adds the batch to totals the
    accumulator owns (``accumulate=1``) and keeps the batch's per-roll table on the device; compute() returns the MusicStats of
    everything seen.  Nothing is read back.  Every batch must have the shape of the first."""

    def __init__(self, pitch_offset=0, threshold=0.5):
        self.pitch_offset, self.threshold = _music_pitch_offset(pitch_offset), threshold
        self._shape, self._totals, self._features = None, None, []

    def update(self, rolls):
        planes, n, h, w = _music_planes(rolls, self.threshold)
        if self._shape is None:
            self._shape, self._totals = (h, w), _music_empty_totals(planes.device)
        elif self._shape != (h, w):
            raise ValueError(f"the accumulator holds {self._shape[0]}x{self._shape[1]} rolls, this batch is {h}x{w}")
        elif planes.device != self._totals.device:
            raise ValueError(f"the accumulator lives on {self._totals.device}, the rolls on {planes.device}")
        if not n:
            return
        features = torch.empty(n, MUSIC_FEATURES, dtype=torch.int32, device=planes.device)
        _music_call(planes, n, h, w, self.pitch_offset, features, self._totals, 1)
        self._features.append(features)

    def compute(self) -> MusicStats:
        if self._shape is None:
            raise RuntimeError("nothing to compute: update() has not been called")
        dev = self._totals.device
        features = torch.cat(self._features) if self._features else torch.empty(0, MUSIC_FEATURES, dtype=torch.int32, device=dev)
        self._features = [features] if self._features else []
        return MusicStats(features=features, totals=self._totals, columns=dict(MUSIC_COLUMNS), height=self._shape[0],
                          width=self._shape[1], pitch_offset=self.pitch_offset)


def _ratio(a, b):
    return a / b if b else _NAN


def _normalised(counts):
    total = sum(counts)
    return [_ratio(c, total) for c in counts]


def _scale_consistency(pc_cells):
    """(the largest share of cells inside a major scale over its 12 roots, the lowest root that reaches it); (nan, -1) without cells"""
    cells = sum(pc_cells)
    if not cells:
        return _NAN, -1
    best, key = -1.0, -1
    for root in range(12):
        share = sum(pc_cells[(root + s) % 12] for s in MAJOR_SCALE) / cells
        if share > best:
            best, key = share, root
    return best, key


def _pitch_range_per_roll(features):
    """highest - lowest + 1 per roll, 0 for an empty one (int64 [n], on the features' device)"""
    f = features.to(torch.int64)
    return (f[:, 6] - f[:, 5] + 1) * f[:, 1]


def music_summary(stats) -> dict:
    """A MusicStats as numbers, with one read-back and float64 arithmetic on the host: ``rolls``, ``empty_roll_rate``,
    ``notes_per_roll``, ``note_density`` (cells / (rolls h w)), ``mean_duration`` (cells / notes, in steps), ``mean_polyphony``
    (cells / sounding steps), ``empty_step_rate`` (the share of time steps with no cell), ``used_pitches`` and ``pitch_range``
    (highest - lowest + 1), both means over the non-empty rolls; the normalised distributions ``pitch_class`` (of cells),
    ``pitch_class_onsets`` (of notes), ``duration`` and ``ioi`` (12 buckets, bucket b holding lengths / gaps in [2^b, 2^(b+1)), the
    last everything from 2048) and ``polyphony`` (steps with k = 0..14 cells, the last k >= 15) as lists; ``pitch_class_entropy``
    in bits; ``scale_consistency``, the largest share of cells whose pitch class lies in a major scale over the 12 roots, and
    ``key``, the lowest root that reaches it (-1 without cells).  A ratio with a zero denominator is nan."""
    totals = stats["totals"]
    host = torch.cat([totals.reshape(-1), _pitch_range_per_roll(stats["features"]).sum().reshape(1)]).cpu().tolist()
    t, range_sum = host[:MUSIC_FEATURES], host[MUSIC_FEATURES]
    col = lambda name: t[MUSIC_COLUMNS[name]]
    rolls, nonempty, cells, notes = t[0], t[1], t[2], t[3]
    poly = col("polyphony")
    out = {"rolls": rolls, "empty_roll_rate": _ratio(rolls - nonempty, rolls), "notes_per_roll": _ratio(notes, rolls),
           "note_density": _ratio(cells, rolls * stats["height"] * stats["width"]), "mean_duration": _ratio(cells, notes),
           "mean_polyphony": _ratio(cells, t[7]), "empty_step_rate": _ratio(poly[0], sum(poly)),
           "used_pitches": _ratio(t[4], nonempty), "pitch_range": _ratio(range_sum, nonempty)}
    for name, source in MUSIC_DISTRIBUTIONS.items():
        out[name] = _normalised(col(source))
    p = out["pitch_class"]
    out["pitch_class_entropy"] = -sum(v * math.log2(v) for v in p if v > 0) if cells else _NAN
    out["scale_consistency"], out["key"] = _scale_consistency(col("pc_cells"))
    return out


def _js_and_overlap(a, b):
    """(Jensen-Shannon divergence in bits, sum of min(p, q)) of two lists of counts; (nan, nan) if either is empty"""
    sa, sb = sum(a), sum(b)
    if not sa or not sb:
        return _NAN, _NAN
    js = overlap = 0.0
    for ca, cb in zip(a, b):
        p, q = ca / sa, cb / sb
        m = 0.5 * (p + q)
        # (each bin's share of the divergence is >= 0: nothing cancels between bins)
        js += (0.5 * p * math.log2(p / m) if p > 0 else 0.0) + (0.5 * q * math.log2(q / m) if q > 0 else 0.0)
        overlap += min(p, q)
    return js, overlap


def _wasserstein1(x, y):
    """sum over integers v of |F_x(v) - F_y(v)| for two host int64 vectors of non-negative values; nan if either is empty"""
    if not x.numel() or not y.numel():
        return _NAN
    size = int(max(x.max(), y.max())) + 1
    fx = torch.bincount(x, minlength=size).cumsum(0).double() / x.numel()
    fy = torch.bincount(y, minlength=size).cumsum(0).double() / y.numel()
    return float((fx - fy).abs().sum())


def _music_host(stats):
    """One read-back of what compare_music needs: (totals as a list, the per-roll scalars as a host int64 [5, n] tensor)"""
    f = stats["features"].to(torch.int64)
    per_roll = torch.stack([f[:, 3], f[:, 2], f[:, 4], _pitch_range_per_roll(stats["features"]), f[:, 9]]).reshape(-1)
    host = torch.cat([stats["totals"].reshape(-1), per_roll]).cpu()
    return host[:MUSIC_FEATURES].tolist(), host[MUSIC_FEATURES:].reshape(len(MUSIC_SCALARS), -1)


def compare_music(a, b) -> dict:
    """How far two sets of rolls are apart as music (two MusicStats; one read-back each).  For each distribution of music_summary
    (``pitch_class``, ``pitch_class_onsets``, ``duration``, ``polyphony``, ``ioi``): ``js_<name>``, the Jensen-Shannon divergence in
    bits (0 identical, 1 disjoint), and ``overlap_<name>`` = sum of min(p, q); both nan when either side has no count.  For each
    per-roll number (``notes``, ``cells``, ``used_pitches``, ``pitch_range``, ``max_polyphony``; an empty roll counts with 0):
    ``mean_<name>_a``, ``mean_<name>_b`` and ``w1_<name>``, the Wasserstein-1 distance of the two empirical distributions (the sum
    over integers v of |F_a(v) - F_b(v)|); nan for a side without rolls.  And ``scale_consistency_a`` / ``_b``."""
    (ta, ra), (tb, rb) = _music_host(a), _music_host(b)
    out = {}
    for name, source in MUSIC_DISTRIBUTIONS.items():
        out[f"js_{name}"], out[f"overlap_{name}"] = _js_and_overlap(ta[MUSIC_COLUMNS[source]], tb[MUSIC_COLUMNS[source]])
    for i, name in enumerate(MUSIC_SCALARS):
        out[f"mean_{name}_a"] = _ratio(int(ra[i].sum()), ra.shape[1])
        out[f"mean_{name}_b"] = _ratio(int(rb[i].sum()), rb.shape[1])
        out[f"w1_{name}"] = _wasserstein1(ra[i], rb[i])
    out["scale_consistency_a"] = _scale_consistency(ta[MUSIC_COLUMNS["pc_cells"]])[0]
    out["scale_consistency_b"] = _scale_consistency(tb[MUSIC_COLUMNS["pc_cells"]])[0]
    return out


def sample_music_stats(model, dataset, num_samples, *, temperature=1.0, seed=None, prior=None, pitch_offset=0, batch_size=256,
                       **note_kwargs) -> dict:
    """Does what the model generates behave like the training set as music?  ``model.sample_notes(num_samples, temperature=...,
    seed=..., cleaned=True, **note_kwargs)`` (``prior``: a ``mixture.LatentMixture`` to draw the latents from), music_statistics of
    the cleaned planes and of ``dataset`` (a ``PianorollDataset`` with "bits" storage on the device, of the model's height).  A
    dataset whose rolls are wider than the model's input is reduced to the centre window of the model's width first, in batches
    of ``batch_size`` through ``data.gather_rolls`` and ``binarize_rolls`` into a MusicStatsAccumulator.  Returns
    ``{"samples": music_summary, "dataset": music_summary, "gap": compare_music(samples, dataset)}``."""
    from .data import PianorollDataset, gather_rolls
    if not isinstance(dataset, PianorollDataset):
        raise TypeError("dataset must be a PianorollDataset")
    if dataset.storage != "bits":
        raise ValueError(f"the dataset must have 'bits' storage, got {dataset.storage!r}")
    if dataset.pinned or not dataset.data.is_cuda:
        raise ValueError("the dataset must be on the device, not in pinned host memory")
    size = int(model.img_size)
    if dataset.height != size or dataset.width < size:
        raise ValueError(f"the dataset's rolls are {dataset.height}x{dataset.width}, the model's {size}x{size}")
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size}")
    off = _music_pitch_offset(pitch_offset)
    if prior is not None:
        note_kwargs = dict(note_kwargs, prior=prior)
    notes = model.sample_notes(int(num_samples), temperature=temperature, seed=seed, cleaned=True, **note_kwargs)
    samples = music_statistics(notes["cleaned"], pitch_offset=off)
    if dataset.width == size:
        data = music_statistics(dataset, pitch_offset=off)
    else:
        acc = MusicStatsAccumulator(off)
        for first in range(0, len(dataset), int(batch_size)):
            acc.update(gather_rolls(dataset.data, dataset.kind, size, first=first, batch=min(int(batch_size), len(dataset) - first),
                                    crop_mode=_lib.CROP_CENTRE))
        data = acc.compute()
    return {"samples": music_summary(samples), "dataset": music_summary(data), "gap": compare_music(samples, data)}


def evaluate(dataloader, model, device, partition_name="Val", verbosity=1, *, nll_samples=0, latent_rolls=0, note_thresholds=None,
             note_events=None, music_stats=False, attributes=False, infill_span=None):
    """nll_samples = K > 0 adds ``nll`` (mean over the samples of -log p(x), importance-weighted with K draws) and ``elbo``
    (mean per-sample ELBO), both in nats per roll (VanillaVAE.log_likelihood); 0 leaves keys, values and printout as the
    reference has them.  latent_rolls = R > 0 keeps the eval forward's own mu / log_var of the first R rolls (loader order)
    and adds ``kl``, ``mi``, ``tc``, ``dwkl`` (nats) and ``active_units`` from latent_statistics on them (default draws and
    seed); 0 leaves everything as it is.  note_thresholds = a float or up to 8 of them routes every reconstruction reduction of
    the pass through one ReconMetricsAccumulator (one HIP pass per batch, nothing read back until the end; ``mse``, ``mae`` and the
    printed ranges come from it) and adds ``bce`` (nats per cell, the ELBO's reconstruction term), ``precision``, ``recall``, ``f1``
    (percent, a note being a cell >= 0.5 in the stimulus and >= note_thresholds[0] in the output), ``note_density`` (percent) and,
    with more than one threshold, ``best_f1`` (percent) and the ``best_threshold`` that gives it; None leaves everything as it is.
    ``bce`` is the UNWEIGHTED term whatever the model's ``pos_weight`` is (as ``nll`` / ``elbo`` are the unweighted Bernoulli), so
    runs trained with different weights stay comparable.
    note_events = a dict of ``generation.extract_notes`` keywords (onset_threshold, sustain_threshold, min_duration, max_gap) plus
    ``onset_tolerance`` (default 1) and ``target_threshold`` (default 0.5) extracts, for every batch, the note events of the
    reconstruction with those keywords and of the stimuli by plain thresholding at ``target_threshold``, matches them
    (note_event_metrics) and adds ``notes_pred``, ``notes_true``, ``matched`` (counts over the pass) and ``note_precision``,
    ``note_recall``, ``note_f1`` (fractions); None leaves results and launches as they are.
    music_stats = True accumulates the musical statistics (music_statistics, cut at 0.5) of the reconstructions and of the stimuli
    during the pass, two library calls per batch and nothing read back until the end, and adds the keys of
    ``compare_music(reconstructions, stimuli)`` prefixed ``music_``; False leaves results and launches as they are.
    attributes = True keeps the eval forward's own means and the attribute counters of the stimuli (roll_attributes, cut at the
    model's ``attr_threshold``; the first 65536 rolls) on the device and adds the Kendall tau-b ``attr_tau_<name>`` between attribute
    and latent dimension for every pair of ``model.attr_reg`` - or, when that is None, for all seven attributes, each against the
    dimension whose |tau| is largest (NaN when every dimension is constant); False leaves results and launches as they are.
    infill_span = (t0, t1) runs, for every batch, ``generation.infill`` on the stimuli - a second eval pass on the batch with those
    columns zeroed, decoded from the posterior mean, so no noise is drawn and every other result keeps its bits - scores the span's
    columns against the stimuli (infill_metrics, both cut at 0.5) and adds ``infill_f1``, ``infill_precision`` and
    ``infill_recall`` (percent); None leaves results and launches as they are.
    Under torch.distributed each rank reports its own shard."""
    if note_events is not None:
        from .generation import extract_notes
        ne_kw = dict(note_events)
        ne_tol, ne_tt = ne_kw.pop("onset_tolerance", 1), ne_kw.pop("target_threshold", 0.5)
        unknown = set(ne_kw) - {"onset_threshold", "sustain_threshold", "min_duration", "max_gap"}
        if unknown:
            raise ValueError(f"note_events has unknown keys {sorted(unknown)}")
        ne_counts = [0, 0, 0]
    notes = None if note_thresholds is None else ReconMetricsAccumulator(note_thresholds, device=device)
    music = (MusicStatsAccumulator(), MusicStatsAccumulator()) if music_stats else None
    attr_mu, attr_counters, attr_n = [], [], 0
    infill_acc = None
    if infill_span is not None:
        from .generation import checked_time_span, infill
        if not isinstance(infill_span, (tuple, list)) or len(infill_span) != 2:
            raise ValueError(f"infill_span must be a pair (t0, t1), got {infill_span!r}")
        it0, it1 = checked_time_span(infill_span[0], infill_span[1], getattr(model, "img_size", infill_span[1]))
        infill_acc = ReconMetricsAccumulator((0.5,), device=device)
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
        if attributes and attr_n < _lib.ATTR_MAX_POINTS:
            k = min(_lib.ATTR_MAX_POINTS - attr_n, stimuli.shape[0])
            attr_mu.append(output["encoded"]["mu"][:k].detach().float().clone())
            attr_counters.append(roll_attributes(stimuli[:k].float(), getattr(model, "attr_threshold", 0.5)))
            attr_n += k
        rec = output["output"]
        if infill_acc is not None:      # (after everything that reads this batch's forward out of the model)
            clean = stimuli if stimuli.dtype == torch.float32 else stimuli.float()
            infill_acc.update(infill(model, clean, it0, it1)[1][..., it0:it1], clean[..., it0:it1])
        if music is not None:
            music[0].update(rec.float())
            music[1].update(stimuli.float())
        if note_events is not None:
            got = extract_notes(rec, **ne_kw)
            want = extract_notes(stimuli.float().contiguous(), onset_threshold=ne_tt)
            for k, c in enumerate(_count_note_matches(_host_events(got), _host_events(want), int(ne_tol))):
                ne_counts[k] += c
        if notes is not None:
            notes.update(rec, stimuli if stimuli.dtype == torch.float32 else stimuli.float())
            n_seen += stimuli.shape[0]
            continue
        d = (rec - stimuli).double()
        se += (d * d).sum()
        ae += d.abs().sum()
        n_elem += d.numel()
        n_seen += stimuli.shape[0]
        stim_min, stim_max = min(stim_min, float(stimuli.min())), max(stim_max, float(stimuli.max()))
        rec_min, rec_max = min(rec_min, float(rec.min())), max(rec_max, float(rec.max()))
    if notes is not None:
        nm = notes.compute()
        (stim_min, stim_max), (rec_min, rec_max) = nm["target_range"], nm["xhat_range"]
        if not nm["count_cells"]:
            stim_min, stim_max, rec_min, rec_max = float("inf"), float("-inf"), float("inf"), float("-inf")
    if verbosity >= 1:
        print(f"input has range  [{stim_min:.03f}, {stim_max:.03f}]")
        print(f"output has range [{rec_min:.03f}, {rec_max:.03f}]")
    results = {"count": n_seen}
    # F.cross_entropy(reconstruction, stimuli) over the single channel C=1 is identically 0 (evaluation.py:66)
    results["cross-entropy"] = 0.0
    if notes is None:
        results["mse"] = 100.0 * float(se) / max(n_elem, 1)
        results["mae"] = 100.0 * float(ae) / max(n_elem, 1)
    else:
        results["mse"], results["mae"], results["bce"] = 100.0 * nm["mse"], 100.0 * nm["mae"], nm["bce"]
        for k in ("precision", "recall", "f1"):
            results[k] = 100.0 * nm[k][0]
        results["note_density"] = 100.0 * nm["note_density"]
        if len(notes.thresholds) > 1:
            best = max(range(len(notes.thresholds)), key=lambda i: nm["f1"][i])     # the first of equals
            results["best_f1"], results["best_threshold"] = 100.0 * nm["f1"][best], notes.thresholds[best]
    if nll_samples:
        results["nll"] = float(nll_sum) / max(n_seen, 1)
        results["elbo"] = float(elbo_sum) / max(n_seen, 1)
    if latent_rolls and lat_n:
        ls = latent_statistics(torch.cat(lat_mu), torch.cat(lat_lv))
        for k in ("kl", "active_units", "mi", "tc", "dwkl"):
            results[k] = ls[k] if k == "active_units" else float(ls[k])
    if note_events is not None:
        results.update(note_event_ratios(*ne_counts))
    if music is not None and n_seen:
        results.update({f"music_{k}": v for k, v in compare_music(music[0].compute(), music[1].compute()).items()})
    if attributes and attr_n:
        reg = getattr(model, "attr_reg", None)
        names = list(reg) if reg is not None else list(ATTRIBUTE_NAMES)
        tau = attribute_correlation(torch.cat(attr_mu), torch.cat(attr_counters), names)
        for k, name in enumerate(names):
            if reg is not None:
                results[f"attr_tau_{name}"] = float(tau[k, reg[name]])
            else:
                mag = torch.nan_to_num(tau[k].abs(), nan=-1.0)
                results[f"attr_tau_{name}"] = float(tau[k, int(mag.argmax())])
    if infill_acc is not None:
        im = infill_acc.compute()
        for k in ("f1", "precision", "recall"):
            results[f"infill_{k}"] = 100.0 * im[k][0]
    if verbosity >= 1:
        print(f"\n{partition_name} evaluation results:")
        for k, v in results.items():
            if k.startswith("music_") or k.startswith("attr_tau_"):
                print(f"  {k + ' ':.<36s} {v:9.5f}")
            elif k in ("note_precision", "note_recall", "note_f1"):
                print(f"  {k + ' ':.<24s} {100.0 * v:6.2f} %")
            elif "count" in k or k == "active_units" or k in ("notes_pred", "notes_true", "matched"):
                print(f"  {k + ' ':.<21s}{v:7d}")
            elif "entropy" in k or k == "bce":
                print(f"  {k + ' ':.<24s} {v:9.5f} nat")
            elif k == "best_threshold":
                print(f"  {k + ' ':.<24s} {v:9.5f}")
            elif k in ("nll", "elbo", "kl", "mi", "tc", "dwkl"):
                print(f"  {k + ' ':.<24s} {v:9.3f} nat")
            else:
                print(f"  {k + ' ':.<24s} {v:6.2f} %")
    return results
