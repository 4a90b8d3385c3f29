"""Dict shapes returned by the model (mirror of the reference's types_helpers.py:15-37)."""
from __future__ import annotations

from typing import TypedDict

from torch import Tensor


class EncoderOutput(TypedDict):
    mu: Tensor
    log_var: Tensor
    pre_latents: Tensor


class ModelOutput(TypedDict):
    output: Tensor
    input: Tensor
    encoded: EncoderOutput
    latents: Tensor


class LossOutput(TypedDict):
    loss: Tensor
    reconstruction_loss: Tensor
    kld_loss: Tensor


class LikelihoodOutput(TypedDict):
    log_likelihood: Tensor    # [B] float64: importance-weighted estimate of log p(x) (nats)
    elbo: Tensor              # [B] float64: per-sample evidence lower bound (nats)
    log_weights: Tensor       # [K, B] float64: log p(x|z_k) + log p(z_k) - log q(z_k|x)


class LatentStatsOutput(TypedDict):
    kl: Tensor                # 0-d float64: mean KL(q(z|x) || N(0, I)) (nats)
    mi: Tensor                # 0-d float64: mutual information I(x;z) under the aggregate posterior (nats)
    tc: Tensor                # 0-d float64: total correlation of the aggregate posterior (nats)
    dwkl: Tensor              # 0-d float64: dimension-wise KL, sum_d KL(q(z_d) || N(0, 1)) (nats); kl = mi + tc + dwkl
    active_units: int         # #{d : var_mu[d] > active_threshold}
    kl_per_dim: Tensor        # [L] float64
    var_mu: Tensor            # [L] float64: population variance over the rolls of mu_d
    dwkl_per_dim: Tensor      # [L] float64
    log_qz: Tensor            # [S, N] float64: log q(z) at each draw
    log_qz_dims: Tensor       # [S, N, L] float64: log q(z_d) at each draw


class ReconMetricsOutput(TypedDict):
    se: Tensor                # 0-d float64: sum over cells of (xhat - target)^2 (the f32 difference, widened)
    ae: Tensor                # 0-d float64: sum of |xhat - target|
    bce: Tensor               # 0-d float64: sum of the ELBO's BCE term (nats)
    n_cells: Tensor           # 0-d int64
    positives: Tensor         # 0-d int64: true notes (target >= target_threshold)
    tp: Tensor                # [T] int64: true and predicted (xhat >= thresholds[t])
    fp: Tensor                # [T] int64: predicted, not true
    fn: Tensor                # [T] int64: true, not predicted
    xhat_range: Tensor        # [2] float64: min, max
    target_range: Tensor      # [2] float64: min, max
    roll_se: Tensor           # [N] float64
    roll_ae: Tensor           # [N] float64
    roll_bce: Tensor          # [N] float64
    roll_positives: Tensor    # [N] int64
    roll_tp: Tensor           # [N, T] int64
    roll_fp: Tensor           # [N, T] int64


class NearestRolls(TypedDict):
    index: Tensor             # [Q, k] int64: the neighbours ascending by (distance, index); -1 where none is left
    distance: Tensor          # [Q, k] int32: min over the shift window of popcount(q XOR shifted roll); -1 in empty slots
    shift: Tensor             # [Q, k, 2] int32: (dy, dt) of the lowest-ranked shift that reaches the distance
    intersection: Tensor      # [Q, k] int32: popcount(q AND shifted roll) at that shift
    query_cells: Tensor       # [Q] int32: popcount(q)
    neighbour_cells: Tensor   # [Q, k] int32: cells of the shifted neighbour, d + 2 * intersection - query_cells (0 in empty slots)
    jaccard: Tensor           # [Q, k] float64: intersection / (d + intersection); 1.0 where both are empty, nan in empty slots


class NoteEvents(TypedDict):
    events: Tensor            # [N, 4] int32: (roll, pitch, onset, duration), ascending by (roll, pitch, onset)
    peaks: Tensor             # [N] float32: the largest input value over the note's cells (NaNs skipped), exact
    offsets: Tensor           # [n + 1] int64: roll r's events are events[offsets[r]:offsets[r + 1]]
    cleaned: Tensor | None    # [n, h, w/8] uint8: the kept cells as bit planes, numpy.packbits order
    total: Tensor             # 0-d int64 view of offsets[n]: the number of events, whatever the capacity


class MusicStats(TypedDict):
    features: Tensor          # [n, 76] int32: one row of counts per roll (include/vae_music.h has the table)
    totals: Tensor            # [76] int64: the column sums; `lowest` the minimum over non-empty rolls, `highest` / `max_polyphony` maxima
    columns: dict             # name -> slice of the 76 columns (evaluation.MUSIC_COLUMNS)
    height: int               # pitch rows of a roll
    width: int                # time steps of a roll
    pitch_offset: int         # the pitch of row 0: row p has pitch class (p + pitch_offset) mod 12
