"""Input and parameter regimes beyond the suite's defaults (binary pianorolls, `perturbed_params`): velocity-valued rolls with a
silent and a full image, and parameters shaped like a trained checkpoint's.  Plain helpers for tests/test_regimes_host.py (which
pins what they guarantee) and tests/test_regimes_gpu.py."""
import numpy as np

from oracle import vae_oracle as vo
from tests.util import perturbed_params

# (H, L, B, generalised): the smallest shapes that reach each kernel family - the reference-exact model, the tiled kernels, the
# three row-streaming kernels (128-pixel rows), partial latent tiles
SHAPES = [(32, 16, 6, False), (64, 16, 5, True), (128, 16, 3, True), (32, 3, 9, False)]
REGIMES = ("velocity", "trained", "velocity+trained")
X_SEED, P_SEED = 21, 41          # the seeds _layer_local_gaps uses for its default batch and parameters


def velocity_roll(B, H, seed, silent=(1,), full=(2,)):
    """A pianoroll with velocities: synth_pianoroll's lines times U(0.2, 1) per cell (values that no 16-bit type holds exactly),
    every 97th cell exactly 1.0, the images in `silent` all 0 and those in `full` all 1.  float64 holding float32 values.
    (Never every image silent: a batch of zeros has zero-variance channels, where the reference itself is ill-conditioned.)"""
    x = vo.synth_pianoroll(B, H, seed).astype(np.float64)
    x = x * np.random.default_rng(seed + 1000).uniform(0.2, 1.0, x.shape)
    x.reshape(-1)[::97] = 1.0
    for b in silent:
        x[b] = 0.0
    for b in full:
        x[b] = 1.0
    assert len(set(silent)) < B
    return x.astype(np.float32).astype(np.float64)


def trained_like_params(L, H, seed, gen):
    """`perturbed_params` pushed to where training takes a checkpoint: BatchNorm gammas of either sign over a wide range with one
    dead (exactly 0) channel per layer, betas that put whole channels on one LeakyReLU branch (+4 / -4), conv rows whose scales
    differ by 32x, fc_var biases down to -8 (collapsed latent dimensions), wide fc_mu biases and a strongly negative output bias."""
    p = perturbed_params(L, H, seed, gen)
    rng = np.random.default_rng(seed + 7)
    for k in p:
        if k.endswith(".1.weight"):
            n = p[k].shape[0]
            gamma = rng.uniform(0.3, 2.5, n) * np.where(rng.random(n) < 0.25, -1.0, 1.0)
            gamma[rng.integers(n)] = 0.0
            beta = 0.5 * rng.standard_normal(n)
            beta[0], beta[1] = 4.0, -4.0
            p[k], p[k[:-len("weight")] + "bias"] = gamma, beta
    for k in p:
        if p[k].ndim == 4:
            p[k] = p[k] * rng.choice([0.25, 1.0, 8.0], p[k].shape[0]).reshape(-1, 1, 1, 1)
    p["fc_var.bias"] = np.linspace(-8.0, 3.0, L)
    p["fc_mu.bias"] = 2.0 * rng.standard_normal(L)
    p["final_layer.3.bias"] = np.full(1, -3.0)
    return p


def regime_inputs(regime, H, L, B, gen, x_seed=X_SEED, p_seed=P_SEED):
    """(x, params) of a regime; "default" is what _layer_local_gaps builds on its own."""
    vel, trained = "velocity" in regime, "trained" in regime
    x = velocity_roll(B, H, x_seed) if vel else vo.synth_pianoroll(B, H, x_seed).astype(np.float64)
    p = trained_like_params(L, H, p_seed, gen) if trained else perturbed_params(L, H, p_seed, gen)
    return x, p


def regime_eps(L, B, x_seed=X_SEED):
    return vo.counter_normal(B * L, x_seed, 5).reshape(B, L).astype(np.float64)


def padding_mask(offs, sizes, total):
    """True on the elements of a flat buffer that belong to no tensor (each tensor is padded to a multiple of 64 floats)."""
    pad = np.ones(int(total), dtype=bool)
    for o, n in zip(offs, sizes):
        pad[o:o + n] = False
    return pad
