"""ctypes binding of the C-ABI library (include/vae_step.h, include/vae_mixture.h for the latent mixture, include/vae_music.h
for the musical statistics, include/vae_fidelity.h for the set-level fidelity metrics, include/vae_attributes.h for the
attribute-regularised latents, include/vae_denoise.h for the denoising corruption and include/vae_average.h for the weight
averaging).

The product path has no CPU fallback: if the HIP library is missing this module
raises at import of the first symbol, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (VAE_STEP_LIB: a diagnostic build of the same library, e.g. `make STAMPS=1 OUT=... OBJD=...` - see tools/diag/gpu_stamps_deep.py)
LIB_PATH = os.environ.get("VAE_STEP_LIB") or os.path.join(_HERE, "lib", "libvae_step_gfx950.so")

NUM_PARAMS = 40
NUM_BN = 8
DTYPE_F32 = 0
DTYPE_BF16 = 1
DTYPE_F16 = 2
RECON_BCE = 0
RECON_MSE = 1
RECON_WBCE = 2      # include/vae_step.h: BCE with a positive-class weight (vae_set_recon_loss_ex)
POS_WEIGHT_MAX = 1024.0
KL_PLAIN = 0        # include/vae_step.h: VAE_KL_*
KL_FREE_BITS = 1
KL_CAPACITY = 2
KL_TC = 3
TC_MAX_BATCH = 4096   # include/vae_step.h: VAE_KL_TC, vae_total_correlation
RECON_METRICS_MAX_THRESHOLDS = 8   # include/vae_step.h: vae_recon_metrics
COMM_ID_BYTES = 128
ROLLS_BYTES, ROLLS_BITS, ROLLS_F32 = 0, 1, 2   # include/vae_step.h: the source kinds of vae_gather_rolls
CROP_RANDOM, CROP_CENTRE = 0, 1
AUGMENT_STREAM = 901                           # counter-generator stream of the augmentation draws
# csrc/augment.cuh, vae_gather_rolls: lanes per workgroup, the cap on workgroups, cells per lane, the most lanes along a row.  A
# workgroup is a tile of TX lanes along a row (the smallest power of two >= w/8, at most 64) by 256/TX rows; the grid's x walks the
# row tiles of one roll (capped), its y the samples (what the cap leaves, at least 1); past either, and past TX, a stride loop
GATHER_THREADS, GATHER_MAX_BLOCKS, GATHER_CELLS_PER_LANE, GATHER_MAX_ROW_LANES = 256, 2048, 8, 64
# csrc/nearest_rolls.cuh, vae_nearest_rolls: queries per workgroup and candidates per LDS tile (rolls of more than
# NEAREST_TILE_ROLL_BYTES take tiles of NEAREST_LARGE_TILE of either), the largest roll, the caps on (2P+1)(2T+1), k and splits
NEAREST_QUERY_TILE, NEAREST_CAND_TILE, NEAREST_TILE_ROLL_BYTES, NEAREST_LARGE_TILE = 16, 16, 4608, 8
NEAREST_MAX_ROLL_BYTES, NEAREST_MAX_SHIFTS, NEAREST_MAX_K, NEAREST_MAX_SPLITS = 8192, 1023, 32, 64
GRAD_CLIP_SCRATCH_BYTES = 8192  # include/vae_step.h: VAE_GRAD_CLIP_SCRATCH_BYTES
# include/vae_mixture.h: covariance kinds, the limits on (components, latent_dim) and the sampler's two counter-generator streams
MIXTURE_FULL, MIXTURE_DIAG = 0, 1
MIXTURE_MAX_COMPONENTS, MIXTURE_MAX_DIM_FULL, MIXTURE_MAX_DIM_DIAG = 64, 128, 4096
MIXTURE_STREAM_U, MIXTURE_STREAM_EPS = 811, 812
# include/vae_music.h: the width of a feature row; the limits of vae_music_roll_stats
MUSIC_FEATURES, MUSIC_MAX_ROLL_BYTES, MUSIC_MAX_PITCH_OFFSET = 76, 8192, 1 << 20
# include/vae_fidelity.h: the limits on the dimension, k, the bandwidths, the splits and a set's size
FID_MAX_DIM, FID_MAX_K, FID_MAX_BANDWIDTHS, FID_MAX_SPLITS, FID_MAX_POINTS = 128, 8, 8, 64, 1 << 22
# include/vae_attributes.h: the counters of a roll (in this order), the attributes made of them (name -> VAE_ATTR_* number) and the limits
ATTR_COUNTERS = ("cells", "notes", "used_pitches", "lowest", "highest", "sounding_steps", "onset_steps", "pitch_sum")
ATTRIBUTES = {"note_density": 0, "note_count": 1, "pitch_range": 2, "mean_pitch": 3, "polyphony": 4, "onset_steps": 5, "used_pitches": 6}
ATTR_MAX_PAIRS, ATTR_MAX_BATCH, ATTR_MAX_DIM, ATTR_MAX_ROWS, ATTR_MAX_CELLS, ATTR_MAX_POINTS = 8, 4096, 4096, 1024, 1 << 20, 65536
# include/vae_denoise.h: the counter-generator streams of note dropout, the time span and the spurious cells; the limits on h and w
DENOISE_STREAM_DROP, DENOISE_STREAM_SPAN, DENOISE_STREAM_ADD = 902, 903, 904
DENOISE_MAX_ROWS, DENOISE_MAX_COLS = 1 << 20, 1 << 20
# include/vae_average.h: the kinds of average; the bytes of the device state (int64 seen_step | int64 n_averaged | f64 last_weight | reserved)
AVG_EMA, AVG_EQUAL = 0, 1
AVG_STATE_BYTES = 32

PARAM_NAMES = (
    [f"encoder.{i}.{j}" for i in range(4) for j in ("0.weight", "0.bias", "1.weight", "1.bias")]
    + ["fc_mu.weight", "fc_mu.bias", "fc_var.weight", "fc_var.bias", "decoder_input.weight", "decoder_input.bias"]
    + [f"decoder.{i}.{j}" for i in range(3) for j in ("0.weight", "0.bias", "1.weight", "1.bias")]
    + ["final_layer.0.weight", "final_layer.0.bias", "final_layer.1.weight", "final_layer.1.bias",
       "final_layer.3.weight", "final_layer.3.bias"]
)
BN_NAMES = [f"encoder.{i}.1" for i in range(4)] + [f"decoder.{i}.1" for i in range(3)] + ["final_layer.1"]

_lib = None


class VaeLibError(RuntimeError):
    pass


def _sig(fn, res, args):
    fn.restype = res
    fn.argtypes = args


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VaeLibError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C torch_vae_amd/csrc`. There is no CPU fallback for the VAE step.")
    L = C.CDLL(LIB_PATH)
    p, i32, i64, u64, f32, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double
    f64p = C.POINTER(C.c_double)
    i64p = C.POINTER(C.c_int64)
    f32p = C.POINTER(C.c_float)
    _sig(L.vae_last_error, C.c_char_p, [])
    _sig(L.vae_abi_version, i32, [])
    _sig(L.vae_param_layout, i32, [i32, i32, i32, i64p, i64p, i64p])
    _sig(L.vae_bn_layout, i32, [i64p, i64p, i64p])
    _sig(L.vae_create, p, [i32, i32, i32, i32, i32])
    _sig(L.vae_destroy, None, [p])
    _sig(L.vae_workspace_bytes, i64, [p])
    _sig(L.vae_forward, i32, [p, p, i32, p, p, p, p, u64, i32, p, p, p, p, p])
    _sig(L.vae_decode, i32, [p, p, i32, p, p, p, i32, p, p])
    _sig(L.vae_pre_latents, i32, [p, p, p])
    _sig(L.vae_last_eps, i32, [p, p, p])
    _sig(L.vae_loss, i32, [p, f32, p, p])
    _sig(L.vae_loss_deferred, i32, [p, f32, p, p])
    _sig(L.vae_elbo_generic, i32, [p, p, p, p, i64, i32, i32, f32, p, p, p, p, p])
    _sig(L.vae_elbo_generic_ex, i32, [p, p, p, p, i64, i32, i32, f32, i32, p, p, p, p, p])
    _sig(L.vae_set_recon_loss, i32, [p, i32])
    _sig(L.vae_set_recon_loss_ex, i32, [p, i32, f64])
    _sig(L.vae_set_recon_target, i32, [p, p])
    _sig(L.vae_set_kl_objective, i32, [p, i32, f64])
    _sig(L.vae_elbo_generic_kl, i32, [p, p, p, p, i64, i32, i32, f32, i32, i32, f64, p, p, p, p, p])
    _sig(L.vae_elbo_generic_w, i32, [p, p, p, p, i64, i32, i32, f32, i32, f64, i32, f64, p, p, p, p, p])
    _sig(L.vae_kl_per_dim, i32, [p, p, p])
    _sig(L.vae_total_correlation, i32, [p, p, p, i32, i32, p, p, p, p])
    _sig(L.vae_last_total_correlation, i32, [p, p, p])
    _sig(L.vae_log_likelihood, i32, [p, p, i32, p, p, i32, i32, p, u64, p, p, p, p])
    _sig(L.vae_latent_stats, i32, [p, p, i64, i32, i32, p, u64, p, p, p, p, p])
    _sig(L.vae_recon_metrics, i32, [p, p, i64, i64, f32p, i32, f32, p, p, p, p, i32, p])
    _sig(L.vae_backward, i32, [p, p, p, p, p, p, p, p, p, p, f32, i32, p])
    _sig(L.vae_backward_part, i32, [p, p, p, p, p, p, p, p, p, p, f32, i32, i32, p])
    _sig(L.vae_encode, i32, [p, p, i32, p, p, p, p, u64, i32, p, p, p, p])
    _sig(L.vae_backward_ex, i32, [p, p, p, p, p, p, p, p, p, p, f32, i32, p, p, p])
    _sig(L.vae_comm_stream, i32, [p, p, C.POINTER(C.c_void_p)])
    _sig(L.vae_comm_unique_id, i32, [p])
    _sig(L.vae_comm_init, i32, [p, i32, i32, p])
    _sig(L.vae_comm_world, i32, [p])
    _sig(L.vae_comm_destroy, i32, [p])
    _sig(L.vae_allreduce_grads, i32, [p, p, i32, i64p, i64p, i32, p])
    _sig(L.vae_broadcast_state, i32, [p, p, p, p, i32, p])
    _sig(L.vae_adamw_step, i32, [p, p, p, p, i32, i64p, i64p, f64p, f64p, f64, f64, f64, f32, i32, p])
    _sig(L.vae_grad_norm, i32, [p, i32, i64p, i64p, f32, p, p, p])
    _sig(L.vae_adamw_step_clipped, i32, [p, p, p, p, i32, i64p, i64p, f64p, f64p, f64, f64, f64, f32, f64, i32, p, p, p, p, p])
    _sig(L.vae_train_step, i32, [p, p, i32, p, p, p, p, p, p, p, u64, f32, i32, i64p, i64p, f64p, f64p, f64, f64, f64,
                                 i32, p, p, p, p, p, p])
    _sig(L.vae_train_step_fused, i32, [p, p, i32, p, p, p, p, p, p, p, u64, f32, i32, i64p, i64p, f64p, f64p, f64, f64, f64, f32,
                                       i32, i32, p, p, p, p, p, p])
    _sig(L.vae_train_step_fused_clipped, i32, [p, p, i32, p, p, p, p, p, p, p, u64, f32, i32, i64p, i64p, f64p, f64p, f64, f64, f64,
                                               f32, f64, i32, p, p, p, p, i32, p, p, p, p, p, p])
    _sig(L.vae_synth_pianoroll, i32, [p, i32, i32, u64, p])
    _sig(L.vae_expand_stimuli, i32, [p, i32, p, i64, p])
    _sig(L.vae_gather_rolls, i32, [p, i32, i64, i32, i32, p, i64, p, u64, u64, u64, i32, i32, i32, f32, p, i32, i32, p])
    _sig(L.vae_augment_params, i32, [p, i32, i32, i32, u64, u64, u64, i32, i32, i32, p])
    _sig(L.vae_extract_notes, i32, [p, i64, i32, i32, f32, f32, i32, i32, p, p, i64, p, p, p])
    _sig(L.vae_nearest_rolls, i32, [p, i32, p, i64, i32, i32, i32, i32, p, i32, i32, p, p, p, p, p, p])
    _sig(L.vae_profile, i32, [p, i32])
    _sig(L.vae_profile_report, i32, [p, C.c_char_p, i64])
    _sig(L.vae_profile_sequence, i32, [p, C.c_char_p, i64])
    _sig(L.vae_profile_timeline, i32, [p, C.c_char_p, i64])
    _sig(L.vae_debug_stamps, i32, [p, C.c_char_p, i32, p])
    _sig(L.vae_debug_tensor, i32, [p, i32, p, i64, p])
    _sig(L.vae_selftest_tr16, i32, [p])
    _sig(L.vae_set_option, i32, [p, C.c_char_p, i32])
    _sig(L.vae_option_info, i32, [i32, C.POINTER(C.c_char_p), C.POINTER(C.c_int)])
    # include/vae_mixture.h
    _sig(L.vae_mixture_factor, i32, [p, i32, i32, i32, p, p, p, p, p, p])
    _sig(L.vae_mixture_log_prob, i32, [p, i64, i32, i32, i32, p, p, p, p, p, p, p, p])
    _sig(L.vae_mixture_mstep, i32, [p, p, i64, i32, i32, i32, f64, p, p, p, p])
    _sig(L.vae_mixture_sample, i32, [i64, i32, i32, i32, p, p, p, f64, u64, p, p, p, p, p])
    _sig(L.vae_mixture_em, i32, [p, i64, i32, i32, i32, i32, f64, p, p, p, p, p, p, p, p, p, p])
    # include/vae_music.h
    _sig(L.vae_music_roll_stats, i32, [p, i64, i32, i32, i32, p, p, i32, p])
    # include/vae_fidelity.h
    _sig(L.vae_fidelity_knn_radii, i32, [p, i64, i32, i32, i32, p, p])
    _sig(L.vae_fidelity_balls, i32, [p, i64, p, i64, i32, p, i32, i32, p, p, p, p])
    _sig(L.vae_fidelity_kernel_sums, i32, [p, i64, p, i64, i32, p, i32, i32, i32, p, p])
    # include/vae_attributes.h (attr / dim: host arrays of int32)
    i32p = C.POINTER(C.c_int32)
    _sig(L.vae_attr_roll_counters, i32, [p, i64, i32, i32, f32, p, p])
    _sig(L.vae_attr_regularizer, i32, [p, i32, i32, p, i32, i32, i32p, i32p, f32, f32, p, p, p])
    _sig(L.vae_attr_concordance, i32, [p, i32, i32, p, i64, i32, i32p, p, p, p, p])
    # include/vae_denoise.h
    _sig(L.vae_denoise_corrupt, i32, [p, p, p, i64, i32, i32, f32, f64, i32, i32, f64, f32, p, u64, u64, u64, p])
    _sig(L.vae_denoise_params, i32, [p, i64, i32, i32, i32, u64, u64, u64, p])
    # include/vae_average.h
    _sig(L.vae_average_update, i32, [p, p, i64, f32, p, p, i64, f32, i32, f64, f64, p, p, p])
    _sig(L.vae_average_swap, i32, [p, p, i64, p, p, i64, p])
    _sig(L.vae_average_state_init, i32, [p, p, i64, p])
    _lib = L
    return L


EXPORTS = [
    "vae_last_error", "vae_abi_version", "vae_param_layout", "vae_bn_layout", "vae_create", "vae_destroy",
    "vae_workspace_bytes", "vae_forward", "vae_decode", "vae_pre_latents", "vae_last_eps", "vae_loss", "vae_loss_deferred", "vae_elbo_generic",
    "vae_set_recon_loss", "vae_set_recon_loss_ex", "vae_set_recon_target", "vae_elbo_generic_ex", "vae_set_kl_objective", "vae_elbo_generic_kl", "vae_elbo_generic_w", "vae_kl_per_dim", "vae_total_correlation", "vae_last_total_correlation", "vae_log_likelihood", "vae_latent_stats",
    "vae_recon_metrics",
    "vae_backward", "vae_backward_part", "vae_encode", "vae_backward_ex", "vae_comm_stream", "vae_comm_unique_id", "vae_comm_init", "vae_comm_world",
    "vae_comm_destroy", "vae_allreduce_grads", "vae_broadcast_state", "vae_adamw_step", "vae_train_step", "vae_train_step_fused",
    "vae_grad_norm", "vae_adamw_step_clipped", "vae_train_step_fused_clipped", "vae_synth_pianoroll", "vae_expand_stimuli", "vae_profile",
    "vae_profile_report", "vae_profile_sequence", "vae_profile_timeline", "vae_debug_stamps", "vae_debug_tensor",
    "vae_selftest_tr16", "vae_set_option", "vae_option_info", "vae_gather_rolls", "vae_augment_params",
    "vae_extract_notes", "vae_nearest_rolls",
]


# include/vae_mixture.h (a header of its own: EXPORTS above is exactly what include/vae_step.h declares)
MIXTURE_EXPORTS = ["vae_mixture_factor", "vae_mixture_log_prob", "vae_mixture_mstep", "vae_mixture_sample", "vae_mixture_em"]

# include/vae_music.h (its own header too)
MUSIC_EXPORTS = ["vae_music_roll_stats"]

# include/vae_fidelity.h (and this one)
FIDELITY_EXPORTS = ["vae_fidelity_knn_radii", "vae_fidelity_balls", "vae_fidelity_kernel_sums"]

# include/vae_attributes.h (and this one)
ATTR_EXPORTS = ["vae_attr_roll_counters", "vae_attr_regularizer", "vae_attr_concordance"]

# include/vae_denoise.h (and this one)
DENOISE_EXPORTS = ["vae_denoise_corrupt", "vae_denoise_params"]

# include/vae_average.h (and this one)
AVERAGE_EXPORTS = ["vae_average_update", "vae_average_swap", "vae_average_state_init"]


def check(rc: int, what: str = ""):
    if rc != 0:
        raise VaeLibError(f"{what}: {lib().vae_last_error().decode()}")


def param_layout(img_size: int, latent_dim: int, generalised: bool):
    offs = (C.c_int64 * NUM_PARAMS)()
    sizes = (C.c_int64 * NUM_PARAMS)()
    total = C.c_int64()
    rc = lib().vae_param_layout(img_size, latent_dim, int(generalised), offs, sizes, C.byref(total))
    if rc != 0:
        raise ValueError(lib().vae_last_error().decode())
    return list(offs), list(sizes), total.value


def bn_layout():
    offs = (C.c_int64 * NUM_BN)()
    ch = (C.c_int64 * NUM_BN)()
    total = C.c_int64()
    check(lib().vae_bn_layout(offs, ch, C.byref(total)), "vae_bn_layout")
    return list(offs), list(ch), total.value


def ptr(t):
    """Device pointer of a torch tensor (or 0 for None)."""
    return 0 if t is None else t.data_ptr()
