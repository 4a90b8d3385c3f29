/* C ABI of the corruption behind the denoising / infilling objective (libvae_step_gfx950.so, beside include/vae_step.h): the encoder
 * sees a corrupted roll, the reconstruction term is taken against the clean one (vae_set_recon_target in vae_step.h; Vincent et al.
 * 2008, "Extracting and Composing Robust Features with Denoising Autoencoders"; Im et al. 2017, "Denoising Criterion for Variational
 * Auto-Encoding Framework").  Two entry points: the corruption of a float32 batch in one launch, and the time spans it draws.
 *
 * Conventions and the stream contract are those of vae_step.h: plain device pointers owned by the caller, work ordered on the
 * explicit stream (the last argument), nothing read back, 0 on success or -1 with "<entry point>: <reason>" in vae_last_error()
 * before anything is enqueued.  No entry point synchronises with the host, none uses an atomic, and every output bit is a function
 * of the arguments: repeated calls give identical bits.
 *
 * THE DRAWS come from the counter generator of vae_step.h, u(i, s) = counter_uniform(i, seed, s) in [0, 1), f64.  Roll b has the
 * counter k = counter0 + b * counter_stride; all counter arithmetic is modulo 2^64. */
#ifndef VAE_DENOISE_H
#define VAE_DENOISE_H
#include <stdint.h>
#include "vae_step.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VAE_DENOISE_STREAM_DROP 902
#define VAE_DENOISE_STREAM_SPAN 903
#define VAE_DENOISE_STREAM_ADD 904
#define VAE_DENOISE_MAX_ROWS (1 << 20)
#define VAE_DENOISE_MAX_COLS (1 << 20)

/* out [n][h][w] f32 = the corruption of clean [n][h][w] f32 (h pitch rows by w time columns: what a training step reads); the two
 * must not overlap.  A cell is ON iff value >= threshold, float32 against float32 (a NaN is off).  In this order:
 *   1. NOTE DROPOUT (stream 902).  A note is a maximal run of ON cells along time within one pitch row (vae_extract_notes with plain
 *      thresholding).  The run [t0, t1) of row p is dropped iff u((k*h + p)*w + t0, 902) < p_drop: all its cells become 0.f.  Cells of
 *      kept notes and OFF cells keep their value, so a velocity roll stays one.
 *   2. TIME-SPAN MASK (stream 903).  With spans == NULL and span_max > 0:
 *          len = span_min + (int)(u(2k, 903) * (span_max - span_min + 1)),   s0 = (int)(u(2k + 1, 903) * (w - len + 1));
 *      with spans [n][2] int32 given, (s0, len) = spans[b] whatever span_min / span_max are, intersected with the roll by the
 *      kernel: columns max(s0, 0) <= t < min(s0 + len, w) (64-bit arithmetic; nothing for len <= 0), so no address outside the
 *      batch is formed for any entry.  Those columns of every row become 0.f.  spans == NULL and span_max == 0: no span.
 *   3. SPURIOUS CELLS (stream 904).  A cell (p, t) that is OFF in clean and outside the span becomes add_value iff
 *      u((k*h + p)*w + t, 904) < p_add.
 * A probability of 0 draws nothing; with all three off out is a copy of clean, bit for bit (NaN payloads included).
 *   hidden [n][h][w/8] uint8, or NULL: numpy.packbits order (column 8j is bit 7 of byte j); a bit is set exactly where out differs
 *      from clean in ON / OFF state, or the cell lies inside the span - the region infilling is scored on.
 * Any h in 1..2^20 and any w in 8..2^20 that is a multiple of 8; n == 0 returns 0 and launches nothing.
 * Refused: null clean or out; clean, out and hidden overlapping one another; n < 0; h or w outside their range, w not a multiple of 8,
 * n * h * w beyond 2^46; p_drop or p_add outside [0, 1] or not finite; span_min < 0, span_min > span_max, span_max > w; threshold or
 * add_value not finite; clean or out not 16-byte, spans not 4-byte aligned. */
int vae_denoise_corrupt(const float* clean, float* out, uint8_t* hidden, int64_t n, int h, int w, float threshold, double p_drop,
                        int span_min, int span_max, double p_add, float add_value, const int32_t* spans, uint64_t seed,
                        uint64_t counter0, uint64_t counter_stride, vae_stream_t stream);

/* spans [n][2] int32 = the (s0, len) vae_denoise_corrupt draws with these arguments and spans == NULL ((0, 0) when span_max == 0).
 * Refused: null spans; n < 0 or beyond 2^40; w outside 8..2^20 or not a multiple of 8; span_min < 0, span_min > span_max, span_max > w; spans not
 * 4-byte aligned.  n == 0 returns 0 and launches nothing. */
int vae_denoise_params(int32_t* spans, int64_t n, int w, int span_min, int span_max, uint64_t seed, uint64_t counter0,
                       uint64_t counter_stride, vae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
