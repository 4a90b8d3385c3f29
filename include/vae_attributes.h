/* C ABI of the attribute-regularised latents (libvae_step_gfx950.so, beside include/vae_step.h): a latent dimension r is tied to a
 * musical attribute a of the roll - how dense, how wide in pitch, how busy in rhythm - by the in-batch loss of Pati & Lerch 2020
 * ("Attribute-based Regularization of Latent Spaces for VAEs"),
 *     L_r = mean_{i,j} | tanh(delta (z_i^r - z_j^r)) - sgn(a_i - a_j) |,
 * so that decoding along z^r turns the attribute up and down.  Three entry points: the integer counters of a float32 batch the
 * attributes are made of, the loss with its gradient on z, and the Kendall concordance sums that say how monotone a dimension is in
 * an attribute over a whole set.
 *
 * Conventions and the stream contract are those of vae_step.h: plain device pointers owned by the caller, work ordered on the
 * explicit stream (the last argument), work space from the stream-ordered allocator, nothing read back, 0 on success or -1 with
 * "<entry point>: <reason>" in vae_last_error() before anything is enqueued.  No entry point synchronises with the host and none
 * uses an atomic: integers are exact, and every floating-point sum runs in an order fixed by the shape, so repeated calls give
 * identical bits.
 *
 * THE COUNTERS of a roll, int32 [VAE_ATTR_COUNTERS], in this order:
 *     cells, notes, used_pitches, lowest, highest, sounding_steps, onset_steps, pitch_sum
 * the first seven as include/vae_music.h defines them (columns 2..8 of its feature row: a note is a maximal run of set cells along
 * time within one pitch row, lowest / highest are -1 / -1 for an empty roll), pitch_sum the sum of the row index over the set cells.
 *
 * THE ATTRIBUTES, f64, each at most one IEEE operation on the counters (so a CPU restatement has the same bits and the same signs):
 *     VAE_ATTR_CELLS        cells
 *     VAE_ATTR_NOTES        notes
 *     VAE_ATTR_PITCH_RANGE  highest - lowest + 1, 0 for an empty roll
 *     VAE_ATTR_MEAN_PITCH   pitch_sum / cells, -1.0 for an empty roll
 *     VAE_ATTR_POLYPHONY    cells / sounding_steps, 0 for an empty roll
 *     VAE_ATTR_ONSET_STEPS  onset_steps
 *     VAE_ATTR_USED_PITCHES used_pitches
 * sgn(x) = (x > 0) - (x < 0) throughout.  The latents handed to vae_attr_regularizer and vae_attr_concordance are to be finite.
 */
#ifndef VAE_ATTRIBUTES_H
#define VAE_ATTRIBUTES_H
#include <stdint.h>
#include "vae_step.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VAE_ATTR_COUNTERS 8
#define VAE_ATTR_CELLS 0
#define VAE_ATTR_NOTES 1
#define VAE_ATTR_PITCH_RANGE 2
#define VAE_ATTR_MEAN_PITCH 3
#define VAE_ATTR_POLYPHONY 4
#define VAE_ATTR_ONSET_STEPS 5
#define VAE_ATTR_USED_PITCHES 6
#define VAE_ATTR_COUNT 7
#define VAE_ATTR_MAX_PAIRS 8
#define VAE_ATTR_MAX_BATCH 4096
#define VAE_ATTR_MAX_DIM 4096
#define VAE_ATTR_MAX_ROWS 1024
#define VAE_ATTR_MAX_CELLS (1 << 20)
#define VAE_ATTR_MAX_POINTS 65536

/* counters [n][VAE_ATTR_COUNTERS] of the rolls [n][h][w] f32 (h pitch rows by w time columns: the batch a training step reads), in
 * one launch and one pass over the rolls.  A cell is set iff value >= threshold (generation.binarize_rolls' rule: a NaN is not set).
 * Any w >= 1; n == 0 returns 0 and launches nothing.  No byte outside rolls and counters is addressed.
 * Refused: null rolls or counters; n < 0; h outside 1..1024; w < 1; h * w above 2^20 (pitch_sum stays below 2^31); n * h * w beyond
 * 2^46; rolls or counters not 4-byte aligned. */
int vae_attr_roll_counters(const float* rolls, int64_t n, int h, int w, float threshold, int32_t* counters, vae_stream_t stream);

/* The regulariser of `npairs` (attribute, dimension) pairs on a batch: z [B][ldz] f32 (the first L columns of a row are the latent),
 * counters [B][8].  attr [npairs] and dim [npairs] are HOST arrays, read before the call returns.
 *   loss [1 + npairs] f64:  loss[1 + k] = 1/B^2 sum_{i,j} | tanh(delta (z_i - z_j)) - sgn(a_i - a_j) | in column dim[k] with attribute
 *                           attr[k] - all B^2 ordered pairs, the diagonal included, as F.l1_loss over the full matrices;
 *                           loss[0] = their unweighted sum.
 *   g_z [B][L] f32, or null: weight * d loss[0] / d z, EVERY element written, zeros in the columns no pair names - the g_z of
 *                           vae_backward / vae_backward_part.  In column dim[k]:
 *                           g_i = weight (2 / B^2) sum_j sign(t_ij - s_ij) delta sech^2(delta (z_i - z_j)),  sign(0) = 0.
 * Each term is formed in f32 from e = exp(-2 |u|), u = delta (z_i - z_j) held as an f32 pair (the difference and the product without
 * their rounding errors, so that a saturated pair's 2 e^{-2|u|} keeps f32 accuracy down to the smallest normal f32; below that an
 * f32 term has none): |t| = tanh |u|, 1 - |t| = 2e / (1 + e), 1 + |t| = 2 / (1 + e), sech^2 = 4e / (1 + e)^2 - none of them through
 * 1 - t^2 or 1 - t, which cancel once a pair saturates; the sign of t - s is taken from the signs of u and s (|t| < 1 for every
 * finite u).  A lane adds its terms in f64, a row is 64 lanes merged by a butterfly,
 * the total a fixed tree over the rows.  The loss bits do not depend on whether g_z is given.
 * Refused: null z, counters, loss, attr or dim; B outside 1..4096; L outside 1..4096; ldz < L; npairs outside 1..8; an attribute
 * outside 0..6; a dim outside 0..L-1; a repeated dim; delta or weight not finite, delta <= 0; z, counters or g_z not 4-byte, loss not
 * 8-byte aligned. */
int vae_attr_regularizer(const float* z, int ldz, int L, const int32_t* counters, int B, int npairs, const int32_t* attr,
                         const int32_t* dim, float delta, float weight, double* loss, float* g_z, vae_stream_t stream);

/* Kendall concordance of every latent dimension with `nattr` attributes over a set: z [N][ldz] f32, counters [N][8], attr [nattr] a
 * HOST array.  Over the pairs i < j, in exact int64:
 *   S [nattr][L]     sum sgn(z_i^d - z_j^d) sgn(a_i - a_j)
 *   ties_z [L]       pairs with z_i^d == z_j^d
 *   ties_a [nattr]   pairs with a_i == a_j
 * (tau_b = S / sqrt((n0 - ties_z)(n0 - ties_a)), n0 = N (N - 1) / 2.)  N < 2 gives zeros.  z must be finite (a NaN compares as a tie).
 * Refused: null z, counters, attr, S, ties_z or ties_a; N outside 0..65536; L outside 1..4096; ldz < L; nattr outside 1..7; an
 * attribute outside 0..6; z or counters not 4-byte, S, ties_z or ties_a not 8-byte aligned. */
int vae_attr_concordance(const float* z, int ldz, int L, const int32_t* counters, int64_t N, int nattr, const int32_t* attr,
                         int64_t* S, int64_t* ties_z, int64_t* ties_a, vae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
