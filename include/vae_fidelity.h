/* C ABI of the set-level fidelity metrics (libvae_step_gfx950.so, beside include/vae_step.h): what two sets of feature vectors -
 * the encodings of the training rolls and of generated rolls - have to do with each other, from their pairwise squared distances:
 * k-NN radii, ball membership and nearest neighbours (precision and recall of Kynkaanniemi et al. 2019, density and coverage of
 * Naeem et al. 2020) and sums of Gaussian kernel values (the kernel MMD^2 of Gretton et al. 2012).  The moments of the Frechet
 * distance need no entry point of their own: vae_mixture_mstep (include/vae_mixture.h) with one component, zero
 * log-responsibilities and reg_covar = 0 gives the f64 mean and the covariance about the mean of a set.
 *
 * Conventions and the stream contract are those of vae_step.h: plain device pointers owned by the caller, work ordered on the
 * explicit stream (the last argument), work space from the stream-ordered allocator, nothing read back, 0 on success or -1 with
 * "<entry point>: <reason>" in vae_last_error() before anything is enqueued.  No entry point synchronises with the host, and none
 * uses an atomic: every reduction runs in an order fixed by the shape and `splits`, so repeated calls give identical bits.
 *
 * Points are f32, row-major [n, D], D in 1..VAE_FID_MAX_DIM, set sizes in 1..2^22.  No byte outside the named buffers is
 * addressed (D needs no padding in the caller's memory).
 *
 * THE DISTANCE, one device function for the three entry points:  d2(a, b) = sum_d (a_d - b_d)^2, each difference formed in f32
 * and squared into the running f32 sum (one fused multiply-add per term), d = 0, 1, ..., D-1 in that order whatever the tile, the
 * lane, the split or the entry point.  So d2(a, b) has the same bits everywhere, d2(a, b) == d2(b, a), and it is within (D + 2) u
 * relative of the exact value (u = 2^-24).  Never the expanded |a|^2 + |b|^2 - 2ab, which cancels for close points.  A
 * non-finite coordinate gives what IEEE arithmetic gives: +inf, or NaN (inf - inf).  A NaN distance is never <= anything and is
 * never the nearest or among the k smallest; a +inf distance is never the nearest or among the k smallest either, but
 * +inf <= +inf holds for a count.
 *
 * splits: 0 lets the library choose from the shape; 1..VAE_FID_MAX_SPLITS cuts the reference set (x itself for
 * vae_fidelity_knn_radii, r, b) into that many contiguous index ranges, one grid row each, whose partial results a second launch
 * merges in split order.  (A range holds ceil(n / splits) references rounded up to a multiple of 4; the last ranges may be
 * empty.)  Integer and order-statistic outputs do not depend on splits; the f64 sums do in their last bits only: the f32 partial
 * sums inside them cover the same references whatever splits is.
 *
 * Refused by every entry point, in this order, before anything is enqueued: a null pointer among those named below; D outside
 * 1..128; a set size outside 1..2^22; splits outside 0..64; then what the entry point adds; then splits * queries beyond 2^26
 * (the partial results of a forced split); then a pointer that is not aligned to its element (4 bytes; 8 for f64).
 */
#ifndef VAE_FIDELITY_H
#define VAE_FIDELITY_H
#include <stdint.h>
#include "vae_step.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VAE_FID_MAX_DIM 128
#define VAE_FID_MAX_K 8
#define VAE_FID_MAX_BANDWIDTHS 8
#define VAE_FID_MAX_SPLITS 64
#define VAE_FID_MAX_POINTS (1 << 22)

/* radii2 [n]: the k-th smallest d2(x_i, x_j) over j != i.  The exclusion is by index, so a duplicate of x_i is a neighbour at
 * distance 0; this is the (k+1)-th smallest of row i with itself included, the radius of the published PRDC code.  +inf where
 * fewer than k finite distances exist.
 * Refused: null x or radii2; k outside 1..8; k >= n. */
int vae_fidelity_knn_radii(const float* x, int64_t n, int D, int k, int splits, float* radii2, vae_stream_t stream);

/* For every query q_i (m of them) against the references r_j (n of them):
 *   counts [m] int32, or null: the number of j with d2(q_i, r_j) <= radii2[j]; radii2 [n] f32 is read only for this;
 *   nearest [m] int32 and nearest_d2 [m] f32: the j of the smallest d2(q_i, r_j), the lowest j on a tie, and that distance; -1 and
 *   +inf when no distance is finite.
 * With exclude_same_index != 0 the pairs i == j are left out of both (q and r are then usually the same set).
 * Refused: null q, r, nearest or nearest_d2; counts without radii2. */
int vae_fidelity_balls(const float* q, int64_t m, const float* r, int64_t n, int D, const float* radii2, int exclude_same_index,
                       int splits, int32_t* counts, int32_t* nearest, float* nearest_d2, vae_stream_t stream);

/* sums [G + 1] f64 in one pass over the pairs (a_i, b_j), i < n, j < m:
 *   sums[g] = sum_ij exp(-gammas[g] * d2(a_i, b_j)) for g < G,   sums[G] = sum_ij d2(a_i, b_j),
 * with exclude_same_index != 0 without the pairs i == j.  gammas [G] f64 is a DEVICE pointer (bandwidths derived from an earlier
 * call's sums[G] need no host read); G in 0..8, G == 0 gives the distance sum alone and reads no gammas.  Each exponential is one
 * f32 hardware exponential of the base-2 pre-scaled exponent (the scale -gamma log2 e is applied as an f32 pair, so it adds one
 * rounding to the exponent): a kernel value e^-t is within (t (D + 3) + 4) u e^-t of exact.  A lane adds at most 64 kernel values
 * in f32; everything above that, and every distance of sums[G], is added in f64 in an order fixed by the shape and splits.
 * Non-finite distances propagate as IEEE arithmetic has them.
 * Refused: null a, b or sums; G outside 0..8; null gammas with G > 0. */
int vae_fidelity_kernel_sums(const float* a, int64_t n, const float* b, int64_t m, int D, const double* gammas, int G,
                             int exclude_same_index, int splits, double* sums, vae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
