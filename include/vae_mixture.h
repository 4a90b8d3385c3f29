/* C ABI of the latent Gaussian mixture (libvae_step_gfx950.so, beside include/vae_step.h): ex-post density estimation on the
 * encodings of a trained VAE (Ghosh et al. 2020) - fit a mixture of K Gaussians to the posterior means of the training rolls on
 * the device and sample latents from it instead of from N(0, I).
 *
 * Conventions and the stream contract are those of vae_step.h: plain device pointers owned by the caller, work ordered on the
 * explicit stream (the last argument), work space from the stream-ordered allocator, nothing read back, 0 on success or a
 * negative code with the message in vae_last_error().  No entry point synchronises with the host, and none uses an atomic:
 * every reduction runs in an order that depends on the shape only, so repeated calls give identical bits.
 *
 * The mixture: weights [K], means [K, L] and covariances, all f64.  kind VAE_MIXTURE_FULL: covariances [K, L, L], the lower
 * Cholesky factor C_k (S_k = C_k C_k^T) and its inverse W_k = C_k^-1 are [K, L, L] row-major with a zero upper triangle, L in
 * 1..128.  kind VAE_MIXTURE_DIAG: variances, their roots C and W = 1 / C are [K, L], L in 1..4096.  logdet[k] = -sum_d log C_k[d,d].
 * K in 1..64; n points with K <= n <= 2^30.  Points x are [n, L] f32.
 */
#ifndef VAE_MIXTURE_H
#define VAE_MIXTURE_H
#include <stdint.h>
#include "vae_step.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VAE_MIXTURE_FULL 0
#define VAE_MIXTURE_DIAG 1
#define VAE_MIXTURE_MAX_COMPONENTS 64
#define VAE_MIXTURE_MAX_DIM_FULL 128
#define VAE_MIXTURE_MAX_DIM_DIAG 4096
#define VAE_MIXTURE_STREAM_U 811   /* counter-generator stream of the uniforms that pick a draw's component (counter: the draw) */
#define VAE_MIXTURE_STREAM_EPS 812 /* counter-generator stream of a draw's normals (counter: draw * L + d) */

/* chol, winv (f64), winv32 (the f32 copy the pairwise kernels read) and logdet from the covariances, one workgroup per
 * component in f64.  status[k] (int32) is the 1-based index of the first pivot that is not > 0, else 0; such a pivot is taken
 * as 1, so the component's outputs stay finite. */
int vae_mixture_factor(const double* covariances, int K, int L, int kind, double* chol, double* winv, float* winv32,
                       double* logdet, int* status, vae_stream_t stream);

/* log p(x_n) under the mixture.  With y = W_k (x_n - m_k) (x - m_k formed directly in f32, the product on the exact-f32 MFMA) and
 * q = |y|^2:  log p_nk = log pi_k + logdet_k - L/2 log 2 pi - q / 2, constants and the logsumexp over k in f64.
 * log_prob [n] f64; log_resp [n, K] f32 = log p_nk - log_prob[n], or null; mean_log_prob: one f64, the mean of log_prob. */
int vae_mixture_log_prob(const float* x, int64_t n, int L, int K, int kind, const double* weights, const double* means,
                         const float* winv32, const double* logdet, double* log_prob, float* log_resp, double* mean_log_prob,
                         vae_stream_t stream);

/* One M-step from log responsibilities [n, K] f32: r = exp(log_resp), N_k = sum_n r_nk + 10 eps_f64, weights = N_k / n,
 * means = sum r x / N_k, then about the new mean covariances = sum r (x - m)(x - m)^T / N_k + reg_covar I (variances for
 * VAE_MIXTURE_DIAG).  Products are f32, accumulated in f32 over at most 64 points and in f64 beyond that. */
int vae_mixture_mstep(const float* log_resp, const float* x, int64_t n, int L, int K, int kind, double reg_covar, double* weights,
                      double* means, double* covariances, vae_stream_t stream);

/* n draws: u_i picks the first component whose f64 cumulative weight exceeds it (the last one takes the remainder), then
 * z_i = m_k + temperature * C_k eps_i.  u [n] f64 in [0, 1) and eps [n, L] f32 replace the counter generator (streams
 * VAE_MIXTURE_STREAM_U / _EPS with `seed`) when non-null.  z [n, L] f32, component [n] int32. */
int vae_mixture_sample(int64_t n, int L, int K, int kind, const double* weights, const double* means, const double* chol,
                       double temperature, uint64_t seed, const double* u, const float* eps, float* z, int* component,
                       vae_stream_t stream);

/* `iters` EM iterations (factor, E-step, M-step) from the state in weights / means / covariances, which are updated in place,
 * then one more factor so that chol / winv / winv32 / logdet belong to the final covariances.  ll_history [iters] f64: the mean
 * log-likelihood each E-step saw.  status [K] int32: the first failed pivot of any factorisation of the run, else 0. */
int vae_mixture_em(const float* x, int64_t n, int L, int K, int kind, int iters, double reg_covar, double* weights, double* means,
                   double* covariances, double* chol, double* winv, float* winv32, double* logdet, int* status,
                   double* ll_history, vae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
