/* C ABI of the MI355X-native VanillaVAE training step (libvae_step_gfx950.so).
 *
 * The reference has no FFI / plugin interface: its hot path is the
 * Python call surface models.VanillaVAE.{forward,loss} + train.train_one_epoch,
 * dispatching to PyTorch ATen.  This library sits BENEATH that surface; each entry
 * point names the reference lines whose arithmetic it replaces.  Paths are relative
 * to /root/reference/midi_autoencoder.
 *
 * Conventions: plain pointers and sizes, no torch types.  All tensor memory
 * (parameters, gradients, optimiser state, inputs, outputs) is owned by the caller
 * (PyTorch's allocator) and borrowed for the call; only scratch is owned by the
 * context.  Work is ordered on the explicit hipStream_t (pass
 * torch.cuda.current_stream().cuda_stream): results of a call are visible to later
 * work on that stream, and a call sees everything enqueued on it before.  Inside
 * vae_forward / vae_backward the context also uses non-blocking side streams of its own
 * (weight packing, weight gradients); they are forked from and joined back into the
 * caller's stream with HIP events before the call returns, so the caller never has to
 * synchronise with them.  Functions return
 * 0 on success or a negative code, with the message in vae_last_error().  A context is
 * not re-entrant; use one per process / GPU.
 *
 * Work space "from the stream-ordered allocator": requests of up to 64 MiB share one block per
 * device and stream, which the library keeps for the life of the process and grows on demand
 * (calls on a stream run in stream order).  After the first call at a size such an entry point
 * allocates nothing and never makes the host wait.  Larger requests, a stream that is being
 * captured into a graph, and hipStreamPerThread are allocated and released on the stream per
 * call; outside a capture the host may then wait for an earlier release.
 *
 * A context holds at most ONE forward (vae_forward, a training step, vae_encode or vae_decode):
 * vae_loss*, vae_backward* and the read-back calls act on it, and the next forward replaces it.
 * A call refused for its arguments (null pointer, batch above max_batch) touches nothing: the
 * previous forward is still held.  A forward-type call that fails after it has started leaves
 * the context holding NO forward - what follows is refused until the next one succeeds.
 * Every forward also starts a new backward: vae_backward_part with part = 2 is refused unless
 * part 1 ran on the SAME forward, and a vae_loss_deferred request dies with its forward.
 */
#ifndef VAE_STEP_H
#define VAE_STEP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vae_ctx vae_ctx;
typedef void* vae_stream_t; /* hipStream_t */

#define VAE_NUM_PARAMS 40 /* tensors of VanillaVAE.state_dict() that are parameters */
#define VAE_NUM_BN 8
#define VAE_DTYPE_F32 0  /* f32 storage, f32-input MFMA: exact f32 FMA-chain arithmetic */
#define VAE_DTYPE_BF16 1 /* bf16 activation/weight storage, bf16 MFMA, f32 accumulate/statistics */
#define VAE_DTYPE_F16 2  /* f16 activation/weight storage, f16 MFMA, f32 accumulate; KL / BCE / BatchNorm statistics in
                          * f32 / f64 as in the other modes.  Stored gradients are scaled by a power of two chosen per
                          * forward (the BCE mean makes dL/dlogit ~ 1/(B*H*W), below the f16 range) and every parameter
                          * gradient is unscaled on output, so callers see ordinary gradients. */

const char* vae_last_error(void);
int vae_abi_version(void);

/* Flat parameter buffer layout.  Tensors appear in the reference's state_dict order
 * (models.py:41-82): encoder.{0..3}.{0.weight,0.bias,1.weight,1.bias}, fc_mu.{weight,bias},
 * fc_var.{weight,bias}, decoder_input.{weight,bias}, decoder.{0..2}.{...}, final_layer.{0.weight,
 * 0.bias,1.weight,1.bias,3.weight,3.bias}; each keeps the reference's own element layout
 * (Conv2d [Cout,Cin,3,3], ConvTranspose2d [Cin,Cout,3,3], Linear [out,in]).
 * generalised=0: flattened_size = 1024 (models.py:33,36; img_size must be 32).
 * generalised=1: flattened_size = 256*(img_size/16)^2 (not reference behaviour).
 * latent_dim: 1..4096; every size in that range runs on every path, anything else is refused here. */
int vae_param_layout(int img_size, int latent_dim, int generalised, int64_t* offsets /*[40]*/,
                     int64_t* sizes /*[40]*/, int64_t* total);
/* BatchNorm running statistics: one f32 buffer, per layer running_mean[C] then running_var[C]. */
int vae_bn_layout(int64_t* offsets /*[8]*/, int64_t* channels /*[8]*/, int64_t* total);

/* Replaces VanillaVAE.__init__'s device state (models.py:10-83): allocates scratch for
 * batches up to max_batch.  dtype: VAE_DTYPE_*. */
vae_ctx* vae_create(int img_size, int latent_dim, int max_batch, int dtype, int generalised);
void vae_destroy(vae_ctx* ctx);
/* bytes of device scratch held by the context */
int64_t vae_workspace_bytes(const vae_ctx* ctx);

/* VanillaVAE.forward (models.py:185-188): encode (:107-145), reparameterize (:177-183),
 * decode (:147-175); also accumulates the ELBO terms of VanillaVAE.loss (:208,:214) and the
 * reconstruction gradient so that vae_loss / vae_backward need no second pass.
 *   x [B,1,H,W] f32 in [0,1];  params: flat buffer (vae_param_layout)
 *   bn_running / num_batches_tracked[8]: updated when train!=0 (momentum 0.1, unbiased var)
 *   eps [B,L] f32: the torch.randn_like draw of models.py:182; NULL -> generated on device
 *       from the counter-based normal generator (seed, stream 5) that oracle/ restates
 *   train=0 uses running statistics (model.eval(), evaluation.py:42)
 *   train=2: a training forward whose standard-ELBO backward follows unconditionally (the fused step, train.py:634-650
 *       as one chain).  The library MAY then leave the output conv, sigmoid and BCE to vae_backward / vae_backward_part,
 *       where one kernel does that layer's forward and backward in a single pass over its input: xhat, the running
 *       statistics of final_layer's BatchNorm and the ELBO scalars (through vae_loss_deferred, which must be used
 *       instead of vae_loss) are then written by the backward, which must be the standard one (use_std = 1, no
 *       upstream gradient on xhat, no loss scale) and can run once.  x and xhat must stay valid until it has run.
 *   outputs: xhat [B,1,H,W], mu/log_var/z [B,L], all f32. */
int vae_forward(vae_ctx* ctx, const float* x, int batch, const float* params, float* bn_running,
                int64_t* num_batches_tracked, const float* eps, uint64_t seed, int train, float* xhat,
                float* mu, float* log_var, float* z, vae_stream_t stream);

/* VanillaVAE.decode (models.py:147-175): z [B,L] -> xhat [B,1,H,W].  train!=0 uses (and updates) batch
 * statistics like a train-mode module call.  Differentiable through vae_backward_ex (not vae_backward); z and xhat
 * must stay valid until that backward has run. */
int vae_decode(vae_ctx* ctx, const float* z, int batch, const float* params, float* bn_running,
               int64_t* num_batches_tracked, int train, float* xhat, vae_stream_t stream);

/* VanillaVAE.encode (models.py:107-145) and the reparameterisation, without the decoder: the same launches as the
 * encoder half of vae_forward, so mu / log_var are bit-identical to its outputs for the same input, parameters and
 * train value.  Arguments as vae_forward.  Differentiable through vae_backward_ex (not vae_backward). */
int vae_encode(vae_ctx* ctx, const float* x, int batch, const float* params, float* bn_running,
               int64_t* num_batches_tracked, const float* eps, uint64_t seed, int train, float* mu,
               float* log_var, float* z, vae_stream_t stream);

/* EncoderOutput.pre_latents (models.py:133, types_helpers.py:20) of the last forward,
 * [B, flattened_size] f32 in the reference's NCHW-flatten order. */
int vae_pre_latents(vae_ctx* ctx, float* out, vae_stream_t stream);
/* eps actually used by the last forward, [B,L]. */
int vae_last_eps(vae_ctx* ctx, float* out, vae_stream_t stream);

/* VanillaVAE.loss (models.py:190-225) for the last forward: out3 = {loss, reconstruction_loss,
 * kld_loss} with kld_loss sign-flipped as at models.py:224 (reconstruction term: the one that forward recorded). */
int vae_loss(vae_ctx* ctx, float kld_weight, float* out3, vae_stream_t stream);
/* The same scalars computed beside the backward instead of in front of it (one launch less on the critical chain):
 * enqueued on a context side stream ordered after `stream`; out3 is ordered into the caller's stream by the NEXT
 * vae_backward / vae_backward_part on this context, which must follow (train-mode forward only).  For callers that read
 * the ELBO after the step, as train_one_epoch does (train.py:644-674). */
int vae_loss_deferred(vae_ctx* ctx, float kld_weight, float* out3, vae_stream_t stream);

/* VanillaVAE.loss (models.py:190-225) on arbitrary caller tensors: xhat/target [n], mu/log_var
 * [B,L].  Optional outputs (NULL to skip): unscaled gradients of the loss w.r.t. xhat, mu, log_var
 * (BCE grad (x-t)/max(x(1-x),1e-12)/n as ATen computes it). */
int vae_elbo_generic(const float* xhat, const float* target, const float* mu, const float* log_var, int64_t n,
                     int batch, int latent_dim, float kld_weight, float* out3, float* g_xhat, float* g_mu,
                     float* g_log_var, vae_stream_t stream);

/* Reconstruction term of the ELBO (models.py:208).  BCE: F.binary_cross_entropy, the reference's (default).  MSE:
 * F.mse_loss, mean (xhat - x)^2 over B*H*W - a Gaussian likelihood for targets anywhere in [0, 1]; gradient
 * ((xhat - x) * 2/N) * (1 - xhat) * xhat w.r.t. the logit, as ATen's mse_loss backward and sigmoid backward round it.
 * out3 keeps its meaning: reconstruction_loss is the chosen term, loss = reconstruction_loss + kld_weight * KL. */
#define VAE_RECON_BCE 0
#define VAE_RECON_MSE 1
/* WBCE: BCE with a positive-class weight w = pos_weight against the sparsity of pianorolls (a few percent of the cells are notes,
 * so "all silent" is a very good solution of the plain mean).  Per cell, with the target t in [0, 1] and W = 1 + (w - 1) t:
 *   reconstruction_loss = mean over B*H*W of W * bce(xhat, t)   = F.binary_cross_entropy(xhat, x, weight = 1 + (w - 1) x)
 *   dL/dlogit           = the BCE dlogit * W
 * The mean divides by N = B*H*W, not by the weight sum, as torch does; the logs keep their -100 clamp; W multiplies after the
 * unweighted term and gradient, in ATen's order, so w = 1 gives the bits of VAE_RECON_BCE.  For 0/1 rolls this is exactly
 * BCEWithLogitsLoss(pos_weight = w).  For velocity rolls the weight grows with how much of a note the cell is and the per-cell
 * optimum stays xhat = t; multiplying only the positive log term would move the optimum, which is why the weight is on the cell.
 * w is a finite number in (0, 1024].  kld_loss, the KL objectives and loss = reconstruction_loss + kld_weight * T are untouched.
 * f16 storage: |dlogit| is bounded by w/N instead of 1/N, so for w > 1 the power-of-two gradient scale of the forward is lowered
 * by 2^ceil(log2 w) (not below 1): the scaled dlogit keeps the bound it has for BCE. */
#define VAE_RECON_WBCE 2
/* reconstruction term of the ELBO for the following forwards of this context (sticky; default BCE).  A forward records
 * the setting: its loss, deferred output conv (train = 2) and backward use the recorded term even if it changes after. */
int vae_set_recon_loss(vae_ctx* ctx, int kind);
/* vae_set_recon_loss for every kind, with the kind's parameter: pos_weight for VAE_RECON_WBCE, 0 for VAE_RECON_BCE / VAE_RECON_MSE.
 * Sticky and recorded by a forward like the kind (its deferred output conv, loss and backward use the recorded weight).  Enqueues
 * nothing: it may be called every step.  Returns -1 for an unknown kind, a pos_weight that is NaN, infinite, <= 0 or > 1024, or a
 * non-zero param with BCE / MSE.  (vae_set_recon_loss itself keeps refusing every kind but BCE / MSE.) */
int vae_set_recon_loss_ex(vae_ctx* ctx, int kind, double param);
/* A reconstruction target apart from the input, for the NEXT forward of this context only (denoising and infilling: x is the
 * corrupted roll the encoder sees, target the clean one the reconstruction term is taken against).  target [B,1,H,W] f32 with the
 * layout, residency and alignment of that forward's x; the caller keeps it alive as long as x, until the backward of that forward
 * has passed (a train = 2 forward reads it in the backward).  One-shot: whichever forward comes next takes the setting out of the
 * context, and only a full forward uses it - vae_forward, vae_train_step, vae_train_step_fused and vae_train_step_fused_clipped;
 * vae_encode, vae_decode and vae_log_likelihood consume and ignore it.  The forward records the pointer: every output-conv kernel
 * (in the forward, or deferred into the backward), and with them vae_loss / vae_loss_deferred and the reconstruction gradient,
 * then read target where they read x; the encoder, encoder.0's weight gradient and dx keep reading x.  Without the call (or with
 * target = NULL, which clears a pending one) the target is x and nothing differs.  Enqueues nothing.  Returns -1 for a null ctx. */
int vae_set_recon_target(vae_ctx* ctx, const float* target);
/* vae_elbo_generic with the reconstruction term chosen per call (recon: VAE_RECON_*); for MSE g_xhat = (xhat - t) * 2/n. */
int vae_elbo_generic_ex(const float* xhat, const float* target, const float* mu, const float* log_var, int64_t n,
                        int batch, int latent_dim, float kld_weight, int recon, float* out3, float* g_xhat,
                        float* g_mu, float* g_log_var, vae_stream_t stream);

/* KL objective of the ELBO: T replaces KL in loss = reconstruction_loss + kld_weight * T.  All in nats, from the forward's f32
 * mu / log_var [B,L]:  kl_d = 1/B sum_b -0.5 (1 + log_var_bd - mu_bd^2 - exp(log_var_bd)),  KL = sum_d kl_d (models.py:214).
 *   VAE_KL_PLAIN      T = KL (default, the reference's)
 *   VAE_KL_FREE_BITS  T = sum_d max(kl_d, param), param = lambda > 0 nats per dimension (Kingma et al. 2016): a dimension whose
 *                     batch-mean KL is not above lambda gets no KL gradient (torch.clamp(kl_d, min=lambda).sum() under autograd)
 *   VAE_KL_CAPACITY   T = |KL - param|, param = C >= 0 nats (Burgess et al. 2018; kld_weight plays gamma): the KL gradient is
 *                     multiplied by sign(KL - C), 0 at equality
 * kl_d, KL and T are reduced in f64 in a fixed order by one extra launch per forward (none for VAE_KL_PLAIN), so the mask / sign
 * decision is the same bits on every run; it stays on the device.  out3 keeps its meaning: kld_loss is the raw KL with the
 * reference's flipped sign whatever the objective (T = (loss - reconstruction_loss) / kld_weight).  The batch is the one this
 * context sees: data-parallel replicas decide on their own batch means.  vae_log_likelihood / vae_latent_stats are unaffected. */
#define VAE_KL_PLAIN 0
#define VAE_KL_FREE_BITS 1
#define VAE_KL_CAPACITY 2
/*   VAE_KL_TC         T = KL + (param - 1) TC, param = tc_weight >= 0 (beta-TCVAE, Chen et al. 2018, in the form KL + (beta - 1) TC):
 *                     TC = 1/B sum_i [log q(z_i) - sum_d log q(z_id)] with q the in-batch mixture 1/B sum_j N(mu_j, diag e^{log_var_j}),
 *                     the query's own component included, at the forward's own z_i = mu_i + eps_i exp(log_var_i / 2) - the quantity
 *                     vae_latent_stats reports as tc for eps = the forward's.  Pairwise kernels beside the decoder compute TC and its
 *                     gradient through both the queries and the components (total_corr.cuh), every sum in a fixed order; the backward adds
 *                     kld_weight (param - 1) dTC/d(mu, log_var) to the plain KL gradient.  Batches of at most 4096; TC is 0 for a batch
 *                     of 1 and for latent_dim 1.  Work space 4 B^2 + O(B latent_dim) bytes, allocated by the first such forward.  f16
 *                     storage: this term shares the power-of-two gradient scale of the rest and is not bounded by the KL gradient. */
#define VAE_KL_TC 3
/* KL objective for the following forwards of this context (sticky; default plain).  A forward records kind and param: its loss,
 * deferred loss and backward (vae_backward, _part, _ex with use_std = 1, the training steps) use the recorded ones even if the
 * setting changes after.  A NaN, negative or infinite param, or VAE_KL_FREE_BITS with param <= 0, returns -1.  Enqueues nothing:
 * a per-step capacity ramp may call it every step. */
int vae_set_kl_objective(vae_ctx* ctx, int kind, double param);
/* vae_elbo_generic_ex with the KL objective chosen per call: g_mu / g_log_var are the gradients of kld_weight * T.  VAE_KL_TC
 * returns -1: the term needs the eps of the forward, which this entry point does not take (vae_total_correlation does). */
int vae_elbo_generic_kl(const float* xhat, const float* target, const float* mu, const float* log_var, int64_t n,
                        int batch, int latent_dim, float kld_weight, int recon, int kl_kind, double kl_param, float* out3,
                        float* g_xhat, float* g_mu, float* g_log_var, vae_stream_t stream);
/* vae_elbo_generic_kl with the reconstruction term's parameter (recon_param: as vae_set_recon_loss_ex's param), the only generic
 * entry point that takes VAE_RECON_WBCE: g_xhat = W * (xhat - t) / max(xhat (1 - xhat), 1e-12) / n.  A bad kind or weight returns
 * -1 before anything is enqueued. */
int vae_elbo_generic_w(const float* xhat, const float* target, const float* mu, const float* log_var, int64_t n,
                       int batch, int latent_dim, float kld_weight, int recon, double recon_param, int kl_kind, double kl_param,
                       float* out3, float* g_xhat, float* g_mu, float* g_log_var, vae_stream_t stream);
/* kl_d [latent_dim] f64 of the last forward (vae_forward, the training steps, vae_encode), device memory, no host
 * synchronisation: the forward's own reduction when it ran with an objective other than plain, else reduced on demand. */
int vae_kl_per_dim(vae_ctx* ctx, double* out, vae_stream_t stream);
/* Total correlation (nats, VAE_KL_TC's definition) of `batch` posteriors [batch, latent_dim] f32 at z = mu + eps exp(log_var / 2), and
 * optionally its gradient: tc one f64, g_mu / g_log_var [batch, latent_dim] f32 = dTC/dmu, dTC/dlog_var (through z as well), each may
 * be NULL.  Device memory, no host synchronisation, context-free; the kernels of the VAE_KL_TC objective, every sum in a fixed order
 * (repeated calls are bit-identical).  Work space 4 batch^2 + 32 batch latent_dim bytes from the stream-ordered allocator.  Returns -1
 * before anything is enqueued for a NULL mu / log_var / eps / tc, batch outside 1..4096 or latent_dim outside 1..4096. */
int vae_total_correlation(const float* mu, const float* log_var, const float* eps, int batch, int latent_dim, double* tc,
                          float* g_mu, float* g_log_var, vae_stream_t stream);
/* TC of the last forward (vae_forward, the training steps, vae_encode; an error after vae_decode or with no forward), one device f64,
 * no host synchronisation: the forward's own value when it ran with VAE_KL_TC, else computed on demand as vae_kl_per_dim does. */
int vae_last_total_correlation(vae_ctx* ctx, double* out, vae_stream_t stream);

/* Importance-weighted log-likelihood (IWAE_K) and per-sample ELBO of x under the model in eval mode.
 * eps [K,B,L] f32 or NULL (device counter generator, seed, stream 6; index (k*B+b)*L+l).
 * Decodes `chunk` draws of the whole batch per pass: chunk*batch <= max_batch.
 * log_w [K,B], log_likelihood [B], elbo [B]: f64, nats; log_w may be NULL.
 *   log_w[k,b]        = log p(x_b|z_kb) + log p(z_kb) - log q(z_kb|x_b),  z_kb = eps_kb * exp(0.5 log_var_b) + mu_b
 *   log_likelihood[b] = logsumexp_k log_w[k,b] - log K
 *   elbo[b]           = mean_k log p(x_b|z_kb) - KL(q(z|x_b) || N(0, I))
 * log p(x|z) follows the context's reconstruction term (vae_set_recon_loss): BCE - Bernoulli, sum over pixels of
 * t log xhat + (1-t) log(1-xhat) with the logs clamped at -100 (normalised only for 0/1 targets); MSE - Gaussian of variance 1/2,
 * -sum (xhat - t)^2 - (H*W/2) log(pi).  VAE_RECON_WBCE counts as BCE here: a weighted BCE is not a likelihood, so log p(x|z), the
 * IWAE bound and the per-sample ELBO stay the unweighted Bernoulli whatever pos_weight is.  BatchNorm uses (and never writes) the
 * running statistics in bn_running.  Nothing is
 * left to differentiate: vae_loss / vae_backward after this call fail until the next forward. */
int vae_log_likelihood(vae_ctx* ctx, const float* x, int batch, const float* params, const float* bn_running,
                       int num_samples, int chunk, const float* eps, uint64_t seed,
                       double* log_w, double* log_likelihood, double* elbo, vae_stream_t stream);

/* Latent diagnostics of n posteriors q(z|x_i) = N(mu_i, diag e^{log_var_i}) ([n, latent_dim] f32, 1 <= latent_dim <= 4096): the
 * aggregate posterior q(z) = 1/n sum_j q(z|x_j), all n components (the query's own included), at draws z[s,i] = eps * exp(0.5 lv_i) + mu_i.
 * eps [draws,n,L] f32, or NULL: element (s*n+i)*L+d of the device counter generator (seed, stream 7).  Outputs f64, nats:
 *   log_qz [draws*n]        log q(z_q)
 *   log_qz_dims [draws*n*L] log q(z_qd)                       (marginal of dimension d)
 *   per_dim [3*L]           kl_per_dim (mean_i KL_d), var_mu (population variance over i of mu_id), dwkl_per_dim
 *   scalars [4]             kl, mi = I(x;z), tc (total correlation), dwkl (dimension-wise KL); kl = mi + tc + dwkl
 * Context-free, on `stream`; every reduction runs in a fixed order (repeated calls are bit-identical).  Its work space, about
 * (12 + 12 draws) n L bytes (more when small shapes split the component range), comes from the stream-ordered allocator. */
int vae_latent_stats(const float* mu, const float* log_var, int64_t n, int latent_dim, int draws, const float* eps, uint64_t seed,
                     double* log_qz, double* log_qz_dims, double* per_dim, double* scalars, vae_stream_t stream);

/* Note-level reconstruction metrics of `rolls` rolls of `roll_len` cells each (xhat, target: [rolls, roll_len] f32, contiguous, any
 * 4-byte-aligned base - a sliced view is fine), in one pass over both tensors.  Per cell, with xh / tg the f32 values as stored:
 *   se  = ((double)(xh - tg))^2          ae = |(double)(xh - tg)|          (the f32 difference, widened)
 *   bce = -(tg max(log xh, -100) + (1 - tg) max(log(1 - xh), -100)) in f32, widened: the ELBO's own BCE term (VAE_RECON_BCE)
 *   true note:  tg >= target_threshold          predicted note at threshold t:  xh >= thresholds[t]   (f32 against f32)
 * thresholds: n_thresholds (1..8) finite floats in HOST memory, read before the call returns; unsorted and repeated values are fine.
 * Device outputs, written in stream order with no host synchronisation:
 *   roll_sums   [rolls][3] f64            se, ae, bce of each roll
 *   roll_counts [rolls][1 + 2 n_thresholds] positives (true notes), then tp, fp per threshold (fn = positives - tp,
 *                                         tn = roll_len - positives - fp)
 *   totals      [8] f64                   se, ae, bce, n_cells, min xhat, max xhat, min target, max target
 *   total_counts[1 + 2 n_thresholds]      as roll_counts, over all rolls
 * accumulate = 1 adds this call to what totals / total_counts hold (sums and counts add, ranges combine; totals whose n_cells is 0 -
 * all zeros - are the empty state), so an evaluation pass keeps its state on the device; 0 overwrites.  rolls = 0 launches nothing and
 * with accumulate = 0 zeroes the totals (the roll pointers and xhat / target may then be NULL).  A roll is cut into chunks of 4096
 * cells, one workgroup each; chunks, rolls and totals are folded in index order without atomics, so the counts are exact and the same
 * call on the same data gives the same bits.  A NaN xhat is never a predicted note and makes the sums NaN; the ranges skip NaNs.
 * Returns -1 before anything is enqueued for a null pointer, n_thresholds outside 1..8, a non-finite threshold, rolls < 0,
 * roll_len < 1 or rolls * ceil(roll_len / 4096) >= 2^31.  Work space (16 bytes per chunk, plus 24 + 8 (1 + 2 n_thresholds) per
 * chunk when roll_len > 4096) comes from the stream-ordered allocator. */
int vae_recon_metrics(const float* xhat, const float* target, int64_t rolls, int64_t roll_len, const float* thresholds,
                      int n_thresholds, float target_threshold, double* roll_sums, int64_t* roll_counts, double* totals,
                      int64_t* total_counts, int accumulate, vae_stream_t stream);

/* loss.backward() (train.py:650) for the last train-mode forward.
 *   grads: flat f32 buffer, same layout as params; every tensor is overwritten.
 *   use_std: 1 adds the gradient of the standard ELBO of vae_loss (reconstruction term fused in
 *           the forward, plus d(kld_weight*KL)/d(mu,log_var), models.py:208-216), scaled by
 *   gscale: device scalar = upstream gradient of loss.backward(), NULL = 1.
 *   g_xhat [B,1,H,W], g_mu/g_log_var/g_z [B,L], g_pre [B,F]: optional additional upstream
 *           gradients on the ModelOutput tensors (NULL = none). */
int vae_backward(vae_ctx* ctx, const float* x, const float* params, float* grads, const float* g_xhat,
                 const float* gscale, const float* g_mu, const float* g_log_var, const float* g_z,
                 const float* g_pre, float kld_weight, int use_std, vae_stream_t stream);
/* The same backward in two halves, for data-parallel callers that start the all-reduce of the decoder
 * gradients while the encoder half still runs: part 1 = output conv + decoder stack (on return every decoder
 * and final_layer gradient is complete in stream order), part 2 = the rest (decoder_input, latent, fc, encoder);
 * part 0 = both (= vae_backward).  Same arguments in both calls. */
int vae_backward_part(vae_ctx* ctx, const float* x, const float* params, float* grads, const float* g_xhat,
                 const float* gscale, const float* g_mu, const float* g_log_var, const float* g_z,
                 const float* g_pre, float kld_weight, int use_std, int part, vae_stream_t stream);
/* The backward of whichever forward ran last on the context: vae_forward (train or eval mode), vae_encode or
 * vae_decode.  Arguments as vae_backward, plus:
 *   dx [B,1,H,W]: dL/dx of a vae_forward / vae_encode input, written when not NULL (else never computed)
 *   dz [B,L]:     dL/dz of a vae_decode input, written when not NULL
 * After an eval-mode forward BatchNorm is differentiated on the running statistics (which are not written).
 * vae_encode: only g_mu / g_log_var / g_pre apply (use_std must be 0, g_xhat and g_z NULL); the decoder's gradients
 * in `grads` are left as they were.  vae_decode: only g_xhat applies (use_std must be 0: there is no target; x may be
 * NULL); the encoder, fc_mu and fc_var gradients in `grads` are left as they were. */
int vae_backward_ex(vae_ctx* ctx, const float* x, const float* params, float* grads, const float* g_xhat,
                    const float* gscale, const float* g_mu, const float* g_log_var, const float* g_z,
                    const float* g_pre, float kld_weight, int use_std, float* dx, float* dz, vae_stream_t stream);
/* A non-blocking stream owned by the context, ordered after everything enqueued on `stream` so far.  Data-parallel
 * callers enqueue the decoder bucket's all-reduce on it right after part 1; it is joined back into the caller's
 * stream at the end of part 2, so the collective overlaps the encoder half without any host-side handshake. */
int vae_comm_stream(vae_ctx* ctx, vae_stream_t stream, vae_stream_t* out);

/* ---- data parallel: one process per GPU, gradients exchanged over RCCL (xGMI inside a node) -------------------------
 * The reference has no exchange step: it only scales the learning rate and the sample counters by
 * WORLD_SIZE (train.py:165-166, 201, 663).  These entry points are the gradient all-reduce north_star asks for, issued
 * by the library itself so that backward kernels, collective and AdamW share streams without a framework hand-off.
 * vae_comm_unique_id: rank 0 fills a VAE_COMM_ID_BYTES id; the host distributes it over any channel it has
 * (torch.distributed's store / broadcast, MPI, a file); every rank then calls vae_comm_init with the device it will run on
 * current.  The communicator belongs to the context (released by vae_comm_destroy / vae_destroy). */
#define VAE_COMM_ID_BYTES 128
int vae_comm_unique_id(void* id /*[VAE_COMM_ID_BYTES]*/);
int vae_comm_init(vae_ctx* ctx, int rank, int world, const void* id /*[VAE_COMM_ID_BYTES]*/);
int vae_comm_world(const vae_ctx* ctx); /* world size of the context's communicator, 0 if none */
int vae_comm_destroy(vae_ctx* ctx);
/* In-place all-reduce over ranks of `nranges` ranges [offsets[i], offsets[i]+sizes[i]) of the flat f32 gradient buffer,
 * as one RCCL group enqueued on `stream`: the caller's stream (ordered after the backward by the stream itself) or the
 * context's communication stream (vae_comm_stream) for the decoder bucket between vae_backward_part 1 and 2.
 * average != 0 leaves the MEAN over ranks (what a data-parallel caller expects in .grad); 0 the sum. */
int vae_allreduce_grads(vae_ctx* ctx, float* grads, int nranges, const int64_t* offsets, const int64_t* sizes, int average,
                        vae_stream_t stream);
/* Identical replicas before the first step: broadcast rank `root`'s flat parameters, BatchNorm running statistics and
 * num_batches_tracked (NULL to skip the latter two) over the context's communicator. */
int vae_broadcast_state(vae_ctx* ctx, float* params, float* bn_running, int64_t* num_batches_tracked, int root,
                        vae_stream_t stream);

/* torch.optim.AdamW.step (train.py:228,656) on up to two contiguous ranges of the flat
 * buffers (the encoder and decoder groups of train.py:210-225), each with the lr and beta1
 * OneCycleLR set for this step (train.py:233-238,659).  step is 1-based.  The hyper-parameters are
 * doubles, as torch holds them: 1 - beta, 1 - lr * weight_decay, the bias corrections and lr / bc1 are
 * formed in double and only then rounded to the float the element-wise update uses (torch's scalar
 * arguments: (float)(1 - 0.999) is 0.001f, not 1.f - 0.999f). */
int vae_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int ngroups,
                   const int64_t* offsets, const int64_t* sizes, const double* lrs, const double* beta1s,
                   double beta2, double eps, double weight_decay, float grad_scale, int step,
                   vae_stream_t stream);

/* Gradient-norm clipping and non-finite step skipping (torch.nn.utils.clip_grad_norm_ in front of AdamW, the skip of
 * torch's GradScaler), with no host synchronisation: the norm, the clip decision and the AdamW step count live on the device.
 *   norm = || g * grad_scale ||_2 over the ranges, all groups together, summed in f64 in a fixed order (deterministic:
 *          the grid does not depend on the device; every rank of a data-parallel job takes the same decision);
 *   coef = min(1, max_grad_norm / (norm + 1e-6)) in f64, rounded once to f32; max_grad_norm <= 0: no clipping (coef 1);
 *   skip_nonfinite and a non-finite norm: parameters and moments untouched, *step held, *skipped += 1; otherwise
 *   *step += 1 and AdamW runs with g * grad_scale * coef and the bias corrections of the new *step.
 * The gradient buffer keeps the unclipped gradient.  `scratch`: VAE_GRAD_CLIP_SCRATCH_BYTES of device memory, 16-byte
 * aligned, owned by the caller and not used by anything else until the stream has passed the call.  step (the device count
 * of updates so far), norm_out and skipped are device scalars.  Bad arguments (ngroups not 1 or 2, a null pointer, a NaN
 * max_grad_norm) return -1 before anything is enqueued. */
#define VAE_GRAD_CLIP_SCRATCH_BYTES 8192
/* The norm alone (a diagnostic): *norm_out = || g * grad_scale ||_2 over the ranges. */
int vae_grad_norm(const float* grads, int ngroups, const int64_t* offsets, const int64_t* sizes, float grad_scale,
                  double* norm_out, void* scratch, vae_stream_t stream);
/* vae_adamw_step with the clipping / skipping above; the host's 1-based step is replaced by the device counter `step`. */
int vae_adamw_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int ngroups,
                           const int64_t* offsets, const int64_t* sizes, const double* lrs, const double* beta1s,
                           double beta2, double eps, double weight_decay, float grad_scale, double max_grad_norm,
                           int skip_nonfinite, int64_t* step, double* norm_out, int64_t* skipped, void* scratch,
                           vae_stream_t stream);

/* One whole training step (train.py:634-659 minus logging): forward, loss, backward, AdamW. */
int vae_train_step(vae_ctx* ctx, const float* x, int batch, float* params, float* grads, float* exp_avg,
                   float* exp_avg_sq, float* bn_running, int64_t* num_batches_tracked, const float* eps,
                   uint64_t seed, float kld_weight, int ngroups, const int64_t* offsets,
                   const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double adam_eps,
                   double weight_decay, int step, float* xhat, float* mu, float* log_var, float* z,
                   float* out3, vae_stream_t stream);

/* The fused training step of torch_vae_amd.train.fused_step as ONE host call (train.py:634-659): forward with the output
 * conv deferred to the backward, ELBO scalars, backward, gradient exchange, AdamW.  exchange: 0 none; 1 one RCCL group over
 * the optimised ranges between the backward and AdamW; 2 bucketed - the last range (decoder) is all-reduced on the context's
 * communication stream under the encoder half of the backward, the others after it, and each range's AdamW launch waits only
 * for its own bucket, so one group's update runs while the other's all-reduce is in flight (the data-parallel layout
 * train.py:165-166,201,663 prepare).  1 and 2 need vae_comm_init and produce bit-identical results. */
int vae_train_step_fused(vae_ctx* ctx, const float* x, int batch, float* params, float* grads, float* exp_avg,
                         float* exp_avg_sq, float* bn_running, int64_t* num_batches_tracked, const float* eps,
                         uint64_t seed, float kld_weight, int ngroups, const int64_t* offsets,
                         const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double adam_eps,
                         double weight_decay, float grad_scale, int step, int exchange, float* xhat, float* mu,
                         float* log_var, float* z, float* out3, vae_stream_t stream);
/* vae_train_step_fused with the clipping / skipping of vae_adamw_step_clipped (the host step replaced by the device
 * counter): the norm is taken AFTER the gradient exchange.  With exchange 2 it waits for every bucket and both groups'
 * AdamW follow it, so the update of one group no longer overlaps the other bucket's all-reduce. */
int vae_train_step_fused_clipped(vae_ctx* ctx, const float* x, int batch, float* params, float* grads, float* exp_avg,
                                 float* exp_avg_sq, float* bn_running, int64_t* num_batches_tracked, const float* eps,
                                 uint64_t seed, float kld_weight, int ngroups, const int64_t* offsets,
                                 const int64_t* sizes, const double* lrs, const double* beta1s, double beta2,
                                 double adam_eps, double weight_decay, float grad_scale, double max_grad_norm,
                                 int skip_nonfinite, int64_t* step, double* norm_out, int64_t* skipped, void* scratch,
                                 int exchange, float* xhat, float* mu, float* log_var, float* z, float* out3,
                                 vae_stream_t stream);

/* Synthetic pianoroll/line batch with the distribution of data_generators.py:45-77
 * (called as at :97-104), seeded; x [B,1,H,H] f32 in {0,1}.  Device-side generator. */
int vae_synth_pianoroll(float* x, int batch, int img_size, uint64_t seed, vae_stream_t stream);

/* Byte or bit-plane stimuli expanded to the float32 batch [B,1,H,W] the step reads (the host side of
 * train.py:630-631: the reference copies float32 stimuli; a 0/1 pianoroll needs 1/4 or 1/32 of those
 * bytes on the host link).  kind 0: one byte per cell, v -> (float)v; kind 1: bit planes, most
 * significant bit first (numpy.packbits order).  `src` is device memory or PINNED host memory (read in
 * place by the kernel; the caller keeps it alive and unchanged until the stream has passed this call);
 * pageable host memory is refused.  n_cells = B*H*W, a multiple of 8. */
int vae_expand_stimuli(const void* src, int kind, float* dst, int64_t n_cells, vae_stream_t stream);

/* One training batch out of a resident set of pianorolls, augmented on the way: picks `batch` rolls, cuts a window of `w` time
 * steps out of each, shifts it in time and transposes it in pitch, and writes the float32 batch [batch,1,h,w] the step reads.
 * The reference's data_transformations.get_transform (RandomCrop for training, CenterCrop for evaluation) as one launch.
 * src holds n_rolls rolls of h rows (pitch) by src_w columns (time), row-major.  kind 0: one byte per cell, dst = (float)v * scale;
 * kind 1: bit planes, most significant bit first (numpy.packbits order), src_w/8 bytes per row, cells 0.f / 1.f; kind 2: float32
 * cells, copied (scale is ignored by kinds 1 and 2).  src is device memory or PINNED host memory read in place, as for
 * vae_expand_stimuli; pageable host memory is refused.
 * With i = index ? index[b] : first + b, for every output cell
 *     dst[b,0,y,x] = S(i, y - dy_b, c0_b + x)   if 0 <= i < n_rolls, 0 <= y - dy_b < h and 0 <= c0_b + x < src_w, else 0
 * dy is clamped to [-h, h] and c0 to [-w, src_w] first (beyond those the roll is all zero anyway).  c0 is crop offset and time
 * shift in one: a shift inside a longer roll shows the neighbouring content, zeros appear only past the roll's ends; pitch is always
 * zero-filled.  An index outside [0, n_rolls) gives a zero roll: the guards live in the kernel, which forms no address outside
 * src[0 .. n_rolls*h*row_bytes) whatever index and params hold (device-resident indices cannot be validated on the host without
 * a synchronisation).
 * (dy_b, c0_b) = params[b] when params (device, [batch,2] int32) is given.  With params NULL they are drawn in the kernel from the
 * counter generator (oracle.counter_uniform) on stream 901, for sample b with counter k = counter0 + b * counter_stride, P =
 * max_pitch_shift, T = max_time_shift and slack s = src_w - w:
 *     dy = (int)(u(2k) * (2P+1)) - P
 *     c0 = (int)(u(2k+1) * (s + 2T + 1)) - T            crop_mode 0 (random window)
 *     c0 = s/2 + (int)(u(2k+1) * (2T+1)) - T            crop_mode 1 (centre window; with P = T = 0 nothing is random)
 * counter_stride lets data-parallel ranks that take every world-th position of one global permutation number their samples by
 * that global position (counter0 = position of the batch's first sample, counter_stride = world): a roll's augmentation is then a
 * function of (seed, position) alone, whatever the batch size and the number of ranks.  A single process passes 1.
 * vae_augment_params writes exactly these draws to params, unclamped, for inspection.
 * Returns -1 before anything is enqueued for: null src or dst; kind outside 0..2; h <= 0; batch < 0 (batch == 0 returns 0 and
 * launches nothing); w or src_w not a positive multiple of 8 (or above 2^30); src_w < w; n_rolls <= 0 or n_rolls * h * row_bytes
 * beyond 2^62; a negative max_*_shift (or one above 2^24); crop_mode outside 0..1; a non-finite scale; dst not 16-byte, index not
 * 8-byte, params or a kind-2 src not 4-byte aligned; a src that is neither device nor pinned host memory. */
int vae_gather_rolls(const void* src, int kind, int64_t n_rolls, int h, int src_w, const int64_t* index, int64_t first,
                     const int32_t* params, uint64_t seed, uint64_t counter0, uint64_t counter_stride, int max_pitch_shift,
                     int max_time_shift, int crop_mode, float scale, float* dst, int batch, int w, vae_stream_t stream);
int vae_augment_params(int32_t* params, int batch, int src_w, int w, uint64_t seed, uint64_t counter0, uint64_t counter_stride,
                       int max_pitch_shift, int max_time_shift, int crop_mode, vae_stream_t stream);

/* Note events out of float pianorolls, the other end of vae_gather_rolls: what a decoded batch holds as notes, and the cleaned
 * batch as bit planes.  rolls is [n][h][w] float32, pitch rows by time columns, row-major (the model's [B,1,H,W] output as it is).
 * All comparisons are float32 against float32; a NaN cell compares false with everything.  For each row (r, p), over t = 0..w-1:
 *   hysteresis  s[-1] = 0; s[t] = 1 if x[t] >= onset_threshold; s[t] = 0 if not (x[t] >= sustain_threshold) (a NaN is off);
 *               otherwise s[t] = s[t-1].  sustain_threshold == onset_threshold is plain thresholding.
 *   bridging    a maximal run of zeros in s of length <= max_gap with a one on both sides becomes ones; runs touching either end
 *               of the row never do; max_gap = 0 changes nothing.
 *   notes       the maximal runs of ones after bridging; runs shorter than min_duration are dropped.
 *   event       of a kept run [t0, t0 + len): events[i] = (r, p, t0, len) and peaks[i] = max x[t] over the run, bridged cells
 *               included and NaNs skipped - an exact value of the input, whatever the order.
 * Events ascend by (roll, pitch, onset).  offsets[r] is the index of roll r's first event and offsets[n] the number of events; both
 * are right whatever the capacity: events with index >= capacity are not written (no slot past the first `capacity` is touched).
 * cleaned, [n][h][w/8] bytes, has bit t of row (r, p) set exactly for the cells of kept notes, most significant bit first
 * (numpy.packbits order): the kind-1 source of vae_gather_rolls and vae_expand_stimuli.
 * events and peaks may both be NULL (a count-only call: offsets alone, and cleaned when given); cleaned may be NULL.  No position
 * depends on an atomic or on arrival order: repeated calls give the same bits.  Nothing synchronises with the host; the work space
 * (one int32 per row, one int64 per 16384 rows) comes from the stream-ordered allocator.
 * Returns -1 before anything is enqueued for: null rolls or offsets; exactly one of events and peaks null; n < 0 (n == 0 zeroes
 * offsets[0] and returns 0); h < 1; w not a multiple of 8 in 8..65536; n * h >= 2^31; a non-finite threshold; sustain_threshold >
 * onset_threshold; min_duration < 1; max_gap < 0; capacity < 0; rolls, events or peaks not 4-byte aligned; offsets not 8-byte
 * aligned.  An event is one 16-byte store where events is 16-byte aligned. */
int vae_extract_notes(const float* rolls, int64_t n, int h, int w, float onset_threshold, float sustain_threshold,
                      int min_duration, int max_gap, int32_t* events /*[capacity][4]*/, float* peaks /*[capacity]*/,
                      int64_t capacity, int64_t* offsets /*[n+1]*/, uint8_t* cleaned /*[n][h][w/8]*/, vae_stream_t stream);

/* Nearest rolls of query rolls under transposition and time shift: is a generated roll new, or a training roll played back?
 * queries is [n_queries][h][w/8] and rolls [n_rolls][h][w/8] bytes, bit planes of h pitch rows by w time columns, most significant
 * bit first (numpy.packbits order: the kind-1 source of vae_gather_rolls, the cleaned planes of vae_extract_notes).  Everything is
 * integer and exact.  With P = max_pitch_shift and T = max_time_shift:
 *   shifted candidate  C'(y, x) = C(y - dy, x - dt) if 0 <= y - dy < h and 0 <= x - dt < w, else 0 - what vae_gather_rolls returns
 *                      for params (dy, c0 = -dt) at width w.  The window is dy in [-P, P], dt in [-T, T].
 *   shift rank         rank 0 is (0, 0); ranks 1, 2, ... are the other (dy, dt) ascending by (dy, dt).
 *   pair               d(q, c) = min over the window of popcount(q XOR C'); the pair's shift is the lowest-ranked one that reaches
 *                      it (against an empty candidate every shift ties and (0, 0) wins); intersection = popcount(q AND C') there.
 *   neighbours         of query i: the rolls j != exclude[i] (exclude may be NULL; an entry outside [0, n_rolls) excludes nothing)
 *                      ascending by (d, j); the first k go to index, distance, shift (dy, dt) and intersection [i][0..k).
 *                      Slots with no candidate left hold index -1, distance -1, shift (0, 0), intersection 0.
 *   query_cells[i]     popcount(q_i).
 * (The shifted neighbour has d + 2 * intersection - query_cells cells; the pair's Jaccard index is intersection / (d + intersection).)
 * Two launches.  The first gives each workgroup a tile of queries and one of `splits` contiguous ranges of rolls and leaves the k
 * best keys (d << 40 | j, with the shift rank) per (query, range) in work space from the stream-ordered allocator; the second merges
 * the ranges per query, counts the intersections and writes the outputs.  Keys are unique, so a k-best list is a set: the result does
 * not depend on arrival order or on splits (0: chosen from n_queries and n_rolls alone; 1..64: as given, for tests), and repeated
 * calls give the same bits.  No atomics; nothing synchronises with the host.  No byte outside queries, rolls and the outputs is
 * addressed, whatever exclude holds.
 * Returns -1 before anything is enqueued for: a null queries, rolls or output pointer; n_queries < 0 (n_queries == 0 returns 0 and
 * launches nothing); n_rolls outside 1..2^40; h < 1; w not a positive multiple of 32; a roll of more than 8192 bytes (h * w / 8;
 * 256 x 256 fits); max_pitch_shift outside 0..h-1; max_time_shift outside 0..w-1; (2P+1)(2T+1) > 1023; k outside 1..32; splits
 * outside 0..64 (or ceil(n_queries / 16) * splits >= 2^31); queries or rolls not 4-byte aligned; index or exclude not 8-byte aligned; distance, shift, intersection or
 * query_cells not 4-byte aligned. */
int vae_nearest_rolls(const uint8_t* queries /*[n_queries][h][w/8]*/, int n_queries,
                      const uint8_t* rolls   /*[n_rolls][h][w/8]*/,   int64_t n_rolls, int h, int w,
                      int max_pitch_shift, int max_time_shift, const int64_t* exclude /*[n_queries] or NULL*/,
                      int k, int splits /*0 = chosen by the library*/,
                      int64_t* index /*[n_queries][k]*/, int32_t* distance /*[n_queries][k]*/,
                      int32_t* shift /*[n_queries][k][2]*/, int32_t* intersection /*[n_queries][k]*/,
                      int32_t* query_cells /*[n_queries]*/, vae_stream_t stream);

/* Per-kernel timing for bench.py's roofline line: when enabled every launch of the step is
 * bracketed by HIP events on the launch stream; the report is a JSON array with, per kernel name,
 * calls, total ms, and total ALGORITHMIC bytes / flops (operand tensors once). */
int vae_profile(vae_ctx* ctx, int enable);
int vae_profile_report(vae_ctx* ctx, char* buf, int64_t capacity);
/* JSON array of the labels of all profiled launches, in launch order. */
int vae_profile_sequence(vae_ctx* ctx, char* buf, int64_t capacity);
/* JSON array [[label, start_ms, end_ms, algorithmic_bytes], ...] of all profiled launches, times relative to
 * the first one: weight gradients run on the context's side streams, so launches overlap. */
int vae_profile_timeline(vae_ctx* ctx, char* buf, int64_t capacity);
/* Diagnostics: per-wave phase cycle counters of the pipelined conv kernel of one layer.  tag = layer label
 * ("final_layer.0" ...), epi = epilogue kind (0 forward, 1 backward, 2 plain; +16 selects the transposed-conv
 * kernel), out = device buffer of grid*waves*8 int64 for the stride-2 conv kernel (6 loop phases + prologue + tail),
 * grid*4*6 for the transposed-conv kernel (NULL switches it off).  Needs a `make STAMPS=1` build. */
int vae_debug_stamps(vae_ctx* ctx, const char* tag, int epi, long long* out);

/* Debug / test hooks: copy an internal NHWC tensor to f32 NCHW.  which: 0..7 raw conv output
 * of BN layer i, 8..15 its dz, 16 decoder_input output, 17 its gradient; 18 the latent gradient of the last backward,
 * [B, 2 latent_dim] f32 (dmu | dlog_var per row, times the f16 gradient scale), and 19 the per-dimension factors [latent_dim] f32 of the last
 * forward's KL objective (an error after a plain forward), both copied as they are; 20 the gradient of the last forward's total
 * correlation, [B, 2 latent_dim] f32 (g_mu | g_log_var per row) before any weight or scale (computed on demand as
 * vae_last_total_correlation does). */
int vae_debug_tensor(vae_ctx* ctx, int which, float* out, int64_t capacity, vae_stream_t stream);
/* hardware self-test of the transposed LDS read used by the bf16 weight-gradient kernel */
int vae_selftest_tr16(vae_stream_t stream);
/* Tuning / diagnostic switches, each listed once as `name [default]`: the default is the value that, passed to vae_set_option,
 * restores the default behaviour (vae_option_info reports the same list).  Figures are MI355X measurements at 128x128, latent 16,
 * batch 256, bf16, and are the record of what was tried.  "16-bit" = bf16 / f16 storage.  An unknown name returns -1.
 * Kernel paths:
 *   use_tr16 [1]            ds_read_b64_tr_b16 in the 16-bit weight-gradient kernels
 *   use_mfma_convout [1]    MFMA versions of the output-conv kernels (16-bit)
 *   use_pipelined [1]       persistent prefetching conv kernels (0: one tile per workgroup)
 *   use_side_stream [1]     weight gradients / weight packing on the context's side streams (the environment variable
 *                           VAE_NO_SIDE_STREAM makes 0 the default of a new context)
 *   use_fused_bn [1]        BatchNorm finalisation inside the consumer kernel's prologue
 *   use_fused_convout [1]   honour train = 2 (output conv forward + backward as one kernel; 16-bit)
 *   use_convout_stream [1]  128-pixel-wide images take the row-streaming form of that kernel; 0 the tiled one
 *   use_fused_wgrad [1]     one pass over (dz, y) for the input AND weight gradient of final_layer.0 / decoder.2 / encoder.1 (16-bit):
 *                           1 all three, 2 the transposed-conv layers final_layer.0 / decoder.2 only, 3 encoder.1 only, anything else none
 *   use_recomp_dz [0]       final_layer.0's dz recomputed from dlogit instead of stored.  Bit-identical and 268 MB less traffic each
 *                           way, but measured SLOWER (1.50 vs 1.33 ms/step): the per-element BatchNorm-backward in accumulator layout
 *                           costs ~20 VALU per element, and the output-conv backward is VALU-bound, not write-bound (134 us without
 *                           the store, 128 us with it).  Kept for the day both epilogues are cheap.
 *   use_raw_wgrad [0]       deep layers' weight gradients read MATERIALISED operands (LeakyReLU(BN(y)) / the BatchNorm-backward gradient,
 *                           written as a side effect by the kernel that stages them first) as plain copies.  Bit-identical; measured
 *                           1 % SLOWER in the step (the extra stores cost the chain more than the weight-gradient kernels gain)
 *   use_deep [1]            workgroup-specialised kernels of the deep layers: bit 0 stride-2 conv products, bit 1 transposed products.
 *                           Three runs each: bit 0 alone 1.262 ms/step, neither 1.267, both 1.279, bit 1 alone 1.279 - the transposed
 *                           kernel's nine LDS-DMA issues per consumer wave and K step (~130 cycles each) cost what its overlap wins
 *   use_latent_mfma [6]     skinny linears around the latent on the exact-f32 MFMA, one 64-feature tile x the whole batch per workgroup,
 *                           no batch split / slabs / reduction launches.  Bits: 1 decoder_input forward, 2 its weight + bias gradient,
 *                           4 fc_mu|fc_var weight (+ bias) gradient, 8 fc input gradient.  Isolated: weight gradients 22 / 26 us against
 *                           30 / 28 us + 4 reductions (26 us); the forward (14 vs 12 us) and the fc input gradient (24 vs 22 us) are
 *                           not faster and stay on the VALU kernels - whose summation order the f32 parity gates were measured with
 *   use_dnf_stream [1]      encoder.1 forward on 128x128 images: row-streaming kernel; 0 the tiled one
 *   use_upf_stream [1]      row-streaming transposed-conv forward on 128x128 images: bit 0 final_layer.0, bit 1 decoder.2 (measures the
 *                           same 32 us as the tiled kernel); 0 the tiled kernels
 *   use_fc_dgrad8 [1]       fc input gradient, 16-bit: 8 channels x 4 rows per thread with 16-byte accesses (bit 1: 512-thread
 *                           workgroups over 64 rows for batches above 32); 0 one channel per thread
 *   use_wgrad_split [1]     deep weight gradients: producer / consumer wave groups; 0 the 8-wave kernel
 * Grid / tile sizing:
 *   knob_up_per_cu [2]      resident workgroups per CU of the transposed-conv kernels: 2 beats 4 by 2 % of the step, 1 and 3 are worse
 *   knob_down_per_cu [2]    the same for the stride-2 conv kernels (measured flat 1-4; at least 1)
 *   knob_bwd_per_cu [0]     cap on both for backward launches (0: none)
 *   knob_nt_max [4]         output channels per workgroup tile of the pipelined kernels, in 32-channel blocks
 *   knob_up_nt_max [1]      the same for the transposed-conv kernels (1: more, smaller workgroups at two waves per SIMD; 2 = one wave
 *                           per SIMD measured 2.5 % slower on the step; at least 1)
 *   knob_wave_nt_max [4]    wave-independent tiles for output tiles of up to this many 32-channel blocks
 *   knob_lay22_min_nt [2]   wave-grid layouts (16-bit) for output tiles of at least this many 32-channel blocks
 *   knob_down_waves [8]     waves of the wide stride-2 conv kernels: 8 = 2x4 wave grid on 128-channel tiles and 4x2 on 64-channel
 *                           tiles, 4 = 2x2
 *   knob_lay42 [1]          0: no 4x2 wave grid on 64-channel tiles (they take the 2x2 one)
 *   knob_pipe_max_cout [256]  the pipelined kernels take layers of up to this many output channels
 *   knob_xcd_map [1]        persistent workgroups walk a contiguous range of work items per XCD; applied where the grid is a
 *                           multiple of 8 and each XCD's share of it a multiple of the output-channel tiles (else, and with 0: interleaved)
 *   knob_rev [4]            reverse tile walk (bit 0 output-conv forward, 1 output-conv backward, 2 backward conv kernels,
 *                           3 weight-gradient kernels, 4 forward conv kernels, 5 alternate per launch): a consumer that starts with
 *                           what its producer wrote last finds it in L2 / the memory-side cache
 *   knob_lean [1]           launches kept off the critical chain (bit 0 reparameterisation noise drawn beside the first conv,
 *                           1 BatchNorm backward of encoder block 0 inside its weight-gradient kernel, 2 vae_loss_deferred
 *                           really on a side stream)
 *   knob_pack_grid [128]    workgroups per tensor of the weight-packing kernel (at least 1)
 *   knob_conv1_grid [512]   most workgroups of encoder.0's forward (few workgroups: one f64 atomic per channel each)
 *   knob_fused_grid [256]   persistent workgroups of the use_fused_wgrad kernels (clamped to 1..512)
 *   knob_convout_grid [1536]  persistent workgroups of the output-conv forward kernel, and
 *   knob_convout_bwd_grid [1024]  of its backward kernel: full rounds of what is resident - 768 / 512 - beat 2048 by 1 %
 *   knob_convout_step_grid [1024]  of the fused (train = 2) kernel (swept 512-4096: 1.328 / 1.323 / 1.334 / 1.341 / 1.354 ms; at
 *                           least 1).  Equal to the backward grid so that both partition the tiles alike: bit-identical statistics
 *   knob_convout_bands [0]  bands per image of the row-streaming output-conv kernel (0: chosen by the launcher)
 *   knob_wgrad_tile [1]     weight-gradient channel tile: 1 = 64x32 also where 64x64 would fit (0), 2 = 32x32
 *   knob_wgrad_wide [1]     128x32-channel tiles on 8 waves where the low-res side has >= 128 channels (16-bit)
 *   knob_wgrad_wgs [128]    split-K workgroup target of the weight gradients on a saturated GPU (at most 1024), and
 *   knob_wgrad_wide_wgs [128]  the same for the wide tile: few workgroups keep them out of the input-gradient chain's way (-4 % step time)
 *   knob_wgrad_cap_mb [48]  bound on a layer's split-K slab traffic, MiB (at most 48: the slabs are sized at vae_create)
 *   knob_wgrad_mid8 [0]     eight waves on the 64x32-channel weight-gradient tile (measured slower; diagnostics)
 * Diagnostics:
 *   knob_wgrad_force_simple [0]  take the 64-bit-offset weight-gradient kernel (the fallback for tensors >= 4 GiB) at any size
 *   knob_wgrad_layer_wgs [0]  (layer mask << 16) | workgroups overrides the weight-gradient split of the masked layers
 *   knob_ablate_b [0]       the pipelined conv kernels skip their weight-fragment reloads (and take the deep layers too: the
 *                           workgroup-specialised kernels of use_deep are off while it is set),
 *   knob_skip_wgrad [0]     bit i skips the separate weight-gradient launch of BatchNorm layer i, and
 *   knob_ablate_f [0]       phase ablation of the fused kernels: results are WRONG when any of the three is set - timing experiments only */
int vae_set_option(vae_ctx* ctx, const char* name, int value);
/* The option list itself, without a context: name and default (as above) of option `index`; 0, or -1 past either end. */
int vae_option_info(int index, const char** name, int* default_value);

#ifdef __cplusplus
}
#endif
#endif
