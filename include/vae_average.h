/* C ABI of the weight averaging beside the training step (libvae_step_gfx950.so, beside include/vae_step.h): an exponential moving
 * average (EMA) or an equal average over the tail of a run (SWA; Izmailov et al. 2018, "Averaging Weights Leads to Wider Optima and
 * Better Generalization") of the flat parameter buffer and the BatchNorm buffer, kept in a second pair of buffers that every entry
 * point of vae_step.h takes in place of the first.  Three entry points: the update, the in-place exchange of two buffer pairs, and
 * the initialisation of the small device state the update keeps.
 *
 * Conventions and the stream contract are those of vae_step.h: plain device pointers owned by the caller, work ordered on the
 * explicit stream (the last argument), nothing read back, 0 on success or -1 with "<entry point>: <reason>" in vae_last_error()
 * before anything is enqueued.  No entry point synchronises with the host, none uses an atomic, and every output bit is a function
 * of the arguments and of what the pointers hold: repeated call sequences give identical bits.
 *
 * A SEGMENT is (avg, src, n, src_scale): n floats at avg are averaged towards s = src * src_scale (s = src exactly when src_scale
 * is 1).  An entry point takes two of them - the parameters and the BatchNorm buffer - in one launch; a segment with n == 0 is
 * absent and its pointers are not looked at.
 *
 * THE STATE is VAE_AVG_STATE_BYTES of device memory, 16-byte aligned: int64 seen_step | int64 n_averaged | f64 last_weight |
 * 8 bytes reserved.  It is read by every workgroup of an update and written by one trailing single-thread launch behind them, so a
 * call takes no argument the host has to change from call to call: a sequence of calls captured once may be replayed. */
#ifndef VAE_AVERAGE_H
#define VAE_AVERAGE_H
#include <stdint.h>
#include "vae_step.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VAE_AVG_EMA 0
#define VAE_AVG_EQUAL 1
#define VAE_AVG_STATE_BYTES 32

/* One averaging update of up to two segments (two launches at most: the streaming kernel and the state's commit).
 *   GATE    the update applies iff opt_step == NULL or *opt_step != seen_step.  opt_step is the device step count of the clipped
 *           optimiser (vae_adamw_step_clipped / vae_train_step_fused_clipped), which does not advance on a skipped step: a skipped
 *           step is invisible to the average, with no host read.  Not applied: avg and the state stay bit-unchanged.  Applied:
 *           seen_step = *opt_step (kept when NULL), n_averaged += 1, last_weight = the w used.
 *   WEIGHT  formed on the device in f64 from n = n_averaged before the update, then rounded once to f32:
 *             n == 0         avg = s, a copy (with src_scale == 1: the bits of src, NaN payloads included); last_weight = 1
 *             VAE_AVG_EMA    d = decay, or min(decay, (1 + n) / (warmup + n)) when warmup > 0;  w = 1 - d
 *             VAE_AVG_EQUAL  w = 1 / (n + 1)
 *   ELEMENT torch.lerp's two branches, each one fused multiply-add: with e = avg[i], s as above,
 *             |w| < 0.5:  avg[i] = fmaf(w, s - e, e)          otherwise:  avg[i] = fmaf(-(1.f - w), s - e, s)
 * Refused: null state; a segment with n > 0 and a null avg or src; n < 0; an avg overlapping a src or the other avg; decay outside
 * [0, 1] or NaN; warmup < 0 or NaN; an unknown kind; a src_scale that is not finite; avg, src or state not 16-byte, opt_step not
 * 8-byte aligned.  n == 0 in both segments returns 0 and launches nothing (the state is not touched). */
int vae_average_update(float* avg0, const float* src0, int64_t n0, float src_scale0, float* avg1, const float* src1, int64_t n1,
                       float src_scale1, int kind, double decay, double warmup, const int64_t* opt_step, void* state,
                       vae_stream_t stream);

/* Exchanges a0 with b0 (n0 floats) and a1 with b1 (n1 floats) in place, bit for bit, in one launch and with no temporary: every
 * element is read and written by one lane.  Refused: a pair with n > 0 and a null pointer; n < 0; any two of the buffers
 * overlapping; a pointer not 16-byte aligned.  n == 0 in both pairs returns 0 and launches nothing. */
int vae_average_swap(float* a0, float* b0, int64_t n0, float* a1, float* b1, int64_t n1, vae_stream_t stream);

/* state = {seen_step = *opt_step (read on the device; -1 when opt_step is NULL), n_averaged, last_weight = 0}: a fresh or reloaded
 * average does not take the optimiser's current step for a new one.  Refused: null or misaligned state, n_averaged < 0, opt_step
 * not 8-byte aligned. */
int vae_average_state_init(void* state, const int64_t* opt_step, int64_t n_averaged, vae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
