// Host-side context of the VAE step: shared by the C-ABI translation units (vae_api.hip; vae_util.hip takes the launch helpers
// and nothing of the context) and the per-storage-type translation units (impl_bf16.hip / impl_f16.hip / impl_f32.hip) that
// instantiate the templated launch code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <type_traits>

#include "../../include/vae_step.h"

int vae_set_error(const char* what, const char* why);   // vae_api.hip; message readable through vae_last_error()

#include "common.cuh"

#define LAUNCH_CHECK(name)                                                        \
    do {                                                                          \
        hipError_t _e = hipGetLastError();                                        \
        if (_e != hipSuccess) return vae_set_error(name, hipGetErrorString(_e)); \
    } while (0)

// Every kernel the host code launches starts here, so that the dynamic-LDS limit is raised before every launch that needs it (above
// 48 KiB; nothing fits above 160 KiB) and the launch error is read after every launch (reported under `name`).  Nothing else.
template <typename K, typename... Args>
static int launch(const char* name, K kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args&... args) {
    if (lds_bytes > 160 * 1024) return vae_set_error("lds", "tile needs more than 160 KiB LDS");
    if (lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return vae_set_error("hipFuncSetAttribute", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
    LAUNCH_CHECK(name);
    return 0;
}

// Run-time value -> template argument: returns f(std::integral_constant<int, V>{}) for the V of Vs... that equals v, an error
// under `what` (the launch) when none does.  f is instantiated for every V listed and for no other, so a call site names exactly
// the kernel variants that exist.
template <int... Vs, typename F>
static int pick_const(const char* what, int v, F&& f) {
    int rc = 0;
    const bool found = ((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return found ? rc : vae_set_error(what, "no kernel variant for this value");
}
template <typename F> static int pick_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// Work space of `bytes` from the stream-ordered allocator for what body(char* base) enqueues on `st`.  Requests of up to
// kScratchKeep bytes share ONE block per (device, stream) in the whole library (the table lives in vae_util.hip), kept between calls
// and grown on demand: calls on a stream run in stream order, so each may overwrite what the one before it left.  (An allocation and
// a release per call made the host WAIT: a hipMallocAsync that finds the block of a hipFreeAsync still pending on the stream blocks
// until the stream has passed that release - the second of two calls in a row waited for everything enqueued in front of the first.)
// A block that has become too small is released on the stream behind its last user, after its successor has been allocated; a
// block is never released otherwise: every stream handle such a call has seen keeps up to kScratchKeep bytes for the life of the
// process.  Larger requests, a stream that is being captured, and hipStreamPerThread (one handle value, another stream in every
// thread) are allocated and released per call as before.  The mutex is held while body enqueues: two threads on one stream must not
// interleave there.  body's error wins over a failed free; a failed allocation returns before body runs.
static const size_t kScratchKeep = (size_t)64 << 20;
std::mutex& stream_scratch_mutex();
// the kept block of (current device, st), at least `bytes` large; the caller holds stream_scratch_mutex()
int kept_stream_scratch(size_t bytes, hipStream_t st, char** base);
template <typename F> static int with_stream_scratch(size_t bytes, hipStream_t st, F&& body) {
    // (a stream that is being captured into a graph takes the per-call form too: the allocation and the release become nodes of
    //  that graph, and a block allocated inside a capture must not be handed to calls outside it)
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
    if (bytes > kScratchKeep || capturing != hipStreamCaptureStatusNone || st == hipStreamPerThread) {
        void* ws = nullptr;
        HIP_CHECK_RET(hipMallocAsync(&ws, bytes, st));
        const int rc = body(static_cast<char*>(ws));
        const hipError_t fe = hipFreeAsync(ws, st);
        if (rc) return rc;
        if (fe != hipSuccess) return vae_set_error("hipFreeAsync", hipGetErrorString(fe));
        return 0;
    }
    std::lock_guard<std::mutex> lock(stream_scratch_mutex());
    char* base = nullptr;
    if (kept_stream_scratch(bytes, st, &base)) return -1;
    return body(base);
}

static const int kBnC[8] = {32, 64, 128, 256, 128, 64, 32, 32};
static const char* const kLayerTag[8] = {"encoder.0", "encoder.1", "encoder.2", "encoder.3", "decoder.0", "decoder.1", "decoder.2", "final_layer.0"};   // profiling / debug tag of BN layer i
static const float kSlope = 0.01f;   // nn.LeakyReLU() default (models.py:47,70,79)
static const float kBnEps = 1e-5f;   // nn.BatchNorm2d default eps
static const float kBnMom = 0.1f;    // nn.BatchNorm2d default momentum

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
static inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

struct Tiling { int lth, ltw, lTB, tiles_x, tiles_y; };
static Tiling make_tiling(int Hs, int Ws, int pixels) {
    const int tw = std::min(Ws, pixels >= 128 ? 16 : 8), th = std::min(Hs, pixels / tw), TB = pixels / (th * tw);
    Tiling t; t.lth = ilog2(th); t.ltw = ilog2(tw); t.lTB = ilog2(TB); t.tiles_x = Ws / tw; t.tiles_y = Hs / th;
    return t;
}

struct BnLayer {
    int C, H, W;            // spatial size of the tensor this BN normalises
    double* stat_f; double* stat_b; float* block; void* y; void* dz;
    int p_gamma, p_beta, p_convw, p_convb;
    // deep layers, 16-bit storage: materialised LeakyReLU(BN(y)) / BatchNorm-backward gradient g (written as a side effect by the
    // pipelined kernel that stages the tensor first) for the weight-gradient kernels; *_ok: valid for the current forward / backward
    void* act = nullptr; void* dy = nullptr; int act_ok = 0, dy_ok = 0;
};

// weight packing descriptors (pack_kernel, edge_kernels.cuh): f32 reference layouts -> MFMA B-operand images of T
struct PackDesc {
    const float* src; const float* src2; void* dst;
    int kind;     // 0 conv [A][Bc][9]; 1 fc (mu|var -> [F/8][npad][8]); 2 decoder_input; 3 tap-major f32 copy [9][C]
    int A, Bc, k_is_first, npad, L, s2;
    long n;       // elements of dst
};

// split-K sizing of the weight-gradient kernels; the slabs are sized at vae_create for the defaults.  Every member but small_wgs (the
// workgroup target of a small problem, which wants them everywhere) is the option knob_wgrad_<member>, documented with the others
struct WgradKnobs { int wgs, cap_mb, tile, wide, wide_wgs, small_wgs = 1024, mid8, force_simple; };

// The last forward of a context: which one ran, with what settings, and what it left for vae_loss* / vae_backward* to consume.
// Exactly two functions change which forward is held: begin_forward and drop_forward (below).  Besides them the record is written
// where a forward's product is made or consumed: decode_impl (the output conv ran or was deferred), launch_kl_shape (kl_pending), launch_tc (tc_done),
// backward_first (convout_pending / dlogit_valid / loss_out3), bwd_clear_stats (bwd_dirty), backward_impl (bwd_half_done),
// vae_loss_deferred (loss_out3 / loss_kw of a deferred output conv) and launch_conv_pipe (walk_dir).  target: begin_forward moves the
// context's pending vae_set_recon_target into it (a FULL forward only; null otherwise), and vae_forward fills in x where none was pending.
struct FwdRecord {
    enum Kind { NONE, FULL, ENCODE, DECODE };   // FULL: vae_forward and the training steps; vae_backward_ex differentiates whichever it was
    Kind kind = NONE;
    int B = 0, trained = 0;                      // batch (the batch statistics' count); the forward's `train` argument
    // settings the forward ran with (vae_set_recon_loss[_ex] / vae_set_kl_objective at that time): its deferred output conv, loss and
    // backward use these, whatever the context's settings are by then.  Kinds without an ELBO record VAE_KL_PLAIN.
    // recon_param: pos_weight of VAE_RECON_WBCE (0 for the other terms).
    int recon = VAE_RECON_BCE, kl_kind = VAE_KL_PLAIN; double kl_param = 0.0; double recon_param = 0.0;
    int kl_pending = 0;                          // kl_shape_kernel / the tc_* kernels of this forward are in flight on side stream KL_SIDE: consumers wait for ev_kl
    int kl_reduced = 0;                          // kl_shape_kernel ran for this forward: kl_d and KL are in kl_ws (behind ev_kl)
    int tc_done = 0;                             // this forward's total correlation and its gradient are in tc_ws (launch_tc; behind ev_kl as well)
    const float* x = nullptr; float *xhat = nullptr, *mu = nullptr, *lv = nullptr, *z = nullptr;   // the caller's tensors (null: the kind has none)
    // what the reconstruction term is taken against (vae_set_recon_target; x itself by default): read by every output-conv kernel, in the
    // forward or deferred into the backward.  The encoder, conv1_wgrad and dx read x.  FULL forwards only: null for the other kinds.
    const float* target = nullptr;
    // f16 storage: the backward runs on gradients multiplied by gmul (a power of two chosen per forward so that the stored
    // dz stay inside the f16 range: the BCE mean makes them O(1/(B*H*W))); every parameter gradient is written times ginv.
    // The backward is linear in the upstream gradient, so this changes no f32 result (powers of two are exact).  1 otherwise.
    float gmul = 1.f, ginv = 1.f;
    // use_fused_convout: a forward with train = 2 (the fused training step) leaves the output conv, sigmoid and BCE to the
    // backward, where ONE kernel does forward and backward of that layer in one pass over y7 (conv_mfma.cuh:
    // convout_step_mfma_kernel).  convout_pending: such a forward is waiting for its backward; pending_f7: the BatchNorm
    // finalisation that kernel's prologue performs; loss_out3 / loss_kw: where vae_loss_deferred wants the ELBO scalars.
    // dlogit_valid: the output conv's gradient of this forward is in c->dlogit and has not been consumed.
    int convout_pending = 0, dlogit_valid = 0; BnFuse pending_f7; float* loss_out3 = nullptr; float loss_kw = 0.f;
    int bwd_dirty = 1;       // the backward statistics need clearing (a forward zeroes every accumulator; a backward dirties its own)
    int bwd_half_done = 0;   // vae_backward_part 1 ran, part 2 may follow
    int walk_dir = 0;        // knob_rev bit 5: tile-walk direction of the next pipelined launch
    explicit operator bool() const { return kind != NONE; }
};

struct vae_ctx {
    // ---- geometry and layouts, fixed at vae_create ----
    int H, L, maxB, dtype, gen, s, s2; int64_t F; int npad_fc, npad_di; size_t esz;
    int64_t poff[VAE_NUM_PARAMS], psz[VAE_NUM_PARAMS], ptotal, bnoff[8], bnc[8], bntotal;
    // ---- resources: device buffers, streams, events ----
    BnLayer lay[8];
    void *d0, *dd0;
    float *eps, *dlat, *dlogit, *dlogit2, *ident, *wout_t;
    void* wp_fwd[8]; void* wp_dg[8];   // indexed by BN layer id (1..7); [0] unused
    void *fcpack, *dipack;
    PackDesc* d_descs; std::vector<PackDesc> h_descs; const float* packed_for = nullptr;
    float* slab; size_t slab_floats;
    // side streams for work only the optimiser consumes (weight gradients, their split-K reductions) and for weight packing
    static constexpr int NSIDE = 3, NFORK = 16;
    hipStream_t side[NSIDE]; float* side_slab[NSIDE]; hipEvent_t ev_fork[NFORK], ev_join[NSIDE], ev_pack; int side_rr = 0, fork_rr = 0, n_side_ok = 0;
    static constexpr int NBUCKET = 2; hipEvent_t ev_bucket[NBUCKET];   // bucketed gradient exchange (vae_train_step_fused): bucket i reduced on the communication stream
    hipStream_t comm; hipEvent_t ev_comm; int comm_busy = 0;   // stream lent to the caller for the mid-backward gradient all-reduce (vae_comm_stream)
    void* nccl_comm = nullptr; int comm_rank = 0, comm_world = 0;   // RCCL communicator owned by the context (vae_comm.hip)
    double* dstats; size_t n_dstats; double* accum;  // accum: [0] reconstruction term (BCE / MSE sum), [1] kl term, [2] sum dlogit
    float* reduce_tmp = nullptr; size_t reduce_tmp_floats = 0; unsigned reduce_slot = 0;   // partial sums of the two-level slab reduction
    float* fused_slab[3] = {nullptr, nullptr, nullptr}; size_t fused_slab_floats = 0;   // split-K slabs of the fused dgrad+wgrad kernels (layers 7, 6, 1)
    // kl_ws (allocated on first use): kl_d [L] f64 | scalars {T, KL} f64 | factor [L] f32 (kl_tk: the ticket word, a 16-byte block of its
    // own), written by kl_shape_kernel on side stream KL_SIDE; ev_kl follows it (fwd.kl_pending: consumers of this forward must wait for it)
    static constexpr int KL_SIDE = 2;
    void* kl_ws = nullptr; unsigned* kl_tk = nullptr; hipEvent_t ev_kl = nullptr;
    unsigned long long* kl_d() const { return static_cast<unsigned long long*>(kl_ws); }
    double* kl_scal() const { return reinterpret_cast<double*>(kl_d() + L); }
    float* kl_factor() const { return reinterpret_cast<float*>(kl_scal() + 2); }
    const double* kl_shaped() const { return fwd.kl_kind != VAE_KL_PLAIN ? kl_scal() : nullptr; }   // loss_finalize_kernel's argument
    // tc_ws (allocated on first use, for the largest batch asked for so far): the total-correlation gradient [B][2L] f32 | the
    // work space of the tc_* kernels (total_corr.cuh), written on side stream KL_SIDE by launch_tc
    void* tc_ws = nullptr; size_t tc_ws_bytes = 0; int tc_ws_B = 0;
    float* tc_grad() const { return static_cast<float*>(tc_ws); }
    // vae_log_likelihood: ps_part (non-null only during its decoder passes) switches the output conv to its per-sample mode
    // (tile partials, target x[b mod ps_tb]; ps_ntile: tiles per image of the kernel taken).  ll_*: its scratch, allocated on first use.
    double* ps_part = nullptr; int ps_tb = 0, ps_ntile = 0;
    float* ll_f = nullptr; double* ll_part = nullptr; double* ll_lat = nullptr;   // ll_f: mu | lv | z0 [maxB*L] | z [maxB*L]
    double* ll_kb = nullptr; size_t ll_kb_n = 0;                                   // [K*B] log p(x|z) | [K*B] log w (grown per call)
    std::vector<void*> allocs; int64_t ws_bytes = 0;
    // ---- tuning switches: plain ints read directly where a launch is shaped.  Names, defaults and the clamps applied on set are the
    // rows of kOptions (vae_api.hip), which vae_create and vae_set_option go through; what each one does, and what was measured with
    // it, is documented once, at vae_set_option in include/vae_step.h ----
    int use_tr16, use_mfma_convout, use_pipelined, use_side_stream, use_fused_bn, use_fused_convout, use_fused_wgrad, use_recomp_dz, use_raw_wgrad,
        use_deep, use_latent_mfma, use_convout_stream, use_dnf_stream, use_upf_stream, use_fc_dgrad8, use_wgrad_split;
    int knob_up_per_cu, knob_down_per_cu, knob_bwd_per_cu, knob_nt_max, knob_up_nt_max, knob_wave_nt_max, knob_lay22_min_nt, knob_lay42,
        knob_down_waves, knob_pipe_max_cout, knob_xcd_map, knob_rev, knob_lean, knob_pack_grid, knob_conv1_grid, knob_fused_grid,
        knob_convout_grid, knob_convout_bwd_grid, knob_convout_step_grid, knob_convout_bands, knob_wgrad_layer_wgs,
        knob_skip_wgrad, knob_ablate_b, knob_ablate_f;
    WgradKnobs wk;
    // ---- settings for the forwards that follow (vae_set_recon_loss[_ex], vae_set_kl_objective); a forward snapshots them into its record ----
    int recon = VAE_RECON_BCE, kl_kind = VAE_KL_PLAIN; double kl_param = 0.0; double recon_param = 0.0;
    const float* recon_target = nullptr;   // vae_set_recon_target: one-shot, consumed (and cleared) by the next begin_forward
    // ---- the last forward ----
    FwdRecord fwd;
    // ---- diagnostics: phase stamps (vae_debug_stamps) and per-kernel timing (bench.py roofline: HIP events on the launch stream) ----
    long long* dbg_buf = nullptr; char dbg_tag[32] = {0}; int dbg_epi = 0;
    int prof = 0; const char* tag = nullptr; struct ProfRec { std::string name; hipEvent_t e0, e1; double bytes, flops; int side; int launches = 1; }; std::vector<ProfRec> prof_recs;
    hipStream_t cur_stream = nullptr; bool cur_stream_set = false;   // the caller's stream of the call in progress (profiling: tells critical-chain launches from side-stream ones)
};

// RAII: brackets the launches of one logical kernel with events when profiling is on.
struct ProfScope {
    vae_ctx* c; hipStream_t st; int idx;
    ProfScope(vae_ctx* c_, const char* name, double bytes, double flops, hipStream_t st_) : c(c_), st(st_), idx(-1) {
        if (!c || !c->prof) return;
        vae_ctx::ProfRec r; r.name = std::string(name) + (c->tag ? std::string(" @") + c->tag : std::string()); r.bytes = bytes; r.flops = flops;
        r.side = (c->cur_stream_set && st != c->cur_stream) ? 1 : 0;   // (the legacy default stream is the null handle)
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
        (void)hipEventRecord(r.e0, st);
        c->prof_recs.push_back(r); idx = (int)c->prof_recs.size() - 1;
    }
    ~ProfScope() { if (idx >= 0) (void)hipEventRecord(c->prof_recs[idx].e1, st); }
    ProfScope(const ProfScope&) = delete;              // a copy would record the end event twice
    ProfScope& operator=(const ProfScope&) = delete;
};

static inline size_t wgrad_slab_floats(const WgradKnobs& k, int B, int Hs, int Ws, int CA, int CB, int* nsplit_out, int* tps_out, int* WA_out, int* WB_out,
                                       bool wide_ok = false, bool big = false) {
    int WA, WB;
    if (wide_ok && k.wide && CA >= 128 && k.tile == 1) { WA = 4; WB = 1; }
    else if (CA >= 64 && CB >= 64 && k.tile == 0) { WA = 2; WB = 2; } else if (CA >= 64 && k.tile <= 1) { WA = 2; WB = 1; } else { WA = 1; WB = 1; }
    Tiling t = make_tiling(Hs, Ws, WG_KP);
    const int TB = 1 << t.lTB;
    const int n_tiles = ((B + TB - 1) / TB) * t.tiles_x * t.tiles_y;
    const int chan_tiles = (CA / (32 * WA)) * (CB / (32 * WB));
    const size_t per = (size_t)9 * CA * CB;
    int nsplit = std::max(1, (!big ? k.small_wgs : (WA == 4 ? k.wide_wgs : k.wgs)) / chan_tiles);
    const size_t cap = ((size_t)k.cap_mb << 20) / 4;  // bound slab traffic to 48 MiB per layer
    nsplit = (int)std::min<size_t>(nsplit, std::max<size_t>(1, cap / per));
    nsplit = std::min(nsplit, n_tiles);
    const int tps = (n_tiles + nsplit - 1) / nsplit;
    nsplit = (n_tiles + tps - 1) / tps;
    *nsplit_out = nsplit; *tps_out = tps; *WA_out = WA; *WB_out = WB;
    return per * nsplit;
}

// f16 storage: the gradient scale of a backward over B images (FwdRecord::gmul / ginv); 1 for the other storage types
static inline void set_grad_scale(vae_ctx* c, int B) {
    // dL/dlogit is O(1/(B*H*W)), far below the smallest f16 normal; 2^ceil(log2(B*H*W)) / 16 puts the stored dz around 2^-4, mid-range
    // VAE_RECON_WBCE (the record's recon / recon_param are set before this runs): |dlogit| <= w/N instead of 1/N, since |BCE dlogit|
    // <= 1/N and the cell weight 1 + (w - 1) t lies between 1 and w.  For w > 1 the exponent is lowered by k = ceil(log2 w), clamped
    // at 0: w / 2^k <= 1, so |dlogit * gmul| <= 2^e0 / N with e0 the BCE exponent - the bound every stored product downstream was
    // sized for; nothing can overflow that could not with BCE.  The price is range at the bottom: the non-note cells (W = 1) sit k
    // binades lower, 2^-(4+k) typical; at the largest weight (k = 10) that is still 2^-14, the smallest f16 normal, and the f16
    // layer-local gate holds at w = 8 and 32 (tests/test_pos_weight_gpu.py).  w <= 1 only shrinks the gradient: unchanged.
    c->fwd.gmul = 1.f; c->fwd.ginv = 1.f;
    if (c->dtype == VAE_DTYPE_F16) {
        int e = std::max(0, ilog2(B) + 2 * ilog2(c->H) - 4);
        // (only a forward that an ELBO follows: vae_encode / vae_decode have no reconstruction gradient of the library's)
        if (c->fwd.kind == FwdRecord::FULL && c->fwd.recon == VAE_RECON_WBCE && c->fwd.recon_param > 1.0) e = std::max(0, e - (int)ceil(log2(c->fwd.recon_param)));
        c->fwd.gmul = ldexpf(1.f, e); c->fwd.ginv = ldexpf(1.f, -e);
    }
}

// every entry point that launches on behalf of the context: the caller's stream of the call in progress (profiling)
static inline void enter(vae_ctx* c, hipStream_t st) { c->cur_stream = st; c->cur_stream_set = true; }

// The context holds no forward: nothing to score or differentiate until the next begin_forward.
static inline void drop_forward(vae_ctx* c) {
    FwdRecord& f = c->fwd;
    f.kind = FwdRecord::NONE; f.B = 0; f.trained = 0;
    f.kl_pending = 0; f.kl_reduced = 0; f.tc_done = 0; f.convout_pending = 0; f.dlogit_valid = 0; f.loss_out3 = nullptr; f.bwd_half_done = 0;
}
// A forward of `kind` over B images starts on `st`: the previous one is gone, the settings are snapshotted, and the statistics'
// memset is the first thing enqueued on `st`.  The entry point then records the caller tensors this kind has (the rest stay null).
static inline int begin_forward(vae_ctx* c, FwdRecord::Kind kind, int B, int train, hipStream_t st) {
    enter(c, st);
    drop_forward(c);
    HIP_CHECK_RET(hipMemsetAsync(c->dstats, 0, c->n_dstats * sizeof(double), st));
    FwdRecord& f = c->fwd;
    f.kind = kind; f.B = B; f.trained = train; f.bwd_dirty = 0; f.recon = c->recon; f.recon_param = c->recon_param;
    const bool elbo = kind == FwdRecord::FULL;   // (no ELBO follows an encoder-only or decoder-only pass)
    f.kl_kind = elbo ? c->kl_kind : VAE_KL_PLAIN; f.kl_param = elbo ? c->kl_param : 0.0;
    f.x = nullptr; f.xhat = f.mu = f.lv = f.z = nullptr;
    f.target = elbo ? c->recon_target : nullptr; c->recon_target = nullptr;   // one-shot: whichever forward comes next consumes it, only a FULL one uses it
    if (kind != FwdRecord::DECODE) f.walk_dir = 1;   // (a pass through the encoder restarts the alternating tile walk)
    set_grad_scale(c, B);
    return 0;
}

// side streams (vae_api.hip)
struct SideFork { hipStream_t st; float* slab; int rc; };
SideFork fork_side(vae_ctx* c, hipStream_t st, int which = -1);
int join_sides(vae_ctx* c, hipStream_t st);
int join_comm(vae_ctx* c, hipStream_t st);
// KL objectives (vae_api.hip): the reduction of the last forward's mu / log_var on side stream KL_SIDE, forked from `st`; and the
// wait a consumer's stream needs before it reads the factors / scalars (nothing when no reduction is outstanding)
int launch_kl_shape(vae_ctx* c, hipStream_t st);
int join_kl(vae_ctx* c, hipStream_t st);
int launch_tc(vae_ctx* c, hipStream_t st);   // total correlation of the held forward and its gradient, same stream and event (vae_api.hip)
int launch_loss_finalize(vae_ctx* c, float* out3, float kld_weight, hipStream_t st);   // loss_finalize_kernel for the last forward (vae_api.hip)

// entry points instantiated once per storage type (impl_bf16.hip, impl_f16.hip, impl_f32.hip)
template <typename T> int pack_weights(vae_ctx* c, const float* params, hipStream_t st);
template <typename T> int forward_impl(vae_ctx* c, const float* x, int B, const float* params, float* bn_running, int64_t* nbt,
                                       const float* eps, uint64_t seed, int train, float* xhat, float* mu, float* lv, float* z, hipStream_t st);
template <typename T> int encode_impl(vae_ctx* c, const float* x, int B, const float* params, float* bn_running, int64_t* nbt,
                                      const float* eps, uint64_t seed, int train, float* mu, float* lv, float* z, hipStream_t st);
template <typename T> int decode_impl(vae_ctx* c, const float* z, int B, const float* params, float* bn_running, int64_t* nbt, int train,
                                      const float* x, float* xhat, hipStream_t st);
template <typename T> int backward_impl(vae_ctx* c, const float* x, const float* params, float* grads, const float* g_xhat, const float* gscale,
                                        const float* g_mu, const float* g_lv, const float* g_z, const float* g_pre, float kld_weight, int add_kl,
                                        int part, hipStream_t st);
template <typename T> int backward_ex_impl(vae_ctx* c, const float* x, const float* params, float* grads, const float* g_xhat, const float* gscale,
                                           const float* g_mu, const float* g_lv, const float* g_z, const float* g_pre, float kld_weight, int add_kl,
                                           float* dx, float* dz, hipStream_t st);
template <typename T> int pre_latents_impl(vae_ctx* c, float* out, hipStream_t st);
template <typename T> int debug_tensor_impl(vae_ctx* c, const void* src, float* out, long n, int C, int HW, hipStream_t st);

#define VAE_INSTANTIATE(T)                                                                                                              \
    template int pack_weights<T>(vae_ctx*, const float*, hipStream_t);                                                                  \
    template int forward_impl<T>(vae_ctx*, const float*, int, const float*, float*, int64_t*, const float*, uint64_t, int, float*,     \
                                 float*, float*, float*, hipStream_t);                                                                  \
    template int encode_impl<T>(vae_ctx*, const float*, int, const float*, float*, int64_t*, const float*, uint64_t, int, float*,      \
                                float*, float*, hipStream_t);                                                                           \
    template int decode_impl<T>(vae_ctx*, const float*, int, const float*, float*, int64_t*, int, const float*, float*, hipStream_t);  \
    template int backward_impl<T>(vae_ctx*, const float*, const float*, float*, const float*, const float*, const float*, const float*, \
                                  const float*, const float*, float, int, int, hipStream_t);                                            \
    template int backward_ex_impl<T>(vae_ctx*, const float*, const float*, float*, const float*, const float*, const float*, const float*, \
                                     const float*, const float*, float, int, float*, float*, hipStream_t);                               \
    template int pre_latents_impl<T>(vae_ctx*, float*, hipStream_t);                                                                    \
    template int debug_tensor_impl<T>(vae_ctx*, const void*, float*, long, int, int, hipStream_t);

// storage-type dispatch: VAE_DISPATCH(c->dtype, forward_impl, (c, ...))
#define VAE_DISPATCH(dtype, fn, args) ((dtype) == VAE_DTYPE_BF16 ? fn<bf16> args : (dtype) == VAE_DTYPE_F16 ? fn<f16> args : fn<float> args)
