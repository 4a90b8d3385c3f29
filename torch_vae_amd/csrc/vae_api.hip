// Context and the C ABI (include/vae_step.h) of the VAE step.  The launch sequencing is templated on the storage
// type and lives in vae_impl.cuh, instantiated by impl_bf16.hip / impl_f16.hip / impl_f32.hip.  The entry points that need neither the
// context nor a helper of this file are in vae_util.hip.
#include <map>
#include <mutex>
#include "vae_ctx.h"
#include "edge_kernels.cuh"
#include "loglik.cuh"
#include "grad_clip.cuh"
#include "total_corr.cuh"

static thread_local std::string g_err;
int vae_set_error(const char* what, const char* why) {
    g_err = std::string(what) + ": " + why;
    return -1;
}

// ---------------------------------------------------------------------------
extern "C" const char* vae_last_error(void) { return g_err.c_str(); }
extern "C" int vae_abi_version(void) { return 1; }

static void param_shapes(int H, int L, int gen, int64_t* sizes) {
    const int s = gen ? H / 16 : 2;
    const int64_t F = 256LL * s * s;
    const int enc_ci[4] = {1, 32, 64, 128}, enc_co[4] = {32, 64, 128, 256};
    int k = 0;
    for (int i = 0; i < 4; ++i) { sizes[k++] = 9LL * enc_ci[i] * enc_co[i]; sizes[k++] = enc_co[i]; sizes[k++] = enc_co[i]; sizes[k++] = enc_co[i]; }
    sizes[k++] = L * F; sizes[k++] = L; sizes[k++] = L * F; sizes[k++] = L; sizes[k++] = F * L; sizes[k++] = F;
    const int dec_ci[3] = {256, 128, 64}, dec_co[3] = {128, 64, 32};
    for (int i = 0; i < 3; ++i) { sizes[k++] = 9LL * dec_ci[i] * dec_co[i]; sizes[k++] = dec_co[i]; sizes[k++] = dec_co[i]; sizes[k++] = dec_co[i]; }
    sizes[k++] = 9 * 32 * 32; sizes[k++] = 32; sizes[k++] = 32; sizes[k++] = 32; sizes[k++] = 9 * 32; sizes[k++] = 1;
}

extern "C" int vae_param_layout(int H, int L, int gen, int64_t* offsets, int64_t* sizes, int64_t* total) {
    if (H < 32 || (H & (H - 1)) || (!gen && H != 32)) return vae_set_error("vae_param_layout", "img_size must be a power of two >= 32 (exactly 32 unless generalised)");
    if (L < 1 || L > 4096) return vae_set_error("vae_param_layout", "latent_dim must be in 1..4096");
    param_shapes(H, L, gen, sizes);
    int64_t off = 0;
    for (int i = 0; i < VAE_NUM_PARAMS; ++i) { offsets[i] = off; off += align_up(sizes[i], 64); }
    *total = off;
    return 0;
}
extern "C" int vae_bn_layout(int64_t* offsets, int64_t* channels, int64_t* total) {
    int64_t off = 0;
    for (int i = 0; i < 8; ++i) { offsets[i] = off; channels[i] = kBnC[i]; off += 2 * kBnC[i]; }
    *total = off;
    return 0;
}

template <typename T> static T* dalloc(vae_ctx* c, size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n * sizeof(T), 256)) != hipSuccess) return nullptr;
    c->allocs.push_back(p); c->ws_bytes += (int64_t)std::max<size_t>(n * sizeof(T), 256);
    return reinterpret_cast<T*>(p);
}

// Side streams and the communication stream are per DEVICE, shared by every context of the process: each extra stream
// beyond HIP's hardware queues (GPU_MAX_HW_QUEUES) shares a queue with another and serialises with it - a second model
// in the process (evaluation copy, another batch size) used to slow the first one's step down by up to 3x.  Contexts of
// one device enqueue in host order, so sharing costs them nothing.  The streams live for the process.
struct DevStreams { hipStream_t side[vae_ctx::NSIDE]; hipStream_t comm; };
static DevStreams* device_streams(int side_prio) {
    static std::mutex mu;
    static std::map<int, DevStreams*> pool;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto it = pool.find(dev);
    if (it != pool.end()) return it->second;
    DevStreams* d = new DevStreams();
    bool ok = true;
    for (int i = 0; i < vae_ctx::NSIDE && ok; ++i) ok = hipStreamCreateWithPriority(&d->side[i], hipStreamNonBlocking, side_prio) == hipSuccess;
    {   // communication stream; VAE_COMM_STREAM_PRIO = high | low picks another priority class (diagnostics of the queue mapping)
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        const char* e = getenv("VAE_COMM_STREAM_PRIO");
        if (e && (!strcmp(e, "high") || !strcmp(e, "low"))) ok = ok && hipStreamCreateWithPriority(&d->comm, hipStreamNonBlocking, !strcmp(e, "high") ? hi : lo) == hipSuccess;
        else ok = ok && hipStreamCreateWithFlags(&d->comm, hipStreamNonBlocking) == hipSuccess;
    }
    if (!ok) { delete d; return nullptr; }
    pool[dev] = d;
    return d;
}

extern "C" void vae_destroy(vae_ctx* c) {
    if (!c) return;
    (void)vae_comm_destroy(c);
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->ll_kb) (void)hipFree(c->ll_kb);
    if (c->n_side_ok) {
        // (the streams belong to the device pool; work of this context still on them is drained first)
        for (int i = 0; i < vae_ctx::NSIDE; ++i) { (void)hipStreamSynchronize(c->side[i]); (void)hipEventDestroy(c->ev_join[i]); }
        (void)hipStreamSynchronize(c->comm);
        for (int i = 0; i < vae_ctx::NFORK; ++i) (void)hipEventDestroy(c->ev_fork[i]);
        (void)hipEventDestroy(c->ev_pack); (void)hipEventDestroy(c->ev_comm);
        if (c->ev_kl) (void)hipEventDestroy(c->ev_kl);
        for (int i = 0; i < vae_ctx::NBUCKET; ++i) (void)hipEventDestroy(c->ev_bucket[i]);
    }
    delete c;
}
extern "C" int64_t vae_workspace_bytes(const vae_ctx* c) { return c ? c->ws_bytes : 0; }

// ---- tuning / diagnostic switches ------------------------------------------------------------------------------------------
// One row per option: name, the int it controls, the default and the normaliser applied on set - the default is in set-value
// terms, i.e. the value that, passed to vae_set_option, restores the default behaviour.  vae_create and vae_set_option go through
// this table and nothing else does: the members are plain ints read directly where a launch is shaped.  What each option does is
// documented at vae_set_option in include/vae_step.h (tests/test_options_host.py holds the two lists together).
struct OptionDef { const char* name; int& (*ref)(vae_ctx&); int def; int (*norm)(int); };
static int opt_any(int v) { return v; }
static int opt_min1(int v) { return std::max(1, v); }
static int opt_fused_grid(int v) { return std::max(1, std::min(v, 512)); }   // the fused kernels' slabs hold 512 workgroups
static int opt_max1024(int v) { return std::min(v, 1024); }
static int opt_max48(int v) { return std::min(v, 48); }                      // the slabs are sized for 48 MiB per layer at vae_create
static int opt_fused_wgrad(int v) { return v == 1 ? 3 : v == 2 ? 1 : v == 3 ? 2 : 0; }   // 1 all, 2 decoder side only, 3 encoder.1 only -> bit 0 decoder (ConvT) kernels, bit 1 encoder.1 kernel
#define OPT(member, def, norm) {#member, [](vae_ctx& c) -> int& { return c.member; }, def, norm}
#define OPT_WK(member, def, norm) {"knob_wgrad_" #member, [](vae_ctx& c) -> int& { return c.wk.member; }, def, norm}
static const OptionDef kOptions[] = {
    OPT(use_tr16, 1, opt_any), OPT(use_mfma_convout, 1, opt_any), OPT(use_pipelined, 1, opt_any), OPT(use_side_stream, 1, opt_any),
    OPT(use_fused_bn, 1, opt_any), OPT(use_fused_convout, 1, opt_any), OPT(use_fused_wgrad, 1, opt_fused_wgrad), OPT(use_recomp_dz, 0, opt_any),
    OPT(use_raw_wgrad, 0, opt_any), OPT(use_deep, 1, opt_any), OPT(use_latent_mfma, 6, opt_any), OPT(use_convout_stream, 1, opt_any),
    OPT(use_dnf_stream, 1, opt_any), OPT(use_upf_stream, 1, opt_any), OPT(use_fc_dgrad8, 1, opt_any), OPT(use_wgrad_split, 1, opt_any),
    OPT(knob_up_per_cu, 2, opt_any), OPT(knob_down_per_cu, 2, opt_min1), OPT(knob_bwd_per_cu, 0, opt_any), OPT(knob_nt_max, 4, opt_any),
    OPT(knob_up_nt_max, 1, opt_min1), OPT(knob_wave_nt_max, 4, opt_any), OPT(knob_lay22_min_nt, 2, opt_any), OPT(knob_lay42, 1, opt_any),
    OPT(knob_down_waves, 8, opt_any), OPT(knob_pipe_max_cout, 256, opt_any), OPT(knob_xcd_map, 1, opt_any), OPT(knob_rev, 4, opt_any),
    OPT(knob_lean, 1, opt_any), OPT(knob_pack_grid, 128, opt_min1), OPT(knob_conv1_grid, 512, opt_any), OPT(knob_fused_grid, 256, opt_fused_grid),
    OPT(knob_convout_grid, 1536, opt_any), OPT(knob_convout_bwd_grid, 1024, opt_any), OPT(knob_convout_step_grid, 1024, opt_min1),
    OPT(knob_convout_bands, 0, opt_any), OPT(knob_wgrad_layer_wgs, 0, opt_any), OPT(knob_skip_wgrad, 0, opt_any), OPT(knob_ablate_b, 0, opt_any),
    OPT(knob_ablate_f, 0, opt_any),
    OPT_WK(tile, 1, opt_any), OPT_WK(wide, 1, opt_any), OPT_WK(mid8, 0, opt_any), OPT_WK(force_simple, 0, opt_any),
    OPT_WK(wgs, 128, opt_max1024), OPT_WK(wide_wgs, 128, opt_max1024), OPT_WK(cap_mb, 48, opt_max48),
};
#undef OPT_WK
#undef OPT
static const OptionDef* find_option(const char* name) {
    for (const OptionDef& o : kOptions) if (name && !strcmp(name, o.name)) return &o;
    return nullptr;
}

extern "C" vae_ctx* vae_create(int H, int L, int maxB, int dtype, int gen) {
    vae_ctx* c = new vae_ctx();
    c->H = H; c->L = L; c->maxB = maxB; c->dtype = dtype; c->gen = gen;
    for (const OptionDef& o : kOptions) o.ref(*c) = o.norm(o.def);
    if (getenv("VAE_NO_SIDE_STREAM")) c->use_side_stream = 0;   // diagnostics: everything on the caller's stream
    if (vae_param_layout(H, L, gen, c->poff, c->psz, &c->ptotal) != 0) { delete c; return nullptr; }
    if (dtype != VAE_DTYPE_F32 && dtype != VAE_DTYPE_BF16 && dtype != VAE_DTYPE_F16) { vae_set_error("vae_create", "bad dtype"); delete c; return nullptr; }
    if (maxB < 1) { vae_set_error("vae_create", "max_batch < 1"); delete c; return nullptr; }
    vae_bn_layout(c->bnoff, c->bnc, &c->bntotal);
    c->s = gen ? H / 16 : 2; c->s2 = c->s * c->s; c->F = 256LL * c->s2;
    c->npad_fc = (int)align_up(2 * L, 32); c->npad_di = (int)align_up(L, 32);
    c->esz = dtype == VAE_DTYPE_F32 ? 4 : 2;
    const size_t B = maxB;
    // BN'd tensors: encoder outputs H/2..H/16, decoder outputs 2s..8s, final convT output H.
    const int hs[8] = {H / 2, H / 4, H / 8, H / 16, 2 * c->s, 4 * c->s, 8 * c->s, 16 * c->s};
    size_t nd = 0;
    for (int i = 0; i < 8; ++i) nd += 4 * kBnC[i];
    nd *= STAT_R;                       // replicas (common.cuh: STAT_R)
    c->n_dstats = nd + 8 * STAT_R;
    c->dstats = dalloc<double>(c, c->n_dstats);
    bool ok = c->dstats != nullptr;
    double* dp = c->dstats;
    for (int i = 0; i < 8 && ok; ++i) {
        BnLayer& l = c->lay[i];
        l.C = kBnC[i]; l.H = hs[i]; l.W = hs[i];
        l.stat_f = dp; dp += 2 * l.C * STAT_R;
        const size_t n = B * l.H * l.W * l.C;
        l.y = dalloc<char>(c, n * c->esz); l.dz = dalloc<char>(c, n * c->esz); l.block = dalloc<float>(c, LC_ROWS * l.C);
        ok = l.y && l.dz && l.block;
        const int base = i < 4 ? 4 * i : (i < 7 ? 22 + 4 * (i - 4) : 34);
        l.p_convw = base; l.p_convb = base + 1; l.p_gamma = base + 2; l.p_beta = base + 3;
    }
    for (int i = 0; i < 8; ++i) { c->lay[i].stat_b = dp; dp += 2 * kBnC[i] * STAT_R; }
    c->accum = dp;
    if (ok) {
        c->d0 = dalloc<char>(c, B * c->F * c->esz); c->dd0 = dalloc<char>(c, B * c->F * c->esz);
        c->eps = dalloc<float>(c, B * L); c->dlat = dalloc<float>(c, B * 2 * L);
        c->dlogit = dalloc<float>(c, B * H * H); c->dlogit2 = dalloc<float>(c, B * H * H); c->ident = dalloc<float>(c, 3 * 256); c->wout_t = dalloc<float>(c, 288);
        ok = c->d0 && c->dd0 && c->eps && c->dlat && c->dlogit && c->dlogit2 && c->ident && c->wout_t;
    }
    // packed weight images
    const int ci[8] = {1, 32, 64, 128, 256, 128, 64, 32}, co[8] = {32, 64, 128, 256, 128, 64, 32, 32};
    for (int i = 1; i < 8 && ok; ++i) {
        const size_t n = (size_t)9 * ci[i] * co[i];
        c->wp_fwd[i] = dalloc<char>(c, n * c->esz); c->wp_dg[i] = dalloc<char>(c, n * c->esz);
        ok = c->wp_fwd[i] && c->wp_dg[i];
    }
    if (ok) {
        c->fcpack = dalloc<char>(c, (size_t)c->F * c->npad_fc * c->esz);
        c->dipack = dalloc<char>(c, (size_t)c->F * c->npad_di * c->esz);
        c->d_descs = dalloc<PackDesc>(c, 32);
        ok = c->fcpack && c->dipack && c->d_descs;
    }
    // slab: max over all split-K users
    size_t slab = 2048 * 288;  // conv1 wgrad / convout bwd: up to 2048 workgroups x 288
    if (ok) {
        int a, b2, wa, wb;
        for (int wide = 0; wide < 2; ++wide)      // both tile shapes (the wide one exists for 16-bit storage only), small- and large-problem targets
            for (int big = 0; big < 2; ++big) {
                if (wide && dtype == VAE_DTYPE_F32) continue;
                for (int i = 1; i < 4; ++i) slab = std::max(slab, wgrad_slab_floats(c->wk, maxB, c->lay[i].H, c->lay[i].W, co[i], ci[i], &a, &b2, &wa, &wb, wide != 0, big != 0));
                for (int i = 4; i < 8; ++i) slab = std::max(slab, wgrad_slab_floats(c->wk, maxB, c->lay[i].H / 2, c->lay[i].W / 2, ci[i], co[i], &a, &b2, &wa, &wb, wide != 0, big != 0));
            }
        const size_t ksteps = c->F / 16;
        slab = std::max(slab, (size_t)std::min<size_t>(ksteps, 512) * maxB * c->npad_fc);
        slab = std::max(slab, (size_t)std::min<size_t>(ksteps, 512) * maxB * c->npad_di);
        slab = std::max(slab, (size_t)8 * (2 * (size_t)L * c->F + c->F));   // fc / decoder_input weight-gradient batch slices
        c->slab_floats = slab;
        c->slab = dalloc<float>(c, slab);
        ok = c->slab != nullptr;
        for (int i = 0; i < vae_ctx::NSIDE && ok; ++i) { c->side_slab[i] = dalloc<float>(c, slab); ok = c->side_slab[i] != nullptr; }
        if (ok) {
            // side-stream priority: VAE_SIDE_PRIORITY=low|high (default: the device's default priority)
            int prio_least = 0, prio_greatest = 0, side_prio = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
            if (const char* e = getenv("VAE_SIDE_PRIORITY")) side_prio = !strcmp(e, "low") ? prio_least : !strcmp(e, "high") ? prio_greatest : 0;
            DevStreams* ds = device_streams(side_prio);
            ok = ds != nullptr;
            for (int i = 0; i < vae_ctx::NSIDE && ok; ++i) {
                c->side[i] = ds->side[i];
                ok = hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming) == hipSuccess;
            }
            for (int i = 0; i < vae_ctx::NFORK && ok; ++i) ok = hipEventCreateWithFlags(&c->ev_fork[i], hipEventDisableTiming) == hipSuccess;
            if (ok) { c->comm = ds->comm;
                      ok = hipEventCreateWithFlags(&c->ev_pack, hipEventDisableTiming) == hipSuccess &&
                           hipEventCreateWithFlags(&c->ev_comm, hipEventDisableTiming) == hipSuccess;
                      for (int i = 0; i < vae_ctx::NBUCKET && ok; ++i) ok = hipEventCreateWithFlags(&c->ev_bucket[i], hipEventDisableTiming) == hipSuccess; }
            c->n_side_ok = ok ? 1 : 0;
        }
    }
    if (ok && dtype != VAE_DTYPE_F32) {   // materialised operands of the deep weight gradients (small tensors)
        for (int i = 1; i <= 5 && ok; ++i) {
            const size_t n = B * c->lay[i].H * c->lay[i].W * c->lay[i].C;
            if (i == 1 || i == 2 || i == 4) { c->lay[i].act = dalloc<char>(c, n * c->esz); ok = ok && c->lay[i].act; }
            if (i >= 2) { c->lay[i].dy = dalloc<char>(c, n * c->esz); ok = ok && c->lay[i].dy; }
        }
    }
    if (ok) { c->reduce_tmp_floats = 64 * 1024; c->reduce_tmp = dalloc<float>(c, c->reduce_tmp_floats); ok = c->reduce_tmp != nullptr; }
    if (ok && dtype != VAE_DTYPE_F32) {
        c->fused_slab_floats = (size_t)512 * 9 * 64 * 32;   // up to 512 workgroups x [9][64][32]
        for (int i = 0; i < 3 && ok; ++i) { c->fused_slab[i] = dalloc<float>(c, c->fused_slab_floats); ok = c->fused_slab[i] != nullptr; }
    }
    if (!ok) { vae_set_error("vae_create", "hipMalloc failed"); vae_destroy(c); return nullptr; }
    std::vector<float> id(3 * 256, 0.f);
    for (int i = 0; i < 256; ++i) id[i] = 1.f;
    if (hipMemcpy(c->ident, id.data(), id.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { vae_set_error("vae_create", "memcpy failed"); vae_destroy(c); return nullptr; }
    return c;
}

extern "C" int vae_option_info(int index, const char** name, int* default_value) {
    if (index < 0 || index >= (int)(sizeof(kOptions) / sizeof(kOptions[0]))) return -1;
    if (name) *name = kOptions[index].name;
    if (default_value) *default_value = kOptions[index].def;
    return 0;
}
extern "C" int vae_set_option(vae_ctx* c, const char* name, int value) {
    if (!c) return vae_set_error("vae_set_option", "null ctx");
    if (const OptionDef* o = find_option(name)) { o->ref(*c) = o->norm(value); return 0; }
    return vae_set_error("vae_set_option", "unknown option");
}
SideFork fork_side(vae_ctx* c, hipStream_t st, int which) {
    SideFork f{st, c->slab, 0};
    if (!c->use_side_stream) return f;
    const int s = which >= 0 ? which : (c->side_rr++ % vae_ctx::NSIDE);
    hipEvent_t ev = c->ev_fork[c->fork_rr++ % vae_ctx::NFORK];
    if (hipEventRecord(ev, st) != hipSuccess || hipStreamWaitEvent(c->side[s], ev, 0) != hipSuccess) {
        f.rc = vae_set_error("fork_side", "event record/wait failed"); return f;
    }
    f.st = c->side[s]; f.slab = c->side_slab[s];
    return f;
}
// join every side stream into `st`
int join_sides(vae_ctx* c, hipStream_t st) {
    if (!c->use_side_stream) return 0;
    for (int i = 0; i < vae_ctx::NSIDE; ++i) {
        HIP_CHECK_RET(hipEventRecord(c->ev_join[i], c->side[i]));
        HIP_CHECK_RET(hipStreamWaitEvent(st, c->ev_join[i], 0));
    }
    return 0;
}
// join the communication stream lent out by vae_comm_stream (work the caller enqueued on it, e.g. an all-reduce)
int join_comm(vae_ctx* c, hipStream_t st) {
    if (!c->comm_busy) return 0;
    HIP_CHECK_RET(hipEventRecord(c->ev_comm, c->comm));
    HIP_CHECK_RET(hipStreamWaitEvent(st, c->ev_comm, 0));
    c->comm_busy = 0;
    return 0;
}
// ---------------------------------------------------------------------------
// the opening of every entry point that runs a batch through the context
static int check_ctx_batch(const char* what, const vae_ctx* c, int B) {
    if (!c) return vae_set_error(what, "null ctx");
    if (B < 1 || B > c->maxB) return vae_set_error(what, "batch exceeds the context's max_batch");
    return 0;
}
extern "C" int vae_forward(vae_ctx* c, const float* x, int B, const float* params, float* bn_running, int64_t* nbt,
                           const float* eps, uint64_t seed, int train, float* xhat, float* mu, float* lv, float* z, vae_stream_t stream) {
    if (check_ctx_batch("vae_forward", c, B)) return -1;
    if (!x || !params || !xhat || !mu || !lv || !z) return vae_set_error("vae_forward", "null tensor pointer");
    if (c->kl_kind == VAE_KL_TC && B > TC_MAX_B) return vae_set_error("vae_forward", "the total-correlation objective (VAE_KL_TC) takes batches of at most 4096");
    hipStream_t st = (hipStream_t)stream;
    if (begin_forward(c, FwdRecord::FULL, B, train, st)) return -1;
    c->fwd.x = x; c->fwd.xhat = xhat; c->fwd.mu = mu; c->fwd.lv = lv; c->fwd.z = z;
    if (!c->fwd.target) c->fwd.target = x;
    const int rc = VAE_DISPATCH(c->dtype, forward_impl, (c, x, B, params, bn_running, nbt, eps, seed, train, xhat, mu, lv, z, st));
    if (rc) drop_forward(c);
    return rc;
}

extern "C" int vae_decode(vae_ctx* c, const float* z, int B, const float* params, float* bn_running, int64_t* nbt, int train,
                          float* xhat, vae_stream_t stream) {
    if (check_ctx_batch("vae_decode", c, B)) return -1;
    if (!z || !params || !xhat) return vae_set_error("vae_decode", "null tensor pointer");
    hipStream_t st = (hipStream_t)stream;
    // what vae_backward_ex needs of a decode-only pass: its BatchNorm mode, z, xhat, the gradient scale; vae_backward refuses it
    if (begin_forward(c, FwdRecord::DECODE, B, train, st)) return -1;
    c->fwd.x = xhat; c->fwd.xhat = xhat; c->fwd.z = const_cast<float*>(z);
    int rc = VAE_DISPATCH(c->dtype, pack_weights, (c, params, st));
    // the reconstruction-loss side outputs of the output-conv kernel are unused here: xhat doubles as the target
    if (!rc) rc = VAE_DISPATCH(c->dtype, decode_impl, (c, z, B, params, bn_running, nbt, train, xhat, xhat, st));
    if (rc) drop_forward(c);
    return rc;
}

extern "C" int vae_encode(vae_ctx* c, const float* x, int B, const float* params, float* bn_running, int64_t* nbt,
                          const float* eps, uint64_t seed, int train, float* mu, float* lv, float* z, vae_stream_t stream) {
    if (check_ctx_batch("vae_encode", c, B)) return -1;
    if (!x || !params || !mu || !lv || !z) return vae_set_error("vae_encode", "null tensor pointer");
    hipStream_t st = (hipStream_t)stream;
    if (begin_forward(c, FwdRecord::ENCODE, B, train, st)) return -1;
    c->fwd.x = x; c->fwd.mu = mu; c->fwd.lv = lv; c->fwd.z = z;
    const int rc = VAE_DISPATCH(c->dtype, encode_impl, (c, x, B, params, bn_running, nbt, eps, seed, train, mu, lv, z, st));
    if (rc) drop_forward(c);
    return rc;
}

// Importance-weighted log-likelihood and per-sample ELBO (loglik.cuh).  One eval-mode encoder pass; then per chunk of draws
// the latent kernel, an eval-mode decoder pass whose output conv runs in its per-sample mode, and the first half of the combine;
// the second half once at the end.  Leaves no forward behind: vae_loss / vae_backward afterwards fail.
extern "C" int vae_log_likelihood(vae_ctx* c, const float* x, int B, const float* params, const float* bn_running, int K, int chunk,
                                  const float* eps, uint64_t seed, double* log_w, double* ll, double* elbo, vae_stream_t stream) {
    if (!c) return vae_set_error("vae_log_likelihood", "null ctx");
    if (!x || !params || !bn_running || !ll || !elbo) return vae_set_error("vae_log_likelihood", "null tensor pointer");
    if (check_ctx_batch("vae_log_likelihood", c, B)) return -1;   // (the batch: here the tensors are checked in front of it)
    if (K < 1 || chunk < 1) return vae_set_error("vae_log_likelihood", "num_samples and chunk must be >= 1");
    if ((int64_t)chunk * B > c->maxB) return vae_set_error("vae_log_likelihood", "chunk * batch exceeds the context's max_batch");
    hipStream_t st = (hipStream_t)stream;
    const int L = c->L, H = c->H;
    const size_t maxB = (size_t)c->maxB;
    if (!c->ll_f) {
        c->ll_f = dalloc<float>(c, 4 * maxB * L);
        c->ll_part = dalloc<double>(c, maxB * (size_t)H * H / 256);   // tiles of 8x32 pixels or larger
        c->ll_lat = dalloc<double>(c, maxB);
        if (!c->ll_f || !c->ll_part || !c->ll_lat) return vae_set_error("vae_log_likelihood", "hipMalloc failed");
    }
    const size_t kb = (size_t)K * B;
    if (c->ll_kb_n < 2 * kb) {
        if (c->ll_kb) { HIP_CHECK_RET(hipDeviceSynchronize()); HIP_CHECK_RET(hipFree(c->ll_kb)); c->ll_kb = nullptr; c->ll_kb_n = 0; }
        void* p = nullptr;
        HIP_CHECK_RET(hipMalloc(&p, 2 * kb * sizeof(double)));
        c->ll_kb = reinterpret_cast<double*>(p); c->ll_kb_n = 2 * kb;
    }
    float* mu = c->ll_f; float* lv = mu + maxB * L; float* z0 = lv + maxB * L; float* zc = z0 + maxB * L;
    double* lpx = c->ll_kb; double* lw = log_w ? log_w : c->ll_kb + kb;
    // an eval-mode encoder pass with decoder passes on top; whatever happens below, the context is left without a forward
    struct Drop { vae_ctx* c; ~Drop() { drop_forward(c); } } drop{c};
    if (begin_forward(c, FwdRecord::ENCODE, B, 0, st)) return -1;
    c->fwd.x = x; c->fwd.mu = mu; c->fwd.lv = lv; c->fwd.z = z0;
    float* bnr = const_cast<float*>(bn_running);   // eval mode: read only
    int rc = VAE_DISPATCH(c->dtype, encode_impl, (c, x, B, params, bnr, nullptr, nullptr, seed, 0, mu, lv, z0, st));
    if (rc) return rc;
    const double cst = c->fwd.recon == VAE_RECON_MSE ? 0.5 * H * H * log(3.14159265358979323846) : 0.0;
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int nk = std::min(chunk, K - k0), R = nk * B;
        IwLatentArgs la; la.mu = mu; la.lv = lv; la.eps = eps; la.z = zc; la.lat = c->ll_lat; la.B = B; la.L = L; la.k0 = k0; la.nk = nk;
        la.seed = (unsigned long long)seed;
        {
            ProfScope ps(c, "iw_latent", 4.0 * R * L * (eps ? 2 : 1) + 8.0 * R, 0, st);
            if (launch("iw_latent_kernel", iw_latent_kernel, dim3((R + 255) / 256), dim3(256), 0, st, la)) return -1;
        }
        c->ps_part = c->ll_part; c->ps_tb = B; c->ps_ntile = 0;
        rc = VAE_DISPATCH(c->dtype, decode_impl, (c, zc, R, params, bnr, nullptr, 0, x, nullptr, st));
        c->ps_part = nullptr;
        if (rc) return rc;
        if (c->ps_ntile < 1) return vae_set_error("vae_log_likelihood", "the output conv did not run in its per-sample mode");
        ProfScope ps(c, "loglik_rows", 8.0 * R * (c->ps_ntile + 3), 0, st);
        if (launch("loglik_rows_kernel", loglik_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, st, c->ll_part, c->ps_ntile, c->ll_lat, R,
                   (long)k0 * B, cst, lpx, lw)) return -1;
    }
    ProfScope ps(c, "loglik_final", 16.0 * kb, 0, st);
    return launch("loglik_final_kernel", loglik_final_kernel, dim3((B + 255) / 256), dim3(256), 0, st, lpx, lw, mu, lv, K, B, L, ll, elbo);
}

extern "C" int vae_set_recon_loss(vae_ctx* c, int kind) {
    if (!c) return vae_set_error("vae_set_recon_loss", "null ctx");
    if (kind != VAE_RECON_BCE && kind != VAE_RECON_MSE) return vae_set_error("vae_set_recon_loss", "kind must be VAE_RECON_BCE or VAE_RECON_MSE");
    c->recon = kind; c->recon_param = 0.0;
    return 0;
}
// kind and parameter of a reconstruction term (vae_set_recon_loss_ex, vae_elbo_generic_w): pos_weight of WBCE a finite number in (0, 1024]
static int check_recon(const char* what, int kind, double param) {
    if (kind != VAE_RECON_BCE && kind != VAE_RECON_MSE && kind != VAE_RECON_WBCE) return vae_set_error(what, "recon must be VAE_RECON_BCE, VAE_RECON_MSE or VAE_RECON_WBCE");
    if (kind == VAE_RECON_WBCE) {
        if (!(param > 0.0) || !(param <= 1024.0)) return vae_set_error(what, "pos_weight must be a finite number in (0, 1024]");   // (a NaN fails both comparisons)
    } else if (param != 0.0) return vae_set_error(what, "the parameter must be 0 for VAE_RECON_BCE / VAE_RECON_MSE");
    return 0;
}
// one-shot: begin_forward (vae_ctx.h) consumes it
extern "C" int vae_set_recon_target(vae_ctx* c, const float* target) {
    if (!c) return vae_set_error("vae_set_recon_target", "null ctx");
    c->recon_target = target;
    return 0;
}
extern "C" int vae_set_recon_loss_ex(vae_ctx* c, int kind, double param) {
    if (!c) return vae_set_error("vae_set_recon_loss_ex", "null ctx");
    if (check_recon("vae_set_recon_loss_ex", kind, param)) return -1;
    c->recon = kind; c->recon_param = kind == VAE_RECON_WBCE ? param : 0.0;
    return 0;
}

// ---- KL objectives (free bits, capacity target; edge_kernels.cuh: kl_shape_kernel) ---------------------------------------------
static int check_kl_objective(const char* what, int kind, double param, bool allow_tc = false) {
    if (kind == VAE_KL_TC && !allow_tc) return vae_set_error(what, "VAE_KL_TC needs the eps of the forward, which this entry point does not have: use vae_total_correlation for the term and its gradient");
    if (kind != VAE_KL_PLAIN && kind != VAE_KL_FREE_BITS && kind != VAE_KL_CAPACITY && kind != VAE_KL_TC) return vae_set_error(what, "kind must be VAE_KL_PLAIN, VAE_KL_FREE_BITS, VAE_KL_CAPACITY or VAE_KL_TC");
    if (param != param || param < 0.0 || std::isinf(param)) return vae_set_error(what, "the parameter must be finite and >= 0");
    if (kind == VAE_KL_FREE_BITS && !(param > 0.0)) return vae_set_error(what, "free bits need lambda > 0 nats per dimension");
    return 0;
}
extern "C" int vae_set_kl_objective(vae_ctx* c, int kind, double param) {
    if (!c) return vae_set_error("vae_set_kl_objective", "null ctx");
    if (check_kl_objective("vae_set_kl_objective", kind, param, true)) return -1;
    c->kl_kind = kind; c->kl_param = kind == VAE_KL_PLAIN ? 0.0 : param;
    return 0;
}
// one launch: every size takes it (VEC = 4 where the rows allow 16-byte loads); the ticket word is zeroed in front of it
static int enqueue_kl_shape(const float* mu, const float* lv, int B, int L, int kind, double param, unsigned long long* kl_d,
                            double* scal, float* factor, unsigned* ticket, hipStream_t st) {
    HIP_CHECK_RET(hipMemsetAsync(ticket, 0, 16, st));
    KlShapeArgs a; a.mu = mu; a.lv = lv; a.kl_d = kl_d; a.factor = factor; a.scal = scal; a.ticket = ticket; a.B = B; a.L = L; a.kind = kind; a.param = param;
    const bool vec = L % 4 == 0 && !(((uintptr_t)mu | (uintptr_t)lv) & 15);
    if (vec) return launch("kl_shape_kernel", kl_shape_kernel<4>, dim3(L / 4), dim3(256), 0, st, a);
    return launch("kl_shape_kernel", kl_shape_kernel<1>, dim3(L), dim3(256), 0, st, a);
}
int launch_kl_shape(vae_ctx* c, hipStream_t st) {
    if (!c->kl_ws) {
        c->kl_ws = dalloc<char>(c, (size_t)c->L * 12 + 16); c->kl_tk = dalloc<unsigned>(c, 4);
        if (!c->kl_ws || !c->kl_tk || (!c->ev_kl && hipEventCreateWithFlags(&c->ev_kl, hipEventDisableTiming) != hipSuccess)) { c->kl_ws = nullptr; return vae_set_error("kl_shape", "allocation failed"); }
    }
    // (the total-correlation objective takes the plain reduction: kl_d and KL; tc_final_kernel then writes T)
    const int kind = c->fwd.kl_kind == VAE_KL_TC ? VAE_KL_PLAIN : c->fwd.kl_kind;
    // always the same side stream: successive reductions of a context write the same buffers and must not overlap
    SideFork f = fork_side(c, st, vae_ctx::KL_SIDE);
    if (f.rc) return f.rc;
    {
        ProfScope ps(c, "kl_shape", 8.0 * c->fwd.B * c->L + 12.0 * c->L, 0, f.st);
        if (enqueue_kl_shape(c->fwd.mu, c->fwd.lv, c->fwd.B, c->L, kind, c->fwd.kl_param, c->kl_d(), c->kl_scal(), c->kl_factor(), c->kl_tk, f.st)) return -1;
    }
    HIP_CHECK_RET(hipEventRecord(c->ev_kl, f.st));
    c->fwd.kl_pending = 1; c->fwd.kl_reduced = 1;
    return 0;
}
int join_kl(vae_ctx* c, hipStream_t st) {
    if (c->fwd.kl_pending) HIP_CHECK_RET(hipStreamWaitEvent(st, c->ev_kl, 0));
    return 0;
}
extern "C" int vae_kl_per_dim(vae_ctx* c, double* out, vae_stream_t stream) {
    if (!c || !c->fwd || !c->fwd.mu || !c->fwd.lv) return vae_set_error("vae_kl_per_dim", "no forward with a posterior (vae_forward, a training step or vae_encode)");
    if (!out) return vae_set_error("vae_kl_per_dim", "null output pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!c->fwd.kl_reduced && launch_kl_shape(c, st)) return -1;   // (the forward was plain: reduce now)
    if (join_kl(c, st)) return -1;
    HIP_CHECK_RET(hipMemcpyAsync(out, c->kl_d(), (size_t)c->L * 8, hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- total correlation (total_corr.cuh) --------------------------------------------------------------------------------------
// The six launches on `st`.  c: profiling labels only (null: the context-free entry point).  gmu / glv null: value only.
static int enqueue_tc(vae_ctx* c, const float* mu, const float* lv, const float* eps, int B, int L, const TcWork& w, double* tc_out,
                      float* gmu, float* glv, int ldo, double* scal, double tc_weight, hipStream_t st) {
    const double bl = (double)B * L, bb = (double)B * B;
    TcSideArgs a; a.z = w.z; a.mu = mu; a.hw = w.hw; a.c2 = w.c2; a.A = w.A; a.lse = w.lse; a.lsed = w.lsed; a.gz = w.gz; a.lv = lv; a.eps = eps;
    a.part = w.part; a.gmu = gmu; a.glv = glv; a.ldo = ldo; a.B = B; a.L = L; a.grad = (gmu || glv) ? 1 : 0;
    const unsigned tiles = (unsigned)((B + TC_TILE - 1) / TC_TILE);
    {
        ProfScope ps(c, "tc_prep", 24.0 * bl, 0, st);
        if (launch("tc_prep_kernel", tc_prep_kernel, dim3((B + 3) / 4), dim3(256), 0, st, mu, lv, eps, B, L, w.z, w.hw, w.c2, w.cj)) return -1;
    }
    {
        ProfScope ps(c, "tc_pair", 12.0 * bl + 4.0 * bb, 3.0 * bb * L, st);
        if (launch("tc_pair_kernel", tc_pair_kernel, dim3(tiles, tiles), dim3(256), 0, st, w.z, mu, w.hw, w.cj, B, L, w.A)) return -1;
    }
    {
        ProfScope ps(c, "tc_row", 4.0 * bb, 0, st);
        if (launch("tc_row_kernel", tc_row_kernel, dim3((B + 3) / 4), dim3(256), 0, st, w.A, B, w.lse)) return -1;
    }
    {
        ProfScope ps(c, "tc_query", 24.0 * bl + 4.0 * bb, (a.grad ? 14.0 : 5.0) * bb * L, st);
        if (launch("tc_query_kernel", tc_query_kernel, dim3(w.npart), dim3(256), 0, st, a)) return -1;
    }
    if (a.grad) {
        ProfScope ps(c, "tc_comp", 36.0 * bl + 4.0 * bb, 12.0 * bb * L, st);
        if (launch("tc_comp_kernel", tc_comp_kernel, dim3(w.npart), dim3(256), 0, st, a)) return -1;
    }
    ProfScope ps(c, "tc_final", 4.0 * B + 8.0 * w.npart, 0, st);
    return launch("tc_final_kernel", tc_final_kernel, dim3(1), dim3(256), 0, st, w.lse, w.part, w.npart, B, L, tc_out, scal, tc_weight);
}
extern "C" int vae_total_correlation(const float* mu, const float* lv, const float* eps, int B, int L, double* tc, float* g_mu,
                                     float* g_lv, vae_stream_t stream) {
    if (!mu || !lv || !eps || !tc) return vae_set_error("vae_total_correlation", "null pointer (mu, log_var, eps, tc)");
    if (B < 1 || B > TC_MAX_B) return vae_set_error("vae_total_correlation", "batch must be in 1..4096");
    if (L < 1 || L > 4096) return vae_set_error("vae_total_correlation", "latent_dim must be in 1..4096");
    hipStream_t st = (hipStream_t)stream;
    return with_stream_scratch(tc_carve(nullptr, B, L, nullptr), st, [&](char* base) -> int {
        TcWork w; tc_carve(base, B, L, &w);
        return enqueue_tc(nullptr, mu, lv, eps, B, L, w, tc, g_mu, g_lv, L, nullptr, 0.0, st);
    });
}
// The context's work space: the gradient [B][2L] (g_mu | g_log_var) in front, the kernels' pieces behind it; sized for the largest
// batch a forward has asked for so far (a larger one frees and allocates again, behind a device synchronisation).
static size_t tc_grad_bytes(int B, int L) { return (size_t)align_up((int64_t)B * 2 * L * 4, 256); }
static int tc_reserve(vae_ctx* c, int B) {
    if (c->tc_ws && c->tc_ws_B >= B) return 0;
    if (c->tc_ws) {
        HIP_CHECK_RET(hipDeviceSynchronize());
        HIP_CHECK_RET(hipFree(c->tc_ws));
        c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), c->tc_ws), c->allocs.end());
        c->ws_bytes -= (int64_t)c->tc_ws_bytes; c->tc_ws = nullptr; c->tc_ws_B = 0; c->tc_ws_bytes = 0;
    }
    const size_t need = tc_grad_bytes(B, c->L) + tc_carve(nullptr, B, c->L, nullptr);
    c->tc_ws = dalloc<char>(c, need);
    if (!c->tc_ws) return vae_set_error("total correlation", "hipMalloc of the work space failed");
    c->tc_ws_B = B; c->tc_ws_bytes = std::max<size_t>(need, 256);
    return 0;
}
static TcWork tc_work(vae_ctx* c) {
    TcWork w; tc_carve(static_cast<char*>(c->tc_ws) + tc_grad_bytes(c->fwd.B, c->L), c->fwd.B, c->L, &w);
    return w;
}
// TC of the held forward and its gradient on side stream KL_SIDE (behind kl_shape_kernel when the forward's objective is VAE_KL_TC:
// tc_final_kernel then turns the KL it left into T); ev_kl follows, as for launch_kl_shape
int launch_tc(vae_ctx* c, hipStream_t st) {
    const int B = c->fwd.B, L = c->L;
    if (B > TC_MAX_B) return vae_set_error("total correlation", "the batch exceeds 4096");
    if (tc_reserve(c, B)) return -1;
    if (!c->ev_kl && hipEventCreateWithFlags(&c->ev_kl, hipEventDisableTiming) != hipSuccess) { c->ev_kl = nullptr; return vae_set_error("total correlation", "event creation failed"); }
    SideFork f = fork_side(c, st, vae_ctx::KL_SIDE);
    if (f.rc) return f.rc;
    const TcWork w = tc_work(c);
    const bool objective = c->fwd.kl_kind == VAE_KL_TC;
    if (enqueue_tc(c, c->fwd.mu, c->fwd.lv, c->eps, B, L, w, w.tc, c->tc_grad(), c->tc_grad() + L, 2 * L, objective ? c->kl_scal() : nullptr,
                   c->fwd.kl_param, f.st)) return -1;
    HIP_CHECK_RET(hipEventRecord(c->ev_kl, f.st));
    c->fwd.kl_pending = 1; c->fwd.tc_done = 1;
    return 0;
}
// the held forward's TC is in the work space (its own launch, or one made now) and ordered in front of `st`
static int ensure_tc(const char* what, vae_ctx* c, hipStream_t st) {
    if (!c || !c->fwd || !c->fwd.mu || !c->fwd.lv) return vae_set_error(what, "no forward with a posterior (vae_forward, a training step or vae_encode)");
    enter(c, st);
    if (!c->fwd.tc_done && launch_tc(c, st)) return -1;
    return join_kl(c, st);
}
extern "C" int vae_last_total_correlation(vae_ctx* c, double* out, vae_stream_t stream) {
    if (!out) return vae_set_error("vae_last_total_correlation", "null output pointer");
    if (ensure_tc("vae_last_total_correlation", c, (hipStream_t)stream)) return -1;
    HIP_CHECK_RET(hipMemcpyAsync(out, tc_work(c).tc, 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// the ELBO scalars {loss, reconstruction, -KL} of the last forward from the context's accumulators (a shaped KL objective: after join_kl)
int launch_loss_finalize(vae_ctx* c, float* out3, float kld_weight, hipStream_t st) {
    return launch("loss_finalize_kernel", loss_finalize_kernel, dim3(1), dim3(64), 0, st, c->accum, out3, 1.0 / ((double)c->fwd.B * c->H * c->H),
                  1.0 / (double)c->fwd.B, kld_weight, STAT_R, c->kl_shaped());
}

extern "C" int vae_loss(vae_ctx* c, float kld_weight, float* out3, vae_stream_t stream) {
    if (!c || !c->fwd) return vae_set_error("vae_loss", "no forward");
    if (c->fwd.convout_pending) return vae_set_error("vae_loss", "the forward ran with train = 2: the ELBO is produced by the backward (use vae_loss_deferred)");
    if (join_kl(c, (hipStream_t)stream)) return -1;
    return launch_loss_finalize(c, out3, kld_weight, (hipStream_t)stream);
}

// Same scalars, computed beside the backward instead of in front of it: enqueued on one of the context's side streams
// (ordered after `stream`), so out3 is ordered into the caller's stream by the NEXT vae_backward / vae_backward_part
// on this context - for callers that only read the ELBO after the backward (train.py:644-674 reads it after the step).
extern "C" int vae_loss_deferred(vae_ctx* c, float kld_weight, float* out3, vae_stream_t stream) {
    if (!c || !c->fwd) return vae_set_error("vae_loss_deferred", "no forward");
    if (!c->fwd.trained || c->fwd.kind != FwdRecord::FULL) return vae_set_error("vae_loss_deferred", "needs a train-mode forward (a backward must follow)");
    if (c->fwd.convout_pending) { c->fwd.loss_out3 = out3; c->fwd.loss_kw = kld_weight; return 0; }   // finalised by the backward, after the fused output-conv kernel
    SideFork f = (c->knob_lean & 4) ? fork_side(c, (hipStream_t)stream) : SideFork{(hipStream_t)stream, c->slab, 0};
    if (f.rc) return f.rc;
    if (c->kl_shaped() && join_kl(c, f.st)) return -1;
    return launch_loss_finalize(c, out3, kld_weight, f.st);
}

// Accumulators of vae_elbo_generic: the entry point has no context, so they live in a per-device ring (one slot per call:
// calls in flight on different streams of a device never share a slot unless more than kGenericSlots overlap).
static constexpr int kGenericSlots = 64, kMaxDevices = 64;
static double* g_generic_ring[kMaxDevices] = {nullptr};
static unsigned g_generic_next[kMaxDevices] = {0};
static int elbo_generic(const char* what, const float* xhat, const float* target, const float* mu, const float* lv, int64_t n, int B, int L,
                        float kld_weight, int recon, int kl_kind, double kl_param, float* out3, float* g_xhat, float* g_mu, float* g_lv,
                        vae_stream_t stream, double recon_param = 0.0, bool allow_wbce = false) {
    if (!allow_wbce && recon != VAE_RECON_BCE && recon != VAE_RECON_MSE) return vae_set_error(what, "recon must be VAE_RECON_BCE or VAE_RECON_MSE");
    if (check_recon(what, recon, recon_param)) return -1;
    if (check_kl_objective(what, kl_kind, kl_param)) return -1;
    if (kl_kind != VAE_KL_PLAIN && (B < 1 || L < 1 || !mu || !lv)) return vae_set_error(what, "the KL objective needs mu / log_var [batch, latent_dim]");
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    HIP_CHECK_RET(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return vae_set_error("vae_elbo_generic", "device index out of range");
    if (!g_generic_ring[dev]) HIP_CHECK_RET(hipMalloc(&g_generic_ring[dev], kGenericSlots * 4 * sizeof(double)));
    double* acc = g_generic_ring[dev] + 4 * (g_generic_next[dev]++ % kGenericSlots);
    HIP_CHECK_RET(hipMemsetAsync(acc, 0, 4 * sizeof(double), st));
    const dim3 grid((unsigned)std::min<long>((n + 255) / 256, 2048));
    const int rc = recon == VAE_RECON_MSE ? launch("mse_kernel", mse_kernel, grid, dim3(256), 0, st, xhat, target, g_xhat, acc, (long)n, (float)(2.0 / (double)n))
                 : recon == VAE_RECON_WBCE ? launch("wbce_kernel", wbce_kernel, grid, dim3(256), 0, st, xhat, target, g_xhat, acc, (long)n, (float)(1.0 / (double)n), (float)recon_param)
                                           : launch("bce_kernel", bce_kernel, grid, dim3(256), 0, st, xhat, target, g_xhat, acc, (long)n, (float)(1.0 / (double)n));
    if (rc) return -1;
    // the KL term and the scalars; factor / scal null and FL 1: the plain objective
    const auto tail = [&](const float* factor, int FL, const double* scal) -> int {
        if (launch("kld_only_kernel", kld_only_kernel, dim3((B * L + 255) / 256), dim3(256), 0, st, mu, lv, acc, B * L, kld_weight / (float)B, g_mu, g_lv,
                   factor, FL)) return -1;
        return launch("loss_finalize_kernel", loss_finalize_kernel, dim3(1), dim3(64), 0, st, acc, out3, 1.0 / (double)n, 1.0 / (double)B, kld_weight, 1, scal);
    };
    if (kl_kind == VAE_KL_PLAIN) return tail(nullptr, 1, nullptr);
    // shaped objective: the reduction in front (its work space from the stream-ordered allocator: kl_d | scalars | factor | ticket block)
    const size_t fac_off = (size_t)L * 8 + 16, tk_off = (fac_off + (size_t)L * 4 + 15) / 16 * 16;
    return with_stream_scratch(tk_off + 16, st, [&](char* base) -> int {
        float* factor = reinterpret_cast<float*>(base + fac_off);
        double* scal = reinterpret_cast<double*>(base + (size_t)L * 8);
        if (enqueue_kl_shape(mu, lv, B, L, kl_kind, kl_param, reinterpret_cast<unsigned long long*>(base), scal, factor,
                             reinterpret_cast<unsigned*>(base + tk_off), st)) return -1;
        return tail(factor, L, scal);
    });
}
extern "C" int vae_elbo_generic_ex(const float* xhat, const float* target, const float* mu, const float* lv, int64_t n, int B, int L,
                                   float kld_weight, int recon, float* out3, float* g_xhat, float* g_mu, float* g_lv, vae_stream_t stream) {
    return elbo_generic("vae_elbo_generic_ex", xhat, target, mu, lv, n, B, L, kld_weight, recon, VAE_KL_PLAIN, 0.0, out3, g_xhat, g_mu, g_lv, stream);
}
extern "C" int vae_elbo_generic_kl(const float* xhat, const float* target, const float* mu, const float* lv, int64_t n, int B, int L,
                                   float kld_weight, int recon, int kl_kind, double kl_param, float* out3, float* g_xhat, float* g_mu,
                                   float* g_lv, vae_stream_t stream) {
    return elbo_generic("vae_elbo_generic_kl", xhat, target, mu, lv, n, B, L, kld_weight, recon, kl_kind, kl_param, out3, g_xhat, g_mu, g_lv, stream);
}
extern "C" int vae_elbo_generic_w(const float* xhat, const float* target, const float* mu, const float* lv, int64_t n, int B, int L,
                                  float kld_weight, int recon, double recon_param, int kl_kind, double kl_param, float* out3, float* g_xhat,
                                  float* g_mu, float* g_lv, vae_stream_t stream) {
    return elbo_generic("vae_elbo_generic_w", xhat, target, mu, lv, n, B, L, kld_weight, recon, kl_kind, kl_param, out3, g_xhat, g_mu, g_lv, stream,
                        recon_param, true);
}
extern "C" int vae_elbo_generic(const float* xhat, const float* target, const float* mu, const float* lv, int64_t n, int B, int L,
                                float kld_weight, float* out3, float* g_xhat, float* g_mu, float* g_lv, vae_stream_t stream) {
    return vae_elbo_generic_ex(xhat, target, mu, lv, n, B, L, kld_weight, VAE_RECON_BCE, out3, g_xhat, g_mu, g_lv, stream);
}

// A non-blocking stream owned by the context, ordered after everything enqueued on `stream` so far.  Work the caller
// puts on it (the all-reduce of the decoder gradients after vae_backward_part(..., 1, ...)) is joined back into the
// caller's stream at the end of vae_backward_part(..., 2, ...).
extern "C" int vae_comm_stream(vae_ctx* c, vae_stream_t stream, vae_stream_t* out) {
    if (!c || !out) return vae_set_error("vae_comm_stream", "null argument");
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t ev = c->ev_fork[c->fork_rr++ % vae_ctx::NFORK];
    HIP_CHECK_RET(hipEventRecord(ev, st));
    HIP_CHECK_RET(hipStreamWaitEvent(c->comm, ev, 0));
    c->comm_busy = 1;
    *out = (vae_stream_t)c->comm;
    return 0;
}
extern "C" int vae_backward_part(vae_ctx* c, const float* x, const float* params, float* grads, const float* g_xhat, const float* gscale,
                                 const float* g_mu, const float* g_lv, const float* g_z, const float* g_pre, float kld_weight, int add_kl,
                                 int part, vae_stream_t stream) {
    if (!c) return vae_set_error("vae_backward", "null ctx");
    if (!x || !params || !grads) return vae_set_error("vae_backward", "null tensor pointer");
    hipStream_t st = (hipStream_t)stream;
    enter(c, st);
    return VAE_DISPATCH(c->dtype, backward_impl, (c, x, params, grads, g_xhat, gscale, g_mu, g_lv, g_z, g_pre, kld_weight, add_kl, part, st));
}
extern "C" int vae_backward_ex(vae_ctx* c, const float* x, const float* params, float* grads, const float* g_xhat, const float* gscale,
                               const float* g_mu, const float* g_lv, const float* g_z, const float* g_pre, float kld_weight, int add_kl,
                               float* dx, float* dz, vae_stream_t stream) {
    if (!c) return vae_set_error("vae_backward_ex", "null ctx");
    if (!params || !grads || (!x && c->fwd.kind != FwdRecord::DECODE)) return vae_set_error("vae_backward_ex", "null tensor pointer");
    hipStream_t st = (hipStream_t)stream;
    enter(c, st);
    return VAE_DISPATCH(c->dtype, backward_ex_impl, (c, x, params, grads, g_xhat, gscale, g_mu, g_lv, g_z, g_pre, kld_weight, add_kl, dx, dz, st));
}
extern "C" int vae_backward(vae_ctx* c, const float* x, const float* params, float* grads, const float* g_xhat, const float* gscale,
                            const float* g_mu, const float* g_lv, const float* g_z, const float* g_pre, float kld_weight, int add_kl,
                            vae_stream_t stream) {
    return vae_backward_part(c, x, params, grads, g_xhat, gscale, g_mu, g_lv, g_z, g_pre, kld_weight, add_kl, 0, stream);
}

// The arguments of the AdamW kernels and their grid.  Every scalar of torch's single-tensor update is formed in double from the Python
// floats and reaches the element-wise kernel as one float: beta, 1 - beta, 1 - lr * weight_decay, eps, and the two that depend on the
// step count, lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t): zero here, filled by vae_adamw_step from its host step, taken from the
// device record by the clipped update.
static dim3 adam_args(AdamArgs& a, float* params, const float* grads, float* m, float* v, int ngroups, const int64_t* offsets,
                      const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double eps, double weight_decay,
                      float grad_scale, int step) {
    a.p = params; a.g = grads; a.m = m; a.v = v; a.ngrp = ngroups; a.beta2 = (float)beta2; a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.grad_scale = grad_scale; a.step = step;
    long nmax = 0;
    for (int i = 0; i < ngroups; ++i) {
        a.grp[i].off = offsets[i]; a.grp[i].n = sizes[i]; nmax = std::max<long>(nmax, sizes[i]);
        a.grp[i].beta1 = (float)beta1s[i]; a.grp[i].omb1 = (float)(1.0 - beta1s[i]); a.grp[i].decay = (float)(1.0 - lrs[i] * weight_decay);
        a.grp[i].step_size = 0.f; a.grp[i].inv_sqrt_bc2 = 0.f;
    }
    return dim3((unsigned)std::min<long>((nmax / 4 + 255) / 256 + 1, 2048), ngroups);
}
extern "C" int vae_adamw_step(float* params, const float* grads, float* m, float* v, int ngroups, const int64_t* offsets,
                              const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double eps, double weight_decay,
                              float grad_scale, int step, vae_stream_t stream) {
    if (ngroups < 1 || ngroups > 2) return vae_set_error("vae_adamw_step", "1 or 2 groups");
    if (step < 1) return vae_set_error("vae_adamw_step", "step is 1-based");
    AdamArgs a;
    const dim3 grid = adam_args(a, params, grads, m, v, ngroups, offsets, sizes, lrs, beta1s, beta2, eps, weight_decay, grad_scale, step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    for (int i = 0; i < ngroups; ++i) {
        const double bc1 = 1.0 - pow(beta1s[i], (double)step);   // torch.optim.AdamW: bias corrections with the CURRENT (cycled) beta1
        a.grp[i].step_size = (float)(lrs[i] / bc1); a.grp[i].inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    }
    return launch("adamw_kernel", adamw_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
}

// Gradient clipping / non-finite skipping (grad_clip.cuh).  The device-side arguments of the clipped update.
struct ClipArgs {
    double max_grad_norm; int skip_nonfinite;
    int64_t* step; double* norm_out; int64_t* skipped; void* scratch;
};
static int check_groups(const char* what, int ngroups, const int64_t* offsets, const int64_t* sizes) {
    if (ngroups < 1 || ngroups > 2) return vae_set_error(what, "1 or 2 groups");
    if (!offsets || !sizes) return vae_set_error(what, "null offsets / sizes");
    for (int i = 0; i < ngroups; ++i)
        if (offsets[i] < 0 || sizes[i] < 1) return vae_set_error(what, "empty or negative range");
    return 0;
}
static int check_clip_args(const char* what, int ngroups, const int64_t* offsets, const int64_t* sizes, const ClipArgs& k) {
    if (check_groups(what, ngroups, offsets, sizes)) return -1;
    if (k.max_grad_norm != k.max_grad_norm) return vae_set_error(what, "max_grad_norm is NaN");
    if (!k.step || !k.norm_out || !k.skipped || !k.scratch) return vae_set_error(what, "null device pointer (step, norm_out, skipped, scratch)");
    if ((uintptr_t)k.scratch % 16) return vae_set_error(what, "scratch must be 16-byte aligned");
    return 0;
}
// sum of squares + finalize on `st`; `clip` null: the norm alone
static int launch_grad_norm(const float* grads, int ngroups, const int64_t* offsets, const int64_t* sizes, float grad_scale,
                            const double* lrs, const double* beta1s, double beta2, const ClipArgs& k, bool clip, hipStream_t st) {
    GradSumsqArgs s;
    s.g = grads; s.grad_scale = grad_scale; s.partial = static_cast<double*>(k.scratch);
    for (int i = 0; i < ngroups; ++i) { s.off[i] = offsets[i]; s.n[i] = sizes[i]; }
    if (launch("grad_sumsq_kernel", grad_sumsq_kernel, dim3(GCLIP_BLOCKS, ngroups), dim3(256), 0, st, s)) return -1;
    GradClipArgs f = {};
    f.partial = s.partial; f.ngrp = ngroups; f.max_norm = k.max_grad_norm; f.skip = k.skip_nonfinite ? 1 : 0;
    f.step = clip ? reinterpret_cast<long long*>(k.step) : nullptr; f.skipped = reinterpret_cast<long long*>(k.skipped);
    f.norm_out = k.norm_out; f.beta2 = beta2;
    for (int i = 0; i < ngroups && clip; ++i) { f.lr[i] = lrs[i]; f.beta1[i] = beta1s[i]; }
    f.rec = reinterpret_cast<GradClipRecord*>(static_cast<char*>(k.scratch) + GCLIP_RECORD_OFF);
    return launch("grad_clip_finalize_kernel", grad_clip_finalize_kernel, dim3(1), dim3(256), 0, st, f);
}
static int adamw_step_clipped(float* params, const float* grads, float* m, float* v, int ngroups, const int64_t* offsets,
                              const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double eps, double weight_decay,
                              float grad_scale, const ClipArgs& k, hipStream_t st) {
    if (launch_grad_norm(grads, ngroups, offsets, sizes, grad_scale, lrs, beta1s, beta2, k, true, st)) return -1;
    AdamArgs a;
    const dim3 grid = adam_args(a, params, grads, m, v, ngroups, offsets, sizes, lrs, beta1s, beta2, eps, weight_decay, grad_scale, 0);
    const GradClipRecord* rec = reinterpret_cast<const GradClipRecord*>(static_cast<const char*>(k.scratch) + GCLIP_RECORD_OFF);
    return launch("adamw_clipped_kernel", adamw_clipped_kernel, grid, dim3(256), 0, st, a, rec);
}

extern "C" int vae_grad_norm(const float* grads, int ngroups, const int64_t* offsets, const int64_t* sizes, float grad_scale,
                             double* norm_out, void* scratch, vae_stream_t stream) {
    if (!grads) return vae_set_error("vae_grad_norm", "null gradient buffer");
    if (check_groups("vae_grad_norm", ngroups, offsets, sizes)) return -1;
    if (!norm_out || !scratch) return vae_set_error("vae_grad_norm", "null device pointer (norm_out, scratch)");
    if ((uintptr_t)scratch % 16) return vae_set_error("vae_grad_norm", "scratch must be 16-byte aligned");
    ClipArgs k = {0.0, 0, nullptr, norm_out, nullptr, scratch};
    return launch_grad_norm(grads, ngroups, offsets, sizes, grad_scale, nullptr, nullptr, 0.0, k, false, (hipStream_t)stream);
}

extern "C" int vae_adamw_step_clipped(float* params, const float* grads, float* m, float* v, int ngroups, const int64_t* offsets,
                                      const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double eps,
                                      double weight_decay, float grad_scale, double max_grad_norm, int skip_nonfinite, int64_t* step,
                                      double* norm_out, int64_t* skipped, void* scratch, vae_stream_t stream) {
    const ClipArgs k = {max_grad_norm, skip_nonfinite, step, norm_out, skipped, scratch};
    if (check_clip_args("vae_adamw_step_clipped", ngroups, offsets, sizes, k)) return -1;
    if (!params || !grads || !m || !v || !lrs || !beta1s) return vae_set_error("vae_adamw_step_clipped", "null pointer argument");
    return adamw_step_clipped(params, grads, m, v, ngroups, offsets, sizes, lrs, beta1s, beta2, eps, weight_decay, grad_scale, k,
                              (hipStream_t)stream);
}

extern "C" int vae_train_step(vae_ctx* c, const float* x, int B, float* params, float* grads, float* m, float* v, float* bn_running,
                              int64_t* nbt, const float* eps, uint64_t seed, float kld_weight, int ngroups, const int64_t* offsets,
                              const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double adam_eps,
                              double weight_decay, int step, float* xhat, float* mu, float* lv, float* z, float* out3, vae_stream_t stream) {
    if (vae_forward(c, x, B, params, bn_running, nbt, eps, seed, 1, xhat, mu, lv, z, stream)) return -1;
    if (vae_loss_deferred(c, kld_weight, out3, stream)) return -1;
    if (vae_backward(c, x, params, grads, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kld_weight, 1, stream)) return -1;
    if (ngroups > 0 && vae_adamw_step(params, grads, m, v, ngroups, offsets, sizes, lrs, beta1s, beta2, adam_eps, weight_decay, 1.f, step, stream)) return -1;
    return 0;
}

// The fused training step as ONE host call (what torch_vae_amd.train.fused_step enqueues per iteration; train.py:634-659):
// forward with the output conv deferred (train = 2), ELBO scalars finalised beside the backward, backward, the gradient
// exchange of a data-parallel job, AdamW.  `exchange`:
//   0  none (single process);
//   1  ONE RCCL group over the `ngroups` optimised ranges on the compute stream, between the last backward kernel and AdamW;
//   2  bucketed: every group's all-reduce runs on the context's communication stream as soon as its gradients are complete
//      (the LAST group of the list - the decoder - after the first half of the backward, under the encoder half; the others
//      after the second half), and every group's AdamW launch waits only for its own bucket's event, so the update of one
//      group runs while the other group's all-reduce is still in flight (train.py:165-166,201,663 prepare this data-parallel
//      layout; the reference itself never exchanges).  Same arithmetic as 1: results are bit-identical.
// Modes 1 and 2 need vae_comm_init.  Outputs (xhat, mu, log_var, z, out3) are caller-owned as in vae_forward / vae_loss.
// `clip` (vae_train_step_fused_clipped): the gradient norm runs after the exchange and the AdamW of every group behind it; with
// exchange 2 that means behind BOTH buckets' events - the update of one group no longer overlaps the other bucket's all-reduce.
static int train_step_fused(vae_ctx* c, const float* x, int B, float* params, float* grads, float* m, float* v, float* bn_running,
                            int64_t* nbt, const float* eps, uint64_t seed, float kld_weight, int ngroups, const int64_t* offsets,
                            const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double adam_eps,
                            double weight_decay, float grad_scale, int step, const ClipArgs* clip, int exchange, float* xhat, float* mu,
                            float* lv, float* z, float* out3, vae_stream_t stream) {
    if (!c) return vae_set_error("vae_train_step_fused", "null ctx");
    if (exchange < 0 || exchange > 2) return vae_set_error("vae_train_step_fused", "exchange must be 0, 1 or 2");
    if (exchange && !c->nccl_comm) return vae_set_error("vae_train_step_fused", "gradient exchange without a communicator: call vae_comm_init first");
    if (exchange && ngroups < 1) return vae_set_error("vae_train_step_fused", "gradient exchange needs the optimised ranges");
    hipStream_t st = (hipStream_t)stream;
    if (vae_forward(c, x, B, params, bn_running, nbt, eps, seed, 2, xhat, mu, lv, z, stream)) return -1;
    if (vae_loss_deferred(c, kld_weight, out3, stream)) return -1;
    if (exchange != 2) {
        if (vae_backward(c, x, params, grads, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kld_weight, 1, stream)) return -1;
        if (exchange == 1 && vae_allreduce_grads(c, grads, ngroups, offsets, sizes, 1, stream)) return -1;
        if (clip) return adamw_step_clipped(params, grads, m, v, ngroups, offsets, sizes, lrs, beta1s, beta2, adam_eps, weight_decay, grad_scale, *clip, st);
        if (ngroups > 0 && vae_adamw_step(params, grads, m, v, ngroups, offsets, sizes, lrs, beta1s, beta2, adam_eps, weight_decay, grad_scale, step, stream)) return -1;
        return 0;
    }
    // bucketed exchange
    if (ngroups > vae_ctx::NBUCKET) return vae_set_error("vae_train_step_fused", "too many groups");
    if (vae_backward_part(c, x, params, grads, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kld_weight, 1, 1, stream)) return -1;
    vae_stream_t cs = nullptr;
    const int last = ngroups - 1;
    if (vae_comm_stream(c, stream, &cs)) return -1;                              // ordered after the first half of the backward
    if (vae_allreduce_grads(c, grads, 1, offsets + last, sizes + last, 1, cs)) return -1;
    HIP_CHECK_RET(hipEventRecord(c->ev_bucket[last], (hipStream_t)cs));
    if (vae_backward_part(c, x, params, grads, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kld_weight, 1, 2, stream)) return -1;   // (joins the communication stream)
    if (last > 0) {
        if (vae_comm_stream(c, stream, &cs)) return -1;                          // ordered after the second half
        if (vae_allreduce_grads(c, grads, last, offsets, sizes, 1, cs)) return -1;
        for (int i = 0; i < last; ++i) HIP_CHECK_RET(hipEventRecord(c->ev_bucket[i], (hipStream_t)cs));
    }
    if (clip) {                                                                  // the norm needs every bucket
        for (int i = last; i >= 0; --i) HIP_CHECK_RET(hipStreamWaitEvent(st, c->ev_bucket[i], 0));
        c->comm_busy = 0;
        return adamw_step_clipped(params, grads, m, v, ngroups, offsets, sizes, lrs, beta1s, beta2, adam_eps, weight_decay, grad_scale, *clip, st);
    }
    for (int i = last; i >= 0; --i) {                                            // decoder first: its bucket has long arrived
        HIP_CHECK_RET(hipStreamWaitEvent(st, c->ev_bucket[i], 0));
        if (vae_adamw_step(params, grads, m, v, 1, offsets + i, sizes + i, lrs + i, beta1s + i, beta2, adam_eps, weight_decay, grad_scale, step, stream)) return -1;
    }
    c->comm_busy = 0;                                                            // every piece of work on the communication stream has been waited for
    return 0;
}
extern "C" int vae_train_step_fused(vae_ctx* c, const float* x, int B, float* params, float* grads, float* m, float* v, float* bn_running,
                                    int64_t* nbt, const float* eps, uint64_t seed, float kld_weight, int ngroups, const int64_t* offsets,
                                    const int64_t* sizes, const double* lrs, const double* beta1s, double beta2, double adam_eps,
                                    double weight_decay, float grad_scale, int step, int exchange, float* xhat, float* mu, float* lv,
                                    float* z, float* out3, vae_stream_t stream) {
    return train_step_fused(c, x, B, params, grads, m, v, bn_running, nbt, eps, seed, kld_weight, ngroups, offsets, sizes, lrs, beta1s, beta2,
                            adam_eps, weight_decay, grad_scale, step, nullptr, exchange, xhat, mu, lv, z, out3, stream);
}
extern "C" int vae_train_step_fused_clipped(vae_ctx* c, const float* x, int B, float* params, float* grads, float* m, float* v,
                                            float* bn_running, int64_t* nbt, const float* eps, uint64_t seed, float kld_weight, int ngroups,
                                            const int64_t* offsets, const int64_t* sizes, const double* lrs, const double* beta1s, double beta2,
                                            double adam_eps, double weight_decay, float grad_scale, double max_grad_norm, int skip_nonfinite,
                                            int64_t* step, double* norm_out, int64_t* skipped, void* scratch, int exchange, float* xhat,
                                            float* mu, float* lv, float* z, float* out3, vae_stream_t stream) {
    const ClipArgs k = {max_grad_norm, skip_nonfinite, step, norm_out, skipped, scratch};
    if (check_clip_args("vae_train_step_fused_clipped", ngroups, offsets, sizes, k)) return -1;   // (before anything is enqueued)
    if (!c) return vae_set_error("vae_train_step_fused_clipped", "null ctx");
    if (!params || !grads || !m || !v || !lrs || !beta1s) return vae_set_error("vae_train_step_fused_clipped", "null pointer argument");
    return train_step_fused(c, x, B, params, grads, m, v, bn_running, nbt, eps, seed, kld_weight, ngroups, offsets, sizes, lrs, beta1s, beta2,
                            adam_eps, weight_decay, grad_scale, 1, &k, exchange, xhat, mu, lv, z, out3, stream);
}

// diagnostic: phase stamps of the pipelined down kernel for one layer ("encoder.3", epi) into out[grid*4*6]
extern "C" int vae_debug_stamps(vae_ctx* c, const char* tag, int epi, long long* out) {
    if (!c) return -1;
    c->dbg_buf = out; c->dbg_epi = epi; strncpy(c->dbg_tag, tag ? tag : "", sizeof(c->dbg_tag) - 1);
    return 0;
}

extern "C" int vae_profile(vae_ctx* c, int enable) {
    if (!c) return vae_set_error("vae_profile", "null ctx");
    for (auto& r : c->prof_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    c->prof_recs.clear(); c->prof = enable;
    return 0;
}
// the end of every profile writer: the text and its NUL into (buf, cap), or a refusal
static int copy_text(const char* what, const std::string& out, char* buf, int64_t cap) {
    if ((int64_t)out.size() + 1 > cap) return vae_set_error(what, "buffer too small");
    memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
}
// JSON: [{"name":..,"calls":n,"ms":total,"bytes":total algorithmic bytes,"flops":total}, ...]
extern "C" int vae_profile_report(vae_ctx* c, char* buf, int64_t cap) {
    if (!c) return vae_set_error("vae_profile_report", "null ctx");
    HIP_CHECK_RET(hipDeviceSynchronize());
    struct Agg { std::string name; int calls; double ms, bytes, flops; int side; };
    std::vector<Agg> agg;
    for (auto& r : c->prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
        Agg* a = nullptr;
        for (auto& x : agg) if (x.name == r.name) a = &x;
        if (!a) { agg.push_back({r.name, 0, 0, 0, 0, r.side}); a = &agg.back(); }
        a->calls += 1; a->ms += ms; a->bytes += r.bytes; a->flops += r.flops;
    }
    std::string out = "[";
    for (size_t i = 0; i < agg.size(); ++i) {
        char line[512];
        snprintf(line, sizeof(line), "%s{\"name\":\"%s\",\"calls\":%d,\"ms\":%.6f,\"bytes\":%.1f,\"flops\":%.1f,\"side\":%d}", i ? "," : "",
                 agg[i].name.c_str(), agg[i].calls, agg[i].ms, agg[i].bytes, agg[i].flops, agg[i].side);
        out += line;
    }
    out += "]";
    return copy_text("vae_profile_report", out, buf, cap);
}

// JSON array of the profiled launch labels in launch order (for matching rocprofv3 dispatches to labels)
extern "C" int vae_profile_sequence(vae_ctx* c, char* buf, int64_t cap) {
    if (!c) return vae_set_error("vae_profile_sequence", "null ctx");
    std::string out = "[";
    for (size_t i = 0; i < c->prof_recs.size(); ++i)
        for (int k = 0; k < c->prof_recs[i].launches; ++k) out += std::string(out.size() > 1 ? "," : "") + "\"" + c->prof_recs[i].name + "\"";
    out += "]";
    return copy_text("vae_profile_sequence", out, buf, cap);
}

// JSON: [[name, start_ms, end_ms, algorithmic_bytes], ...] relative to the first recorded launch (shows the overlap of the streams)
extern "C" int vae_profile_timeline(vae_ctx* c, char* buf, int64_t cap) {
    if (!c) return vae_set_error("vae_profile_timeline", "null ctx");
    HIP_CHECK_RET(hipDeviceSynchronize());
    std::string out = "[";
    for (size_t i = 0; i < c->prof_recs.size(); ++i) {
        float t0 = 0.f, t1 = 0.f;
        (void)hipEventElapsedTime(&t0, c->prof_recs[0].e0, c->prof_recs[i].e0);
        (void)hipEventElapsedTime(&t1, c->prof_recs[0].e0, c->prof_recs[i].e1);
        char tmp[96]; snprintf(tmp, sizeof(tmp), "\",%.4f,%.4f,%.0f]", t0, t1, c->prof_recs[i].bytes);
        out += std::string(i ? ",[\"" : "[\"") + c->prof_recs[i].name + tmp;
    }
    out += "]";
    return copy_text("vae_profile_timeline", out, buf, cap);
}

extern "C" int vae_pre_latents(vae_ctx* c, float* out, vae_stream_t stream) {
    if (!c || !c->fwd) return vae_set_error("vae_pre_latents", "no forward");
    return VAE_DISPATCH(c->dtype, pre_latents_impl, (c, out, (hipStream_t)stream));
}
extern "C" int vae_last_eps(vae_ctx* c, float* out, vae_stream_t stream) {
    if (!c || !c->fwd) return vae_set_error("vae_last_eps", "no forward");
    HIP_CHECK_RET(hipMemcpyAsync(out, c->eps, (size_t)c->fwd.B * c->L * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int vae_debug_tensor(vae_ctx* c, int which, float* out, int64_t capacity, vae_stream_t stream) {
    if (!c || !c->fwd) return vae_set_error("vae_debug_tensor", "no forward");
    const void* src; int C, HW;
    if (which == 18) {   // the latent gradient [B, 2L] f32: no layout to convert
        const long n = (long)c->fwd.B * 2 * c->L;
        if (n > capacity) return vae_set_error("vae_debug_tensor", "output too small");
        HIP_CHECK_RET(hipMemcpyAsync(out, c->dlat, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return 0;
    }
    if (which == 19) {   // the per-dimension factors of the last forward's KL objective [L] f32 (an objective other than plain)
        if (c->fwd.kl_kind == VAE_KL_PLAIN || !c->fwd.kl_pending) return vae_set_error("vae_debug_tensor", "the last forward ran with the plain KL objective");
        if (c->L > capacity) return vae_set_error("vae_debug_tensor", "output too small");
        if (join_kl(c, (hipStream_t)stream)) return -1;
        HIP_CHECK_RET(hipMemcpyAsync(out, c->kl_factor(), (size_t)c->L * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return 0;
    }
    if (which == 20) {   // the gradient of the last forward's total correlation [B, 2L] f32 (g_mu | g_log_var), before any weight or scale
        const long n = (long)c->fwd.B * 2 * c->L;
        if (n > capacity) return vae_set_error("vae_debug_tensor", "output too small");
        if (ensure_tc("vae_debug_tensor", c, (hipStream_t)stream)) return -1;
        HIP_CHECK_RET(hipMemcpyAsync(out, c->tc_grad(), (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return 0;
    }
    if (which >= 0 && which < 16) { const BnLayer& l = c->lay[which & 7]; src = which < 8 ? l.y : l.dz; C = l.C; HW = l.H * l.W; }
    else if (which == 16 || which == 17) { src = which == 16 ? c->d0 : c->dd0; C = 256; HW = c->s2; }
    else return vae_set_error("vae_debug_tensor", "bad tensor id");
    const long n = (long)c->fwd.B * C * HW;
    if (n > capacity) return vae_set_error("vae_debug_tensor", "output too small");
    return VAE_DISPATCH(c->dtype, debug_tensor_impl, (c, src, out, n, C, HW, (hipStream_t)stream));
}
