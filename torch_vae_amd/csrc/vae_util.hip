// Context-free utilities of the C ABI (include/vae_step.h): data synthesis and stimulus expansion, the ds_read_b64_tr_b16 self-test,
// latent diagnostics, reconstruction metrics, the resident-pianoroll gather with its augmentation, the note-event extraction and
// the nearest-roll search.
// Nothing here touches a context; the one thing shared with vae_api.hip is the table of kept stream work space (below).
#include "vae_ctx.h"
#include "latent_stats.cuh"
#include "recon_metrics.cuh"
#include "augment.cuh"
#include "note_events.cuh"
#include "nearest_rolls.cuh"

// The kept work space of with_stream_scratch (vae_ctx.h): one table and one mutex for the whole library.
struct StreamScratch { void* p = nullptr; size_t cap = 0; };
std::mutex& stream_scratch_mutex() { static std::mutex mu; return mu; }
int kept_stream_scratch(size_t bytes, hipStream_t st, char** base) {
    static std::map<std::pair<int, hipStream_t>, StreamScratch> kept;
    int dev = 0;
    HIP_CHECK_RET(hipGetDevice(&dev));
    StreamScratch& s = kept[std::make_pair(dev, st)];
    if (!s.p || s.cap < bytes) {
        const size_t cap = std::max<size_t>((bytes + 4095) / 4096 * 4096, 4096);
        void* ws = nullptr;
        HIP_CHECK_RET(hipMallocAsync(&ws, cap, st));
        if (s.p) (void)hipFreeAsync(s.p, st);
        s.p = ws; s.cap = cap;
    }
    *base = static_cast<char*>(s.p);
    return 0;
}

// data_generators.py:45-77 restated with the counter generator (stream 777); one workgroup per image
__global__ void synth_pianoroll_kernel(float* x, int H, unsigned long long seed, int max_lines) {
    const int b = blockIdx.x;
    const int width = 1 + (int)(counter_uniform(0, seed, 777) * 4);
    const unsigned long long base = 1 + (unsigned long long)b * (1 + 4 * max_lines);
    const int n_lines = 1 + (int)(counter_uniform(base, seed, 777) * max_lines);
    for (int p = threadIdx.x; p < H * H; p += blockDim.x) {
        const int py = p / H, px = p % H;
        float v = 0.f;
        for (int li = 0; li < n_lines; ++li) {
            const unsigned long long k = base + 1 + 4ULL * li;
            const bool vert = counter_uniform(k, seed, 777) < 0.5;
            const int pos = (int)(counter_uniform(k + 1, seed, 777) * H);
            const int start = (int)(counter_uniform(k + 2, seed, 777) * H);
            const int end = start + (int)(counter_uniform(k + 3, seed, 777) * (H - start));
            const int lo = max(0, pos - width / 2), hi = min(H, pos + width / 2 + 1);
            const int along = vert ? py : px, across = vert ? px : py;
            if (along >= start && along < end && across >= lo && across < hi) v = 1.f;
        }
        x[(size_t)b * H * H + p] = v;
    }
}
extern "C" int vae_synth_pianoroll(float* x, int B, int H, uint64_t seed, vae_stream_t stream) {
    return launch("synth_pianoroll_kernel", synth_pianoroll_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, H, (unsigned long long)seed, 20);
}

// Byte / bit-plane stimuli -> the float32 batch the kernels read (train.py:630 copies float32 stimuli; pianorolls are 0/1 cells).
// kind 0: one byte per cell (uint8 / bool), value v -> (float)v; kind 1: bit planes, most significant bit first (numpy.packbits
// order), bit -> 0.f / 1.f.  The source may be device memory or PINNED host memory: the kernel then reads the batch straight over
// the host link (0.5 MB of bit planes or 4 MB of bytes for 256 images of 128x128), which removes the separate copy and its
// queue hand-over from the step's dependent chain.
__global__ void expand_bytes_kernel(const uint32_t* __restrict__ src, float* __restrict__ dst, long n4) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const uint32_t w = __builtin_nontemporal_load(src + i);
        *reinterpret_cast<f32x4*>(dst + 4 * i) = f32x4{(float)(w & 255u), (float)((w >> 8) & 255u), (float)((w >> 16) & 255u), (float)(w >> 24)};
    }
}
__global__ void expand_bits_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, long nbytes) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nbytes; i += (long)gridDim.x * blockDim.x) {
        const uint32_t w = __builtin_nontemporal_load(src + i);
        *reinterpret_cast<f32x4*>(dst + 8 * i) = f32x4{(float)((w >> 7) & 1u), (float)((w >> 6) & 1u), (float)((w >> 5) & 1u), (float)((w >> 4) & 1u)};
        *reinterpret_cast<f32x4*>(dst + 8 * i + 4) = f32x4{(float)((w >> 3) & 1u), (float)((w >> 2) & 1u), (float)((w >> 1) & 1u), (float)(w & 1u)};
    }
}
// The address the device uses for a source that a kernel reads in place: device memory as is, pinned host memory through its
// mapping; anything else (pageable host memory) is refused under `what` - a kernel must not dereference it - and null returned.
static const void* device_source(const char* what, const void* src) {
    hipPointerAttribute_t at; memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, src) != hipSuccess) (void)hipGetLastError();
    else if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) return src;
    else if (at.type == hipMemoryTypeHost && at.devicePointer) return at.devicePointer;
    vae_set_error(what, "the source is neither device nor pinned host memory");
    return nullptr;
}
extern "C" int vae_expand_stimuli(const void* src, int kind, float* dst, int64_t n_cells, vae_stream_t stream) {
    if (!src || !dst) return vae_set_error("vae_expand_stimuli", "null pointer");
    if (kind != 0 && kind != 1) return vae_set_error("vae_expand_stimuli", "kind must be 0 (bytes) or 1 (bit planes)");
    if (n_cells < 0 || n_cells % 8) return vae_set_error("vae_expand_stimuli", "the number of cells must be a multiple of 8");
    if (n_cells == 0) return 0;
    const void* dsrc = device_source("vae_expand_stimuli", src);
    if (!dsrc) return -1;
    if ((reinterpret_cast<uintptr_t>(dsrc) & 3) || (reinterpret_cast<uintptr_t>(dst) & 15)) return vae_set_error("vae_expand_stimuli", "source must be 4-byte, destination 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long n = n_cells / (kind == 0 ? 4 : 8);   // words of four byte cells, or bytes of eight bit cells
    const dim3 grid((unsigned)std::min<long>((n + 255) / 256, 2048));
    if (kind == 0) return launch("expand_stimuli_kernel", expand_bytes_kernel, grid, dim3(256), 0, st, reinterpret_cast<const uint32_t*>(dsrc), dst, n);
    return launch("expand_stimuli_kernel", expand_bits_kernel, grid, dim3(256), 0, st, reinterpret_cast<const uint8_t*>(dsrc), dst, n);
}

// Resident pianorolls -> one augmented float32 batch (augment.cuh); the draws alone for inspection.  Both are one launch.
static const char* augment_refusal(int batch, int src_w, int w, int P, int T, int crop_mode) {
    if (batch < 0) return "batch must be >= 0";
    if (w <= 0 || w % 8 || src_w <= 0 || src_w % 8 || src_w > (1 << 30)) return "w and src_w must be positive multiples of 8 (at most 2^30)";
    if (src_w < w) return "src_w must be >= w";
    if (P < 0 || T < 0 || P > (1 << 24) || T > (1 << 24)) return "max_pitch_shift and max_time_shift must be in [0, 2^24]";
    if (crop_mode != 0 && crop_mode != 1) return "crop_mode must be 0 (random) or 1 (centre)";
    return nullptr;
}
extern "C" int vae_gather_rolls(const void* src, int kind, int64_t n_rolls, int h, int src_w, const int64_t* index, int64_t first,
                                const int32_t* params, uint64_t seed, uint64_t counter0, uint64_t counter_stride, int max_pitch_shift,
                                int max_time_shift, int crop_mode, float scale, float* dst, int batch, int w, vae_stream_t stream) {
    const char* what = "vae_gather_rolls";
    if (!src || !dst) return vae_set_error(what, "null pointer (src, dst)");
    if (kind < 0 || kind > 2) return vae_set_error(what, "kind must be 0 (bytes), 1 (bit planes) or 2 (float32)");
    if (h <= 0) return vae_set_error(what, "h must be > 0");
    if (const char* why = augment_refusal(batch, src_w, w, max_pitch_shift, max_time_shift, crop_mode)) return vae_set_error(what, why);
    const int64_t row_bytes = kind == 1 ? src_w / 8 : (int64_t)src_w * (kind == 2 ? 4 : 1);
    if (n_rolls <= 0 || n_rolls > ((int64_t)1 << 62) / ((int64_t)h * row_bytes)) return vae_set_error(what, "n_rolls must be > 0 (and the source below 2^62 bytes)");
    if (!std::isfinite(scale)) return vae_set_error(what, "scale must be finite");
    if ((reinterpret_cast<uintptr_t>(dst) & 15) || (reinterpret_cast<uintptr_t>(index) & 7) || (reinterpret_cast<uintptr_t>(params) & 3))
        return vae_set_error(what, "dst must be 16-byte, index 8-byte, params 4-byte aligned");
    if (batch == 0) return 0;
    const void* dsrc = device_source(what, src);
    if (!dsrc) return -1;
    if (kind == 2 && (reinterpret_cast<uintptr_t>(dsrc) & 3)) return vae_set_error(what, "a float32 source must be 4-byte aligned");
    GatherArgs a{dsrc, (long)n_rolls, h, src_w, reinterpret_cast<const long*>(index), (long)first, params, (unsigned long long)seed,
                 (unsigned long long)counter0, (unsigned long long)counter_stride, max_pitch_shift, max_time_shift, crop_mode, scale, dst, batch, w, 0};
    // workgroup tile: TX = 2^lg_tx lanes along a row (covering its w/8 work items where 64 lanes can) by AUG_THREADS / TX rows.
    // grid x: row tiles of one roll, y: samples; at most AUG_MAX_BLOCKS workgroups, the rest is stride loops
    int lg_tx = 0;
    while ((1 << lg_tx) < w / 8 && lg_tx < 6) ++lg_tx;
    const long rows = AUG_THREADS >> lg_tx;
    const unsigned gx = (unsigned)std::min<long>((h + rows - 1) / rows, AUG_MAX_BLOCKS);
    const dim3 grid(gx, (unsigned)std::min<long>(batch, std::max<long>(1, AUG_MAX_BLOCKS / gx)));
    a.lg_tx = lg_tx;
    return pick_const<0, 1, 2>("gather_rolls_kernel", kind, [&](auto K) {
        return launch("gather_rolls_kernel", gather_rolls_kernel<decltype(K)::value>, grid, dim3(AUG_THREADS), 0, (hipStream_t)stream, a); });
}
extern "C" int vae_augment_params(int32_t* params, int batch, int src_w, int w, uint64_t seed, uint64_t counter0, uint64_t counter_stride,
                                  int max_pitch_shift, int max_time_shift, int crop_mode, vae_stream_t stream) {
    const char* what = "vae_augment_params";
    if (!params) return vae_set_error(what, "null pointer (params)");
    if (const char* why = augment_refusal(batch, src_w, w, max_pitch_shift, max_time_shift, crop_mode)) return vae_set_error(what, why);
    if (reinterpret_cast<uintptr_t>(params) & 3) return vae_set_error(what, "params must be 4-byte aligned");
    if (batch == 0) return 0;
    const dim3 grid((unsigned)std::min<long>(((long)batch + AUG_THREADS - 1) / AUG_THREADS, AUG_MAX_BLOCKS));
    return launch("augment_params_kernel", augment_params_kernel, grid, dim3(AUG_THREADS), 0, (hipStream_t)stream, params, batch, src_w - w,
                  (unsigned long long)seed, (unsigned long long)counter0, (unsigned long long)counter_stride, max_pitch_shift, max_time_shift, crop_mode);
}

// Latent diagnostics (latent_stats.cuh).  Launches: prep (tables, z), joint and dims pairwise kernels over split component ranges,
// two merges, the per-dimension moments, the scalar combine.  Work space from the stream-ordered allocator, freed on the stream.
// The split counts depend on (n, L, draws) only, so a given shape always reduces in the same order.
extern "C" int vae_latent_stats(const float* mu, const float* lv, int64_t n, int L, int S, const float* eps, uint64_t seed,
                                double* log_qz, double* log_qz_dims, double* per_dim, double* scalars, vae_stream_t stream) {
    if (!mu || !lv || !log_qz || !log_qz_dims || !per_dim || !scalars) return vae_set_error("vae_latent_stats", "null tensor pointer");
    if (n < 1 || n > (int64_t)1 << 30) return vae_set_error("vae_latent_stats", "n must be in [1, 2^30]");
    if (L < 1 || L > 4096) return vae_set_error("vae_latent_stats", "latent_dim must be in [1, 4096]");
    if (S < 1) return vae_set_error("vae_latent_stats", "draws must be >= 1");
    const long N = (long)n, SN = (long)S * N;
    if (SN > ((long)1 << 40) / L) return vae_set_error("vae_latent_stats", "draws * n * latent_dim too large");
    hipStream_t st = (hipStream_t)stream;
    // split of the component range: enough waves for the 256 CUs, at least 256 components per split, at most 64 splits
    auto splits = [&](long waves, long target, int tile, int& jper) {
        long ns = std::max<long>(1, std::min<long>({(target + waves - 1) / waves, (N + 255) / 256, 64}));
        jper = (int)(((N + ns - 1) / ns + tile - 1) / tile * tile);
        return (int)((N + jper - 1) / jper);
    };
    const long jblocks = (SN + 256 * LS_QR - 1) / (256 * LS_QR);
    int jper_j = 0;
    const int nsj = splits(jblocks * 4, 2048, LS_JT, jper_j);
    const int DB = std::min(L, LS_DB), QG = 256 / DB, ndt = (L + DB - 1) / DB;
    const long dblocks = (long)ndt * ((SN + (long)QG * LS_QR - 1) / ((long)QG * LS_QR));
    int jper_d = 0;
    const int nsd = splits(dblocks * 4, 4096, LS_JD, jper_d);
    if (jblocks > INT32_MAX || dblocks > INT32_MAX) return vae_set_error("vae_latent_stats", "grid too large");
    const size_t nl = (size_t)N * L, snl = (size_t)SN * L;
    size_t off[8], tot = 0;
    const size_t sz[7] = {snl * 4, nl * 8, nl * 4, (size_t)N * 4, (size_t)nsj * SN * 8, (size_t)nsd * snl * 8, (size_t)4 * L * 8};
    for (int k = 0; k < 7; ++k) { off[k] = tot; tot += (sz[k] + 255) / 256 * 256; }
    const double lnN = log((double)N);
    return with_stream_scratch(tot, st, [&](char* base) -> int {
        float* z = reinterpret_cast<float*>(base + off[0]);
        float2* mh = reinterpret_cast<float2*>(base + off[1]);
        float* c2 = reinterpret_cast<float*>(base + off[2]);
        float* cj = reinterpret_cast<float*>(base + off[3]);
        float2* pj = reinterpret_cast<float2*>(base + off[4]);
        float2* pd = reinterpret_cast<float2*>(base + off[5]);
        double* dstat = reinterpret_cast<double*>(base + off[6]);
        const dim3 blk(256);
        if (launch("lstat_prep_kernel", lstat_prep_kernel, dim3((unsigned)((N + 3) / 4)), blk, 0, st, mu, lv, eps, (unsigned long long)seed,
                   (int)N, L, S, z, mh, c2, cj)) return -1;
        if (launch("lstat_joint_kernel", lstat_joint_kernel, dim3((unsigned)jblocks, nsj), blk, 0, st, z, mh, cj, SN, (int)N, L, jper_j, pj)) return -1;
        if (launch("lstat_dims_kernel", lstat_dims_kernel, dim3((unsigned)dblocks, nsd), blk, 0, st, z, mh, c2, SN, (int)N, L, DB, ndt, jper_d, pd)) return -1;
        if (launch("lstat_merge_kernel", lstat_merge_kernel, dim3((unsigned)std::min<long>((SN + 255) / 256, 4096)), blk, 0, st, pj, nsj, SN, lnN,
                   log_qz)) return -1;
        if (launch("lstat_merge_kernel", lstat_merge_kernel, dim3((unsigned)std::min<long>((long)(snl + 255) / 256, 8192)), blk, 0, st, pd, nsd,
                   (long)snl, lnN, log_qz_dims)) return -1;
        if (launch("lstat_moments_kernel", lstat_moments_kernel, dim3(L), blk, 0, st, mu, lv, log_qz_dims, (int)N, SN, L, per_dim, dstat)) return -1;
        return launch("lstat_final_kernel", lstat_final_kernel, dim3(1), blk, 0, st, log_qz, SN, dstat, L, scalars);
    });
}

// Note-level reconstruction metrics (recon_metrics.cuh).  Two launches: the pass over the cells, one workgroup per (roll, chunk), and
// the fold of chunks into rolls and of rolls into the totals, one wave per output field.  The per-chunk ranges (and, for rolls longer than one
// chunk, the per-chunk sums and counts) go through the stream-ordered allocator; nothing is read back.
extern "C" int vae_recon_metrics(const float* xhat, const float* target, int64_t rolls, int64_t roll_len, const float* thresholds,
                                 int n_thresholds, float target_threshold, double* roll_sums, int64_t* roll_counts, double* totals,
                                 int64_t* total_counts, int accumulate, vae_stream_t stream) {
    const char* what = "vae_recon_metrics";
    if (!thresholds || !totals || !total_counts) return vae_set_error(what, "null pointer (thresholds, totals, total_counts)");
    if (n_thresholds < 1 || n_thresholds > RM_MAX_T) return vae_set_error(what, "n_thresholds must be in 1..8");
    RmThresholds th{};
    for (int k = 0; k < n_thresholds; ++k) {
        if (!std::isfinite(thresholds[k])) return vae_set_error(what, "thresholds must be finite");
        th.t[k] = thresholds[k];
    }
    if (!std::isfinite(target_threshold)) return vae_set_error(what, "target_threshold must be finite");
    if (rolls < 0) return vae_set_error(what, "rolls must be >= 0");
    if (roll_len < 1) return vae_set_error(what, "roll_len must be >= 1");
    if (accumulate != 0 && accumulate != 1) return vae_set_error(what, "accumulate must be 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    const int ncnt = 1 + 2 * n_thresholds;
    if (rolls == 0) {
        if (!accumulate) {
            HIP_CHECK_RET(hipMemsetAsync(totals, 0, 8 * sizeof(double), st));
            HIP_CHECK_RET(hipMemsetAsync(total_counts, 0, ncnt * sizeof(int64_t), st));
        }
        return 0;
    }
    if (!xhat || !target || !roll_sums || !roll_counts) return vae_set_error(what, "null pointer (xhat, target, roll_sums, roll_counts)");
    if ((reinterpret_cast<uintptr_t>(xhat) | reinterpret_cast<uintptr_t>(target)) & 3) return vae_set_error(what, "xhat and target must be 4-byte aligned");
    const int64_t nchunks = (roll_len - 1) / RM_CHUNK + 1;
    if (rolls > INT32_MAX / nchunks) return vae_set_error(what, "rolls * ceil(roll_len / 4096) must stay below 2^31");
    if (roll_len > ((int64_t)1 << 52) / rolls) return vae_set_error(what, "rolls * roll_len must stay below 2^52");
    const size_t np = (size_t)(rolls * nchunks);
    const size_t rng_bytes = (np * 4 * sizeof(float) + 255) / 256 * 256, sum_bytes = (np * 3 * sizeof(double) + 255) / 256 * 256;
    const bool split = nchunks > 1;
    return with_stream_scratch(rng_bytes + (split ? sum_bytes + np * ncnt * sizeof(int64_t) : 0), st, [&](char* base) -> int {
        float* pr = reinterpret_cast<float*>(base);
        double* ps = split ? reinterpret_cast<double*>(base + rng_bytes) : roll_sums;
        long long* pc = split ? reinterpret_cast<long long*>(base + rng_bytes + sum_bytes) : reinterpret_cast<long long*>(roll_counts);
        // the threshold count is a template argument: the counters stay in registers
        if (pick_const<1, 2, 3, 4, 5, 6, 7, 8>("recon_metrics_kernel", n_thresholds, [&](auto T) {
                return launch("recon_metrics_kernel", recon_metrics_kernel<decltype(T)::value>, dim3((unsigned)np), dim3(RM_THREADS), 0, st, xhat,
                              target, (long)roll_len, (long)nchunks, th, target_threshold, ps, pc, pr); })) return -1;
        return launch("recon_metrics_fold_kernel", recon_metrics_fold_kernel, dim3(1 + (3 + ncnt + 3) / 4), dim3(RM_THREADS), 0, st, (long)rolls,
                      (long)nchunks, ncnt, (double)rolls * (double)roll_len, ps, pc, pr, roll_sums, reinterpret_cast<long long*>(roll_counts), totals,
                      reinterpret_cast<long long*>(total_counts), accumulate);
    });
}

// Note events of float pianorolls (note_events.cuh).  Launches: the count per row, the one-workgroup scan (which also writes offsets),
// the write of events, peaks and cleaned planes - skipped when no events are asked for (the count launch then writes the planes).  Work space: one int32 per row and one
// int64 per scan tile, from the stream-ordered allocator; nothing is read back.
extern "C" int vae_extract_notes(const float* rolls, int64_t n, int h, int w, float onset_threshold, float sustain_threshold,
                                 int min_duration, int max_gap, int32_t* events, float* peaks, int64_t capacity, int64_t* offsets,
                                 uint8_t* cleaned, vae_stream_t stream) {
    const char* what = "vae_extract_notes";
    if (!rolls || !offsets) return vae_set_error(what, "null pointer (rolls, offsets)");
    if (!events != !peaks) return vae_set_error(what, "events and peaks must both be given or both be null");
    if (n < 0) return vae_set_error(what, "n must be >= 0");
    if (h < 1) return vae_set_error(what, "h must be >= 1");
    if (w < 8 || w > NE_MAX_W || w % 8) return vae_set_error(what, "w must be a multiple of 8 in 8..65536");
    if (n > (int64_t)INT32_MAX / h) return vae_set_error(what, "n * h must stay below 2^31");
    if (!std::isfinite(onset_threshold) || !std::isfinite(sustain_threshold)) return vae_set_error(what, "the thresholds must be finite");
    if (sustain_threshold > onset_threshold) return vae_set_error(what, "sustain_threshold must be <= onset_threshold");
    if (min_duration < 1) return vae_set_error(what, "min_duration must be >= 1");
    if (max_gap < 0) return vae_set_error(what, "max_gap must be >= 0");
    if (capacity < 0) return vae_set_error(what, "capacity must be >= 0");
    if ((reinterpret_cast<uintptr_t>(rolls) | reinterpret_cast<uintptr_t>(peaks) | reinterpret_cast<uintptr_t>(events)) & 3)
        return vae_set_error(what, "rolls, events and peaks must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(offsets) & 7) return vae_set_error(what, "offsets must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIP_CHECK_RET(hipMemsetAsync(offsets, 0, sizeof(int64_t), st));
        return 0;
    }
    const long nrows = (long)n * h;
    const size_t cnt_bytes = ((size_t)nrows * sizeof(int) + 255) / 256 * 256, ntiles = (size_t)((nrows + NE_TILE - 1) >> NE_TILE_LG);
    const dim3 grid((unsigned)((nrows + NE_ROWS - 1) / NE_ROWS)), blk(NE_THREADS);
    const size_t lds = (size_t)NE_ROWS * ((w + 63) / 64) * sizeof(ne_u64);
    return with_stream_scratch(cnt_bytes + ntiles * sizeof(long long), st, [&](char* base) -> int {
        int* counts = reinterpret_cast<int*>(base);
        long long* tile_base = reinterpret_cast<long long*>(base + cnt_bytes);
        const bool planes_only = !events && cleaned;
        if (pick_bool(planes_only, [&](auto P) {
                return launch("note_count_kernel", note_count_kernel<decltype(P)::value>, grid, blk, lds, st, rolls, nrows, w, onset_threshold,
                              sustain_threshold, min_duration, max_gap, counts, reinterpret_cast<unsigned char*>(cleaned)); })) return -1;
        if (launch("note_scan_kernel", note_scan_kernel, dim3(1), dim3(NE_SCAN_THREADS), 0, st, counts, nrows, h, tile_base,
                   reinterpret_cast<long long*>(offsets), (long)n)) return -1;
        if (!events) return 0;
        return launch("note_emit_kernel", note_emit_kernel, grid, blk, lds, st, rolls, nrows, h, w, onset_threshold, sustain_threshold,
                      min_duration, max_gap, (const int*)counts, (const long long*)tile_base, reinterpret_cast<int*>(events), peaks,
                      (long long)capacity, reinterpret_cast<unsigned char*>(cleaned));
    });
}

// Nearest rolls under transposition and time shift (nearest_rolls.cuh).  Two launches: the search over (query tiles, splits), which
// leaves one k-best list per (query, split) in work space from the stream-ordered allocator, and the merge, one wave per query, which
// also counts the intersections and the query cells.  splits = 0: what brings the grid to 1024 workgroups, at most one split per
// candidate tile and at most NR_MAX_SPLITS - a function of (n_queries, n_rolls) and the tile sizes alone.
extern "C" int vae_nearest_rolls(const uint8_t* queries, int n_queries, const uint8_t* rolls, int64_t n_rolls, int h, int w,
                                 int max_pitch_shift, int max_time_shift, const int64_t* exclude, int k, int splits, int64_t* index,
                                 int32_t* distance, int32_t* shift, int32_t* intersection, int32_t* query_cells, vae_stream_t stream) {
    const char* what = "vae_nearest_rolls";
    const int P = max_pitch_shift, T = max_time_shift;
    if (!queries || !rolls || !index || !distance || !shift || !intersection || !query_cells)
        return vae_set_error(what, "null pointer (queries, rolls, index, distance, shift, intersection, query_cells)");
    if (n_queries < 0) return vae_set_error(what, "n_queries must be >= 0");
    if (n_rolls < 1 || n_rolls > ((int64_t)1 << NR_INDEX_BITS)) return vae_set_error(what, "n_rolls must be in 1..2^40");
    if (h < 1) return vae_set_error(what, "h must be >= 1");
    if (w < 32 || w % 32) return vae_set_error(what, "w must be a positive multiple of 32");
    if ((int64_t)h * (w / 8) > NR_MAX_ROLL_BYTES) return vae_set_error(what, "a roll (h * w / 8 bytes) must fit 8192 bytes");
    if (P < 0 || P >= h) return vae_set_error(what, "max_pitch_shift must be in 0..h-1");
    if (T < 0 || T >= w) return vae_set_error(what, "max_time_shift must be in 0..w-1");
    if ((int64_t)(2 * P + 1) * (2 * T + 1) > NR_MAX_SHIFTS) return vae_set_error(what, "(2 max_pitch_shift + 1) * (2 max_time_shift + 1) must be <= 1023");
    if (k < 1 || k > NR_MAX_K) return vae_set_error(what, "k must be in 1..32");
    if (splits < 0 || splits > NR_MAX_SPLITS) return vae_set_error(what, "splits must be in 0..64");
    if ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(rolls)) & 3) return vae_set_error(what, "queries and rolls must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(exclude)) & 7) return vae_set_error(what, "index and exclude must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(distance) | reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(intersection) |
         reinterpret_cast<uintptr_t>(query_cells)) & 3)
        return vae_set_error(what, "distance, shift, intersection and query_cells must be 4-byte aligned");
    if (n_queries == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int wd = w / 32, words = h * wd;
    const bool large = words * 4 > NR_TILE_ROLL_BYTES;
    const int qt = large ? NR_LARGE_TILE : NR_QUERY_TILE, ct = large ? NR_LARGE_TILE : NR_CAND_TILE;
    const long qtiles = ((long)n_queries + qt - 1) / qt;
    if (splits == 0) splits = (int)std::max<long>(1, std::min<long>({(1024 + qtiles - 1) / qtiles, (long)((n_rolls + ct - 1) / ct), (long)NR_MAX_SPLITS}));
    if (qtiles * splits > INT32_MAX) return vae_set_error(what, "query tiles * splits must stay below 2^31");
    // 0: no time shift, 16-byte LDS reads; 1: no time shift, dwords; 2: any window; 3: |dt| < 32 on rows of whole 16-byte chunks;
    // 4: |dt| < 32 on rows of one chunk
    const int mode = T == 0 ? ((wd % 4 == 0 || (P == 0 && words % 4 == 0)) ? 0 : 1) : ((wd % 4 == 0 && T < 32) ? (wd == 4 ? 4 : 3) : 2);
    const size_t lds = (size_t)(qt + ct) * (((words + 7) & ~7) + 4) * sizeof(unsigned);
    const size_t nlist = (size_t)n_queries * splits * k, key_bytes = (nlist * sizeof(nr_u64) + 255) / 256 * 256;
    return with_stream_scratch(key_bytes + nlist * sizeof(unsigned), st, [&](char* base) -> int {
        NrArgs a{reinterpret_cast<const unsigned*>(queries), n_queries, reinterpret_cast<const unsigned*>(rolls), (long)n_rolls, h, wd, P, T,
                 reinterpret_cast<const long long*>(exclude), k, splits, reinterpret_cast<nr_u64*>(base), reinterpret_cast<unsigned*>(base + key_bytes),
                 reinterpret_cast<long long*>(index), distance, shift, intersection, query_cells};
        const dim3 grid((unsigned)(qtiles * splits));
        if (pick_const<0, 1, 2, 3, 4>("nearest_rolls_kernel", mode, [&](auto M) {
                if (large) return launch("nearest_rolls_kernel", nearest_rolls_kernel<NR_LARGE_TILE, 1, decltype(M)::value>, grid, dim3(64), lds, st, a);
                return launch("nearest_rolls_kernel", nearest_rolls_kernel<4, 4, decltype(M)::value>, grid, dim3(256), lds, st, a); })) return -1;
        return launch("nearest_merge_kernel", nearest_merge_kernel, dim3((unsigned)n_queries), dim3(64), 0, st, a);
    });
}

// Self-test of ds_read_b64_tr_b16: a 16x32 tile of 16-bit words M[k][c] = k*32 + c staged as
// [k][c]; the k-major fragment of lane (r,h) must come back as M[8h+j][r].
__global__ void selftest_tr16_kernel(int* bad) {
    __shared__ __attribute__((aligned(16))) short tile[16 * 32];
    const int lane = threadIdx.x;
    for (int i = lane; i < 16 * 32; i += 64) tile[i] = (short)i;
    __syncthreads();
    const int g4 = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3, r = lane & 31, h = lane >> 5;
    int nbad = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int k = 8 * (g4 >> 1) + 4 * half + q;
        const char* ad = reinterpret_cast<const char*>(tile) + k * 64 + (16 * (g4 & 1) + 4 * p) * 2;
        s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))ad);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if ((int)v[e] != (8 * h + 4 * half + e) * 32 + r) ++nbad;
    }
    if (nbad) atomicAdd(bad, nbad);
}
// Kernel-shaped variant: rows at an arbitrary pitch/base, row gather at stride (the wgrad G operand).
__global__ void selftest_tr16b_kernel(int* bad, int* info, int pitch, int base, int rowstride) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int lane = threadIdx.x;
    short* t = reinterpret_cast<short*>(sm);
    for (int i = lane; i < 8192; i += 64) t[i] = (short)(i * 7 + 3);
    __syncthreads();
    const int g4 = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3, r = lane & 31, h = lane >> 5;
    int nbad = 0;
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int k = ks * 16 + 8 * (g4 >> 1) + 4 * half + q;
            const char* ad = sm + base + (k * rowstride) * pitch + (16 * (g4 & 1) + 4 * p) * 2;
            s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))ad);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = ks * 16 + 8 * h + 4 * half + e;
                const short want = *reinterpret_cast<const short*>(sm + base + (kk * rowstride) * pitch + r * 2);
                if (v[e] != want) { if (nbad == 0 && lane < 64) { info[lane * 4] = ks * 100 + half * 10 + e; info[lane * 4 + 1] = v[e]; info[lane * 4 + 2] = want; } ++nbad; }
            }
        }
    }
    if (nbad) atomicAdd(bad, nbad);
}
extern "C" int vae_selftest_tr16(vae_stream_t stream) {
    int* d = nullptr; int h[1 + 256];
    HIP_CHECK_RET(hipMalloc(&d, sizeof(h)));
    const int cfgs[5][3] = {{64, 0, 1}, {144, 1536, 1}, {80, 768, 1}, {144, 1536, 2}, {80, 768, 3}};
    std::string msg;
    HIP_CHECK_RET(hipMemsetAsync(d, 0, sizeof(h), (hipStream_t)stream));
    hipLaunchKernelGGL(selftest_tr16_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d);
    HIP_CHECK_RET(hipMemcpyAsync(h, d, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_CHECK_RET(hipStreamSynchronize((hipStream_t)stream));
    if (h[0]) msg += "basic:" + std::to_string(h[0]) + " ";
    for (int c = 0; c < 5; ++c) {
        HIP_CHECK_RET(hipMemsetAsync(d, 0, sizeof(h), (hipStream_t)stream));
        hipLaunchKernelGGL(selftest_tr16b_kernel, dim3(1), dim3(64), 16384, (hipStream_t)stream, d, d + 1, cfgs[c][0], cfgs[c][1], cfgs[c][2]);
        HIP_CHECK_RET(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_CHECK_RET(hipStreamSynchronize((hipStream_t)stream));
        if (h[0]) {
            msg += "cfg" + std::to_string(c) + ":" + std::to_string(h[0]) + "[";
            for (int l = 0; l < 64; l += 9) msg += "L" + std::to_string(l) + ":" + std::to_string(h[1 + l * 4]) + "," + std::to_string(h[2 + l * 4]) + "," + std::to_string(h[3 + l * 4]) + " ";
            msg += "] ";
        }
    }
    (void)hipFree(d);
    if (!msg.empty()) return vae_set_error("ds_read_b64_tr_b16 self-test", msg.c_str());
    return 0;
}
