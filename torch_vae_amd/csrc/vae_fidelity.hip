// The set-level fidelity metrics of the C ABI (include/vae_fidelity.h; kernels in set_distance.cuh).  Context-free, like
// vae_util.hip; work space comes from with_stream_scratch, nothing is read back and nothing waits for the device.
#include "vae_ctx.h"
#include "../../include/vae_fidelity.h"
#include "set_distance.cuh"

static_assert(SD_MAX_DIM == VAE_FID_MAX_DIM && SD_MAX_K == VAE_FID_MAX_K && SD_MAX_G == VAE_FID_MAX_BANDWIDTHS &&
              SD_MAX_SPLITS == VAE_FID_MAX_SPLITS && SD_MAX_POINTS == VAE_FID_MAX_POINTS,
              "set_distance.cuh and include/vae_fidelity.h disagree on a limit");

namespace {

const char* fid_shape_refusal(int D, int64_t a, int64_t b, int splits) {
    if (D < 1 || D > SD_MAX_DIM) return "D must be in 1..128";
    if (a < 1 || a > SD_MAX_POINTS || b < 1 || b > SD_MAX_POINTS) return "set sizes must be in 1..2^22";
    if (splits < 0 || splits > SD_MAX_SPLITS) return "splits must be in 0..64";
    return nullptr;
}
bool fid_misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1); }
const char* fid_partials_refusal(int64_t queries, int splits) {
    return (int64_t)splits * queries > ((int64_t)1 << 26) ? "splits * queries must stay within 2^26" : nullptr;
}

int fid_dp(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : D <= 64 ? 64 : 128; }
long fid_qblocks(int64_t queries, int D) { const long per = (long)SD_THREADS * sd_qr(fid_dp(D)); return (long)((queries + per - 1) / per); }
// splits = 0: enough ranges that about 1024 workgroups exist, none shorter than one tile
int fid_splits(int splits, int64_t queries, int64_t refs, int D) {
    if (splits) return splits;
    const long qb = fid_qblocks(queries, D), tiles = (long)((refs + SD_JT - 1) / SD_JT);
    return (int)std::max<long>(1, std::min<long>(std::min<long>((1024 + qb - 1) / qb, tiles), SD_MAX_SPLITS));
}
size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

extern "C" int vae_fidelity_knn_radii(const float* x, int64_t n, int D, int k, int splits, float* radii2, vae_stream_t stream) {
    const char* what = "vae_fidelity_knn_radii";
    if (!x || !radii2) return vae_set_error(what, "null pointer (x, radii2)");
    if (const char* why = fid_shape_refusal(D, n, n, splits)) return vae_set_error(what, why);
    if (k < 1 || k > SD_MAX_K) return vae_set_error(what, "k must be in 1..8");
    if (k >= n) return vae_set_error(what, "k must be < n");
    if (const char* why = fid_partials_refusal(n, splits)) return vae_set_error(what, why);
    if (fid_misaligned(x, 4) || fid_misaligned(radii2, 4)) return vae_set_error(what, "x and radii2 must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int sp = fid_splits(splits, n, n, D);
    const dim3 grid((unsigned)fid_qblocks(n, D), (unsigned)sp);
    SdKnnArgs a{x, (long)n, D, k, sp, radii2, nullptr};
    return with_stream_scratch((size_t)sp * n * SD_MAX_K * sizeof(float), st, [&](char* base) -> int {
        a.part = reinterpret_cast<float*>(base);
        if (pick_const<16, 32, 64, 128>(what, fid_dp(D), [&](auto dp) {
                return launch("sd_knn_kernel", sd_knn_kernel<decltype(dp)::value>, grid, dim3(SD_THREADS), 0, st, a);
            })) return -1;
        return launch("sd_knn_merge_kernel", sd_knn_merge_kernel, dim3((unsigned)((n + SD_THREADS - 1) / SD_THREADS)), dim3(SD_THREADS), 0, st, a);
    });
}

extern "C" int vae_fidelity_balls(const float* q, int64_t m, const float* r, int64_t n, int D, const float* radii2, int exclude_same_index,
                                  int splits, int32_t* counts, int32_t* nearest, float* nearest_d2, vae_stream_t stream) {
    const char* what = "vae_fidelity_balls";
    if (!q || !r || !nearest || !nearest_d2) return vae_set_error(what, "null pointer (q, r, nearest, nearest_d2)");
    if (const char* why = fid_shape_refusal(D, m, n, splits)) return vae_set_error(what, why);
    if (counts && !radii2) return vae_set_error(what, "counts needs radii2");
    if (const char* why = fid_partials_refusal(m, splits)) return vae_set_error(what, why);
    if (fid_misaligned(q, 4) || fid_misaligned(r, 4) || fid_misaligned(radii2, 4) || fid_misaligned(counts, 4) || fid_misaligned(nearest, 4) ||
        fid_misaligned(nearest_d2, 4))
        return vae_set_error(what, "every pointer must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int sp = fid_splits(splits, m, n, D);
    const dim3 grid((unsigned)fid_qblocks(m, D), (unsigned)sp);
    SdBallArgs a{q, (long)m, r, (long)n, D, counts ? radii2 : nullptr, exclude_same_index != 0, sp, counts, nearest, nearest_d2, nullptr, nullptr, nullptr};
    auto first = [&](auto dp) { return launch("sd_balls_kernel", sd_balls_kernel<decltype(dp)::value>, grid, dim3(SD_THREADS), 0, st, a); };
    if (sp == 1) return pick_const<16, 32, 64, 128>(what, fid_dp(D), first);
    const size_t each = up256((size_t)sp * m * 4);
    return with_stream_scratch(3 * each, st, [&](char* base) -> int {
        a.part_counts = reinterpret_cast<int*>(base);
        a.part_nearest = reinterpret_cast<int*>(base + each);
        a.part_d2 = reinterpret_cast<float*>(base + 2 * each);
        if (pick_const<16, 32, 64, 128>(what, fid_dp(D), first)) return -1;
        return launch("sd_balls_merge_kernel", sd_balls_merge_kernel, dim3((unsigned)((m + SD_THREADS - 1) / SD_THREADS)), dim3(SD_THREADS), 0, st, a);
    });
}

extern "C" int vae_fidelity_kernel_sums(const float* a_, int64_t n, const float* b, int64_t m, int D, const double* gammas, int G,
                                        int exclude_same_index, int splits, double* sums, vae_stream_t stream) {
    const char* what = "vae_fidelity_kernel_sums";
    if (!a_ || !b || !sums) return vae_set_error(what, "null pointer (a, b, sums)");
    if (const char* why = fid_shape_refusal(D, n, m, splits)) return vae_set_error(what, why);
    if (G < 0 || G > SD_MAX_G) return vae_set_error(what, "G must be in 0..8");
    if (G > 0 && !gammas) return vae_set_error(what, "null gammas with G > 0");
    if (const char* why = fid_partials_refusal(n, splits)) return vae_set_error(what, why);
    if (fid_misaligned(a_, 4) || fid_misaligned(b, 4) || fid_misaligned(gammas, 8) || fid_misaligned(sums, 8))
        return vae_set_error(what, "a and b must be 4-byte, gammas and sums 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int sp = fid_splits(splits, n, m, D);
    const dim3 grid((unsigned)fid_qblocks(n, D), (unsigned)sp);
    const long slots = (long)grid.x * sp;
    SdSumArgs a{a_, (long)n, b, (long)m, D, gammas, G, exclude_same_index != 0, sp, nullptr, sums};
    return with_stream_scratch((size_t)slots * (SD_MAX_G + 1) * sizeof(double), st, [&](char* base) -> int {
        a.part = reinterpret_cast<double*>(base);
        if (pick_const<16, 32, 64, 128>(what, fid_dp(D), [&](auto dp) {
                return launch("sd_sums_kernel", sd_sums_kernel<decltype(dp)::value>, grid, dim3(SD_THREADS), 0, st, a);
            })) return -1;
        return launch("sd_sums_merge_kernel", sd_sums_merge_kernel, dim3((unsigned)(G + 1)), dim3(SD_THREADS), 0, st, a, slots);
    });
}
