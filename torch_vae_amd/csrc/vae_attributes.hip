// The attribute-regularised latents of the C ABI (include/vae_attributes.h; kernels in roll_attributes.cuh).  Context-free, like
// vae_util.hip; work space comes from with_stream_scratch, nothing is read back and nothing waits for the device.
#include "vae_ctx.h"
#include "../../include/vae_attributes.h"
#include "roll_attributes.cuh"

static_assert(RA_COUNTERS == VAE_ATTR_COUNTERS && RA_ATTRS == VAE_ATTR_COUNT && RA_MAX_PAIRS == VAE_ATTR_MAX_PAIRS &&
              RA_MAX_B == VAE_ATTR_MAX_BATCH && RA_MAX_L == VAE_ATTR_MAX_DIM && RA_MAX_ROWS == VAE_ATTR_MAX_ROWS &&
              RA_MAX_CELLS == VAE_ATTR_MAX_CELLS && RA_MAX_POINTS == VAE_ATTR_MAX_POINTS,
              "roll_attributes.cuh and include/vae_attributes.h disagree on a limit");
static_assert(VAE_ATTR_CELLS == 0 && VAE_ATTR_NOTES == 1 && VAE_ATTR_PITCH_RANGE == 2 && VAE_ATTR_MEAN_PITCH == 3 && VAE_ATTR_POLYPHONY == 4 &&
              VAE_ATTR_ONSET_STEPS == 5 && VAE_ATTR_USED_PITCHES == 6, "ra_attr_value switches on these numbers");

namespace {
bool attr_misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1); }
}  // namespace

extern "C" int vae_attr_roll_counters(const float* rolls, int64_t n, int h, int w, float threshold, int32_t* counters, vae_stream_t stream) {
    const char* what = "vae_attr_roll_counters";
    if (!rolls || !counters) return vae_set_error(what, "null pointer (rolls, counters)");
    if (n < 0) return vae_set_error(what, "n must be >= 0");
    if (h < 1 || h > RA_MAX_ROWS) return vae_set_error(what, "h must be in 1..1024");
    if (w < 1) return vae_set_error(what, "w must be >= 1");
    if ((int64_t)h * w > RA_MAX_CELLS) return vae_set_error(what, "a roll (h * w cells) must stay within 2^20");
    if (n > ((int64_t)1 << 46) / ((int64_t)h * w)) return vae_set_error(what, "n * h * w must stay within 2^46");
    if (attr_misaligned(rolls, 4) || attr_misaligned(counters, 4)) return vae_set_error(what, "rolls and counters must be 4-byte aligned");
    if (n == 0) return 0;
    RaCounterArgs a{rolls, (long)n, h, w, threshold, counters};
    const unsigned blocks = (unsigned)std::min<int64_t>(n, RA_MAX_BLOCKS);
    return pick_const<1, 2, 4>(what, w <= 64 ? 1 : w <= 128 ? 2 : 4, [&](auto k) {
        return launch("attr_roll_counters_kernel", attr_roll_counters_kernel<decltype(k)::value>, dim3(blocks), dim3(64 * RA_WAVES), 0, (hipStream_t)stream, a);
    });
}

extern "C" int vae_attr_regularizer(const float* z, int ldz, int L, const int32_t* counters, int B, int npairs, const int32_t* attr,
                                    const int32_t* dim, float delta, float weight, double* loss, float* g_z, vae_stream_t stream) {
    const char* what = "vae_attr_regularizer";
    if (!z || !counters || !loss || !attr || !dim) return vae_set_error(what, "null pointer (z, counters, loss, attr, dim)");
    if (B < 1 || B > RA_MAX_B) return vae_set_error(what, "B must be in 1..4096");
    if (L < 1 || L > RA_MAX_L) return vae_set_error(what, "L must be in 1..4096");
    if (ldz < L) return vae_set_error(what, "ldz must be >= L");
    if (npairs < 1 || npairs > RA_MAX_PAIRS) return vae_set_error(what, "npairs must be in 1..8");
    RaRegArgs a{};
    for (int k = 0; k < npairs; ++k) {
        if (attr[k] < 0 || attr[k] >= RA_ATTRS) return vae_set_error(what, "unknown attribute (0..6)");
        if (dim[k] < 0 || dim[k] >= L) return vae_set_error(what, "dim must be in 0..L-1");
        for (int q = 0; q < k; ++q)
            if (dim[q] == dim[k]) return vae_set_error(what, "a dim is named twice");
        a.attr[k] = attr[k]; a.dim[k] = dim[k];
    }
    if (!std::isfinite(delta) || !std::isfinite(weight)) return vae_set_error(what, "delta and weight must be finite");
    if (!(delta > 0.f)) return vae_set_error(what, "delta must be > 0");
    if (attr_misaligned(z, 4) || attr_misaligned(counters, 4) || attr_misaligned(g_z, 4) || attr_misaligned(loss, 8))
        return vae_set_error(what, "z, counters and g_z must be 4-byte, loss 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    a.z = z; a.ldz = ldz; a.L = L; a.counters = counters; a.B = B; a.npairs = npairs; a.delta = delta; a.gz = g_z;
    a.gscale = (double)weight * 2.0 * (double)delta / ((double)B * (double)B);
    const int rows = 4 * RA_REG_ROWS;
    return with_stream_scratch((size_t)npairs * B * sizeof(double), st, [&](char* base) -> int {
        a.rowloss = reinterpret_cast<double*>(base);
        if (launch("attr_reg_rows_kernel", attr_reg_rows_kernel, dim3((unsigned)((B + rows - 1) / rows), (unsigned)npairs), dim3(256), 0, st, a)) return -1;
        return launch("attr_reg_final_kernel", attr_reg_final_kernel, dim3(1), dim3(256), 0, st, (const double*)a.rowloss, B, npairs, loss);
    });
}

extern "C" int vae_attr_concordance(const float* z, int ldz, int L, const int32_t* counters, int64_t N, int nattr, const int32_t* attr,
                                    int64_t* S, int64_t* ties_z, int64_t* ties_a, vae_stream_t stream) {
    const char* what = "vae_attr_concordance";
    if (!z || !counters || !attr || !S || !ties_z || !ties_a) return vae_set_error(what, "null pointer (z, counters, attr, S, ties_z, ties_a)");
    if (N < 0 || N > RA_MAX_POINTS) return vae_set_error(what, "N must be in 0..65536");
    if (L < 1 || L > RA_MAX_L) return vae_set_error(what, "L must be in 1..4096");
    if (ldz < L) return vae_set_error(what, "ldz must be >= L");
    if (nattr < 1 || nattr > RA_ATTRS) return vae_set_error(what, "nattr must be in 1..7");
    RaConcordArgs a{};
    for (int k = 0; k < nattr; ++k) {
        if (attr[k] < 0 || attr[k] >= RA_ATTRS) return vae_set_error(what, "unknown attribute (0..6)");
        a.attr[k] = attr[k];
    }
    if (attr_misaligned(z, 4) || attr_misaligned(counters, 4) || attr_misaligned(S, 8) || attr_misaligned(ties_z, 8) || attr_misaligned(ties_a, 8))
        return vae_set_error(what, "z and counters must be 4-byte, S, ties_z and ties_a 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    a.z = z; a.ldz = ldz; a.L = L; a.counters = counters; a.N = (long)N; a.nattr = nattr;
    a.S = reinterpret_cast<long long*>(S); a.ties_z = reinterpret_cast<long long*>(ties_z); a.ties_a = reinterpret_cast<long long*>(ties_a);
    const long outputs = (long)nattr * L + L + nattr;
    const dim3 mgrid((unsigned)((outputs + RA_THREADS - 1) / RA_THREADS));
    if (N < 2) {
        a.splits = 1;
        return launch("attr_concord_merge_kernel", attr_concord_merge_kernel, mgrid, dim3(RA_THREADS), 0, st, a, 0L, 0LL);
    }
    const long qb = (long)((N + RA_THREADS - 1) / RA_THREADS), chunks = (L + RA_DP - 1) / RA_DP, tiles = (long)((N + RA_JT - 1) / RA_JT);
    // enough partner ranges that about 1024 workgroups exist, none shorter than one tile
    a.splits = (int)std::max<long>(1, std::min<long>(std::min<long>((1024 + qb * chunks - 1) / (qb * chunks), tiles), RA_MAX_SPLITS));
    const long slots = qb * a.splits;
    const long long n0 = (long long)N * (N - 1) / 2;
    return with_stream_scratch((size_t)chunks * slots * RA_COLS * sizeof(int), st, [&](char* base) -> int {
        a.part = reinterpret_cast<int*>(base);
        if (launch("attr_concord_kernel", attr_concord_kernel, dim3((unsigned)qb, (unsigned)a.splits, (unsigned)chunks), dim3(RA_THREADS), 0, st, a)) return -1;
        return launch("attr_concord_merge_kernel", attr_concord_merge_kernel, mgrid, dim3(RA_THREADS), 0, st, a, slots, n0);
    });
}
