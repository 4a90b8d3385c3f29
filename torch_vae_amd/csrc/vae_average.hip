// The weight averaging of the C ABI (include/vae_average.h; kernels in weight_average.cuh).  Context-free, like vae_denoise.hip: no
// work space, nothing read back and nothing waits for the device.  An update is two launches (the streaming kernel, the state's
// commit), the exchange and the state's initialisation one each.
#include "vae_ctx.h"
#include "../../include/vae_average.h"
#include "weight_average.cuh"

static_assert(WA_EMA == VAE_AVG_EMA && WA_EQUAL == VAE_AVG_EQUAL, "weight_average.cuh and include/vae_average.h disagree on a kind");
static_assert(sizeof(AvgState) == VAE_AVG_STATE_BYTES, "weight_average.cuh and include/vae_average.h disagree on the state");

namespace {
const int64_t kMaxFloats = (int64_t)1 << 40;
bool wa_misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1); }
bool wa_overlap(const void* p, int64_t np, const void* q, int64_t nq) {
    if (np <= 0 || nq <= 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)nq * 4 && b < a + (uintptr_t)np * 4;
}
// two (x, y, n) pairs, as both streaming entry points take them; 0 when they are fine.  A pair with n == 0 is absent.
int wa_check_pairs(const char* what, const char* names, const void* x0, const void* y0, int64_t n0, const void* x1, const void* y1, int64_t n1) {
    static thread_local char msg[160];
    if (n0 < 0 || n1 < 0) return vae_set_error(what, "n must be >= 0");
    if (n0 > kMaxFloats || n1 > kMaxFloats) return vae_set_error(what, "n must stay within 2^40");
    if ((n0 > 0 && (!x0 || !y0)) || (n1 > 0 && (!x1 || !y1))) { snprintf(msg, sizeof msg, "null pointer (%s)", names); return vae_set_error(what, msg); }
    const void* p[4] = {x0, y0, x1, y1};
    const int64_t n[4] = {n0, n0, n1, n1};
    for (int i = 0; i < 4; ++i)
        if (n[i] > 0 && wa_misaligned(p[i], 16)) { snprintf(msg, sizeof msg, "%s must be 16-byte aligned", names); return vae_set_error(what, msg); }
    return 0;
}
unsigned wa_blocks(int64_t n0, int64_t n1) {
    const int64_t nv = std::max(n0, n1) >> 2;
    return (unsigned)std::min<int64_t>(std::max<int64_t>((nv + WA_THREADS - 1) / WA_THREADS, 1), WA_MAX_BLOCKS);
}
}  // namespace

extern "C" int vae_average_update(float* avg0, const float* src0, int64_t n0, float src_scale0, float* avg1, const float* src1, int64_t n1,
                                  float src_scale1, int kind, double decay, double warmup, const int64_t* opt_step, void* state,
                                  vae_stream_t stream) {
    const char* what = "vae_average_update";
    if (!state) return vae_set_error(what, "null pointer (state)");
    if (wa_check_pairs(what, "avg, src", avg0, src0, n0, avg1, src1, n1)) return -1;
    if (wa_misaligned(state, 16) || wa_misaligned(opt_step, 8)) return vae_set_error(what, "state must be 16-byte, opt_step 8-byte aligned");
    if (kind != VAE_AVG_EMA && kind != VAE_AVG_EQUAL) return vae_set_error(what, "kind must be VAE_AVG_EMA or VAE_AVG_EQUAL");
    if (!(decay >= 0.0 && decay <= 1.0)) return vae_set_error(what, "decay must lie in [0, 1]");   // (a NaN fails both comparisons)
    if (!(warmup >= 0.0) || !std::isfinite(warmup)) return vae_set_error(what, "warmup must be finite and >= 0");
    if (!std::isfinite(src_scale0) || !std::isfinite(src_scale1)) return vae_set_error(what, "src_scale must be finite");
    if (wa_overlap(avg0, n0, src0, n0) || wa_overlap(avg0, n0, src1, n1) || wa_overlap(avg1, n1, src0, n0) || wa_overlap(avg1, n1, src1, n1) ||
        wa_overlap(avg0, n0, avg1, n1))
        return vae_set_error(what, "avg must not overlap src or the other avg");
    if (wa_overlap(state, VAE_AVG_STATE_BYTES / 4, avg0, n0) || wa_overlap(state, VAE_AVG_STATE_BYTES / 4, avg1, n1))
        return vae_set_error(what, "avg must not overlap the state");
    if (n0 == 0 && n1 == 0) return 0;
    AvgArgs a{{{avg0, src0, (long)n0, src_scale0}, {avg1, src1, (long)n1, src_scale1}}, kind, decay, warmup,
              reinterpret_cast<const long long*>(opt_step), static_cast<const AvgState*>(state)};
    if (launch("average_update_kernel", average_update_kernel, dim3(wa_blocks(n0, n1)), dim3(WA_THREADS), 0, (hipStream_t)stream, a)) return -1;
    return launch("average_commit_kernel", average_commit_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kind, decay, warmup,
                  reinterpret_cast<const long long*>(opt_step), static_cast<AvgState*>(state));
}

extern "C" int vae_average_swap(float* a0, float* b0, int64_t n0, float* a1, float* b1, int64_t n1, vae_stream_t stream) {
    const char* what = "vae_average_swap";
    if (wa_check_pairs(what, "a, b", a0, b0, n0, a1, b1, n1)) return -1;
    if (wa_overlap(a0, n0, b0, n0) || wa_overlap(a0, n0, a1, n1) || wa_overlap(a0, n0, b1, n1) || wa_overlap(b0, n0, a1, n1) ||
        wa_overlap(b0, n0, b1, n1) || wa_overlap(a1, n1, b1, n1))
        return vae_set_error(what, "the buffers must not overlap");
    if (n0 == 0 && n1 == 0) return 0;
    SwapArgs s{{a0, a1}, {b0, b1}, {(long)n0, (long)n1}};
    return launch("average_swap_kernel", average_swap_kernel, dim3(wa_blocks(n0, n1)), dim3(WA_THREADS), 0, (hipStream_t)stream, s);
}

extern "C" int vae_average_state_init(void* state, const int64_t* opt_step, int64_t n_averaged, vae_stream_t stream) {
    const char* what = "vae_average_state_init";
    if (!state) return vae_set_error(what, "null pointer (state)");
    if (wa_misaligned(state, 16) || wa_misaligned(opt_step, 8)) return vae_set_error(what, "state must be 16-byte, opt_step 8-byte aligned");
    if (n_averaged < 0) return vae_set_error(what, "n_averaged must be >= 0");
    return launch("average_state_init_kernel", average_state_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<AvgState*>(state),
                  reinterpret_cast<const long long*>(opt_step), (long long)n_averaged);
}
