// The corruption of the C ABI (include/vae_denoise.h; kernels in roll_corrupt.cuh).  Context-free, like vae_util.hip: one launch
// per call, no work space, nothing read back and nothing waits for the device.
#include "vae_ctx.h"
#include "../../include/vae_denoise.h"
#include "roll_corrupt.cuh"

static_assert(DN_STREAM_DROP == VAE_DENOISE_STREAM_DROP && DN_STREAM_SPAN == VAE_DENOISE_STREAM_SPAN && DN_STREAM_ADD == VAE_DENOISE_STREAM_ADD,
              "roll_corrupt.cuh and include/vae_denoise.h disagree on a stream");

namespace {
bool dn_misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1); }
bool dn_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}
// the arguments both entry points share; 0 when they are fine
int dn_check_span(const char* what, int64_t n, int w, int span_min, int span_max) {
    if (n < 0) return vae_set_error(what, "n must be >= 0");
    if (w < 8 || w > VAE_DENOISE_MAX_COLS || (w & 7)) return vae_set_error(what, "w must be a multiple of 8 in 8..2^20");
    if (span_min < 0 || span_min > span_max || span_max > w) return vae_set_error(what, "the span needs 0 <= span_min <= span_max <= w");
    return 0;
}
}  // namespace

extern "C" int vae_denoise_corrupt(const float* clean, float* out, uint8_t* hidden, int64_t n, int h, int w, float threshold, double p_drop,
                                   int span_min, int span_max, double p_add, float add_value, const int32_t* spans, uint64_t seed,
                                   uint64_t counter0, uint64_t counter_stride, vae_stream_t stream) {
    const char* what = "vae_denoise_corrupt";
    if (!clean || !out) return vae_set_error(what, "null pointer (clean, out)");
    if (dn_check_span(what, n, w, span_min, span_max)) return -1;
    if (h < 1 || h > VAE_DENOISE_MAX_ROWS) return vae_set_error(what, "h must be in 1..2^20");
    if (n > ((int64_t)1 << 46) / ((int64_t)h * w)) return vae_set_error(what, "n * h * w must stay within 2^46");
    if (!(p_drop >= 0.0 && p_drop <= 1.0) || !(p_add >= 0.0 && p_add <= 1.0)) return vae_set_error(what, "p_drop and p_add must lie in [0, 1]");   // (a NaN fails both comparisons)
    if (!std::isfinite(threshold) || !std::isfinite(add_value)) return vae_set_error(what, "threshold and add_value must be finite");
    if (dn_misaligned(clean, 16) || dn_misaligned(out, 16) || dn_misaligned(spans, 4)) return vae_set_error(what, "clean and out must be 16-byte, spans 4-byte aligned");
    const size_t cells = (size_t)n * h * w;
    if (dn_overlap(clean, cells * 4, out, cells * 4) || (hidden && (dn_overlap(hidden, cells / 8, out, cells * 4) || dn_overlap(hidden, cells / 8, clean, cells * 4))))
        return vae_set_error(what, "clean, out and hidden must not overlap");
    if (n == 0) return 0;
    const long rows = (long)n * h;
    CorruptArgs a{clean, out, hidden, rows, h, w, threshold, p_drop, span_min, span_max, p_add, add_value, spans,
                  (dn_u64)seed, (dn_u64)counter0, (dn_u64)counter_stride};
    const long per = DN_THREADS / 64;
    const unsigned blocks = (unsigned)std::min<long>((rows + per - 1) / per, DN_MAX_BLOCKS);
    return launch("denoise_corrupt_kernel", denoise_corrupt_kernel, dim3(blocks), dim3(DN_THREADS), 0, (hipStream_t)stream, a);
}

extern "C" int vae_denoise_params(int32_t* spans, int64_t n, int w, int span_min, int span_max, uint64_t seed, uint64_t counter0,
                                  uint64_t counter_stride, vae_stream_t stream) {
    const char* what = "vae_denoise_params";
    if (!spans) return vae_set_error(what, "null pointer (spans)");
    if (dn_check_span(what, n, w, span_min, span_max)) return -1;
    if (n > ((int64_t)1 << 40)) return vae_set_error(what, "n must stay within 2^40");
    if (dn_misaligned(spans, 4)) return vae_set_error(what, "spans must be 4-byte aligned");
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
    return launch("denoise_params_kernel", denoise_params_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<int*>(spans), (long)n, w,
                  span_min, span_max, (dn_u64)seed, (dn_u64)counter0, (dn_u64)counter_stride);
}
