// The latent Gaussian mixture of the C ABI (include/vae_mixture.h; kernels in latent_mixture.cuh): factor, log_prob (the E-step),
// M-step, sample, and the EM loop that enqueues `iters` iterations of the first three from one call.  Context-free, like
// vae_util.hip; work space comes from with_stream_scratch, nothing is read back and nothing waits for the device.
#include "vae_ctx.h"
#include "../../include/vae_mixture.h"
#include "latent_mixture.cuh"

namespace {

const char* mix_shape_refusal(int K, int L, int kind) {
    if (kind != MIX_FULL && kind != MIX_DIAG) return "kind must be 0 (full) or 1 (diag)";
    if (K < 1 || K > MIX_MAX_K) return "components must be in 1..64";
    if (kind == MIX_FULL && (L < 1 || L > MIX_MAX_L_FULL)) return "latent_dim must be in 1..128 for full covariances";
    if (kind == MIX_DIAG && (L < 1 || L > MIX_MAX_L_DIAG)) return "latent_dim must be in 1..4096 for diagonal covariances";
    return nullptr;
}
const char* mix_points_refusal(int64_t n, int K) {
    if (n < K) return "n must be >= components";
    if (n > (int64_t)1 << 30) return "n must be <= 2^30";
    return nullptr;
}
bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1); }

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

int enqueue_factor(const double* cov, int K, int L, int kind, double* chol, double* winv, float* winv32, double* logdet, int* status,
                   int sticky, hipStream_t st) {
    if (kind == MIX_DIAG)
        return launch("mix_factor_diag_kernel", mix_factor_diag_kernel, dim3(K), dim3(256), 0, st, cov, L, chol, winv, winv32, logdet, status, sticky);
    const size_t lds = (size_t)L * (L + 1) * sizeof(double);   // two packed triangles
    return launch("mix_factor_kernel", mix_factor_kernel, dim3(K), dim3(256), lds, st, cov, L, chol, winv, winv32, logdet, status, sticky);
}

// E-step: block_sum holds estep_blocks(n) doubles of work space
long estep_blocks(int64_t n) { return (long)((n + MIX_PTS - 1) / MIX_PTS); }
int enqueue_estep(const float* x, int64_t n, int L, int K, int kind, const double* pi, const double* m, const float* w32,
                  const double* logdet, double* log_prob, float* log_resp, double* mean_ll, double* block_sum, hipStream_t st) {
    MixEArgs a{x, (long)n, L, K, pi, m, w32, logdet, log_prob, log_resp, block_sum};
    const long nb = estep_blocks(n);
    if (kind == MIX_FULL) { if (launch("mix_estep_full_kernel", mix_estep_full_kernel, dim3((unsigned)nb), dim3(256), 0, st, a)) return -1; }
    else if (launch("mix_estep_diag_kernel", mix_estep_diag_kernel, dim3((unsigned)nb), dim3(256), 0, st, a)) return -1;
    return launch("mix_mean_kernel", mix_mean_kernel, dim3(1), dim3(256), 0, st, (const double*)block_sum, nb, (double)n, mean_ll);
}

// M-step.  The point range is cut into `splits` runs of whole 64-point chunks; the count depends on (n, K, L, kind) only: enough
// workgroups for the card, at most 64, and the SYRK's partials ([splits, K, L, L] f64) kept within 32 MiB.
struct MstepPlan { int splits; long per; size_t off_n, off_v, off_nk, off_s, bytes; };
MstepPlan mstep_plan(int64_t n, int L, int K, int kind) {
    MstepPlan p;
    const long chunks = (long)((n + MIX_ACC_POINTS - 1) / MIX_ACC_POINTS);
    long s = std::min<long>(64, std::max<long>(1, 1024 / K));
    if (kind == MIX_FULL) s = std::min<long>(s, std::max<long>(1, ((long)32 << 20) / ((long)K * L * L * 8)));
    s = std::max<long>(1, std::min(s, chunks));
    p.per = (chunks + s - 1) / s * MIX_ACC_POINTS;
    p.splits = (int)((n + p.per - 1) / p.per);
    size_t o = 0;
    p.off_n = o; o += up256((size_t)p.splits * K * 8);
    p.off_v = o; o += up256((size_t)p.splits * K * L * 8);
    p.off_nk = o; o += up256((size_t)K * 8);
    p.off_s = o; o += kind == MIX_FULL ? up256((size_t)p.splits * K * L * L * 8) : 0;
    p.bytes = o;
    return p;
}
int enqueue_mstep(const float* log_resp, const float* x, int64_t n, int L, int K, int kind, double reg, double* pi, double* m, double* cov,
                  const MstepPlan& p, char* ws, hipStream_t st) {
    double* part_n = reinterpret_cast<double*>(ws + p.off_n);
    double* part_v = reinterpret_cast<double*>(ws + p.off_v);
    double* Nk = reinterpret_cast<double*>(ws + p.off_nk);
    double* part_s = reinterpret_cast<double*>(ws + p.off_s);
    const dim3 g1(p.splits, K, (L + 127) / 128);
    if (launch("mix_msums_kernel<1>", mix_msums_kernel<1>, g1, dim3(128), 0, st, log_resp, x, (long)n, L, K, p.per, (const double*)nullptr, part_n, part_v)) return -1;
    if (launch("mix_mmeans_kernel", mix_mmeans_kernel, dim3(K), dim3(256), 0, st, (const double*)part_n, (const double*)part_v, p.splits, K, L, (double)n, Nk, pi, m)) return -1;
    if (kind == MIX_DIAG) {
        if (launch("mix_msums_kernel<2>", mix_msums_kernel<2>, g1, dim3(128), 0, st, log_resp, x, (long)n, L, K, p.per, (const double*)m, part_n, part_v)) return -1;
        return launch("mix_mvar_kernel", mix_mvar_kernel, dim3(K), dim3(256), 0, st, (const double*)part_v, p.splits, K, L, (const double*)Nk, reg, cov);
    }
    const int rc = pick_const<1, 2, 3, 4, 5, 6, 7, 8>("mix_msyrk_kernel", (L + 15) / 16, [&](auto NT) {
        return launch("mix_msyrk_kernel", mix_msyrk_kernel<decltype(NT)::value>, dim3(p.splits, K), dim3(256), 0, st, log_resp, x, (long)n, L, K, p.per,
                      (const double*)m, part_s);
    });
    if (rc) return rc;
    return launch("mix_mcov_kernel", mix_mcov_kernel, dim3((L * L + 255) / 256, K), dim3(256), 0, st, (const double*)part_s, p.splits, K, L, (const double*)Nk, reg, cov);
}

}  // namespace

extern "C" int vae_mixture_factor(const double* cov, int K, int L, int kind, double* chol, double* winv, float* winv32, double* logdet,
                                  int* status, vae_stream_t stream) {
    const char* what = "vae_mixture_factor";
    if (!cov || !chol || !winv || !winv32 || !logdet || !status) return vae_set_error(what, "null pointer (covariances, chol, winv, winv32, logdet, status)");
    if (const char* why = mix_shape_refusal(K, L, kind)) return vae_set_error(what, why);
    if (misaligned(cov, 8) || misaligned(chol, 8) || misaligned(winv, 8) || misaligned(logdet, 8) || misaligned(winv32, 4) || misaligned(status, 4))
        return vae_set_error(what, "f64 pointers must be 8-byte, winv32 and status 4-byte aligned");
    return enqueue_factor(cov, K, L, kind, chol, winv, winv32, logdet, status, 0, (hipStream_t)stream);
}

extern "C" int vae_mixture_log_prob(const float* x, int64_t n, int L, int K, int kind, const double* weights, const double* means,
                                    const float* winv32, const double* logdet, double* log_prob, float* log_resp, double* mean_log_prob,
                                    vae_stream_t stream) {
    const char* what = "vae_mixture_log_prob";
    if (!x || !weights || !means || !winv32 || !logdet || !log_prob || !mean_log_prob)
        return vae_set_error(what, "null pointer (x, weights, means, winv32, logdet, log_prob, mean_log_prob)");
    if (const char* why = mix_shape_refusal(K, L, kind)) return vae_set_error(what, why);
    if (const char* why = mix_points_refusal(n, K)) return vae_set_error(what, why);
    if (misaligned(weights, 8) || misaligned(means, 8) || misaligned(logdet, 8) || misaligned(log_prob, 8) || misaligned(mean_log_prob, 8) ||
        misaligned(x, 4) || misaligned(winv32, 4) || misaligned(log_resp, 4))
        return vae_set_error(what, "f64 pointers must be 8-byte, f32 pointers 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    return with_stream_scratch((size_t)estep_blocks(n) * 8, st, [&](char* base) -> int {
        return enqueue_estep(x, n, L, K, kind, weights, means, winv32, logdet, log_prob, log_resp, mean_log_prob, reinterpret_cast<double*>(base), st);
    });
}

extern "C" int vae_mixture_mstep(const float* log_resp, const float* x, int64_t n, int L, int K, int kind, double reg_covar, double* weights,
                                 double* means, double* cov, vae_stream_t stream) {
    const char* what = "vae_mixture_mstep";
    if (!log_resp || !x || !weights || !means || !cov) return vae_set_error(what, "null pointer (log_resp, x, weights, means, covariances)");
    if (const char* why = mix_shape_refusal(K, L, kind)) return vae_set_error(what, why);
    if (const char* why = mix_points_refusal(n, K)) return vae_set_error(what, why);
    if (!std::isfinite(reg_covar) || reg_covar < 0.0) return vae_set_error(what, "reg_covar must be finite and >= 0");
    if (misaligned(weights, 8) || misaligned(means, 8) || misaligned(cov, 8) || misaligned(x, 4) || misaligned(log_resp, 4))
        return vae_set_error(what, "f64 pointers must be 8-byte, f32 pointers 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const MstepPlan p = mstep_plan(n, L, K, kind);
    return with_stream_scratch(p.bytes, st, [&](char* base) -> int {
        return enqueue_mstep(log_resp, x, n, L, K, kind, reg_covar, weights, means, cov, p, base, st);
    });
}

extern "C" int vae_mixture_sample(int64_t n, int L, int K, int kind, const double* weights, const double* means, const double* chol,
                                  double temperature, uint64_t seed, const double* u, const float* eps, float* z, int* component,
                                  vae_stream_t stream) {
    const char* what = "vae_mixture_sample";
    if (!weights || !means || !chol || !z || !component) return vae_set_error(what, "null pointer (weights, means, chol, z, component)");
    if (const char* why = mix_shape_refusal(K, L, kind)) return vae_set_error(what, why);
    if (n < 0 || n > (int64_t)1 << 30) return vae_set_error(what, "n must be in 0..2^30");
    if (!std::isfinite(temperature)) return vae_set_error(what, "temperature must be finite");
    if (misaligned(weights, 8) || misaligned(means, 8) || misaligned(chol, 8) || misaligned(u, 8) || misaligned(eps, 4) || misaligned(z, 4) ||
        misaligned(component, 4))
        return vae_set_error(what, "f64 pointers must be 8-byte, f32 and int32 pointers 4-byte aligned");
    if (n == 0) return 0;
    MixSArgs a{(long)n, L, K, kind, weights, means, chol, temperature, (unsigned long long)seed, u, eps, z, component};
    const long work = kind == MIX_FULL ? (long)((n + MIX_SDRAWS - 1) / MIX_SDRAWS) : (long)((n * L + 255) / 256);
    return launch("mix_sample_kernel", mix_sample_kernel, dim3((unsigned)std::min<long>(work, 8192)), dim3(256), 0, (hipStream_t)stream, a);
}

extern "C" int vae_mixture_em(const float* x, int64_t n, int L, int K, int kind, int iters, double reg_covar, double* weights, double* means,
                              double* cov, double* chol, double* winv, float* winv32, double* logdet, int* status, double* ll_history,
                              vae_stream_t stream) {
    const char* what = "vae_mixture_em";
    if (!x || !weights || !means || !cov || !chol || !winv || !winv32 || !logdet || !status || !ll_history)
        return vae_set_error(what, "null pointer (x, weights, means, covariances, chol, winv, winv32, logdet, status, ll_history)");
    if (const char* why = mix_shape_refusal(K, L, kind)) return vae_set_error(what, why);
    if (const char* why = mix_points_refusal(n, K)) return vae_set_error(what, why);
    if (iters < 1) return vae_set_error(what, "iters must be >= 1");
    if (!std::isfinite(reg_covar) || reg_covar < 0.0) return vae_set_error(what, "reg_covar must be finite and >= 0");
    if (misaligned(weights, 8) || misaligned(means, 8) || misaligned(cov, 8) || misaligned(chol, 8) || misaligned(winv, 8) || misaligned(logdet, 8) ||
        misaligned(ll_history, 8) || misaligned(x, 4) || misaligned(winv32, 4) || misaligned(status, 4))
        return vae_set_error(what, "f64 pointers must be 8-byte, f32 and int32 pointers 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const MstepPlan p = mstep_plan(n, L, K, kind);
    const size_t off_lr = up256(p.bytes), off_lp = off_lr + up256((size_t)n * K * 4), off_bs = off_lp + up256((size_t)n * 8);
    const size_t total = off_bs + up256((size_t)estep_blocks(n) * 8);
    return with_stream_scratch(total, st, [&](char* base) -> int {
        float* log_resp = reinterpret_cast<float*>(base + off_lr);
        double* log_prob = reinterpret_cast<double*>(base + off_lp);
        double* block_sum = reinterpret_cast<double*>(base + off_bs);
        HIP_CHECK_RET(hipMemsetAsync(status, 0, (size_t)K * sizeof(int), st));
        for (int it = 0; it < iters; ++it) {
            if (enqueue_factor(cov, K, L, kind, chol, winv, winv32, logdet, status, 1, st)) return -1;
            if (enqueue_estep(x, n, L, K, kind, weights, means, winv32, logdet, log_prob, log_resp, ll_history + it, block_sum, st)) return -1;
            if (enqueue_mstep(log_resp, x, n, L, K, kind, reg_covar, weights, means, cov, p, base, st)) return -1;
        }
        return enqueue_factor(cov, K, L, kind, chol, winv, winv32, logdet, status, 1, st);
    });
}
