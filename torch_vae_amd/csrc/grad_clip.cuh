// Gradient-norm clipping and non-finite step skipping for AdamW (vae_grad_norm, vae_adamw_step_clipped,
// vae_train_step_fused_clipped; vae_api.hip).  Three launches on the caller's stream, no host synchronisation:
//   grad_sumsq_kernel    grid (GCLIP_BLOCKS, ngroups): one f64 partial of sum (g * grad_scale)^2 per workgroup
//   grad_clip_finalize   one workgroup: the partials in a fixed order -> norm, clip coefficient, apply flag, the device
//                        step counter and the bias corrections of that step -> GradClipRecord
//   adamw_clipped_kernel adamw_kernel's update with the record's coefficient and bias corrections (nothing when !apply)
// The grid does not depend on the device and no float atomics are used: the norm is the same bits on every run and rank.
#pragma once
#include "edge_kernels.cuh"

constexpr int GCLIP_BLOCKS = 256;                          // partials per group
constexpr size_t GCLIP_RECORD_OFF = 2 * GCLIP_BLOCKS * 8;  // byte offset of the record in the caller's scratch buffer

// What the finalize kernel leaves for the update (in the caller's scratch, behind the partials).
struct GradClipRecord {
    int apply;                 // finite || !skip_nonfinite
    float coef;                // min(1, max_norm / (norm + 1e-6)) formed in f64, rounded once; 1 without clipping
    float step_size[2];        // lr / (1 - beta1^t) per group
    float inv_sqrt_bc2;        // 1 / sqrt(1 - beta2^t)
};

// sum over a 256-thread workgroup (waves of 64: shuffle, then the four wave sums through LDS, in wave order)
__device__ __forceinline__ double gclip_block_sum(double s) {
    __shared__ double red[4];
    s = wave_sum(s);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

struct GradSumsqArgs {
    const float* g; long off[2], n[2]; float grad_scale;
    double* partial;           // [ngroups][GCLIP_BLOCKS]
};
// 256 threads; f32x4 loads over the range (ranges start on 256-byte boundaries, a tail finishes in scalars, as adamw_kernel)
static __global__ void __launch_bounds__(256) grad_sumsq_kernel(GradSumsqArgs a) {
    const long off = a.off[blockIdx.y], n = a.n[blockIdx.y];
    const long n4 = (off & 3) == 0 ? n >> 2 : 0;
    const long stride = (long)gridDim.x * blockDim.x;
    double s = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.g + off + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const double x = (double)(g[e] * a.grad_scale); s += x * x; }
    }
    for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double x = (double)(a.g[off + i] * a.grad_scale);
        s += x * x;
    }
    s = gclip_block_sum(s);
    if (threadIdx.x == 0) a.partial[blockIdx.y * GCLIP_BLOCKS + blockIdx.x] = s;
}

struct GradClipArgs {
    const double* partial; int ngrp;
    double max_norm;           // <= 0: no clipping
    int skip;                  // skip_nonfinite
    long long* step;           // device AdamW step count (null: the norm alone, vae_grad_norm)
    long long* skipped;
    double* norm_out;
    double lr[2], beta1[2], beta2;
    GradClipRecord* rec;
};
// One workgroup of 256 threads.  Thread t adds partials t, t + 256, ... in that order, then gclip_block_sum.
static __global__ void __launch_bounds__(256) grad_clip_finalize_kernel(GradClipArgs a) {
    double s = 0.0;
    for (int i = threadIdx.x; i < a.ngrp * GCLIP_BLOCKS; i += 256) s += a.partial[i];
    s = gclip_block_sum(s);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(s);
    *a.norm_out = norm;
    if (!a.step) return;
    const bool finite = isfinite(norm);
    const bool apply = finite || !a.skip;
    double coef = 1.0;
    if (a.max_norm > 0.0) {
        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1); a NaN coefficient (NaN norm) passes through
        const double c = a.max_norm / (norm + 1e-6);
        coef = (c < 1.0 || c != c) ? c : 1.0;
    }
    const long long t = *a.step + (apply ? 1 : 0);
    *a.step = t;
    if (!apply) *a.skipped = *a.skipped + 1;
    GradClipRecord r;
    r.apply = apply ? 1 : 0;
    r.coef = (float)coef;
    r.step_size[0] = r.step_size[1] = 0.f;
    r.inv_sqrt_bc2 = 0.f;
    if (apply) {
        // the host expressions of vae_adamw_step, in double, rounded once (torch: bias corrections with the current beta1)
        for (int i = 0; i < a.ngrp; ++i) r.step_size[i] = (float)(a.lr[i] / (1.0 - pow(a.beta1[i], (double)t)));
        r.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(a.beta2, (double)t)));
    }
    *a.rec = r;
}

// adamw_kernel with the step's bias corrections and clip coefficient from the record; the whole grid returns when !apply.
static __global__ void adamw_clipped_kernel(AdamArgs a, const GradClipRecord* rec) {
    if (!rec->apply) return;
    AdamGroup gr = a.grp[blockIdx.y];
    gr.step_size = rec->step_size[blockIdx.y];
    gr.inv_sqrt_bc2 = rec->inv_sqrt_bc2;
    adamw_range<true>(a, gr, rec->coef);
}
