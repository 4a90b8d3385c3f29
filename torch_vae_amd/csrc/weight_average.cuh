// Weight averaging beside the training step (include/vae_average.h: vae_average_update, vae_average_swap, vae_average_state_init):
// an EMA or an equal average of the flat parameter buffer and the BatchNorm buffer, both segments in ONE streaming launch, plus a
// single-thread launch behind it that commits the small device state.  Pure streaming: per element 4 bytes of src and 4 of avg
// read, 4 of avg written, with 16-byte loads and stores; a capped grid walks each segment in a stride loop.  No atomics, no LDS,
// nothing read back; every bit is a function of the arguments and of what the pointers hold.
//
// The gate and the weight are formed by EVERY workgroup from the same three words (seen_step, n_averaged, *opt_step), which nothing
// writes while the streaming kernel runs: the only writer is average_commit_kernel, one thread, behind it in stream order.  So the
// host passes nothing that changes from call to call, and a captured sequence replays correctly.
//
// Where it can go wrong, and what guards it (tests/test_average_gpu.py walks every one past its edge):
//   vector guard  i < n / 4 in the stride loop; 64-bit indices throughout
//   scalar tail   the last n % 4 floats of a segment, by the first lanes of workgroup 0, past the vector part and below n
//   alignment     avg and src 16-byte aligned (checked by the host): a float4 is whole or absent
//   rounding      torch.lerp's two branches with the fused multiply-add written out (fmaf) and the two roundings in front of it
//                 (src * scale, s - e) under `#pragma clang fp contract(off)`: the compiler would otherwise fuse them into
//                 fma(src, scale, -e), one rounding where the contract has two (__fmul_rn is a plain product to it).  The formula
//                 then does not depend on the build's contraction setting.  1.f - w is exact for 0.5 <= w <= 1 (Sterbenz)
//   first update  n_averaged == 0 copies and never reads avg: whatever avg held (NaNs included) is gone; with scale == 1 no arithmetic
//                 touches the value, so the bits of src arrive
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int WA_THREADS = 256;
constexpr int WA_MAX_BLOCKS = 2048;    // capped grid (8 workgroups per CU); the rest is a stride loop
constexpr int WA_EMA = 0, WA_EQUAL = 1;   // include/vae_average.h: VAE_AVG_*

struct AvgState { long long seen_step; long long n_averaged; double last_weight; long long reserved; };
struct AvgSeg { float* avg; const float* src; long n; float scale; };
struct AvgArgs { AvgSeg seg[2]; int kind; double decay, warmup; const long long* opt_step; const AvgState* state; };
struct SwapArgs { float* a[2]; float* b[2]; long n[2]; };

// the gate and the weight of the update that `st` and `opt_step` ask for (include/vae_average.h: GATE, WEIGHT)
struct AvgPlan { bool apply, copy; float w; long long step; };
__device__ __forceinline__ AvgPlan wa_plan(int kind, double decay, double warmup, const long long* opt_step, const AvgState* st) {
    AvgPlan p;
    const long long seen = st->seen_step, n = st->n_averaged;
    p.step = opt_step ? *opt_step : seen;
    p.apply = !opt_step || p.step != seen;
    p.copy = n == 0;
    double w = 1.0;
    if (!p.copy) {
        if (kind == WA_EQUAL) w = 1.0 / ((double)n + 1.0);
        else {
            double d = decay;
            if (warmup > 0.0) d = fmin(decay, (1.0 + (double)n) / (warmup + (double)n));
            w = 1.0 - d;
        }
    }
    p.w = (float)w;
    return p;
}

// MODE 0: copy; 1: |w| < 0.5; 2: otherwise.  nomw = -(1.f - w)
template <bool SCALED, int MODE>
__device__ __forceinline__ float wa_elem(float e, float v, float scale, float w, float nomw) {
#pragma clang fp contract(off)
    const float s = SCALED ? v * scale : v;
    if (MODE == 0) return s;
    const float d = s - e;
    return MODE == 1 ? fmaf(w, d, e) : fmaf(nomw, d, s);
}

template <bool SCALED, int MODE>
__device__ __forceinline__ void wa_segment(const AvgSeg& g, float w, float nomw) {
    const long nv = g.n >> 2;
    float4* __restrict__ a4 = reinterpret_cast<float4*>(g.avg);
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(g.src);
    const long stride = (long)gridDim.x * WA_THREADS;
    for (long i = blockIdx.x * (long)WA_THREADS + threadIdx.x; i < nv; i += stride) {
        const float4 v = s4[i];
        float4 e = v;
        if (MODE != 0) e = a4[i];
        e.x = wa_elem<SCALED, MODE>(e.x, v.x, g.scale, w, nomw);
        e.y = wa_elem<SCALED, MODE>(e.y, v.y, g.scale, w, nomw);
        e.z = wa_elem<SCALED, MODE>(e.z, v.z, g.scale, w, nomw);
        e.w = wa_elem<SCALED, MODE>(e.w, v.w, g.scale, w, nomw);
        a4[i] = e;
    }
    if (blockIdx.x == 0 && (long)threadIdx.x < (g.n & 3)) {
        const long i = (nv << 2) + threadIdx.x;
        const float v = g.src[i];
        g.avg[i] = wa_elem<SCALED, MODE>(MODE != 0 ? g.avg[i] : v, v, g.scale, w, nomw);
    }
}

template <bool SCALED>
__device__ __forceinline__ void wa_segment_mode(const AvgSeg& g, int mode, float w, float nomw) {
    if (mode == 0) wa_segment<SCALED, 0>(g, w, nomw);
    else if (mode == 1) wa_segment<SCALED, 1>(g, w, nomw);
    else wa_segment<SCALED, 2>(g, w, nomw);
}

__global__ __launch_bounds__(WA_THREADS) void average_update_kernel(AvgArgs a) {
    const AvgPlan p = wa_plan(a.kind, a.decay, a.warmup, a.opt_step, a.state);
    if (!p.apply) return;
    const float nomw = -(1.f - p.w);
    const int mode = p.copy ? 0 : (fabsf(p.w) < 0.5f ? 1 : 2);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (a.seg[k].n <= 0) continue;
        if (a.seg[k].scale == 1.f) wa_segment_mode<false>(a.seg[k], mode, p.w, nomw);
        else wa_segment_mode<true>(a.seg[k], mode, p.w, nomw);
    }
}

// the one writer of the state: a single thread, behind every reader in stream order
__global__ void average_commit_kernel(int kind, double decay, double warmup, const long long* opt_step, AvgState* st) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const AvgPlan p = wa_plan(kind, decay, warmup, opt_step, st);
    if (!p.apply) return;
    st->seen_step = p.step;
    st->n_averaged = st->n_averaged + 1;
    st->last_weight = (double)p.w;
}

__global__ void average_state_init_kernel(AvgState* st, const long long* opt_step, long long n_averaged) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    st->seen_step = opt_step ? *opt_step : -1;
    st->n_averaged = n_averaged;
    st->last_weight = 0.0;
    st->reserved = 0;
}

__global__ __launch_bounds__(WA_THREADS) void average_swap_kernel(SwapArgs s) {
    const long stride = (long)gridDim.x * WA_THREADS;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const long n = s.n[k];
        if (n <= 0) continue;
        const long nv = n >> 2;
        float4* __restrict__ a4 = reinterpret_cast<float4*>(s.a[k]);
        float4* __restrict__ b4 = reinterpret_cast<float4*>(s.b[k]);
        for (long i = blockIdx.x * (long)WA_THREADS + threadIdx.x; i < nv; i += stride) {
            const float4 x = a4[i], y = b4[i];
            a4[i] = y; b4[i] = x;
        }
        if (blockIdx.x == 0 && (long)threadIdx.x < (n & 3)) {
            const long i = (nv << 2) + threadIdx.x;
            const float x = s.a[k][i], y = s.b[k][i];
            s.a[k][i] = y; s.b[k][i] = x;
        }
    }
}
