// Device-resident pianoroll gather with fused augmentation (include/vae_step.h: vae_gather_rolls, vae_augment_params).
// One launch per batch: every lane writes 8 consecutive cells of one output row as two 16-byte stores, the lanes of a wave cover
// consecutive columns (then the next row: a roll of dst is contiguous), the source is read once per epoch and so with non-temporal loads.
// Pure streaming: B*h*w*4 bytes written, the source cells read, 8 bytes of index per roll.
//
// Where it can go wrong, and what guards it (tests/test_augment_gpu.py sweeps every one past its edge):
//   roll guard   (unsigned long)i < n_rolls, else the roll is zero and no source address is formed
//   row guard    0 <= y - dy < h (dy clamped to [-h, h] first)
//   column guard per source byte (bit planes) or per cell; c0 is clamped to [-w, src_w] first, so c0 + x cannot overflow
//   bit planes   output byte column j starts at source bit c0 + 8j = 8q + r with q the FLOOR quotient and 0 <= r < 8, also for
//                negative starts; the byte is funnelled out of source bytes q and q + 1, a byte outside [0, src_w/8) reads as 0
#pragma once
#include "edge_kernels.cuh"

constexpr int AUG_STREAM = 901;        // counter-generator stream of the augmentation draws
constexpr int AUG_THREADS = 256;       // lanes per workgroup
constexpr int AUG_MAX_BLOCKS = 2048;   // capped grid; the rest is stride loops (torch_vae_amd/_lib.py restates both)

// (dy, c0) of the sample with counter k: the formulas of vae_gather_rolls in include/vae_step.h.  A range of one value needs no
// draw ((int)(u * 1) is 0 for every u in [0, 1)), so the identity / centre-crop settings hash nothing.
__device__ __forceinline__ void augment_draw(unsigned long long k, unsigned long long seed, int P, int T, int slack, int crop_mode,
                                             int& dy, int& c0) {
    dy = P ? (int)(counter_uniform(2 * k, seed, AUG_STREAM) * (double)(2 * P + 1)) - P : 0;
    const int range = (crop_mode == 0 ? slack : 0) + 2 * T + 1;
    const int c = range > 1 ? (int)(counter_uniform(2 * k + 1, seed, AUG_STREAM) * (double)range) : 0;
    c0 = (crop_mode == 0 ? 0 : slack / 2) + c - T;
}

__global__ void augment_params_kernel(int* __restrict__ params, int batch, int slack, unsigned long long seed, unsigned long long counter0,
                                      unsigned long long stride, int P, int T, int crop_mode) {
    for (long b = blockIdx.x * (long)blockDim.x + threadIdx.x; b < batch; b += (long)gridDim.x * blockDim.x) {
        int dy, c0;
        augment_draw(counter0 + (unsigned long long)b * stride, seed, P, T, slack, crop_mode, dy, c0);
        params[2 * b] = dy; params[2 * b + 1] = c0;
    }
}

struct GatherArgs {
    const void* src; long n_rolls; int h, src_w;
    const long* index; long first;
    const int* params;
    unsigned long long seed, counter0, stride; int P, T, crop_mode;
    float scale; float* dst; int batch, w, lg_tx;
};

// KIND 0 bytes, 1 bit planes, 2 float32.  A workgroup is a tile of TX = 2^lg_tx lanes along a row (the smallest power of two that
// covers the w/8 work items of a row, at most 64) by AUG_THREADS / TX rows, so a lane finds its row y and its work item j (the 8
// cells dst[b,0,y,8j .. 8j+7]) with a shift and a mask; where w/8 is that power of two the lanes of a wave write consecutive
// memory across rows.  Grid: x walks the row tiles of one roll, y the samples, both with a stride loop under a capped grid.  The
// sample is the same for a whole workgroup, so everything per sample - index, draws, clamps, roll guard - is scalar code.
template <int KIND>
__global__ void gather_rolls_kernel(const GatherArgs a) {
    const unsigned wb = (unsigned)a.w >> 3, tx = threadIdx.x & ((1u << a.lg_tx) - 1), ty = threadIdx.x >> a.lg_tx;
    const unsigned TX = 1u << a.lg_tx, TY = AUG_THREADS >> a.lg_tx;
    const size_t row_bytes = KIND == 1 ? (size_t)(a.src_w >> 3) : (size_t)a.src_w * (KIND == 2 ? 4 : 1);
    for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const long i = a.index ? a.index[b] : (long)((unsigned long)a.first + (unsigned long)b);
        int dy, c0;
        if (a.params) { dy = a.params[2 * (size_t)b]; c0 = a.params[2 * (size_t)b + 1]; }
        else augment_draw(a.counter0 + (unsigned long long)b * a.stride, a.seed, a.P, a.T, a.src_w - a.w, a.crop_mode, dy, c0);
        dy = min(max(dy, -a.h), a.h);
        c0 = min(max(c0, -a.w), a.src_w);
        const bool roll_ok = (unsigned long)i < (unsigned long)a.n_rolls;
        float* out = a.dst + (size_t)b * a.h * a.w;
        for (long y = (long)blockIdx.x * TY + ty; y < a.h; y += (long)gridDim.x * TY) {
            const long sy = y - dy;
            for (unsigned j = tx; j < wb; j += TX) {
                const int start = c0 + 8 * (int)j;   // first source column of this lane's 8 cells; in [-w, src_w + w - 8]
                f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
                if (roll_ok && sy >= 0 && sy < a.h && start > -8 && start < a.src_w) {
                    // (inside this branch the row exists and at least one of the 8 cells lies inside it)
                    const uint8_t* row = static_cast<const uint8_t*>(a.src) + ((size_t)i * a.h + (size_t)sy) * row_bytes;
                    if (KIND == 1) {
                        const int r = start & 7, q = (start - r) / 8, rb = a.src_w >> 3;   // start = 8q + r, floor quotient, 0 <= r < 8
                        const uint32_t b0 = (q >= 0 && q < rb) ? __builtin_nontemporal_load(row + q) : 0u;
                        const uint32_t b1 = (r && q + 1 >= 0 && q + 1 < rb) ? __builtin_nontemporal_load(row + q + 1) : 0u;
                        const uint32_t v = (((b0 << 8) | b1) >> (8 - r)) & 255u;
                        lo = f32x4{(float)((v >> 7) & 1u), (float)((v >> 6) & 1u), (float)((v >> 5) & 1u), (float)((v >> 4) & 1u)};
                        hi = f32x4{(float)((v >> 3) & 1u), (float)((v >> 2) & 1u), (float)((v >> 1) & 1u), (float)(v & 1u)};
                    } else if (KIND == 0) {
                        float c[8];
                        if (start >= 0 && start + 8 <= a.src_w && !(reinterpret_cast<uintptr_t>(row + start) & 7)) {
                            const uint64_t v = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(row + start));
#pragma unroll
                            for (int e = 0; e < 8; ++e) c[e] = (float)(uint32_t)((v >> (8 * e)) & 255u) * a.scale;
                        } else {
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const int sx = start + e;
                                c[e] = (sx >= 0 && sx < a.src_w) ? (float)__builtin_nontemporal_load(row + sx) * a.scale : 0.f;
                            }
                        }
                        lo = f32x4{c[0], c[1], c[2], c[3]}; hi = f32x4{c[4], c[5], c[6], c[7]};
                    } else {
                        const float* frow = reinterpret_cast<const float*>(row);
                        if (start >= 0 && start + 8 <= a.src_w && !(reinterpret_cast<uintptr_t>(frow + start) & 15)) {
                            lo = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(frow + start));
                            hi = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(frow + start) + 1);
                        } else {
                            float c[8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const int sx = start + e;
                                c[e] = (sx >= 0 && sx < a.src_w) ? __builtin_nontemporal_load(frow + sx) : 0.f;
                            }
                            lo = f32x4{c[0], c[1], c[2], c[3]}; hi = f32x4{c[4], c[5], c[6], c[7]};
                        }
                    }
                }
                float* cell = out + ((size_t)y * wb + j) * 8;
                *reinterpret_cast<f32x4*>(cell) = lo;
                *reinterpret_cast<f32x4*>(cell + 4) = hi;
            }
        }
    }
}
