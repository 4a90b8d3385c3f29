// Kernels of the differentiable paths outside the training step (vae_backward_ex): the BatchNorm backward of an
// eval-mode forward, the latent gradient of a decode-only pass and the input gradient of encoder.0.
#pragma once
#include "edge_kernels.cuh"

// BatchNorm backward on the running statistics (eval mode).  y_bn = (y - rm) * invstd * gamma + beta with invstd = 1/sqrt(rv + eps)
// constant, so dL/dy = dz * gamma * invstd:  p0 = gamma*invstd, p1 = p2 = 0.  The producers of dz left sum dz and sum dz*xhat with
// xhat = y*invstd + xm read from the eval coefficients bn_eval_coef_kernel wrote (LC_INVSTD, LC_XM), so dgamma = sum dz*xhat and
// dbeta = sum dz.  Unlike train mode the conv bias before the BatchNorm has a gradient: sum dL/dy = p0 * sum dz.
// Consumers read p0..p2 from the block (BNF_NONE); every gradient is written times ginv (f16 gradient scaling).
static __global__ void bn_eval_bwd_kernel(BnFuse f) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int C = f.C;
    if (c >= C) return;
    const double sdz = stat_sum(f.stat, C, c), sdzx = stat_sum(f.stat, C, C + c);
    const double s = (double)f.gamma[c] * (double)f.block[LC_INVSTD * C + c];
    f.block[LC_P0 * C + c] = (float)s; f.block[LC_P1 * C + c] = 0.f; f.block[LC_P2 * C + c] = 0.f;
    f.dgamma[c] = (float)(sdzx * (double)f.ginv); f.dbeta[c] = (float)(sdz * (double)f.ginv);
    if (f.dconv_bias) f.dconv_bias[c] = (float)(s * sdz * (double)f.ginv);
}

// dL/dz of a decode-only pass: the split-K slabs of decoder_input's input-gradient GEMM ([nslab][B][npad], column l < L) summed in
// slab order, the f16 gradient scale removed, written as f32 [B,L].
static __global__ void latent_dz_kernel(const float* __restrict__ slab, int nslab, int npad, int B, int L, float ginv, float* __restrict__ dz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * L) return;
    const int b = i / L, l = i - b * L;
    const float* p = slab + (size_t)b * npad + l;
    const size_t ss = (size_t)B * npad;
    float s = 0.f;
    for (int k = 0; k < nslab; ++k) s += p[k * ss];
    dz[i] = s * ginv;
}

// Input gradient of encoder.0 (Conv2d 1 -> 32, k3, s2, p1): a transposed conv from the 32-channel half-resolution gradient back to
// one channel at full resolution.  Prologue: encoder.0's BatchNorm backward, g = dz*p0 + y*p1 + p2 (as conv1_wgrad_kernel; dz already
// carries the LeakyReLU mask), p0..p2 from the coefficient block the backward finalised for the weight gradient.
// Four lanes share an output-grid position (b, oy, ox), 8 channels each, and produce the 2x2 input pixels (2oy..2oy+1, 2ox..2ox+1):
//   dx[2oy  ][2ox  ] = W11 g(oy,ox)
//   dx[2oy  ][2ox+1] = W12 g(oy,ox) + W10 g(oy,ox+1)
//   dx[2oy+1][2ox  ] = W21 g(oy,ox) + W01 g(oy+1,ox)
//   dx[2oy+1][2ox+1] = W22 g(oy,ox) + W20 g(oy,ox+1) + W02 g(oy+1,ox) + W00 g(oy+1,ox+1)      (Wij = weight[c][0][i][j])
// A wave's 16 positions read 1 KiB runs of dz / y; the right and lower neighbours are re-read by the adjacent threads from L2.
// The weights sit in LDS (in registers they took 72 VGPRs per lane and halved the occupancy).
// Bandwidth-bound: reads 2 * B*(H/2)*(W/2)*32 storage elements, writes B*H*W floats (times ginv: f16 gradient scaling).
template <typename T>
__global__ __launch_bounds__(256) void conv1_dgrad_kernel(const T* __restrict__ dz, const T* __restrict__ y, const float* __restrict__ gcoef,
                                                          const float* __restrict__ w, float* __restrict__ dx, int B, int H, int W, float ginv) {
    __shared__ f32x4 wsh[9][8];   // tap-major copy of the weights: [t][channel / 4]; a lane reads its 8 channels as two 16-byte words
    const int tid = threadIdx.x, cg = tid & 3;
    for (int j = tid; j < 288; j += 256) reinterpret_cast<float*>(wsh)[(j % 9) * 32 + j / 9] = w[j];
    const int Ho = H >> 1, Wo = W >> 1, lw = 31 - __builtin_clz(Wo), lh = 31 - __builtin_clz(Ho);   // (H, W: powers of two)
    const int P = B * Ho * Wo;
    float p0[8], p1[8], p2[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { const int ch = cg * 8 + c; p0[c] = gcoef[ch]; p1[c] = gcoef[32 + ch]; p2[c] = gcoef[64 + ch]; }
    __syncthreads();
    // taps each neighbour feeds, per output of the 2x2 block: (o00, o01, o10, o11); -1 = none
    constexpr int kTap[4][4] = {{4, 5, 7, 8}, {-1, 3, -1, 6}, {-1, -1, 1, 2}, {-1, -1, -1, 0}};
    const int n_iter = (P + 63) / 64;
    for (int it = blockIdx.x; it < n_iter; it += gridDim.x) {
        const int q = it * 64 + (tid >> 2);
        const bool ok = q < P;
        const int qq = ok ? q : 0;
        const int ox = qq & (Wo - 1), oy = (qq >> lw) & (Ho - 1), b = qq >> (lw + lh);
        const bool okx = ok && ox + 1 < Wo, oky = ok && oy + 1 < Ho;
        float dv[4][8], yv[4][8];   // neighbours (oy,ox) (oy,ox+1) (oy+1,ox) (oy+1,ox+1): all eight loads in flight together
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = u == 0 ? ok : u == 1 ? okx : u == 2 ? oky : (okx && oky);
            if (in) {
                const size_t pix = ((size_t)b * Ho + oy + (u >> 1)) * Wo + ox + (u & 1);
                load8<T>(dz + pix * 32 + cg * 8, dv[u]); load8<T>(y + pix * 32 + cg * 8, yv[u]);
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) { dv[u][c] = 0.f; yv[u][c] = 0.f; }
            }
        }
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = u == 0 ? ok : u == 1 ? okx : u == 2 ? oky : (okx && oky);
            float g[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) g[c] = in ? dv[u][c] * p0[c] + yv[u][c] * p1[c] + p2[c] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = kTap[u][k];
                if (t < 0) continue;
                const f32x4 wa = wsh[t][2 * cg], wb = wsh[t][2 * cg + 1];
#pragma unroll
                for (int c = 0; c < 4; ++c) o[k] += wa[c] * g[c] + wb[c] * g[4 + c];
            }
        }
#pragma unroll
        for (int m = 1; m < 4; m <<= 1)
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] += __shfl_xor(o[k], m, 64);
        if (ok && cg < 2) {
            f32x2 v;
            v[0] = o[2 * cg] * ginv; v[1] = o[2 * cg + 1] * ginv;
            *reinterpret_cast<f32x2*>(dx + ((size_t)b * H + 2 * oy + cg) * W + 2 * ox) = v;
        }
    }
}
