// Pairwise squared distances between two sets of f32 points and what the fidelity metrics take from them (include/vae_fidelity.h):
// the k smallest of a row (sd_knn_kernel), counts inside per-reference balls and the nearest reference (sd_balls_kernel), sums of
// Gaussian kernel values and of the distances (sd_sums_kernel).  Nothing of the [queries x references] matrix is ever stored.
//
// Lane map (the one lstat_joint_kernel of latent_stats.cuh uses): a workgroup of 256 lanes, a lane owns QR queries and all of d -
// the queries sit in registers, padded with zeros from D to DP (DP = 16, 32, 64 or 128; QR = 4, 4, 2, 1: 128 query registers at
// the most) - and a tile of SD_JT reference points sits in LDS, [SD_JT][DP] with zeros past D and past the last point, shared by
// the block.  Every lane of a wave reads the same 16 bytes of a reference row, a broadcast with no bank conflict, and a lane
// works on JB = 4, 4, 4, 2 references at once (QR x JB independent sums).  grid.x walks the queries, grid.y the `splits` ranges of the
// reference set; the three kernels are three epilogues over the same tile walk (sd_walk).
//
// sd_term / the loop of sd_walk IS the distance of the header: the difference in f32, squared into the running sum by one fused
// multiply-add, d ascending.  The padded terms add (0 - 0)^2 = +0 to a sum that is >= +0, inf or NaN: no bit changes, so the order
// over d depends on D only and d2 has the same bits in every kernel, tile position and split.  (fmaf is written out: left to the
// compiler, contraction could differ between the three instantiations.)
//
// A split's results go to work space and a second launch merges them in split order (sd_*_merge_kernel); with one split
// sd_balls_kernel writes the outputs itself (sd_knn_kernel always leaves the pick of the k-th to the merge: picking by a run-time k
// from the sorted registers would turn them into an indexed array in scratch memory).  No atomics: the f64 sums are reduced lane -> block (an LDS tree) -> the block's
// slot -> sd_sums_merge_kernel (slots strided over 256 lanes, then the same tree), all fixed by the shape and splits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SD_MAX_DIM 128
#define SD_MAX_K 8
#define SD_MAX_G 8
#define SD_MAX_SPLITS 64
#define SD_MAX_POINTS (1 << 22)
#define SD_THREADS 256
#define SD_JT 64               // reference points per LDS tile
#define SD_LOG2E 1.4426950408889634

__host__ __device__ constexpr int sd_qr(int DP) { return DP <= 32 ? 4 : (DP == 64 ? 2 : 1); }   // queries per lane
__host__ __device__ constexpr int sd_jb(int DP) { return DP <= 64 ? 4 : 2; }                  // references per step of a lane (SD_JT is a multiple)
// references per split: a multiple of 4, so that the steps of 4 or 2 references a lane takes - and with them the f32 partial sums of
// sd_sums_kernel - fall on the same references whatever `splits` is (the last splits may be empty)
__host__ __device__ inline long sd_split_len(long n, int splits) { return ((n + splits - 1) / splits + 3) / 4 * 4; }

__device__ __forceinline__ float sd_term(float a, float b, float acc) {
    const float t = a - b;
    return __fmaf_rn(t, t, acc);
}

// ascending best[0..7] <- with v, if v is below best[7] (a NaN never is, +inf never is)
__device__ __forceinline__ void sd_insert8(float (&best)[SD_MAX_K], float v) {
    if (v < best[7]) {
        best[7] = v < best[6] ? best[6] : v;
        best[6] = v < best[5] ? best[5] : fminf(v, best[6]);
        best[5] = v < best[4] ? best[4] : fminf(v, best[5]);
        best[4] = v < best[3] ? best[3] : fminf(v, best[4]);
        best[3] = v < best[2] ? best[2] : fminf(v, best[3]);
        best[2] = v < best[1] ? best[1] : fminf(v, best[2]);
        best[1] = v < best[0] ? best[0] : fminf(v, best[1]);
        best[0] = fminf(v, best[0]);
    }
}
__device__ __forceinline__ float sd_pick8(const float (&best)[SD_MAX_K], int k) {
    float v = best[0];
#pragma unroll
    for (int s = 1; s < SD_MAX_K; ++s) v = (k - 1 == s) ? best[s] : v;
    return v;
}

// The QR queries of this lane: query r is point q0 + r * SD_THREADS + threadIdx.x (consecutive lanes, consecutive points: the
// outputs leave coalesced); one past the set is all zeros and is masked by the epilogues.
template <int DP, int QR>
__device__ __forceinline__ void sd_load_queries(const float* __restrict__ x, long count, int D, long q0, float (&q)[QR][DP]) {
#pragma unroll
    for (int r = 0; r < QR; ++r) {
        const long i = q0 + (long)r * SD_THREADS + threadIdx.x;
        const float* src = x + (i < count ? i : 0) * D;
#pragma unroll
        for (int d = 0; d < DP; ++d) q[r][d] = (i < count && d < D) ? src[d] : 0.f;
    }
}

// Walks the references [j0, j1) tile by tile.  on_tile(t0, jn): every lane, after the tile's points are stored and before the
// barrier (stage what else the tile needs).  begin() / pair(r, j, d2) / end(): per step of sd_jb(DP) references, pair for each of the
// lane's QR queries and each reference j of the step that exists.
template <int DP, int QR, typename OnTile, typename Begin, typename Pair, typename End>
__device__ __forceinline__ void sd_walk(const float* __restrict__ refs, long j0, long j1, int D, const float (&q)[QR][DP], float* tile,
                                        OnTile&& on_tile, Begin&& begin, Pair&& pair, End&& end) {
    constexpr int SD_JB = sd_jb(DP);
    for (long t0 = j0; t0 < j1; t0 += SD_JT) {
        const int jn = (int)(j1 - t0 < SD_JT ? j1 - t0 : SD_JT);
        __syncthreads();                                         // the tile before this one has been read by everybody
        for (int e = threadIdx.x; e < SD_JT * DP; e += SD_THREADS) {
            const int j = e / DP, d = e % DP;
            tile[e] = (j < jn && d < D) ? refs[(t0 + j) * D + d] : 0.f;
        }
        on_tile(t0, jn);
        __syncthreads();
        for (int jj = 0; jj < jn; jj += SD_JB) {                 // (jn is the same in every lane; rows past it are zeros, not read as results)
            float acc[QR][SD_JB];
#pragma unroll
            for (int r = 0; r < QR; ++r)
#pragma unroll
                for (int b = 0; b < SD_JB; ++b) acc[r][b] = 0.f;
#pragma unroll
            for (int d = 0; d < DP; d += 4) {
                float4 v[SD_JB];
#pragma unroll
                for (int b = 0; b < SD_JB; ++b) v[b] = *reinterpret_cast<const float4*>(tile + (jj + b) * DP + d);
#pragma unroll
                for (int r = 0; r < QR; ++r)
#pragma unroll
                    for (int b = 0; b < SD_JB; ++b) {
                        float s = acc[r][b];
                        s = sd_term(q[r][d + 0], v[b].x, s);
                        s = sd_term(q[r][d + 1], v[b].y, s);
                        s = sd_term(q[r][d + 2], v[b].z, s);
                        s = sd_term(q[r][d + 3], v[b].w, s);
                        acc[r][b] = s;
                    }
            }
            begin();
#pragma unroll
            for (int b = 0; b < SD_JB; ++b)
                if (jj + b < jn) {
#pragma unroll
                    for (int r = 0; r < QR; ++r) pair(r, t0 + jj + b, acc[r][b]);
                }
            end();
        }
    }
}

struct SdRange { long j0, j1; };
__device__ __forceinline__ SdRange sd_split_range(long n, int splits) {
    const long len = sd_split_len(n, splits), first = (long)blockIdx.y * len;
    const long j0 = first < n ? first : n;
    return {j0, j0 + len < n ? j0 + len : n};
}

// ---- k-NN radii ---------------------------------------------------------------------------------------------------------------------
struct SdKnnArgs {
    const float* x; long n; int D, k, splits;
    float* radii2;     // [n], written by sd_knn_merge_kernel
    float* part;       // [splits][n][8]: the 8 smallest of every split, ascending
};

template <int DP>
__global__ __launch_bounds__(SD_THREADS) void sd_knn_kernel(SdKnnArgs a) {
    constexpr int QR = sd_qr(DP);
    __shared__ __attribute__((aligned(16))) float tile[SD_JT * DP];
    const long q0 = (long)blockIdx.x * (SD_THREADS * QR);
    float q[QR][DP];
    sd_load_queries<DP, QR>(a.x, a.n, a.D, q0, q);
    float best[QR][SD_MAX_K];
#pragma unroll
    for (int r = 0; r < QR; ++r)
#pragma unroll
        for (int s = 0; s < SD_MAX_K; ++s) best[r][s] = INFINITY;
    const SdRange rg = sd_split_range(a.n, a.splits);
    sd_walk<DP, QR>(a.x, rg.j0, rg.j1, a.D, q, tile, [](long, int) {}, [] {},
                    [&](int r, long j, float d2) {
                        const long i = q0 + (long)r * SD_THREADS + threadIdx.x;
                        if (j != i) sd_insert8(best[r], d2);
                    }, [] {});
#pragma unroll
    for (int r = 0; r < QR; ++r) {
        const long i = q0 + (long)r * SD_THREADS + threadIdx.x;
        if (i >= a.n) continue;
        float4* dst = reinterpret_cast<float4*>(a.part + ((long)blockIdx.y * a.n + i) * SD_MAX_K);
        dst[0] = make_float4(best[r][0], best[r][1], best[r][2], best[r][3]);
        dst[1] = make_float4(best[r][4], best[r][5], best[r][6], best[r][7]);
    }
}

__global__ __launch_bounds__(SD_THREADS) void sd_knn_merge_kernel(SdKnnArgs a) {
    const long i = (long)blockIdx.x * SD_THREADS + threadIdx.x;
    if (i >= a.n) return;
    float best[SD_MAX_K];
#pragma unroll
    for (int s = 0; s < SD_MAX_K; ++s) best[s] = INFINITY;
    for (int sp = 0; sp < a.splits; ++sp) {
        const float4* src = reinterpret_cast<const float4*>(a.part + ((long)sp * a.n + i) * SD_MAX_K);
        const float4 lo = src[0], hi = src[1];
        sd_insert8(best, lo.x); sd_insert8(best, lo.y); sd_insert8(best, lo.z); sd_insert8(best, lo.w);
        sd_insert8(best, hi.x); sd_insert8(best, hi.y); sd_insert8(best, hi.z); sd_insert8(best, hi.w);
    }
    a.radii2[i] = sd_pick8(best, a.k);
}

// ---- ball membership and the nearest reference ----------------------------------------------------------------------------------------
struct SdBallArgs {
    const float* q; long m; const float* r; long n; int D;
    const float* radii2;       // [n] or null (then no counts)
    int exclude, splits;
    int* counts; int* nearest; float* nearest_d2;          // [m]; counts may be null
    int* part_counts; int* part_nearest; float* part_d2;   // [splits][m], used when splits > 1
};

template <int DP>
__global__ __launch_bounds__(SD_THREADS) void sd_balls_kernel(SdBallArgs a) {
    constexpr int QR = sd_qr(DP);
    __shared__ __attribute__((aligned(16))) float tile[SD_JT * DP];
    __shared__ float rad[SD_JT];
    const long q0 = (long)blockIdx.x * (SD_THREADS * QR);
    float q[QR][DP];
    sd_load_queries<DP, QR>(a.q, a.m, a.D, q0, q);
    int cnt[QR], bi[QR];
    float bd[QR];
#pragma unroll
    for (int r = 0; r < QR; ++r) { cnt[r] = 0; bi[r] = -1; bd[r] = INFINITY; }
    const bool counting = a.radii2 != nullptr;
    const SdRange rg = sd_split_range(a.n, a.splits);
    long tile0 = 0;                 // the first reference of the tile in LDS
    sd_walk<DP, QR>(a.r, rg.j0, rg.j1, a.D, q, tile,
                    [&](long t0, int jn) {
                        if (counting && (int)threadIdx.x < jn) rad[threadIdx.x] = a.radii2[t0 + threadIdx.x];
                        tile0 = t0;
                    },
                    [] {},
                    [&](int r, long j, float d2) {
                        const long i = q0 + (long)r * SD_THREADS + threadIdx.x;
                        if (a.exclude && j == i) return;
                        if (counting) cnt[r] += d2 <= rad[j - tile0] ? 1 : 0;
                        if (d2 < bd[r]) { bd[r] = d2; bi[r] = (int)j; }
                    }, [] {});
#pragma unroll
    for (int r = 0; r < QR; ++r) {
        const long i = q0 + (long)r * SD_THREADS + threadIdx.x;
        if (i >= a.m) continue;
        if (a.splits == 1) {
            if (a.counts) a.counts[i] = cnt[r];
            a.nearest[i] = bi[r];
            a.nearest_d2[i] = bd[r];
        } else {
            const long o = (long)blockIdx.y * a.m + i;
            a.part_counts[o] = cnt[r];
            a.part_nearest[o] = bi[r];
            a.part_d2[o] = bd[r];
        }
    }
}

__global__ __launch_bounds__(SD_THREADS) void sd_balls_merge_kernel(SdBallArgs a) {
    const long i = (long)blockIdx.x * SD_THREADS + threadIdx.x;
    if (i >= a.m) return;
    int cnt = 0, bi = -1;
    float bd = INFINITY;
    for (int sp = 0; sp < a.splits; ++sp) {          // ascending ranges: a strict < keeps the lowest index of a tie
        const long o = (long)sp * a.m + i;
        cnt += a.part_counts[o];
        const float d = a.part_d2[o];
        if (d < bd) { bd = d; bi = a.part_nearest[o]; }
    }
    if (a.counts) a.counts[i] = cnt;
    a.nearest[i] = bi;
    a.nearest_d2[i] = bd;
}

// ---- kernel sums ----------------------------------------------------------------------------------------------------------------------
struct SdSumArgs {
    const float* a; long n; const float* b; long m; int D;
    const double* gammas; int G, exclude, splits;
    double* part;      // [splits * gridDim.x][SD_MAX_G + 1]
    double* sums;      // [G + 1]
};

// fixed-order sum of one f64 per lane over the block; the result is valid in lane 0.  red: 256 doubles
__device__ __forceinline__ double sd_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = SD_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

template <int DP>
__global__ __launch_bounds__(SD_THREADS) void sd_sums_kernel(SdSumArgs a) {
    constexpr int QR = sd_qr(DP);
    __shared__ __attribute__((aligned(16))) float tile[SD_JT * DP];
    static_assert(SD_JT * 16 * sizeof(float) >= SD_THREADS * sizeof(double), "the tile doubles as the reduction buffer");
    const long q0 = (long)blockIdx.x * (SD_THREADS * QR);
    float q[QR][DP];
    sd_load_queries<DP, QR>(a.a, a.n, a.D, q0, q);
    // exponent of 2 for bandwidth g: (c_hi + c_lo) * d2 with c_hi + c_lo = -gamma log2 e to f64 accuracy
    float chi[SD_MAX_G], clo[SD_MAX_G];
#pragma unroll
    for (int g = 0; g < SD_MAX_G; ++g) {
        const double c = g < a.G ? -a.gammas[g] * SD_LOG2E : 0.0;
        chi[g] = (float)c;
        clo[g] = (float)(c - (double)chi[g]);
        if (!(fabs(c) <= 3.0e38)) clo[g] = 0.f;      // (an overflowing or NaN scale stays what f32 makes of it)
    }
    double S[SD_MAX_G + 1];
#pragma unroll
    for (int g = 0; g <= SD_MAX_G; ++g) S[g] = 0.0;
    float step[SD_MAX_G];                              // at most QR * sd_jb(DP) <= 16 kernel values in f32
    const SdRange rg = sd_split_range(a.m, a.splits);
    sd_walk<DP, QR>(a.b, rg.j0, rg.j1, a.D, q, tile, [](long, int) {},
                    [&] {
#pragma unroll
                        for (int g = 0; g < SD_MAX_G; ++g) step[g] = 0.f;
                    },
                    [&](int r, long j, float d2) {
                        const long i = q0 + (long)r * SD_THREADS + threadIdx.x;
                        if (i >= a.n || (a.exclude && j == i)) return;
                        S[SD_MAX_G] += (double)d2;
                        const float capped = fminf(d2, 3.0e38f);       // the low part of the scale times +inf must not meet the high part's -inf
#pragma unroll
                        for (int g = 0; g < SD_MAX_G; ++g)
                            if (g < a.G) step[g] += __builtin_amdgcn_exp2f(__fmaf_rn(chi[g], d2, clo[g] * capped));
                    },
                    [&] {
#pragma unroll
                        for (int g = 0; g < SD_MAX_G; ++g) S[g] += (double)step[g];
                    });
    double* red = reinterpret_cast<double*>(tile);
    double* dst = a.part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (SD_MAX_G + 1);
#pragma unroll
    for (int g = 0; g <= SD_MAX_G; ++g) {
        if (g < a.G || g == SD_MAX_G) {
            const double t = sd_block_sum(S[g], red);
            if (threadIdx.x == 0) dst[g] = t;
        }
    }
}

// sums[g] <- the slots of column g (block g of the grid; the last block takes the distance column), slot p by lane p mod 256
__global__ __launch_bounds__(SD_THREADS) void sd_sums_merge_kernel(SdSumArgs a, long slots) {
    __shared__ double red[SD_THREADS];
    const int col = (int)blockIdx.x < a.G ? (int)blockIdx.x : SD_MAX_G;
    double v = 0.0;
    for (long p = threadIdx.x; p < slots; p += SD_THREADS) v += a.part[p * (SD_MAX_G + 1) + col];
    const double t = sd_block_sum(v, red);
    if (threadIdx.x == 0) a.sums[blockIdx.x] = t;
}
