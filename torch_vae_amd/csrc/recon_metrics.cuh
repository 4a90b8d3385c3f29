// Note-level reconstruction metrics (vae_recon_metrics, vae_util.hip): one pass over (xhat, target) gives, per roll and in total, the
// f64 sums of the squared error, the absolute error and the ELBO's own BCE term, the number of true notes, and for up to RM_MAX_T
// output thresholds the true / false positives; plus the value ranges of both tensors.
//   recon_metrics_kernel<T>: one workgroup per (roll, chunk of RM_CHUNK cells).  A lane reads 16 bytes of each tensor per step (a
//       scalar head up to the first 16-byte boundary of xhat and a scalar tail, so any 4-byte-aligned base and any roll length run;
//       the target takes four dword loads instead where its misalignment differs from xhat's) and has all of the chunk's loads in
//       flight before it uses the first.  The note predicates are wave ballots: a count is one compare and two scalar instructions per
//       cell and threshold, lives in wave-uniform registers and needs no cross-lane reduction.  The sums are f64 per lane in cell
//       order, then a fixed xor tree over the wave, then the four waves in order.  The workgroup stores one partial record.
//   recon_metrics_fold_kernel: one wave per output field (3 sums, 1 + 2T counts, 4 range ends).  Lane l folds the chunks of rolls l,
//       l + 64, ... in chunk order into the per-roll outputs and those rolls in order into its own partial, then the same wave tree;
//       lane 0 writes or accumulates the field's total.
// The chunking depends on roll_len alone, the fold on (rolls, chunks) alone: no atomics, nothing depends on the grid or on arrival
// order, and a repeated call gives the same bits.  Counts are integers: exact.  A NaN xhat compares false with every threshold (never a
// predicted note) and makes the sums NaN; fminf / fmaxf leave it out of the ranges.
#pragma once
#include "common.cuh"

constexpr int RM_THREADS = 256;
constexpr int RM_CHUNK = 4096;   // cells per workgroup: 4 x (256 lanes x 4 cells)
constexpr int RM_VSTEPS = RM_CHUNK / (RM_THREADS * 4);
constexpr int RM_MAX_T = 8;
constexpr int RM_MAX_COUNTS = 1 + 2 * RM_MAX_T;
struct RmThresholds { float t[RM_MAX_T]; };

template <int T> struct RmAcc {
    double se = 0.0, ae = 0.0, bce = 0.0;
    float xmin = INFINITY, xmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    int pos = 0, tp[T], pred[T];   // wave-uniform
};

// One cell per lane; every lane of the wave calls it (the ballots), `ok` says whether the lane holds a cell.
template <int T> __device__ __forceinline__ void rm_cell(RmAcc<T>& a, float xh, float tg, bool ok, const RmThresholds& th, float tt) {
    const unsigned long long mt = __ballot(ok && tg >= tt);
    a.pos += __popcll(mt);
#pragma unroll
    for (int k = 0; k < T; ++k) {
        const unsigned long long mp = __ballot(ok && xh >= th.t[k]);
        a.pred[k] += __popcll(mp);
        a.tp[k] += __popcll(mp & mt);
    }
    if (ok) {
        const double d = (double)(xh - tg);
        a.se += d * d;
        a.ae += fabs(d);
        const float b = recon_term<VAE_RECON_BCE>(xh, tg);
        a.bce += (double)(xh == xh ? b : xh);   // the term's fmaxf clamps would turn log(NaN) into -100
        a.xmin = fminf(a.xmin, xh); a.xmax = fmaxf(a.xmax, xh);
        a.tmin = fminf(a.tmin, tg); a.tmax = fmaxf(a.tmax, tg);
    }
}

// Partial record p = roll * nchunks + chunk: part_sums[p][3] = se, ae, bce; part_counts[p][1 + 2T] = positives, then tp, fp per
// threshold; part_rng[p][4] = min / max of xhat, min / max of target.
template <int T>
static __global__ __launch_bounds__(RM_THREADS) void recon_metrics_kernel(const float* __restrict__ xhat, const float* __restrict__ target,
                                                                          long roll_len, long nchunks, RmThresholds th, float tt,
                                                                          double* __restrict__ part_sums, long long* __restrict__ part_counts,
                                                                          float* __restrict__ part_rng) {
    constexpr int NC = 1 + 2 * T;
    __shared__ double s_sum[4][3];
    __shared__ int s_cnt[4][NC];
    __shared__ float s_rng[4][4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const long p = blockIdx.x, r = p / nchunks, c0 = (p - r * nchunks) * RM_CHUNK;
    const int len = (int)min((long)RM_CHUNK, roll_len - c0);
    const float* __restrict__ x = xhat + r * roll_len + c0;
    const float* __restrict__ t = target + r * roll_len + c0;
    const int head = min(len, (int)((4 - ((reinterpret_cast<uintptr_t>(x) >> 2) & 3)) & 3));   // cells before xhat's 16-byte boundary
    const bool t_vec = (reinterpret_cast<uintptr_t>(t + head) & 15) == 0;
    const int nvec = (len - head) >> 2, tail0 = head + nvec * 4, ntail = len - tail0;

    float4 xv[RM_VSTEPS], tv[RM_VSTEPS];
#pragma unroll
    for (int j = 0; j < RM_VSTEPS; ++j) {
        const int v = j * RM_THREADS + tid;
        xv[j] = tv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v < nvec) {
            const int i = head + 4 * v;
            xv[j] = *reinterpret_cast<const float4*>(x + i);
            tv[j] = t_vec ? *reinterpret_cast<const float4*>(t + i) : make_float4(t[i], t[i + 1], t[i + 2], t[i + 3]);
        }
    }
    RmAcc<T> a;
#pragma unroll
    for (int k = 0; k < T; ++k) a.tp[k] = a.pred[k] = 0;
    if (w == 0 && head + ntail > 0) {   // the at most 3 + 3 head and tail cells: lanes 0.. of wave 0
        const int i = lane < head ? lane : tail0 + (lane - head);
        const bool ok = lane < head + ntail;
        rm_cell<T>(a, ok ? x[i] : 0.f, ok ? t[i] : 0.f, ok, th, tt);
    }
#pragma unroll
    for (int j = 0; j < RM_VSTEPS; ++j) {
        if (j * RM_THREADS + w * 64 < nvec) {   // wave-uniform
            const bool ok = j * RM_THREADS + tid < nvec;
            rm_cell<T>(a, xv[j].x, tv[j].x, ok, th, tt);
            rm_cell<T>(a, xv[j].y, tv[j].y, ok, th, tt);
            rm_cell<T>(a, xv[j].z, tv[j].z, ok, th, tt);
            rm_cell<T>(a, xv[j].w, tv[j].w, ok, th, tt);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        a.se += __shfl_xor(a.se, o); a.ae += __shfl_xor(a.ae, o); a.bce += __shfl_xor(a.bce, o);
        a.xmin = fminf(a.xmin, __shfl_xor(a.xmin, o)); a.xmax = fmaxf(a.xmax, __shfl_xor(a.xmax, o));
        a.tmin = fminf(a.tmin, __shfl_xor(a.tmin, o)); a.tmax = fmaxf(a.tmax, __shfl_xor(a.tmax, o));
    }
    if (lane == 0) {
        s_sum[w][0] = a.se; s_sum[w][1] = a.ae; s_sum[w][2] = a.bce;
        s_rng[w][0] = a.xmin; s_rng[w][1] = a.xmax; s_rng[w][2] = a.tmin; s_rng[w][3] = a.tmax;
        s_cnt[w][0] = a.pos;
#pragma unroll
        for (int k = 0; k < T; ++k) { s_cnt[w][1 + 2 * k] = a.tp[k]; s_cnt[w][2 + 2 * k] = a.pred[k] - a.tp[k]; }
    }
    __syncthreads();
    if (tid < 3) part_sums[p * 3 + tid] = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
    if (tid < NC) part_counts[p * NC + tid] = (long long)(s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid]);
    if (tid < 4) {
        const float v0 = s_rng[0][tid], v1 = s_rng[1][tid], v2 = s_rng[2][tid], v3 = s_rng[3][tid];
        part_rng[p * 4 + tid] = (tid & 1) ? fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)) : fminf(fminf(v0, v1), fminf(v2, v3));
    }
}

// Chunks -> rolls -> totals, one wave per field so that the fields' dependent loads overlap (one workgroup walking the fields in turn
// paid a memory round trip per field).  Lane l of a field's wave folds the chunks of rolls l, l + 64, ... in chunk order into the per-roll
// output and those rolls in order into its own partial, then a fixed xor tree.  Workgroup 0: the four range fields, one per wave, and
// n_cells; workgroups 1..: wave g = (blockIdx.x - 1) * 4 + wave is sum field g (g < 3) or count field g - 3.  With nchunks == 1 the partial
// records ARE the per-roll outputs (the caller passes the same pointers).  totals[8] = se, ae, bce, n_cells, min / max xhat, min / max
// target; total_counts[ncnt].  accumulate: sums and counts add, ranges combine - unless the totals hold no cell yet (n_cells == 0: an
// all-zero state is the empty one; only workgroup 0 reads or writes n_cells).
static __global__ __launch_bounds__(RM_THREADS) void recon_metrics_fold_kernel(long rolls, long nchunks, int ncnt, double n_cells,
                                                                               const double* __restrict__ part_sums,
                                                                               const long long* __restrict__ part_counts,
                                                                               const float* __restrict__ part_rng, double* roll_sums,
                                                                               long long* roll_counts, double* __restrict__ totals,
                                                                               long long* __restrict__ total_counts, int accumulate) {
    __shared__ float s_r[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool add = accumulate != 0;
    if (blockIdx.x == 0) {
        const bool mx = w & 1;
        float acc = mx ? -INFINITY : INFINITY;
        for (long r = lane; r < rolls; r += 64)
            for (long c = 0; c < nchunks; ++c) {
                const float v = part_rng[(r * nchunks + c) * 4 + w];
                acc = mx ? fmaxf(acc, v) : fminf(acc, v);
            }
        for (int o = 32; o > 0; o >>= 1) {
            const float v = __shfl_xor(acc, o);
            acc = mx ? fmaxf(acc, v) : fminf(acc, v);
        }
        if (lane == 0) s_r[w] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            const bool held = add && totals[3] > 0.0;
            for (int f = 0; f < 4; ++f) {
                double v = (double)s_r[f];
                if (held) v = (f & 1) ? fmax(totals[4 + f], v) : fmin(totals[4 + f], v);
                totals[4 + f] = v;
            }
            totals[3] = add ? totals[3] + n_cells : n_cells;
        }
        return;
    }
    const int g = (blockIdx.x - 1) * 4 + w;   // wave-uniform
    if (g < 3) {
        double acc = 0.0;
        for (long r = lane; r < rolls; r += 64) {
            double v = part_sums[r * nchunks * 3 + g];
            for (long c = 1; c < nchunks; ++c) v += part_sums[(r * nchunks + c) * 3 + g];
            if (nchunks > 1) roll_sums[r * 3 + g] = v;
            acc += v;
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) totals[g] = add ? totals[g] + acc : acc;
    } else if (g - 3 < ncnt) {
        const int f = g - 3;
        long long acc = 0;
        for (long r = lane; r < rolls; r += 64) {
            long long v = part_counts[r * nchunks * ncnt + f];
            for (long c = 1; c < nchunks; ++c) v += part_counts[(r * nchunks + c) * ncnt + f];
            if (nchunks > 1) roll_counts[r * ncnt + f] = v;
            acc += v;
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) total_counts[f] = add ? total_counts[f] + acc : acc;
    }
}
