// A mixture of K Gaussians in the L-dimensional latent space, fitted to encodings and sampled from (include/vae_mixture.h,
// vae_mixture.hip): weights pi[K], means m[K,L], covariances S[K,L,L] (f64; kind MIX_DIAG: variances [K,L]), the lower Cholesky
// factor C_k (S_k = C_k C_k^T), its inverse W_k = C_k^-1 (f64, and an f32 copy for the pairwise kernels) and
// logdet_k = -sum_d log C_k[d,d] = log det W_k.
//   mix_factor_kernel       one workgroup per component, f64, packed lower triangles of C and W in LDS: Cholesky-Crout column by
//   mix_factor_diag_kernel  column, then W by forward substitution (one thread per column of W).  status[k] = 1-based index of the
//                           first pivot that is not > 0 (the pivot is then taken as 1, so every output stays finite), else 0.
//   mix_estep_full_kernel   q_nk = |W_k (x_n - m_k)|^2 for 64 points per workgroup: per component one [64 x L].[L x L] product on the
//                           exact-f32 MFMA (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain).  x sits in LDS once; the A operand
//                           x - m_k is formed on the fly in f32 (no expanded quadratic form); W_k^T comes through LDS in tiles of 16
//                           output columns, only rows j <= d of the triangle; y is squared and summed straight from the
//                           accumulators and never written; the next tile is fetched into registers during the products.  One
//                           path for every L in 1..128.
//   mix_estep_diag_kernel   the same q for diagonal W: four lanes per point share the components, all of d walked in order in
//                           chunks of 32 through LDS (the lstat_joint_kernel pattern with K components in place of n).
//                           Both end in mix_estep_finish: log p_nk = log pi_k + logdet_k - L/2 log 2 pi - q/2 and the logsumexp
//                           over k in f64, log_resp in f32, and the block's sum of log_prob in point order.
//   mix_mean_kernel         the block sums added in block order (a fixed tree over 256 lanes), divided by n.
//   mix_msums_kernel        M-step, both kinds: per (split, component) N_k = sum r and sum r x (PASS 1), or for MIX_DIAG the
//                           centred sum r (x - m)^2 (PASS 2); r = exp(log_resp) in f64, cast once to f32 for the products.
//   mix_mmeans_kernel       merges PASS 1 in split order: N_k (+ 10 eps_f64), pi = N_k / n, m = sum r x / N_k.
//   mix_msyrk_kernel        M-step, full: sum_n r (x - m)(x - m)^T about the NEW mean (a centred second pass loses nothing to
//                           cancellation) as a weighted SYRK on the exact-f32 MFMA, A = r d, B = d; each wave owns lower-triangle
//                           16x16 tiles; the next 64-point chunk is fetched into registers during the products.
//   mix_mcov_kernel         merges the splits in split order in f64, divides by N_k, adds reg_covar on the diagonal, mirrors.
//   mix_sample_kernel       draw i: u_i picks the first k whose f64 cumulative weight exceeds u (the last takes the remainder);
//                           z_i = m_k + temperature C_k eps_i accumulated in f64, rounded once.
// ACCUMULATION.  Every M-step product is f32; products are accumulated in f32 over at most MIX_ACC_POINTS = 64 points and in f64
// beyond that (the SYRK's MFMA chain runs over one 64-point chunk, then its accumulators are added to f64 ones).
// GENERATOR.  The sampler uses counter streams MIX_STREAM_U = 811 (uniforms that pick the component, counter i) and
// MIX_STREAM_EPS = 812 (normals, counter i * L + d) - nothing else uses them (5, 6, 7, 99, 123, 777 and 901 are taken).
// No atomics anywhere; every reduction runs in an order that depends on the shape only, so repeated calls give the same bits.
#pragma once
#include "edge_kernels.cuh"

constexpr int MIX_FULL = 0, MIX_DIAG = 1;
constexpr int MIX_MAX_K = 64;
constexpr int MIX_MAX_L_FULL = 128;
constexpr int MIX_MAX_L_DIAG = 4096;
constexpr int MIX_ACC_POINTS = 64;          // f32 accumulation length of the M-step
constexpr int MIX_PTS = 64;                 // points per workgroup, E-step
constexpr int MIX_XS = 132;                 // LDS stride of a point's x in the E-step: 16 points x 4 columns hit 64 banks
constexpr int MIX_DS = 144;                 // LDS stride of a point's centred x in the SYRK: 4 points x 16 columns hit 64 banks
constexpr int MIX_DCH = 32;                 // dimensions per LDS chunk, diagonal E-step
constexpr int MIX_DXS = 36;                 // and its point stride
constexpr unsigned long long MIX_STREAM_U = 811ULL, MIX_STREAM_EPS = 812ULL;
#define MIX_LOG2PI 1.8378770664093453
#define MIX_TINY 2.220446049250313e-15      // 10 eps_f64, added to every N_k

__device__ __forceinline__ int mix_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// ---- factor ------------------------------------------------------------------------------------------------------------------
// sticky: a non-zero status[k] from an earlier call is kept (the EM loop zeroes it once and reads it once at the end).
static __global__ __launch_bounds__(256) void mix_factor_kernel(const double* __restrict__ S, int L, double* __restrict__ Cout,
                                                                double* __restrict__ Wout, float* __restrict__ W32,
                                                                double* __restrict__ logdet, int* __restrict__ status, int sticky) {
    extern __shared__ __attribute__((aligned(16))) char mix_smem[];
    double* Cp = reinterpret_cast<double*>(mix_smem);   // packed lower triangle of C
    double* Wp = Cp + L * (L + 1) / 2;                  // packed lower triangle of W
    __shared__ int s_bad;
    const int k = blockIdx.x, tid = threadIdx.x;
    const double* Sk = S + (size_t)k * L * L;
    if (tid == 0) s_bad = 0;
    for (int e = tid; e < L * L; e += 256) {
        const int i = e / L, j = e - i * L;
        if (j <= i) Cp[mix_tri(i, j)] = Sk[e];
    }
    __syncthreads();
    for (int j = 0; j < L; ++j) {
        // column j: C[i][j] = (S[i][j] - sum_{l<j} C[i][l] C[j][l]) / C[j][j], rows i >= j in parallel
        double v = 0.0;
        const int i = j + tid;
        if (i < L) {
            v = Cp[mix_tri(i, j)];
            const double* ri = Cp + mix_tri(i, 0);
            const double* rj = Cp + mix_tri(j, 0);
            double v1 = 0.0, v2 = 0.0, v3 = 0.0;          // four chains: the LDS reads of a step do not wait for the one before
            int l = 0;
            for (; l + 3 < j; l += 4) { v -= ri[l] * rj[l]; v1 -= ri[l + 1] * rj[l + 1]; v2 -= ri[l + 2] * rj[l + 2]; v3 -= ri[l + 3] * rj[l + 3]; }
            for (; l < j; ++l) v -= ri[l] * rj[l];
            v = (v + v1) + (v2 + v3);
        }
        if (tid == 0) {
            if (!(v > 0.0)) { if (!s_bad) s_bad = j + 1; v = 1.0; }
            Cp[mix_tri(j, j)] = sqrt(v);
        }
        __syncthreads();
        if (i < L && tid > 0) Cp[mix_tri(i, j)] = v / Cp[mix_tri(j, j)];
        __syncthreads();
    }
    // W = C^-1: column c, rows i = c..L-1 in order; W[i][c] = (delta_ic - sum_{l=c}^{i-1} C[i][l] W[l][c]) / C[i][i]
    for (int c = tid; c < L; c += 256) {
        for (int i = c; i < L; ++i) {
            double v = i == c ? 1.0 : 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
            const double* ri = Cp + mix_tri(i, 0);
            int l = c, o = mix_tri(c, c);                 // o = mix_tri(l, c): the next row's entry is l + 1 further on
            for (; l + 3 < i; l += 4) {
                const int o1 = o + l + 1, o2 = o1 + l + 2, o3 = o2 + l + 3;
                v -= ri[l] * Wp[o]; v1 -= ri[l + 1] * Wp[o1]; v2 -= ri[l + 2] * Wp[o2]; v3 -= ri[l + 3] * Wp[o3];
                o = o3 + l + 4;
            }
            for (; l < i; ++l) { v -= ri[l] * Wp[o]; o += l + 1; }
            Wp[mix_tri(i, c)] = ((v + v1) + (v2 + v3)) / ri[i];
        }
    }
    __syncthreads();
    double* Ck = Cout + (size_t)k * L * L;
    double* Wk = Wout + (size_t)k * L * L;
    float* Wf = W32 + (size_t)k * L * L;
    for (int e = tid; e < L * L; e += 256) {
        const int i = e / L, j = e - i * L;
        const double c = j <= i ? Cp[mix_tri(i, j)] : 0.0, w = j <= i ? Wp[mix_tri(i, j)] : 0.0;
        Ck[e] = c; Wk[e] = w; Wf[e] = (float)w;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int d = 0; d < L; ++d) s += log(Cp[mix_tri(d, d)]);
        logdet[k] = -s;
        status[k] = (sticky && status[k]) ? status[k] : s_bad;
    }
}

static __global__ __launch_bounds__(256) void mix_factor_diag_kernel(const double* __restrict__ var, int L, double* __restrict__ Cout,
                                                                     double* __restrict__ Wout, float* __restrict__ W32,
                                                                     double* __restrict__ logdet, int* __restrict__ status, int sticky) {
    __shared__ double red[256];
    __shared__ int bad[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    int b = 0;
    for (int d = tid; d < L; d += 256) {
        double v = var[(size_t)k * L + d];
        if (!(v > 0.0)) { if (!b) b = d + 1; v = 1.0; }
        const double c = sqrt(v), w = 1.0 / c;
        Cout[(size_t)k * L + d] = c; Wout[(size_t)k * L + d] = w; W32[(size_t)k * L + d] = (float)w;
        s += log(c);
    }
    red[tid] = s; bad[tid] = b ? b : 0x7fffffff;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[tid] += red[tid + o]; bad[tid] = min(bad[tid], bad[tid + o]); }
        __syncthreads();
    }
    if (tid == 0) {
        logdet[k] = -red[0];
        const int nb = bad[0] == 0x7fffffff ? 0 : bad[0];
        status[k] = (sticky && status[k]) ? status[k] : nb;
    }
}

// ---- E-step ------------------------------------------------------------------------------------------------------------------
struct MixEArgs {
    const float* x; long n; int L, K;
    const double* pi; const double* m; const float* w32; const double* logdet;
    double* log_prob; float* log_resp; double* block_sum;   // log_resp may be null; block_sum [gridDim.x]
};

// qs[p * K + k] holds q of the block's point p: four lanes per point share the components.  Fixed order throughout.
__device__ __forceinline__ void mix_estep_finish(const MixEArgs& a, const float* qs, double* cs, double* lps, long p0) {
    const int tid = threadIdx.x, p = tid >> 2, sub = tid & 3;
    for (int k = tid; k < a.K; k += 256) cs[k] = log(a.pi[k]) + a.logdet[k] - 0.5 * a.L * MIX_LOG2PI;
    __syncthreads();
    const long n = p0 + p;
    double mx = -INFINITY;
    for (int k = sub; k < a.K; k += 4) mx = fmax(mx, cs[k] - 0.5 * (double)qs[p * a.K + k]);
    mx = fmax(mx, __shfl_xor(mx, 1)); mx = fmax(mx, __shfl_xor(mx, 2));
    if (!(mx > -INFINITY)) mx = 0.0;                       // every component at -inf: the sum below is 0, log_prob -inf
    double s = 0.0;
    for (int k = sub; k < a.K; k += 4) s += exp(cs[k] - 0.5 * (double)qs[p * a.K + k] - mx);
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2);
    const double lse = mx + log(s);
    if (n < a.n) {
        if (sub == 0) a.log_prob[n] = lse;
        if (a.log_resp)
            for (int k = sub; k < a.K; k += 4) a.log_resp[n * a.K + k] = (float)(cs[k] - 0.5 * (double)qs[p * a.K + k] - lse);
    }
    if (sub == 0) lps[p] = n < a.n ? lse : 0.0;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < MIX_PTS; ++i) t += lps[i];
        a.block_sum[blockIdx.x] = t;
    }
}

static __global__ __launch_bounds__(256) void mix_estep_full_kernel(MixEArgs a) {
    __shared__ float xs[MIX_PTS * MIX_XS];        // the block's points, columns >= L zero             33 KiB
    __shared__ float wt[MIX_MAX_L_FULL * 16];     // W_k^T tile: wt[j * 16 + dd] = W_k[d0 + dd][j]       8 KiB
    __shared__ float ms[MIX_MAX_L_FULL];          // (float) m_k, zero past L
    __shared__ float qs[MIX_PTS * MIX_MAX_K];     //                                                    16 KiB
    __shared__ double cs[MIX_MAX_K];
    __shared__ double lps[MIX_PTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
    const int L = a.L, K = a.K;
    const long p0 = (long)blockIdx.x * MIX_PTS;
    const int Lp = (L + 3) & ~3;
    // Global loads go out in batches with nothing that waits between them: a select on a loaded value would make the next load wait,
    // so every load is issued (from a valid address) and the selects follow the batch.
    for (int b = 0; b < MIX_PTS * MIX_MAX_L_FULL / 256; b += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + (b + u) * 256, p = e >> 7, j = e & 127;
            v[u] = a.x[(p0 + p < a.n && j < L) ? (p0 + p) * L + j : 0];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + (b + u) * 256, p = e >> 7, j = e & 127;
            xs[p * MIX_XS + j] = (p0 + p < a.n && j < L) ? v[u] : 0.f;
        }
    }
    const int ndt = (L + 15) >> 4;
    const float* xrow = xs + (wave * 16 + r) * MIX_XS + h;   // A operand: point wave*16 + r, column 4s + h
    // The W_k^T tile of (component k, column tile dt): at most 8 elements a thread, fetched into registers while the tile before it is
    // multiplied and put into LDS after it; with the first tile of a component comes its mean.
    float wv[8];
    double mv = 0.0;
    auto fetch_tile = [&](int k, int dt) {
        const int d0 = dt * 16, jend = min(Lp, d0 + 16);     // rows j <= d of the triangle, padded to whole MFMA steps
        const float* Wk = a.w32 + (size_t)k * L * L;
        if (dt == 0 && tid < MIX_MAX_L_FULL) mv = a.m[(size_t)k * L + (tid < L ? tid : 0)];
#pragma unroll
        for (int u = 0; u < 8; ++u) {                        // element (dd, j) of a [16][128] frame, j fastest: rows of W are contiguous
            const int e = tid + u * 256, dd = e >> 7, j = e & 127, d = d0 + dd;   // (no division by jend: it is no power of two)
            wv[u] = Wk[(j < jend && d < L && j <= d) ? (size_t)d * L + j : 0];
        }
    };
    auto put_tile = [&](int dt) {
        const int d0 = dt * 16, jend = min(Lp, d0 + 16);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + u * 256, dd = e >> 7, j = e & 127, d = d0 + dd;
            if (j < jend) wt[j * 16 + dd] = (d < L && j <= d) ? wv[u] : 0.f;
        }
    };
    fetch_tile(0, 0);
    for (int k = 0; k < K; ++k) {
        __syncthreads();                                     // ms (and, k = 0: xs) of the previous component consumed / written
        if (tid < MIX_MAX_L_FULL) ms[tid] = tid < L ? (float)mv : 0.f;
        float qp[4] = {0.f, 0.f, 0.f, 0.f};
        for (int dt = 0; dt < ndt; ++dt) {
            const int d0 = dt * 16, jend = min(Lp, d0 + 16);
            __syncthreads();                                 // the previous tile has been read (first tile: ms is visible after the next barrier)
            put_tile(dt);
            __syncthreads();
            if (dt + 1 < ndt) fetch_tile(k, dt + 1);
            else if (k + 1 < K) fetch_tile(k + 1, 0);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < jend; j0 += 4) {
                const float av = xrow[j0] - ms[j0 + h];
                const float bv = wt[(j0 + h) * 16 + r];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) qp[i] = fmaf(acc[i], acc[i], qp[i]);   // y[point 4h + i][d0 + r], squared
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                        // sum over the 16 columns a row's lanes hold
            float v = qp[i];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
            if (r == 0) qs[(wave * 16 + 4 * h + i) * K + k] = v;
        }
    }
    __syncthreads();
    mix_estep_finish(a, qs, cs, lps, p0);
}

static __global__ __launch_bounds__(256) void mix_estep_diag_kernel(MixEArgs a) {
    __shared__ float xs[MIX_PTS * MIX_DXS];
    __shared__ float2 mw[MIX_MAX_K * MIX_DCH];    // (m, w) of the chunk
    __shared__ float qs[MIX_PTS * MIX_MAX_K];
    __shared__ double cs[MIX_MAX_K];
    __shared__ double lps[MIX_PTS];
    const int tid = threadIdx.x, p = tid >> 2, sub = tid & 3;
    const int L = a.L, K = a.K;
    const long p0 = (long)blockIdx.x * MIX_PTS;
    float qa[MIX_MAX_K / 4];
#pragma unroll
    for (int kk = 0; kk < MIX_MAX_K / 4; ++kk) qa[kk] = 0.f;
    for (int d0 = 0; d0 < L; d0 += MIX_DCH) {
        const int dl = min(MIX_DCH, L - d0);
        __syncthreads();
        for (int e = tid; e < MIX_PTS * MIX_DCH; e += 256) {
            const int pp = e >> 5, dd = e & 31;
            xs[pp * MIX_DXS + dd] = (p0 + pp < a.n && dd < dl) ? a.x[(p0 + pp) * L + d0 + dd] : 0.f;
        }
        for (int e = tid; e < K * MIX_DCH; e += 256) {
            const int k = e >> 5, dd = e & 31;
            mw[e] = dd < dl ? make_float2((float)a.m[(size_t)k * L + d0 + dd], a.w32[(size_t)k * L + d0 + dd]) : make_float2(0.f, 0.f);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MIX_MAX_K / 4; ++kk) {
            const int k = kk * 4 + sub;
            if (k < K) {
                float q = qa[kk];
                for (int dd = 0; dd < dl; ++dd) {
                    const float2 c = mw[k * MIX_DCH + dd];
                    const float y = (xs[p * MIX_DXS + dd] - c.x) * c.y;
                    q = fmaf(y, y, q);
                }
                qa[kk] = q;
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < MIX_MAX_K / 4; ++kk)
        if (kk * 4 + sub < K) qs[p * K + kk * 4 + sub] = qa[kk];
    __syncthreads();
    mix_estep_finish(a, qs, cs, lps, p0);
}

// out[0] = (sum of part[0..n_part) in a fixed order) / n
static __global__ __launch_bounds__(256) void mix_mean_kernel(const double* __restrict__ part, long n_part, double n, double* __restrict__ out) {
    __shared__ double red[256];
    double t = 0.0;
    for (long i = threadIdx.x; i < n_part; i += 256) t += part[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0] / n;
}

// ---- M-step ------------------------------------------------------------------------------------------------------------------
// grid (splits, K, ceil(L / 128)), 128 threads: thread d of the tile.  PASS 1: part_n[split][k] = sum r, part_v[split][k][d] = sum r x.
// PASS 2 (MIX_DIAG): part_v[split][k][d] = sum r (x - m)^2 about the new mean m.
template <int PASS>
static __global__ __launch_bounds__(128) void mix_msums_kernel(const float* __restrict__ log_resp, const float* __restrict__ x, long n,
                                                               int L, int K, long per, const double* __restrict__ mean,
                                                               double* __restrict__ part_n, double* __restrict__ part_v) {
    __shared__ float r32[MIX_ACC_POINTS];
    __shared__ double r64[MIX_ACC_POINTS];
    const int tid = threadIdx.x, k = blockIdx.y, d = blockIdx.z * 128 + tid, split = blockIdx.x;
    const long n0 = min(n, split * per), n1 = min(n, n0 + per);
    const float mf = (PASS == 2 && d < L) ? (float)mean[(size_t)k * L + d] : 0.f;
    double acc = 0.0, cnt = 0.0;
    for (long c0 = n0; c0 < n1; c0 += MIX_ACC_POINTS) {
        const int cn = (int)min((long)MIX_ACC_POINTS, n1 - c0);
        __syncthreads();
        if (tid < cn) {
            const double rr = exp((double)log_resp[(c0 + tid) * K + k]);
            r64[tid] = rr; r32[tid] = (float)rr;
        }
        __syncthreads();
        if (d < L) {
            float t = 0.f;
            for (int i = 0; i < cn; ++i) {
                const float xv = x[(c0 + i) * L + d];
                if (PASS == 1) t = fmaf(r32[i], xv, t);
                else { const float df = xv - mf; t = fmaf(r32[i] * df, df, t); }
            }
            acc += (double)t;
        }
        if (PASS == 1 && tid == 0 && blockIdx.z == 0)
            for (int i = 0; i < cn; ++i) cnt += r64[i];
    }
    if (d < L) part_v[((size_t)split * K + k) * L + d] = acc;
    if (PASS == 1 && tid == 0 && blockIdx.z == 0) part_n[(size_t)split * K + k] = cnt;
}

// one block per component: N_k, pi_k and m_k from the splits in split order
static __global__ __launch_bounds__(256) void mix_mmeans_kernel(const double* __restrict__ part_n, const double* __restrict__ part_v,
                                                                int splits, int K, int L, double n, double* __restrict__ Nk,
                                                                double* __restrict__ pi, double* __restrict__ mean) {
    const int k = blockIdx.x;
    double N = 0.0;
    for (int s = 0; s < splits; ++s) N += part_n[(size_t)s * K + k];
    N += MIX_TINY;
    if (threadIdx.x == 0) { Nk[k] = N; pi[k] = N / n; }
    for (int d = threadIdx.x; d < L; d += 256) {
        double v = 0.0;
        for (int s = 0; s < splits; ++s) v += part_v[((size_t)s * K + k) * L + d];
        mean[(size_t)k * L + d] = v / N;
    }
}

// MIX_DIAG: var[k][d] = sum over the splits of PASS 2 / N_k + reg
static __global__ __launch_bounds__(256) void mix_mvar_kernel(const double* __restrict__ part_v, int splits, int K, int L,
                                                              const double* __restrict__ Nk, double reg, double* __restrict__ var) {
    const int k = blockIdx.x;
    for (int d = threadIdx.x; d < L; d += 256) {
        double v = 0.0;
        for (int s = 0; s < splits; ++s) v += part_v[((size_t)s * K + k) * L + d];
        var[(size_t)k * L + d] = v / Nk[k] + reg;
    }
}

// grid (splits, K), 256 threads; NT = ceil(L / 16) tile rows, T = NT (NT + 1) / 2 tiles, wave w owns tiles w, w + 4, ...
// part[split][k][a][b] (a >= b within the tiles owned; the upper halves of the diagonal tiles are written too, mirrored later).
template <int NT>
static __global__ __launch_bounds__(256) void mix_msyrk_kernel(const float* __restrict__ log_resp, const float* __restrict__ x, long n,
                                                               int L, int K, long per, const double* __restrict__ mean,
                                                               double* __restrict__ part) {
    constexpr int T = NT * (NT + 1) / 2, TPW = (T + 3) / 4;
    __shared__ float ds[MIX_ACC_POINTS * MIX_DS];   // x - m_k of the chunk, zero past L and past the range   36 KiB
    __shared__ float rs[MIX_ACC_POINTS];
    __shared__ float ms[NT * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
    const int k = blockIdx.y, split = blockIdx.x;
    const long n0 = min(n, split * per), n1 = min(n, n0 + per);
    if (tid < NT * 16) ms[tid] = tid < L ? (float)mean[(size_t)k * L + tid] : 0.f;
    double acc[TPW][4];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i] = 0.0;
    // A chunk's x and log_resp are fetched into registers while the chunk before it is multiplied (every load issued, from a valid
    // address, the selects at the store: see mix_estep_full_kernel) and centred into LDS after it.
    constexpr int NLD = MIX_ACC_POINTS * NT * 16 / 256;
    float pv[NLD], lrv = 0.f;
    auto fetch = [&](long c0, int cn) {
        if (tid < MIX_ACC_POINTS) lrv = log_resp[(c0 + (tid < cn ? tid : 0)) * K + k];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int e = tid + u * 256, i = e / (NT * 16), d = e - i * (NT * 16);
            pv[u] = x[(i < cn && d < L) ? (c0 + i) * L + d : c0 * L];
        }
    };
    if (n0 < n1) fetch(n0, (int)min((long)MIX_ACC_POINTS, n1 - n0));
    for (long c0 = n0; c0 < n1; c0 += MIX_ACC_POINTS) {
        const int cn = (int)min((long)MIX_ACC_POINTS, n1 - c0);
        __syncthreads();                                 // the previous chunk has been read (first: ms written)
        if (tid < MIX_ACC_POINTS) rs[tid] = tid < cn ? (float)exp((double)lrv) : 0.f;
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int e = tid + u * 256, i = e / (NT * 16), d = e - i * (NT * 16);
            ds[i * MIX_DS + d] = (i < cn && d < L) ? pv[u] - ms[d] : 0.f;
        }
        __syncthreads();
        {   // the next chunk; after the last one the same again, unused
            const long cx = c0 + MIX_ACC_POINTS < n1 ? c0 + MIX_ACC_POINTS : c0;
            fetch(cx, (int)min((long)MIX_ACC_POINTS, n1 - cx));
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int tile = wave + 4 * t;               // tile -> (row tile ta, column tile tb), row-major over the triangle
            if (tile < T) {
                int ta = 0;
                while ((ta + 1) * (ta + 2) / 2 <= tile) ++ta;
                const int tb = tile - ta * (ta + 1) / 2;
                f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int s = 0; s < MIX_ACC_POINTS / 4; ++s) {
                    const int i = 4 * s + h;
                    const float av = rs[i] * ds[i * MIX_DS + ta * 16 + r];
                    const float bv = ds[i * MIX_DS + tb * 16 + r];
                    c = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[t][i] += (double)c[i];
            }
        }
    }
    double* out = part + ((size_t)split * K + k) * L * L;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tile = wave + 4 * t;
        if (tile < T) {
            int ta = 0;
            while ((ta + 1) * (ta + 2) / 2 <= tile) ++ta;
            const int tb = tile - ta * (ta + 1) / 2;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ra = ta * 16 + 4 * h + i, cb = tb * 16 + r;
                if (ra < L && cb < L) out[(size_t)ra * L + cb] = acc[t][i];
            }
        }
    }
}

// S[k][a][b] = sum over the splits of part[.][k][max(a,b)][min(a,b)] / N_k + reg [a == b]; grid (ceil(L*L / 256), K)
static __global__ __launch_bounds__(256) void mix_mcov_kernel(const double* __restrict__ part, int splits, int K, int L,
                                                              const double* __restrict__ Nk, double reg, double* __restrict__ S) {
    const int k = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= L * L) return;
    const int a = e / L, b = e - a * L, hi = max(a, b), lo = min(a, b);
    double v = 0.0;
    for (int s = 0; s < splits; ++s) v += part[(((size_t)s * K + k) * L + hi) * L + lo];
    S[(size_t)k * L * L + e] = v / Nk[k] + (a == b ? reg : 0.0);
}

// ---- sample ------------------------------------------------------------------------------------------------------------------
struct MixSArgs {
    long n; int L, K, kind;
    const double* pi; const double* m; const double* chol;
    double temperature; unsigned long long seed;
    const double* u; const float* eps;               // optional explicit draws: u [n], eps [n, L]
    float* z; int* component;
};
constexpr int MIX_SDRAWS = 8;                        // draws per block pass, full covariance

__device__ __forceinline__ int mix_pick(const double* cum, int K, double u) {
    int k = 0;
    while (k < K - 1 && !(cum[k] > u)) ++k;          // the last component takes the remainder
    return k;
}

static __global__ __launch_bounds__(256) void mix_sample_kernel(MixSArgs a) {
    __shared__ double cum[MIX_MAX_K];
    __shared__ float es[MIX_SDRAWS * MIX_MAX_L_FULL];
    __shared__ int comp[MIX_SDRAWS];
    const int tid = threadIdx.x, L = a.L, K = a.K;
    if (tid == 0) {
        double c = 0.0;
        for (int k = 0; k < K; ++k) { c += a.pi[k]; cum[k] = c; }
    }
    __syncthreads();
    if (a.kind == MIX_DIAG) {                        // elementwise: every thread picks its draw's component itself
        const long total = a.n * L;
        for (long e = (long)blockIdx.x * 256 + tid; e < total; e += (long)gridDim.x * 256) {
            const long i = e / L;
            const int d = (int)(e - i * L);
            const double uu = a.u ? a.u[i] : counter_uniform((unsigned long long)i, a.seed, MIX_STREAM_U);
            const int k = mix_pick(cum, K, uu);
            const float ev = a.eps ? a.eps[e] : counter_normal_at((unsigned long long)e, a.seed, MIX_STREAM_EPS);
            a.z[e] = (float)(a.m[(size_t)k * L + d] + a.temperature * (a.chol[(size_t)k * L + d] * (double)ev));
            if (d == 0) a.component[i] = k;
        }
        return;
    }
    const long passes = (a.n + MIX_SDRAWS - 1) / MIX_SDRAWS;
    for (long ps = blockIdx.x; ps < passes; ps += gridDim.x) {
        const long i0 = ps * MIX_SDRAWS;
        const int cn = (int)min((long)MIX_SDRAWS, a.n - i0);
        __syncthreads();                             // the previous pass has been read
        if (tid < cn) {
            const long i = i0 + tid;
            const double uu = a.u ? a.u[i] : counter_uniform((unsigned long long)i, a.seed, MIX_STREAM_U);
            const int k = mix_pick(cum, K, uu);
            comp[tid] = k; a.component[i] = k;
        }
        for (int e = tid; e < cn * L; e += 256) {
            const long g = i0 * L + e;
            const int ii = e / L, d = e - ii * L;
            es[ii * MIX_MAX_L_FULL + d] = a.eps ? a.eps[g] : counter_normal_at((unsigned long long)g, a.seed, MIX_STREAM_EPS);
        }
        __syncthreads();
        for (int e = tid; e < cn * L; e += 256) {
            const int ii = e / L, d = e - ii * L, k = comp[ii];
            const double* row = a.chol + ((size_t)k * L + d) * L;
            double s = 0.0;
            for (int j = 0; j <= d; ++j) s += row[j] * (double)es[ii * MIX_MAX_L_FULL + j];
            a.z[i0 * L + e] = (float)(a.m[(size_t)k * L + d] + a.temperature * s);
        }
    }
}
