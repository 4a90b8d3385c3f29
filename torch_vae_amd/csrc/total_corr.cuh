// Total correlation of a TRAINING batch and its gradient (beta-TCVAE, Chen et al. 2018; vae_total_correlation and the VAE_KL_TC
// objective, vae_api.hip).  From the forward's f32 mu, log_var and eps [B][L], in nats:
//   z_i = mu_i + eps_i exp(lv_i / 2),   a(i,j,d) = -1/2 (log 2 pi + lv_jd + (z_id - mu_jd)^2 e^{-lv_jd})
//   log q(z_i) = logsumexp_j sum_d a - log B,   log q(z_id) = logsumexp_j a - log B      (the query's own component included)
//   TC = 1/B sum_i [log q(z_i) - sum_d log q(z_id)]
// latent_stats.cuh computes the same quantity for diagnostics over thousands of posteriors (a lane owns 4 queries, splits hold at
// least 256 components, no backward); here N = B is a few hundred, so the pairs themselves are the parallel axis.  Base 2 throughout
// (every a pre-scaled by log2 e: one v_exp_f32 per exponential).  Launches, in order:
//   tc_prep_kernel   one wave per row j: z, hw = -1/2 log2e e^{-lv}, c2 = -1/2 log2e (log 2 pi + lv) [B][L], cj = sum_d c2 (f64)
//   tc_pair_kernel   one thread per pair (i,j), 16x16 tiles staged through LDS: A[i][j] = sum_d a(i,j,d).  (z - mu)^2 e^{-lv} is
//                    formed directly (no expanded quadratic form, which cancels for narrow posteriors); TC_DC terms are summed in f32,
//                    the chunks and the constant in f64, so the only rounding at the magnitude of A is the final one to f32
//   tc_row_kernel    one wave per query i: lse_i = log2 sum_j 2^A[i][j], online maximum from -1e30 (follows the data: finite even when
//                    every component but the query's own underflows), lanes merged by a butterfly
//   tc_query_kernel  one lane per (i,d), the components split over the workgroup's TC_JS waves.  Pass 1: the per-dimension online
//                    logsumexp lsed_id, the waves' (max, sum) pairs merged in wave order; pass 2: gz_id = dTC/dz_id.  Wave 0 also
//                    leaves the f64 sum of its 64 lsed values for the scalar
//   tc_comp_kernel   one lane per (j,d), the queries split the same way: dTC/dmu_jd, dTC/dlv_jd through the mixture components,
//                    plus the chain terms of gz_jd (z_j depends on mu_j and lv_j)
//   tc_final_kernel  one workgroup: TC in f64, thread-strided sums and a fixed tree; T = KL + (tc_weight - 1) TC into the
//                    objective's scalar slot when there is one
// With w_ij = 2^(A_ij - lse_i), w_ijd = 2^(a_ijd - lsed_id), u = (w_ij - w_ijd)/B, r = z_id - mu_jd, v = e^{-lv_jd}:
//   gz_id = sum_j u (-r v),   gmu_jd = sum_i u r v + gz_jd,   glv_jd = sum_i u (r^2 v - 1)/2 + gz_jd eps_jd exp(lv_jd / 2)/2
// Every sum runs in a fixed order and nothing is accumulated with atomics: repeated calls are bit-identical.  The latents are f32
// whatever the storage type, so there is one instantiation.
#pragma once
#include "edge_kernels.cuh"

#define TC_LOG2E 1.4426950408889634
#define TC_LN2 0.6931471805599453
#define TC_LOG2PI 1.8378770664093453   // log(2 pi)
constexpr int TC_MAX_B = 4096;   // A is [B][B] f32: 64 MiB at the limit
constexpr int TC_TILE = 16;      // pair kernel: 16 x 16 pairs per workgroup
constexpr int TC_DL = 64;        // pair kernel: dimensions per LDS stage
constexpr int TC_DC = 8;         // pair kernel: dimensions per f32 chunk
constexpr int TC_JS = 4;         // query / component kernels: waves (loop slices) per workgroup
constexpr int TC_EL = 64;        // query / component kernels: (row, d) elements per workgroup, one per lane

// Work space of one evaluation, carved from one allocation (256-byte aligned pieces)
struct TcWork {
    float *z, *hw, *c2, *A, *lse, *lsed, *gz;
    double *cj, *part, *tc;
    int npart;
};
static inline size_t tc_carve(void* base, int B, int L, TcWork* w) {
    const size_t bl = (size_t)B * L;
    const int npart = (int)((bl + TC_EL - 1) / TC_EL);
    const size_t sz[10] = {bl * 4, bl * 4, bl * 4, (size_t)B * B * 4, (size_t)B * 4, bl * 4, bl * 4, (size_t)B * 8, (size_t)npart * 8, 8};
    size_t off[10], tot = 0;
    for (int k = 0; k < 10; ++k) { off[k] = tot; tot += (sz[k] + 255) / 256 * 256; }
    if (w) {
        char* p = static_cast<char*>(base);
        w->z = reinterpret_cast<float*>(p + off[0]); w->hw = reinterpret_cast<float*>(p + off[1]); w->c2 = reinterpret_cast<float*>(p + off[2]);
        w->A = reinterpret_cast<float*>(p + off[3]); w->lse = reinterpret_cast<float*>(p + off[4]); w->lsed = reinterpret_cast<float*>(p + off[5]);
        w->gz = reinterpret_cast<float*>(p + off[6]); w->cj = reinterpret_cast<double*>(p + off[7]); w->part = reinterpret_cast<double*>(p + off[8]);
        w->tc = reinterpret_cast<double*>(p + off[9]); w->npart = npart;
    }
    return tot;
}

static __global__ __launch_bounds__(256) void tc_prep_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                             const float* __restrict__ eps, int B, int L, float* __restrict__ z,
                                                             float* __restrict__ hw, float* __restrict__ c2, double* __restrict__ cj) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= B) return;   // whole waves only
    double cs = 0.0;
    for (int d = lane; d < L; d += 64) {
        const size_t e = (size_t)j * L + d;
        const float m = mu[e], v = lv[e];
        const double c = -0.5 * TC_LOG2E * (TC_LOG2PI + (double)v);
        cs += c;
        hw[e] = (float)(-0.5 * TC_LOG2E * exp(-(double)v));
        c2[e] = (float)c;
        z[e] = eps[e] * expf(0.5f * v) + m;   // as latent_fwd_kernel forms it
    }
    for (int o = 32; o > 0; o >>= 1) cs += __shfl_xor(cs, o);
    if (lane == 0) cj[j] = cs;
}

// A[i][j], i = blockIdx.y * 16 + (tid >> 4), j = blockIdx.x * 16 + (tid & 15).  Rows past B are staged as zeros (hw = 0 adds 0).
static __global__ __launch_bounds__(256) void tc_pair_kernel(const float* __restrict__ z, const float* __restrict__ mu,
                                                             const float* __restrict__ hw, const double* __restrict__ cj, int B, int L,
                                                             float* __restrict__ A) {
    __shared__ float s_z[TC_TILE][TC_DL + 1], s_m[TC_TILE][TC_DL + 1], s_h[TC_TILE][TC_DL + 1];   // (+1: the 16 rows fall into 16 banks)
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = blockIdx.y * TC_TILE, j0 = blockIdx.x * TC_TILE;
    double acc = 0.0;
    for (int d0 = 0; d0 < L; d0 += TC_DL) {
        const int dl = min(TC_DL, L - d0);
        __syncthreads();
        for (int e = tid; e < TC_TILE * TC_DL; e += 256) {
            const int row = e / TC_DL, dd = e - row * TC_DL;
            const bool in = dd < dl;
            const bool qi = in && i0 + row < B, cjn = in && j0 + row < B;
            s_z[row][dd] = qi ? z[(size_t)(i0 + row) * L + d0 + dd] : 0.f;
            s_m[row][dd] = cjn ? mu[(size_t)(j0 + row) * L + d0 + dd] : 0.f;
            s_h[row][dd] = cjn ? hw[(size_t)(j0 + row) * L + d0 + dd] : 0.f;
        }
        __syncthreads();
        for (int dc = 0; dc < dl; dc += TC_DC) {   // (the stage is zero-padded to TC_DL, a multiple of TC_DC)
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < TC_DC; ++k) {
                const float df = s_z[ti][dc + k] - s_m[tj][dc + k];
                t = fmaf(df * df, s_h[tj][dc + k], t);
            }
            acc += (double)t;
        }
    }
    const int i = i0 + ti, j = j0 + tj;
    if (i < B && j < B) A[(size_t)i * B + j] = (float)(acc + cj[j]);
}

// (max, sum) of a base-2 online logsumexp: fold one exponent in, merge two states
__device__ __forceinline__ void tc_fold(float& m, float& s, float a) {
    if (a > m) { s = s * __builtin_amdgcn_exp2f(m - a) + 1.f; m = a; }
    else s += __builtin_amdgcn_exp2f(a - m);
}
__device__ __forceinline__ void tc_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = s * __builtin_amdgcn_exp2f(m - mn) + s2 * __builtin_amdgcn_exp2f(m2 - mn);
    m = mn;
}

static __global__ __launch_bounds__(256) void tc_row_kernel(const float* __restrict__ A, int B, float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;   // whole waves only
    float m = -1e30f, s = 0.f;
    for (int j = lane; j < B; j += 64) tc_fold(m, s, A[(size_t)i * B + j]);
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        tc_merge(m, s, m2, s2);
    }
    if (lane == 0) lse[i] = m + log2f(s);
}

struct TcSideArgs {
    const float* z; const float* mu; const float* hw; const float* c2; const float* A; const float* lse;
    float* lsed; float* gz;          // query kernel: written; component kernel: read
    const float* lv; const float* eps;
    double* part;                    // query kernel: f64 sum of the workgroup's lsed
    float* gmu; float* glv; int ldo; // component kernel: dTC/dmu, dTC/dlv at [j * ldo + d] (either may be null)
    int B, L, grad;                  // grad 0: the query kernel stops after pass 1
};

// Lane (i,d) = element blockIdx.x * 64 + lane; wave w of the workgroup takes components [w * per, (w + 1) * per).
static __global__ __launch_bounds__(256) void tc_query_kernel(TcSideArgs a) {
    __shared__ float s_m[TC_JS][TC_EL], s_s[TC_JS][TC_EL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long e = (long)blockIdx.x * TC_EL + lane, n = (long)a.B * a.L;
    const bool ok = e < n;
    const int i = ok ? (int)(e / a.L) : 0, d = ok ? (int)(e - (long)i * a.L) : 0;
    const int per = (a.B + TC_JS - 1) / TC_JS, j0 = w * per, j1 = min(a.B, j0 + per);
    const float zq = a.z[(size_t)i * a.L + d];
    float m = -1e30f, s = 0.f;
    for (int j = j0; j < j1; ++j) {
        const size_t at = (size_t)j * a.L + d;
        const float df = zq - a.mu[at];
        tc_fold(m, s, fmaf(df * df, a.hw[at], a.c2[at]));
    }
    s_m[w][lane] = m; s_s[w][lane] = s;
    __syncthreads();
    m = s_m[0][lane]; s = s_s[0][lane];
#pragma unroll
    for (int k = 1; k < TC_JS; ++k) tc_merge(m, s, s_m[k][lane], s_s[k][lane]);   // every wave merges in wave order: the same bits
    const float ld = m + log2f(s);
    if (w == 0) {
        if (ok) a.lsed[e] = ld;
        double p = ok ? (double)ld : 0.0;
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
        if (lane == 0) a.part[blockIdx.x] = p;
    }
    if (!a.grad) return;
    const float li = a.lse[i], invb = 1.f / (float)a.B;
    float g = 0.f;
    for (int j = j0; j < j1; ++j) {
        const size_t at = (size_t)j * a.L + d;
        const float h = a.hw[at], df = zq - a.mu[at];
        const float wd = __builtin_amdgcn_exp2f(fmaf(df * df, h, a.c2[at]) - ld);
        const float wj = __builtin_amdgcn_exp2f(a.A[(size_t)i * a.B + j] - li);
        g = fmaf((wj - wd) * invb, df * h, g);   // u * (-r v) in units of v = -2 ln2 hw: scaled below
    }
    __syncthreads();
    s_s[w][lane] = g;
    __syncthreads();
    if (w == 0 && ok) {
        float t = s_s[0][lane];
#pragma unroll
        for (int k = 1; k < TC_JS; ++k) t += s_s[k][lane];
        a.gz[e] = t * (float)(2.0 * TC_LN2);   // -r v = df * hw * 2 ln2
    }
}

// Lane (j,d) = element blockIdx.x * 64 + lane; wave w takes queries [w * per, (w + 1) * per).
static __global__ __launch_bounds__(256) void tc_comp_kernel(TcSideArgs a) {
    __shared__ float s_a[TC_JS][TC_EL], s_b[TC_JS][TC_EL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long e = (long)blockIdx.x * TC_EL + lane, n = (long)a.B * a.L;
    const bool ok = e < n;
    const int j = ok ? (int)(e / a.L) : 0, d = ok ? (int)(e - (long)j * a.L) : 0;
    const int per = (a.B + TC_JS - 1) / TC_JS, i0 = w * per, i1 = min(a.B, i0 + per);
    const size_t me = (size_t)j * a.L + d;
    const float mj = a.mu[me], h = a.hw[me], c = a.c2[me], invb = 1.f / (float)a.B;
    float gm = 0.f, gl = 0.f;   // sum_i u * (df hw), sum_i u * (df^2 hw)   (hw = -v log2e / 2)
    float us = 0.f;             // sum_i u
    for (int i = i0; i < i1; ++i) {
        const size_t at = (size_t)i * a.L + d;
        const float df = a.z[at] - mj, dd = df * df, q = dd * h;
        const float wd = __builtin_amdgcn_exp2f(fmaf(dd, h, c) - a.lsed[at]);   // the exponent as the query kernel formed it
        const float wj = __builtin_amdgcn_exp2f(a.A[(size_t)i * a.B + j] - a.lse[i]);
        const float u = (wj - wd) * invb;
        gm = fmaf(u, df * h, gm); gl = fmaf(u, q, gl); us += u;
    }
    s_a[w][lane] = gm; s_b[w][lane] = gl;
    __syncthreads();
    float tm = s_a[0][lane], tl = s_b[0][lane];
#pragma unroll
    for (int k = 1; k < TC_JS; ++k) { tm += s_a[k][lane]; tl += s_b[k][lane]; }
    __syncthreads();
    s_a[w][lane] = us;
    __syncthreads();
    if (w != 0 || !ok) return;
    float tu = s_a[0][lane];
#pragma unroll
    for (int k = 1; k < TC_JS; ++k) tu += s_a[k][lane];
    const float k2 = (float)(-2.0 * TC_LN2);   // r v = df hw * k2,  r^2 v = q * k2
    const float gzj = a.gz[me];
    if (a.gmu) a.gmu[(size_t)j * a.ldo + d] = tm * k2 + gzj;
    if (a.glv) a.glv[(size_t)j * a.ldo + d] = 0.5f * (tl * k2 - tu) + gzj * 0.5f * a.eps[me] * expf(0.5f * a.lv[me]);
}

// TC = ln2/B (sum_i lse_i - sum_id lsed_id) + (L - 1) ln B.  scal (null: none): [0] T = [1] KL + (tc_weight - 1) TC.
static __global__ __launch_bounds__(256) void tc_final_kernel(const float* __restrict__ lse, const double* __restrict__ part, int npart,
                                                              int B, int L, double* __restrict__ tc, double* scal, double tc_weight) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < B; i += 256) s += (double)lse[i];
    for (int k = tid; k < npart; k += 256) s -= part[k];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const double v = TC_LN2 * red[0] / (double)B + (double)(L - 1) * log((double)B);
        *tc = v;
        if (scal) scal[0] = scal[1] + (tc_weight - 1.0) * v;
    }
}
