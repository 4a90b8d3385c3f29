// Latent-space diagnostics (vae_latent_stats, vae_util.hip): the aggregate posterior q(z) = 1/N sum_j q(z|x_j) of N encoded rolls,
// evaluated at S draws z ~ q(z|x_i) per roll, whole (log q(z)) and per dimension (log q(z_d)).  From these and the analytic terms the
// f64 kernels at the end form KL, MI = I(x;z), TC and dimension-wise KL (beta-TCVAE decomposition, Chen et al. 2018), and the
// per-dimension moments behind active units (Burda et al. 2016).
//   a(z, j, d) = -1/2 (log 2 pi + lv[j,d] + (z - mu[j,d])^2 e^{-lv[j,d]})          log N(z; mu_jd, sigma_jd^2)
//   log_qz[q]        = logsumexp_j sum_d a(z_qd, j, d) - log N
//   log_qz_dims[q,d] = logsumexp_j a(z_qd, j, d) - log N
// The pairwise part runs in base 2 (every a pre-scaled by log2 e, so each exponential is one v_exp_f32) in two kernels with different
// lane maps, because the joint term sums over d BEFORE its exponential and the per-dimension terms exponentiate every d:
//   lstat_joint_kernel: a lane owns 4 queries and all of d; per tile of LS_JT components it accumulates the 4 x LS_JT sums over d in
//                       registers (3 VALU per triple, no exponential; chunks of LS_DC terms summed apart, the constant added last,
//                       which keeps the f32 sum within ~1e-5 nats at L = 128 even for sigma = e^-5), then folds them into an online
//                       (max, sum) state: one exp per (query, component) pair plus one rescale per tile.
//   lstat_dims_kernel:  a lane owns 4 queries of one dimension d; per component it forms a (3 VALU) and folds it into that dimension's
//                       online state in blocks of 8 (max, then one exp per triple and one rescale per block).
// Both read the components from LDS, shared by the lane's 4 queries so the LDS return path (128 B/clk/CU) stays well below the VALU
// rate.  The split does not depend on L: one lane per query with per-dimension state would need 2L registers, one lane per (query, d)
// for the joint term a cross-lane sum per component.  (z - mu)^2 e^{-lv} is formed directly in f32; no expanded quadratic form, which
// cancels for small sigma.  The online maximum starts at -1e30 (not -inf, so an empty or all -inf range stays NaN-free) and follows the
// data, so the result is finite even when every component but the query's own underflows.  The component range is split over
// gridDim.y; partial (max, sum) pairs are merged in split order in f64 (lstat_merge_kernel).  No atomics anywhere: repeated calls are
// bit-identical.
#pragma once
#include "edge_kernels.cuh"

#define LS_LOG2E 1.4426950408889634
#define LS_LN2 0.6931471805599453
#define LS_LOG2PI 1.8378770664093453
constexpr int LS_QR = 4;     // queries per lane (both pairwise kernels)
constexpr int LS_JT = 16;    // components per register tile, joint kernel
constexpr int LS_DL = 128;   // dimensions per LDS stage, joint kernel
constexpr int LS_DC = 8;     // dimensions per register chunk, joint kernel
constexpr int LS_JD = 32;    // components per LDS stage, dims kernel
constexpr int LS_DB = 64;    // max dimensions per block, dims kernel

// Per component i (one wave each): the base-2 tables mh[i,d] = (mu, -1/2 log2e e^{-lv}), c2[i,d] = -1/2 log2e (log 2 pi + lv) and
// cj[i] = sum_d c2[i,d]; and z[s,i,d] = eps * exp(0.5 lv) + mu for every draw s, formed as iw_latent_kernel forms it.  eps[(s*N+i)*L+d]
// comes from the caller or from stream 7 of the counter generator.
static __global__ __launch_bounds__(256) void lstat_prep_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                const float* __restrict__ eps, unsigned long long seed, int N, int L,
                                                                int S, float* __restrict__ z, float2* __restrict__ mh,
                                                                float* __restrict__ c2, float* __restrict__ cj) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;   // whole waves only
    double cs = 0.0;
    for (int d = lane; d < L; d += 64) {
        const long e0 = i * L + d;
        const float m = mu[e0], v = lv[e0];
        const double c = -0.5 * LS_LOG2E * (LS_LOG2PI + (double)v);
        cs += c;
        mh[e0] = make_float2(m, (float)(-0.5 * LS_LOG2E * exp(-(double)v)));
        c2[e0] = (float)c;
        const float sd = expf(0.5f * v);
        for (int s = 0; s < S; ++s) {
            const long g = ((long)s * N + i) * L + d;
            const float e = eps ? eps[g] : counter_normal_at((unsigned long long)g, seed, 7ULL);
            z[g] = e * sd + m;
        }
    }
    for (int o = 32; o > 0; o >>= 1) cs += __shfl_xor(cs, o);
    if (lane == 0) cj[i] = (float)cs;
}

// Joint term: lane owns queries q0 + r*64 (r < LS_QR) of its block's 256*LS_QR; components [j0, j1) of split blockIdx.y.
// part[blockIdx.y][q] = (max, sum) of the base-2 online logsumexp.
static __global__ __launch_bounds__(256) void lstat_joint_kernel(const float* __restrict__ z, const float2* __restrict__ mh,
                                                                 const float* __restrict__ cj, long SN, int N, int L, int jper,
                                                                 float2* __restrict__ part) {
    __shared__ float2 s_mh[LS_JT * LS_DL];
    __shared__ float s_c[LS_JT];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const long qb = (long)blockIdx.x * (256 * LS_QR) + (long)w * (64 * LS_QR) + lane;
    long q[LS_QR];
    bool live[LS_QR];
#pragma unroll
    for (int r = 0; r < LS_QR; ++r) { q[r] = qb + r * 64; live[r] = q[r] < SN; }
    const int j0 = blockIdx.y * jper, j1 = min(N, j0 + jper);
    float m[LS_QR], s[LS_QR];
#pragma unroll
    for (int r = 0; r < LS_QR; ++r) { m[r] = -1e30f; s[r] = 0.f; }
    for (int jt = j0; jt < j1; jt += LS_JT) {
        float acc[LS_QR][LS_JT];
        __syncthreads();
        if (tid < LS_JT) s_c[tid] = jt + tid < j1 ? cj[jt + tid] : -INFINITY;   // missing components: a = -inf
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < LS_JT; ++jj)
#pragma unroll
            for (int r = 0; r < LS_QR; ++r) acc[r][jj] = 0.f;
        for (int d0 = 0; d0 < L; d0 += LS_DL) {
            const int dl = min(LS_DL, L - d0);
            const int dlp = (dl + LS_DC - 1) / LS_DC * LS_DC;
            __syncthreads();
            for (int e = tid; e < LS_JT * dlp; e += 256) {
                const int jj = e / dlp, dd = e - jj * dlp, j = jt + jj;
                s_mh[jj * LS_DL + dd] = (j < j1 && dd < dl) ? mh[(long)j * L + d0 + dd] : make_float2(0.f, 0.f);
            }
            __syncthreads();
            for (int dc = 0; dc < dlp; dc += LS_DC) {
                float zc[LS_QR][LS_DC];
#pragma unroll
                for (int r = 0; r < LS_QR; ++r)
#pragma unroll
                    for (int k = 0; k < LS_DC; ++k) {
                        const int d = d0 + dc + k;
                        zc[r][k] = (live[r] && d < L) ? z[q[r] * L + d] : 0.f;   // padded d: mu = hw = 0, adds 0
                    }
#pragma unroll
                for (int jj = 0; jj < LS_JT; ++jj) {
                    float t[LS_QR];   // the chunk's LS_DC terms summed apart first: fewer roundings at the running sum's magnitude
#pragma unroll
                    for (int r = 0; r < LS_QR; ++r) t[r] = 0.f;
#pragma unroll
                    for (int k = 0; k < LS_DC; ++k) {
                        const float2 c = s_mh[jj * LS_DL + dc + k];
#pragma unroll
                        for (int r = 0; r < LS_QR; ++r) {
                            const float df = zc[r][k] - c.x;
                            t[r] = fmaf(df * df, c.y, t[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < LS_QR; ++r) acc[r][jj] += t[r];
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < LS_JT; ++jj) {
            const float c = s_c[jj];   // the constant last: it is the largest term for narrow posteriors
#pragma unroll
            for (int r = 0; r < LS_QR; ++r) acc[r][jj] += c;
        }
#pragma unroll
        for (int r = 0; r < LS_QR; ++r) {
            float bm = acc[r][0];
#pragma unroll
            for (int jj = 1; jj < LS_JT; ++jj) bm = fmaxf(bm, acc[r][jj]);
            const float mn = fmaxf(m[r], bm);
            float t = s[r] * __builtin_amdgcn_exp2f(m[r] - mn);
#pragma unroll
            for (int jj = 0; jj < LS_JT; ++jj) t += __builtin_amdgcn_exp2f(acc[r][jj] - mn);
            m[r] = mn; s[r] = t;
        }
    }
#pragma unroll
    for (int r = 0; r < LS_QR; ++r)
        if (live[r]) part[(long)blockIdx.y * SN + q[r]] = make_float2(m[r], s[r]);
}

// Per-dimension terms: block = QG = 256/DB lane groups x DB dimensions of dimension tile dt; lane (g, dd) owns queries
// qb + g*LS_QR + r of dimension dt*DB + dd.  part[blockIdx.y][q*L + d] = (max, sum), base 2.
static __global__ __launch_bounds__(256) void lstat_dims_kernel(const float* __restrict__ z, const float2* __restrict__ mh,
                                                                const float* __restrict__ c2, long SN, int N, int L, int DB, int ndt,
                                                                int jper, float2* __restrict__ part) {
    __shared__ float4 s_t[LS_JD * LS_DB];   // (mu, hw, c, -)
    const int tid = threadIdx.x, QG = 256 / DB;
    const int dt = blockIdx.x % ndt;
    const long qt = blockIdx.x / ndt;
    const int g = tid / DB, dd = tid - g * DB, d = dt * DB + dd;
    const bool lane_ok = g < QG && d < L;
    long q[LS_QR];
    bool live[LS_QR];
    float zv[LS_QR], m[LS_QR], s[LS_QR];
#pragma unroll
    for (int r = 0; r < LS_QR; ++r) {
        q[r] = qt * (QG * LS_QR) + (long)g * LS_QR + r;
        live[r] = lane_ok && q[r] < SN;
        zv[r] = live[r] ? z[q[r] * L + d] : 0.f;
        m[r] = -1e30f; s[r] = 0.f;
    }
    const int j0 = blockIdx.y * jper, j1 = min(N, j0 + jper);
    const int dl = min(DB, L - dt * DB);
    for (int jt = j0; jt < j1; jt += LS_JD) {
        __syncthreads();
        for (int e = tid; e < LS_JD * DB; e += 256) {
            const int jj = e / DB, de = e - jj * DB, j = jt + jj;
            float4 v = make_float4(0.f, 0.f, -INFINITY, 0.f);   // missing component: a = -inf
            if (j < j1 && de < dl) {
                const long o = (long)j * L + dt * DB + de;
                const float2 t = mh[o];
                v = make_float4(t.x, t.y, c2[o], 0.f);
            }
            s_t[e] = v;
        }
        __syncthreads();
        for (int jb = 0; jb < LS_JD; jb += 8) {
            float a[LS_QR][8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 c = s_t[(jb + k) * DB + dd];
#pragma unroll
                for (int r = 0; r < LS_QR; ++r) {
                    const float df = zv[r] - c.x;
                    a[r][k] = fmaf(df * df, c.y, c.z);
                }
            }
#pragma unroll
            for (int r = 0; r < LS_QR; ++r) {
                float bm = a[r][0];
#pragma unroll
                for (int k = 1; k < 8; ++k) bm = fmaxf(bm, a[r][k]);
                const float mn = fmaxf(m[r], bm);
                float t = s[r] * __builtin_amdgcn_exp2f(m[r] - mn);
#pragma unroll
                for (int k = 0; k < 8; ++k) t += __builtin_amdgcn_exp2f(a[r][k] - mn);
                m[r] = mn; s[r] = t;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < LS_QR; ++r)
        if (live[r]) part[(long)blockIdx.y * SN * L + q[r] * L + d] = make_float2(m[r], s[r]);
}

// out[i] = ln 2 * (M + log2 sum_k s_k 2^(m_k - M)) - log N over the nsplit partials of element i, in split order, f64.
static __global__ void lstat_merge_kernel(const float2* __restrict__ part, int nsplit, long n, double lnN, double* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        double M = -1e300;
        for (int k = 0; k < nsplit; ++k) M = fmax(M, (double)part[(long)k * n + i].x);
        double S = 0.0;
        for (int k = 0; k < nsplit; ++k) {
            const float2 p = part[(long)k * n + i];
            S += (double)p.y * exp2((double)p.x - M);
        }
        out[i] = LS_LN2 * (M + log2(S)) - lnN;
    }
}

// Sum over the 256 threads of a block in a fixed tree (all threads get the result).
static __device__ double lstat_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One block per dimension d: per_dim[d] = kl_per_dim, per_dim[L+d] = var_mu (two-pass), per_dim[2L+d] = dwkl_per_dim, and for the
// scalars dstat[d] = mean_i KL_d, dstat[L+d] = mean_i E_q log q(z_d|x), dstat[2L+d] = mean_i E_q log p(z_d),
// dstat[3L+d] = mean_q log q(z_d).  Thread t sums i = t, t+256, ... in order, then lstat_block_sum.
static __global__ __launch_bounds__(256) void lstat_moments_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                   const double* __restrict__ lqd, int N, long SN, int L,
                                                                   double* __restrict__ per_dim, double* __restrict__ dstat) {
    __shared__ double red[256];
    const int d = blockIdx.x, tid = threadIdx.x;
    double smu = 0.0, skl = 0.0, slv = 0.0, sxe = 0.0, slq = 0.0;
    for (long i = tid; i < N; i += 256) {
        const double m = mu[i * L + d], v = lv[i * L + d], ev = exp(v);
        smu += m;
        skl += 0.5 * (m * m + ev - 1.0 - v);
        slv += v;
        sxe += m * m + ev;
    }
    for (long q = tid; q < SN; q += 256) slq += lqd[q * L + d];
    const double mean = lstat_block_sum(smu, red) / N;
    double svar = 0.0;
    for (long i = tid; i < N; i += 256) {
        const double t = (double)mu[i * L + d] - mean;
        svar += t * t;
    }
    skl = lstat_block_sum(skl, red) / N;
    slv = lstat_block_sum(slv, red) / N;
    sxe = lstat_block_sum(sxe, red) / N;
    slq = lstat_block_sum(slq, red) / (double)SN;
    svar = lstat_block_sum(svar, red) / N;
    if (tid == 0) {
        per_dim[d] = skl;
        per_dim[L + d] = svar;
        per_dim[2 * L + d] = slq + 0.5 * (LS_LOG2PI + sxe);
        dstat[d] = skl;
        dstat[L + d] = -0.5 * (LS_LOG2PI + 1.0 + slv);
        dstat[2 * L + d] = -0.5 * (LS_LOG2PI + sxe);
        dstat[3 * L + d] = slq;
    }
}

// scalars = {kl, mi, tc, dwkl}: mean_q log_qz in a fixed tree, the per-dimension means summed over d in order.
static __global__ __launch_bounds__(256) void lstat_final_kernel(const double* __restrict__ lq, long SN, const double* __restrict__ dstat,
                                                                 int L, double* __restrict__ scalars) {
    __shared__ double red[256];
    double t = 0.0;
    for (long q = threadIdx.x; q < SN; q += 256) t += lq[q];
    const double mlq = lstat_block_sum(t, red) / (double)SN;
    if (threadIdx.x == 0) {
        double kl = 0.0, ng = 0.0, xe = 0.0, lp = 0.0;
        for (int d = 0; d < L; ++d) { kl += dstat[d]; ng += dstat[L + d]; xe += dstat[2 * L + d]; lp += dstat[3 * L + d]; }
        scalars[0] = kl;
        scalars[1] = ng - mlq;
        scalars[2] = mlq - lp;
        scalars[3] = lp - xe;
    }
}
