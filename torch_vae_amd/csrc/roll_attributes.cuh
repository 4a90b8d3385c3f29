// Attribute-regularised latents (include/vae_attributes.h; Pati & Lerch 2020): the integer counters of a float32 batch, the in-batch
// regulariser with its gradient on z, and the Kendall concordance sums of a whole set.
//
// attr_roll_counters_kernel   one WORKGROUP (4 waves) per roll, one pass over the f32 cells; the waves share the rows in groups of 4.  A
//                             row is read 64 columns per lane-load and turned into a 64-bit ballot m, which is wave-uniform: everything
//                             after the compare runs on the scalar unit (popcounts, shifts, ORs) while the vector unit only loads and
//                             compares.  Onsets are m & ~((m << 1) | carry), carry the row's cell in front of the word; the columns that
//                             sound / hold an onset are the OR of m / of the onsets down the rows - per wave in registers, across the
//                             four waves through 64 bytes of LDS.  K = 1, 2 or 4 words (up to 256 columns) of those ORs are held at
//                             once; a wider roll takes another pass over the rows for the next 256 columns (the carry across passes is
//                             re-read from the roll, one uniform load per row).  Which rows are used is kept per lane (row p in lane
//                             p mod 64, bit p / 64: h <= 1024), so a row that sounds in two passes counts once.  The loads of a row
//                             never depend on a ballot (columns past w are clamped into the row and masked in the compare), so the
//                             row loop keeps K x RA_RU loads in flight per lane.  Bound: HBM reads, 4 bytes per cell; a batch of a
//                             few hundred rolls is bound by the latency of its eight dependent rounds of loads instead.
// attr_reg_rows_kernel        grid (B / 16, pairs): a wave owns 4 rows i of one pair's column, the lanes stride the partners j, which
//                             sit in LDS a tile at a time (z_j f32, a_j f64).  Terms in f32, lane sums in f64, a butterfly over the
//                             lanes: the row's loss sum to work space, its gradient to g_z.  Row 0 of the grid also writes the zeros
//                             of the unregularised columns.  Bound: B^2 x pairs exponentials - 0.13 G at the limits.
// attr_reg_final_kernel       one workgroup: the pairs' means in f64 (thread-strided sums, a fixed tree) and their sum.
// attr_concord_kernel         tiled like set_distance.cuh (queries in registers, a tile of partners in LDS, grid.y over contiguous
//                             ranges of the partners; its helpers compute distances over contiguous rows and its kernels are
//                             defined in that header, so nothing of it is included here): a lane owns one query i - 16 latent dimensions
//                             and the 7 attribute values in registers - and a tile of 64 partners j sits in LDS, read as broadcasts.
//                             Signs are -1 / 0 / +1 held as f32, and the 7 x 16 sums are f32 fused multiply-adds: a lane sees at most
//                             65536 partners, so every sum is an integer below 2^24 and exact.  Ties are counted as non-ties (sgn^2).
//                             Only j > i counts: tiles below the block's first query are skipped, the diagonal ones masked per lane.
//                             grid (queries / 256, splits of the partner range, L / 16); a block's 135 integer sums go to work space.
//                             Bound: vector ALU, about 190 operations per pair and 16 dimensions.
// attr_concord_merge_kernel   one lane per output: the blocks' integers added in int64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RA_COUNTERS 8
#define RA_ATTRS 7
#define RA_MAX_PAIRS 8
#define RA_MAX_B 4096
#define RA_MAX_L 4096
#define RA_MAX_ROWS 1024
#define RA_MAX_CELLS (1 << 20)
#define RA_MAX_POINTS 65536
#define RA_WAVES 4            // counters: waves per workgroup (one roll)
#define RA_RU 4                // counters: rows whose loads are in flight together
#define RA_MAX_BLOCKS (1 << 16)
#define RA_REG_ROWS 4         // regulariser: rows per wave
#define RA_REG_TILE 1024      // regulariser: partners per LDS tile
#define RA_THREADS 256        // concordance: queries (lanes) per workgroup
#define RA_MAX_SPLITS 64       // concordance: ranges of the partner set
#define RA_DP 16              // concordance: latent dimensions per lane
#define RA_JT 64              // concordance: partners per LDS tile
#define RA_COLS (RA_ATTRS * RA_DP + RA_DP + RA_ATTRS)   // concordance: integers a block leaves (S | non-ties of z | non-ties of a)

// the attribute values of include/vae_attributes.h from one roll's counters: at most one IEEE operation each
__device__ __forceinline__ double ra_attr_value(const int* __restrict__ c, int attr) {
    const int cells = c[0];
    switch (attr) {
    case 0: return (double)cells;
    case 1: return (double)c[1];
    case 2: return cells > 0 ? (double)(c[4] - c[3] + 1) : 0.0;
    case 3: return cells > 0 ? (double)c[7] / (double)cells : -1.0;
    case 4: return cells > 0 ? (double)cells / (double)c[5] : 0.0;
    case 5: return (double)c[6];
    default: return (double)c[2];
    }
}

// ---- counters -------------------------------------------------------------------------------------------------------------------------
struct RaCounterArgs { const float* rolls; long n; int h, w; float thr; int* counters; };

template <int K>      // K: 64-column words held per pass over the rows (1, 2 or 4: the fewest that cover w, at most 256 columns)
static __global__ __launch_bounds__(64 * RA_WAVES) void attr_roll_counters_kernel(RaCounterArgs a) {
    __shared__ unsigned long long s_or[RA_WAVES][2 * K];
    __shared__ int s_sum[RA_WAVES][6];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long per = (long)a.h * a.w;
    for (long r = blockIdx.x; r < a.n; r += gridDim.x) {
        const float* __restrict__ x = a.rolls + r * per;
        int cells = 0, notes = 0, psum = 0;          // of this wave's rows
        int sounding = 0, onset_steps = 0;           // of the roll (wave 0)
        unsigned rowused = 0;
        for (int c0 = 0; c0 < a.w; c0 += 64 * K) {
            unsigned long long col[K], ons[K];
            int cl[K];       // this lane's column of word k, clamped into the row; ok: it exists
            bool ok[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                col[k] = 0; ons[k] = 0;
                const int c = c0 + 64 * k + lane;
                ok[k] = c < a.w;
                cl[k] = ok[k] ? c : a.w - 1;
            }
            // RA_RU rows at a time, every load of them issued in front of the first ballot (the tail clamps the row and masks it);
            // wave v takes the groups v, v + 4, ...
            for (int p0 = wave * RA_RU; p0 < a.h; p0 += RA_WAVES * RA_RU) {
                float v[RA_RU][K], vc[RA_RU];
#pragma unroll
                for (int u = 0; u < RA_RU; ++u) {
                    const float* __restrict__ row = x + min(p0 + u, a.h - 1) * a.w;
#pragma unroll
                    for (int k = 0; k < K; ++k) v[u][k] = row[cl[k]];
                    vc[u] = row[c0 > 0 ? c0 - 1 : 0];      // (uniform) the cell in front of this pass: rolls wider than 256 columns only
                }
#pragma unroll
                for (int u = 0; u < RA_RU; ++u) {
                    const int p = p0 + u;
                    const bool rowok = p < a.h;
                    unsigned long long carry = (c0 > 0 && vc[u] >= a.thr) ? 1ull : 0ull;
                    int rc = 0;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const unsigned long long m = __ballot(rowok && ok[k] && v[u][k] >= a.thr);
                        const unsigned long long on = m & ~((m << 1) | carry);
                        carry = m >> 63;
                        rc += __popcll(m);
                        notes += __popcll(on);
                        col[k] |= m; ons[k] |= on;
                    }
                    cells += rc;
                    psum += p * rc;
                    if (rc && (p & 63) == lane) rowused |= 1u << (p >> 6);
                }
            }
            // the pass's columns: the OR of the four waves' rows
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) { s_or[wave][k] = col[k]; s_or[wave][K + k] = ons[k]; }
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    unsigned long long c = 0, o = 0;
#pragma unroll
                    for (int v = 0; v < RA_WAVES; ++v) { c |= s_or[v][k]; o |= s_or[v][K + k]; }
                    sounding += __popcll(c); onset_steps += __popcll(o);
                }
            }
            __syncthreads();
        }
        int used = __popc(rowused);
        int lo = rowused ? lane + 64 * (__ffs(rowused) - 1) : 0x7fffffff;
        int hi = rowused ? lane + 64 * (31 - __clz(rowused)) : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            used += __shfl_xor(used, o);
            lo = min(lo, __shfl_xor(lo, o));
            hi = max(hi, __shfl_xor(hi, o));
        }
        if (lane == 0) {
            s_sum[wave][0] = cells; s_sum[wave][1] = notes; s_sum[wave][2] = psum; s_sum[wave][3] = used; s_sum[wave][4] = lo; s_sum[wave][5] = hi;
        }
        __syncthreads();
        if (wave == 0) {
            cells = notes = psum = used = 0; lo = 0x7fffffff; hi = -1;
#pragma unroll
            for (int v = 0; v < RA_WAVES; ++v) {
                cells += s_sum[v][0]; notes += s_sum[v][1]; psum += s_sum[v][2]; used += s_sum[v][3];
                lo = min(lo, s_sum[v][4]); hi = max(hi, s_sum[v][5]);
            }
            if (cells == 0) lo = -1;
            const int out = lane == 0 ? cells : lane == 1 ? notes : lane == 2 ? used : lane == 3 ? lo : lane == 4 ? hi : lane == 5 ? sounding
                          : lane == 6 ? onset_steps : psum;
            if (lane < RA_COUNTERS) a.counters[r * RA_COUNTERS + lane] = out;
        }
        __syncthreads();      // (s_sum and s_or are the next roll's too)
    }
}

// ---- regulariser ------------------------------------------------------------------------------------------------------------------------
struct RaRegArgs {
    const float* z; int ldz, L; const int* counters; int B, npairs;
    int attr[RA_MAX_PAIRS], dim[RA_MAX_PAIRS];
    float delta; double gscale;      // gscale = weight * 2 * delta / B^2
    double* rowloss;                 // [npairs][B]: sum_j of row i's terms
    float* gz;                       // [B][L] or null
};

static __global__ __launch_bounds__(256) void attr_reg_rows_kernel(RaRegArgs a) {
    __shared__ float s_z[RA_REG_TILE];
    __shared__ double s_a[RA_REG_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.y, attr = a.attr[k], dim = a.dim[k];
    const int rows = 4 * RA_REG_ROWS, b0 = blockIdx.x * rows, i0 = b0 + wave * RA_REG_ROWS;
    if (a.gz && k == 0) {          // the zeros of the columns no pair names (the pairs' columns are written below, by their own blocks)
        for (int e = tid; e < rows * a.L; e += 256) {
            const int i = b0 + e / a.L, d = e % a.L;
            bool named = false;
            for (int q = 0; q < a.npairs; ++q) named |= a.dim[q] == d;
            if (i < a.B && !named) a.gz[(size_t)i * a.L + d] = 0.f;
        }
    }
    float zi[RA_REG_ROWS];
    double ai[RA_REG_ROWS], ls[RA_REG_ROWS], gs[RA_REG_ROWS];
#pragma unroll
    for (int r = 0; r < RA_REG_ROWS; ++r) {
        const int i = min(i0 + r, a.B - 1);
        zi[r] = a.z[(size_t)i * a.ldz + dim];
        ai[r] = ra_attr_value(a.counters + (size_t)i * RA_COUNTERS, attr);
        ls[r] = 0.0; gs[r] = 0.0;
    }
    for (int t0 = 0; t0 < a.B; t0 += RA_REG_TILE) {
        const int jn = min(RA_REG_TILE, a.B - t0);
        __syncthreads();
        for (int j = tid; j < jn; j += 256) {
            s_z[j] = a.z[(size_t)(t0 + j) * a.ldz + dim];
            s_a[j] = ra_attr_value(a.counters + (size_t)(t0 + j) * RA_COUNTERS, attr);
        }
        __syncthreads();
        for (int j = lane; j < jn; j += 64) {
            const float zj = s_z[j];
            const double aj = s_a[j];
#pragma unroll
            for (int r = 0; r < RA_REG_ROWS; ++r) {
                // u = delta (z_i - z_j) as an f32 pair u + ul (the difference by TwoSum, the product by an fma): a saturated pair's
                // term is 2 e^{-2|u|}, whose relative error is 2 |u| times that of u - 1e-5 at |u| = 40 if u were one rounded f32
                const float nzj = -zj, d = zi[r] + nzj, bb = d - zi[r], dl = (zi[r] - (d - bb)) + (nzj - bb);
                const float u = a.delta * d, ul = __fmaf_rn(a.delta, d, -u) + a.delta * dl, au = fabsf(u);
                const int su = (u > 0.f) - (u < 0.f), s = (ai[r] > aj) - (ai[r] < aj);
                const float e0 = expf(-2.f * au), e = __fmaf_rn(e0, -2.f * (float)su * ul, e0), q = 1.f / (1.f + e);
                // |t - s|: s = 0: |t|;  t towards s: 1 - |t| = 2e/(1+e);  away from it (or u = 0, e = 1): 1 + |t| = 2/(1+e)
                const float term = s == 0 ? tanhf(au) : (s * su > 0 ? 2.f * e * q : 2.f * q);
                const float sech2 = 4.f * e * q * q;
                const int sg = s == 0 ? su : -s;      // sign(t - s), |t| < 1
                ls[r] += (double)term;
                gs[r] += (double)((float)sg * sech2);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RA_REG_ROWS; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { ls[r] += __shfl_xor(ls[r], o); gs[r] += __shfl_xor(gs[r], o); }
        const int i = i0 + r;
        if (lane == 0 && i < a.B) {
            a.rowloss[(size_t)k * a.B + i] = ls[r];
            if (a.gz) a.gz[(size_t)i * a.L + dim] = (float)(a.gscale * gs[r]);
        }
    }
}

static __global__ __launch_bounds__(256) void attr_reg_final_kernel(const double* __restrict__ rowloss, int B, int npairs, double* __restrict__ loss) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int k = 0; k < npairs; ++k) {
        double s = 0.0;
        for (int i = tid; i < B; i += 256) s += rowloss[(size_t)k * B + i];
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            const double v = red[0] / ((double)B * (double)B);
            loss[1 + k] = v;
            total += v;
        }
        __syncthreads();
    }
    if (tid == 0) loss[0] = total;
}

// ---- concordance ------------------------------------------------------------------------------------------------------------------------
struct RaConcordArgs {
    const float* z; int ldz, L; const int* counters; long N; int nattr, splits;
    int attr[RA_ATTRS];
    int* part;                       // [gridDim.z][gridDim.y * gridDim.x][RA_COLS]
    long long* S; long long* ties_z; long long* ties_a;
};

static __global__ __launch_bounds__(RA_THREADS) void attr_concord_kernel(RaConcordArgs a) {
    __shared__ __attribute__((aligned(16))) float t_z[RA_JT * RA_DP];
    __shared__ __attribute__((aligned(16))) double t_a[RA_JT * (RA_ATTRS + 1)];
    __shared__ int red[RA_THREADS / 64][RA_COLS];
    const int tid = threadIdx.x, d0 = blockIdx.z * RA_DP;
    const long q0 = (long)blockIdx.x * RA_THREADS, i = q0 + tid;
    const bool have = i < a.N;
    float zq[RA_DP];
    double aq[RA_ATTRS];
#pragma unroll
    for (int d = 0; d < RA_DP; ++d) zq[d] = (have && d0 + d < a.L) ? a.z[i * a.ldz + d0 + d] : 0.f;
#pragma unroll
    for (int k = 0; k < RA_ATTRS; ++k) aq[k] = (have && k < a.nattr) ? ra_attr_value(a.counters + i * RA_COUNTERS, a.attr[k]) : 0.0;
    float acc[RA_ATTRS][RA_DP], nz[RA_DP], na[RA_ATTRS];
#pragma unroll
    for (int k = 0; k < RA_ATTRS; ++k) {
        na[k] = 0.f;
#pragma unroll
        for (int d = 0; d < RA_DP; ++d) acc[k][d] = 0.f;
    }
#pragma unroll
    for (int d = 0; d < RA_DP; ++d) nz[d] = 0.f;
    const long len = (a.N + a.splits - 1) / a.splits, r0 = (long)blockIdx.y * len;      // this block's range of partners
    const long rg_j0 = r0 < a.N ? r0 : a.N, rg_j1 = r0 + len < a.N ? r0 + len : a.N;
    const long first = rg_j0 > q0 + 1 ? rg_j0 : q0 + 1;       // partners at or below the block's first query pair with nobody here
    const long mine = have ? i : a.N;                          // (a lane past the set pairs with nobody)
    for (long t0 = first; t0 < rg_j1; t0 += RA_JT) {
        const int jn = (int)(rg_j1 - t0 < RA_JT ? rg_j1 - t0 : RA_JT);
        __syncthreads();
        for (int e = tid; e < RA_JT * RA_DP; e += RA_THREADS) {
            const int j = e / RA_DP, d = e % RA_DP;
            t_z[e] = (j < jn && d0 + d < a.L) ? a.z[(t0 + j) * a.ldz + d0 + d] : 0.f;
        }
        for (int e = tid; e < RA_JT * (RA_ATTRS + 1); e += RA_THREADS) {
            const int j = e / (RA_ATTRS + 1), k = e % (RA_ATTRS + 1);
            t_a[e] = (j < jn && k < a.nattr) ? ra_attr_value(a.counters + (t0 + j) * RA_COUNTERS, a.attr[k]) : 0.0;
        }
        __syncthreads();
        for (int jj = 0; jj < jn; ++jj) {
            if (t0 + jj <= mine) continue;
            float sz[RA_DP], sa[RA_ATTRS];
#pragma unroll
            for (int d = 0; d < RA_DP; d += 4) {
                const float4 v = *reinterpret_cast<const float4*>(t_z + jj * RA_DP + d);
                sz[d + 0] = (float)(zq[d + 0] > v.x) - (float)(zq[d + 0] < v.x);
                sz[d + 1] = (float)(zq[d + 1] > v.y) - (float)(zq[d + 1] < v.y);
                sz[d + 2] = (float)(zq[d + 2] > v.z) - (float)(zq[d + 2] < v.z);
                sz[d + 3] = (float)(zq[d + 3] > v.w) - (float)(zq[d + 3] < v.w);
            }
#pragma unroll
            for (int k = 0; k < RA_ATTRS; ++k) {
                const double v = t_a[jj * (RA_ATTRS + 1) + k];
                sa[k] = (float)(aq[k] > v) - (float)(aq[k] < v);
                na[k] = __fmaf_rn(sa[k], sa[k], na[k]);
            }
#pragma unroll
            for (int d = 0; d < RA_DP; ++d) nz[d] = __fmaf_rn(sz[d], sz[d], nz[d]);
#pragma unroll
            for (int k = 0; k < RA_ATTRS; ++k)
#pragma unroll
                for (int d = 0; d < RA_DP; ++d) acc[k][d] = __fmaf_rn(sa[k], sz[d], acc[k][d]);
        }
    }
    // lane -> wave (butterfly on integers) -> block (LDS) -> the block's slot
    const int lane = tid & 63, wave = tid >> 6;
    auto fold = [&](float v, int col) {
        int s = (int)v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) red[wave][col] = s;
    };
#pragma unroll
    for (int k = 0; k < RA_ATTRS; ++k)
#pragma unroll
        for (int d = 0; d < RA_DP; ++d) fold(acc[k][d], k * RA_DP + d);
#pragma unroll
    for (int d = 0; d < RA_DP; ++d) fold(nz[d], RA_ATTRS * RA_DP + d);
#pragma unroll
    for (int k = 0; k < RA_ATTRS; ++k) fold(na[k], RA_ATTRS * RA_DP + RA_DP + k);
    __syncthreads();
    const long slot = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (tid < RA_COLS) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < RA_THREADS / 64; ++w) s += red[w][tid];
        a.part[slot * RA_COLS + tid] = s;
    }
}

// one lane per output: S [nattr][L] | ties_z [L] | ties_a [nattr]; slots = blocks per chunk of 16 dimensions (0: N < 2, all zeros)
static __global__ __launch_bounds__(RA_THREADS) void attr_concord_merge_kernel(RaConcordArgs a, long slots, long long n0) {
    const long o = (long)blockIdx.x * RA_THREADS + threadIdx.x, nS = (long)a.nattr * a.L;
    if (o >= nS + a.L + a.nattr) return;
    int chunk, col;
    if (o < nS) { const int k = (int)(o / a.L), d = (int)(o % a.L); chunk = d / RA_DP; col = k * RA_DP + d % RA_DP; }
    else if (o < nS + a.L) { const int d = (int)(o - nS); chunk = d / RA_DP; col = RA_ATTRS * RA_DP + d % RA_DP; }
    else { chunk = 0; col = RA_ATTRS * RA_DP + RA_DP + (int)(o - nS - a.L); }
    long long s = 0;
    const int* p = a.part + ((long)chunk * slots) * RA_COLS + col;
    for (long t = 0; t < slots; ++t) s += p[t * RA_COLS];
    if (o < nS) a.S[o] = s;
    else if (o < nS + a.L) a.ties_z[o - nS] = n0 - s;
    else a.ties_a[o - nS - a.L] = n0 - s;
}
