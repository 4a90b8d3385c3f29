// Nearest training rolls of query rolls under transposition and time shift (include/vae_step.h: vae_nearest_rolls).  Rolls are bit
// planes, h rows of w/32 dwords, most significant bit first within a byte.  The distance of a pair is the smallest
// popcount(q XOR C') over the window of shifted candidates C'(y, x) = C(y - dy, x - dt), zero outside the frame.
//   nearest_rolls_kernel  grid query tiles x splits.  A workgroup keeps QPW queries per wave and CT = 64 / QPW candidates in LDS
//                         (4 and 16 in four waves; 8 and 8 in one wave for rolls above NR_TILE_ROLL_BYTES) and gives every lane one
//                         (query, candidate) pair per candidate tile: lane = (query of the wave) * CT + candidate.  The lane walks
//                         the pair's dwords for every shift and keeps min(d << 10 | shift rank).  The wave then folds its lanes'
//                         (d << 40 | j) keys into the sorted k-best list of each of its queries; list entry i lives in lane i.
//                         The lists go to work space, one per (query, split).
//   nearest_merge_kernel  one wave per query: folds the splits' lists into one in the same way, then for each of the k winners
//                         counts popcount(q AND C') at the winning shift straight from global memory, and popcount(q).
// The shifts.  A transposition is a dword offset of dy * w/32 into the candidate; rows of q without a source row count popcount(q).
// A time shift needs the row as one big-endian number: staging swaps the bytes of every dword (only when T > 0: XOR and popcount
// do not care about bit order), and word i of the shifted row is alignbit(W(i - kk - 1), W(i - kk), dt & 31) with kk = dt >> 5
// (arithmetic) and W = 0 outside the row - one formula for both directions.  Zero fill is therefore index arithmetic; no dword
// outside a roll is ever addressed.
// LDS.  A roll's stride is S = roundup(words, 8) + 4 dwords, so 16 candidates 16 bytes wide land on 16 disjoint groups of four
// banks: the ds_read_b128 of a 16-lane group is conflict-free, and the queries of a wave (same stride) are broadcasts on other banks.
// Keys are unique (j is part of them), so a k-best list is a set: it does not depend on the order keys arrive in, on the number of
// splits or on the tiles.  No atomics; nothing synchronises with the host.
#pragma once
#include "common.cuh"

constexpr int NR_QUERY_TILE = 16;          // queries per workgroup: four waves of NR_QPW = 4
constexpr int NR_CAND_TILE = 16;           // candidates per LDS tile: 64 / NR_QPW
constexpr int NR_TILE_ROLL_BYTES = 4608;   // rolls above this take the one-wave workgroup of NR_LARGE_TILE queries and candidates
constexpr int NR_LARGE_TILE = 8;
constexpr int NR_MAX_ROLL_BYTES = 8192;
constexpr int NR_MAX_SHIFTS = 1023;        // (2P+1)(2T+1); a shift rank has ten bits
constexpr int NR_MAX_K = 32;
constexpr int NR_MAX_SPLITS = 64;
constexpr int NR_INDEX_BITS = 40;          // key = d << 40 | j
typedef unsigned long long nr_u64;
typedef __attribute__((ext_vector_type(4))) unsigned nr_u32x4;
constexpr nr_u64 NR_NONE = ~0ull;

struct NrArgs {
    const unsigned* queries; int n_queries;
    const unsigned* rolls; long n_rolls;
    int h, wd, P, T;                 // wd: dwords per row
    const long long* exclude;
    int k, splits;
    nr_u64* ws_keys; unsigned* ws_rank;   // [n_queries][splits][k]
    long long* index; int* distance; int* shift; int* intersection; int* query_cells;
};

__device__ __forceinline__ int nr_stride(int words) { return ((words + 7) & ~7) + 4; }
// rank 0 is (0, 0); the others ascend by (dy, dt).  lin = (dy + P) * (2T + 1) + dt + T.
__device__ __forceinline__ unsigned nr_rank(int lin, int lin0) { return lin < lin0 ? lin + 1 : lin == lin0 ? 0 : lin; }
__device__ __forceinline__ int nr_lin(int rank, int lin0) { return rank == 0 ? lin0 : rank <= lin0 ? rank - 1 : rank; }

// nwords dwords (one tile: fewer than 2^31) from global to LDS rolls of stride S (source rolls are contiguous), 16 bytes at a time
// where the source allows.
template <bool SWAP>
__device__ __forceinline__ void nr_stage(const unsigned* __restrict__ src, int nwords, int words, int S, unsigned* dst, int tid, int nthreads) {
    if ((words & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const unsigned w4 = words >> 2;
        for (unsigned i = tid; i < (unsigned)(nwords >> 2); i += nthreads) {
            nr_u32x4 v = reinterpret_cast<const nr_u32x4*>(src)[i];
            if (SWAP) v = nr_u32x4{__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w)};
            const unsigned r = i / w4, o = i - r * w4;
            *reinterpret_cast<nr_u32x4*>(dst + r * S + 4 * o) = v;
        }
    } else {
        for (unsigned i = tid; i < (unsigned)nwords; i += nthreads) {
            const unsigned v = src[i];
            const unsigned r = i / (unsigned)words, o = i - r * words;
            dst[r * S + o] = SWAP ? __builtin_bswap32(v) : v;
        }
    }
}

// The same in two halves for the candidate tiles: the next tile's 16-byte loads are issued into registers before the current tile is
// searched and stored to LDS after it, so a workgroup does not sit out the memory latency between two barriers.  Only where the
// tile is at most NR_PF loads per thread and the source allows 16-byte loads; nr_stage otherwise.  A thread's LDS places are the same
// for every tile: off[] is computed once, so the loop over tiles has no division.
constexpr int NR_PF = 8;
__device__ __forceinline__ void nr_places(int (&off)[NR_PF], int words, int S, int tid, int nthreads) {
    const unsigned w4 = words >> 2;
#pragma unroll
    for (int u = 0; u < NR_PF; ++u) {
        const unsigned i = tid + u * nthreads, r = i / w4;
        off[u] = (int)(r * S + 4 * (i - r * w4));
    }
}
// (nwords > 0.  Every load is issued, past the tile's end at the tile's last chunk: a load under a condition would have to be waited
// for where the branches join, which is before the search; nr_put leaves those registers alone.)
__device__ __forceinline__ void nr_fetch(const unsigned* __restrict__ src, int nwords, nr_u32x4 (&v)[NR_PF], int tid, int nthreads) {
    const int last = (nwords >> 2) - 1;
#pragma unroll
    for (int u = 0; u < NR_PF; ++u) v[u] = reinterpret_cast<const nr_u32x4*>(src)[min(tid + u * nthreads, last)];
}
template <bool SWAP>
__device__ __forceinline__ void nr_put(const nr_u32x4 (&v)[NR_PF], const int (&off)[NR_PF], int nwords, unsigned* dst, int tid, int nthreads) {
#pragma unroll
    for (int u = 0; u < NR_PF; ++u) {
        if (tid + u * nthreads < (nwords >> 2)) {
            nr_u32x4 x = v[u];
            if (SWAP) x = nr_u32x4{__builtin_bswap32(x.x), __builtin_bswap32(x.y), __builtin_bswap32(x.z), __builtin_bswap32(x.w)};
            *reinterpret_cast<nr_u32x4*>(dst + off[u]) = x;
        }
    }
}

// MODE 0: T == 0, 16-byte reads (every offset a multiple of four dwords); 1: T == 0, dword reads; 2: any window, dword reads;
// 3: |dt| < 32 and rows of whole 16-byte chunks; 4: |dt| < 32 and rows of one chunk (w = 128: no neighbouring dword).  Returns the
// minimum over the window of d << 10 | rank.
template <int MODE>
__device__ __forceinline__ unsigned nr_pair(const unsigned* qp, const unsigned* cp, int h, int wd, int P, int T) {
    unsigned best = ~0u;
    const int words = h * wd, lin0 = P * (2 * T + 1) + T;
    int lin = 0;
    for (int dy = -P; dy <= P; ++dy) {
        const int y0 = max(0, dy), y1 = min(h, h + dy);   // rows of q that have a source row
        unsigned dout = 0;                                // the others face zeros
        if (MODE == 0 || MODE >= 3) {
            for (int j = 0; j < y0 * wd; j += 4) { const nr_u32x4 a = *reinterpret_cast<const nr_u32x4*>(qp + j); dout = __popc(a.x) + dout; dout = __popc(a.y) + dout; dout = __popc(a.z) + dout; dout = __popc(a.w) + dout; }
            for (int j = y1 * wd; j < words; j += 4) { const nr_u32x4 a = *reinterpret_cast<const nr_u32x4*>(qp + j); dout = __popc(a.x) + dout; dout = __popc(a.y) + dout; dout = __popc(a.z) + dout; dout = __popc(a.w) + dout; }
        } else {
            for (int j = 0; j < y0 * wd; ++j) dout = __popc(qp[j]) + dout;
            for (int j = y1 * wd; j < words; ++j) dout = __popc(qp[j]) + dout;
        }
        const unsigned* qs = qp + y0 * wd;
        const unsigned* cs = cp + (y0 - dy) * wd;
        const int n = (y1 - y0) * wd;
        if (MODE == 0) {
            unsigned d0 = dout, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll 4
            for (int j = 0; j < n; j += 4) {
                const nr_u32x4 a = *reinterpret_cast<const nr_u32x4*>(qs + j), b = *reinterpret_cast<const nr_u32x4*>(cs + j);
                d0 = __popc(a.x ^ b.x) + d0; d1 = __popc(a.y ^ b.y) + d1; d2 = __popc(a.z ^ b.z) + d2; d3 = __popc(a.w ^ b.w) + d3;
            }
            best = min(best, ((d0 + d1 + d2 + d3) << 10) | nr_rank(lin++, lin0));
        } else if (MODE == 1) {
            unsigned d = dout;
            for (int j = 0; j < n; ++j) d = __popc(qs[j] ^ cs[j]) + d;
            best = min(best, (d << 10) | nr_rank(lin++, lin0));
        } else if (MODE == 2) {
            for (int dt = -T; dt <= T; ++dt) {
                const int kk = dt >> 5, rr = dt & 31;
                unsigned d = dout;
                for (int y = 0; y < y1 - y0; ++y) {
                    const unsigned* qr = qs + y * wd;
                    const unsigned* cr = cs + y * wd;
                    for (int i = 0; i < wd; ++i) {
                        const int jl = i - kk, jh = jl - 1;
                        const unsigned lo = (jl >= 0 && jl < wd) ? cr[jl] : 0u, hi = (jh >= 0 && jh < wd) ? cr[jh] : 0u;
                        d = __popc(qr[i] ^ __builtin_amdgcn_alignbit(hi, lo, rr)) + d;
                    }
                }
                best = min(best, (d << 10) | nr_rank(lin++, lin0));
            }
        } else if (MODE == 4) {
            for (int dt = -T; dt <= T; ++dt) {
                const int rr = dt & 31;
                unsigned d0 = dout, d1 = 0, d2 = 0, d3 = 0;
                if (dt >= 0) {
#pragma unroll 4
                    for (int j = 0; j < n; j += 4) {
                        const nr_u32x4 a = *reinterpret_cast<const nr_u32x4*>(qs + j), b = *reinterpret_cast<const nr_u32x4*>(cs + j);
                        d0 = __popc(a.x ^ (b.x >> rr)) + d0; d1 = __popc(a.y ^ __builtin_amdgcn_alignbit(b.x, b.y, rr)) + d1;
                        d2 = __popc(a.z ^ __builtin_amdgcn_alignbit(b.y, b.z, rr)) + d2; d3 = __popc(a.w ^ __builtin_amdgcn_alignbit(b.z, b.w, rr)) + d3;
                    }
                } else {
#pragma unroll 4
                    for (int j = 0; j < n; j += 4) {
                        const nr_u32x4 a = *reinterpret_cast<const nr_u32x4*>(qs + j), b = *reinterpret_cast<const nr_u32x4*>(cs + j);
                        d0 = __popc(a.x ^ __builtin_amdgcn_alignbit(b.x, b.y, rr)) + d0; d1 = __popc(a.y ^ __builtin_amdgcn_alignbit(b.y, b.z, rr)) + d1;
                        d2 = __popc(a.z ^ __builtin_amdgcn_alignbit(b.z, b.w, rr)) + d2; d3 = __popc(a.w ^ (b.w << (32 - rr))) + d3;
                    }
                }
                best = min(best, ((d0 + d1 + d2 + d3) << 10) | nr_rank(lin++, lin0));
            }
        } else {
            for (int dt = -T; dt <= T; ++dt) {
                const int rr = dt & 31;
                unsigned d0 = dout, d1 = 0, d2 = 0, d3 = 0;
                for (int y = 0; y < y1 - y0; ++y) {
                    const unsigned* qr = qs + y * wd;
                    const unsigned* cr = cs + y * wd;
                    for (int i = 0; i < wd; i += 4) {
                        const nr_u32x4 a = *reinterpret_cast<const nr_u32x4*>(qr + i), b = *reinterpret_cast<const nr_u32x4*>(cr + i);
                        unsigned s0, s1, s2, s3;
                        if (dt >= 0) {   // word i from (i - 1, i)
                            const unsigned e = i > 0 ? cr[i - 1] : 0u;
                            s0 = __builtin_amdgcn_alignbit(e, b.x, rr); s1 = __builtin_amdgcn_alignbit(b.x, b.y, rr);
                            s2 = __builtin_amdgcn_alignbit(b.y, b.z, rr); s3 = __builtin_amdgcn_alignbit(b.z, b.w, rr);
                        } else {         // word i from (i, i + 1)
                            const unsigned e = i + 4 < wd ? cr[i + 4] : 0u;
                            s0 = __builtin_amdgcn_alignbit(b.x, b.y, rr); s1 = __builtin_amdgcn_alignbit(b.y, b.z, rr);
                            s2 = __builtin_amdgcn_alignbit(b.z, b.w, rr); s3 = __builtin_amdgcn_alignbit(b.w, e, rr);
                        }
                        d0 = __popc(a.x ^ s0) + d0; d1 = __popc(a.y ^ s1) + d1; d2 = __popc(a.z ^ s2) + d2; d3 = __popc(a.w ^ s3) + d3;
                    }
                }
                best = min(best, ((d0 + d1 + d2 + d3) << 10) | nr_rank(lin++, lin0));
            }
        }
    }
    return best;
}

__device__ __forceinline__ nr_u64 nr_wave_min(nr_u64 m) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const nr_u64 t = __shfl_xor(m, o); m = t < m ? t : m; }
    return m;
}

// Folds the lanes' keys (NR_NONE: nothing) into the wave's ascending list, entry i in lane i; only the first k entries are kept
// exact (entry k - 1 is the bar a key has to pass).  The keys are unique, so the owner of the minimum is one lane.
__device__ __forceinline__ void nr_insert(nr_u64& lk, unsigned& lr, nr_u64 key, unsigned rank, int k, int lane) {
    nr_u64 bar = __shfl(lk, k - 1);
    bool pending = key < bar;
    while (__ballot(pending)) {
        const nr_u64 m = nr_wave_min(pending ? key : NR_NONE);
        const int owner = __ffsll((long long)__ballot(pending && key == m)) - 1;
        const unsigned r = __shfl(rank, owner);
        const int pos = __popcll(__ballot(lk < m));
        const nr_u64 uk = __shfl_up(lk, 1);
        const unsigned ur = __shfl_up(lr, 1);
        if (lane > pos) { lk = uk; lr = ur; }
        else if (lane == pos) { lk = m; lr = r; }
        bar = __shfl(lk, k - 1);
        pending = pending && lane != owner && key < bar;
    }
}

template <int QPW, int WAVES, int MODE>
static __global__ __launch_bounds__(64 * WAVES) void nearest_rolls_kernel(NrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned nr_lds[];
    constexpr int CT = 64 / QPW, QT = QPW * WAVES, NT = 64 * WAVES;
    constexpr bool SWAP = MODE >= 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ci = lane % CT, ql = lane / CT;
    const int words = a.h * a.wd, S = nr_stride(words);
    unsigned* qlds = nr_lds;
    unsigned* clds = nr_lds + QT * S;
    // Workgroups b, b + 8, ... share an XCD and its L2: give them consecutive places in (split, query tile) order, so that the query
    // tiles that read one range of rolls do it through one L2.  A bijection of the grid; speed only.
    const long nwg = gridDim.x, qtiles = ((long)a.n_queries + QT - 1) / QT;
    const long xq = nwg / 8, xr = nwg % 8, xcd = blockIdx.x % 8;
    const long place = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + blockIdx.x / 8;
    const long split = place / qtiles, q0 = (place - split * qtiles) * QT;
    const int nq = (int)min((long)QT, (long)a.n_queries - q0);
    const long per = (a.n_rolls + a.splits - 1) / a.splits;
    const long r0 = min(a.n_rolls, split * per), r1 = min(a.n_rolls, r0 + per);
    nr_stage<SWAP>(a.queries + q0 * words, nq * words, words, S, qlds, tid, NT);
    const int myq = wave * QPW + ql;
    const bool qvalid = myq < nq;
    const long long excl = (a.exclude && qvalid) ? a.exclude[q0 + myq] : -1;
    nr_u64 lk[QPW];
    unsigned lr[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) { lk[i] = NR_NONE; lr[i] = 0; }
    const bool pf = (words & 3) == 0 && (reinterpret_cast<uintptr_t>(a.rolls) & 15) == 0 && CT * words <= 4 * NR_PF * NT;   // uniform
    nr_u32x4 pv[NR_PF];
    int off[NR_PF];
    if (pf) nr_places(off, words, S, tid, NT);
    if (pf && r0 < r1) nr_fetch(a.rolls + r0 * words, (int)min((long)CT, r1 - r0) * words, pv, tid, NT);
    for (long t0 = r0; t0 < r1; t0 += CT) {
        __syncthreads();   // the previous tile has been read
        const int nc = (int)min((long)CT, r1 - t0);
        if (pf) nr_put<SWAP>(pv, off, nc * words, clds, tid, NT);
        else nr_stage<SWAP>(a.rolls + t0 * words, nc * words, words, S, clds, tid, NT);
        __syncthreads();
        if (pf) {   // the next tile; after the last one the same tile again, unused (no branch around the loads: see nr_fetch)
            const long tn = t0 + CT < r1 ? t0 + CT : t0;
            nr_fetch(a.rolls + tn * words, (int)min((long)CT, r1 - tn) * words, pv, tid, NT);
        }
        const long j = t0 + ci;
        const bool valid = qvalid && ci < nc && j != excl;
        nr_u64 key = NR_NONE;
        unsigned rank = 0;
        if (valid) {
            const unsigned p = nr_pair<MODE>(qlds + myq * S, clds + ci * S, a.h, a.wd, a.P, a.T);
            key = ((nr_u64)(p >> 10) << NR_INDEX_BITS) | (nr_u64)j;
            rank = p & 1023u;
        }
#pragma unroll
        for (int i = 0; i < QPW; ++i) nr_insert(lk[i], lr[i], ql == i ? key : NR_NONE, rank, a.k, lane);
    }
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
        const long q = q0 + wave * QPW + i;
        if (q < a.n_queries && lane < a.k) {
            const long o = (q * a.splits + split) * a.k + lane;
            a.ws_keys[o] = lk[i];
            a.ws_rank[o] = lr[i];
        }
    }
}

__device__ __forceinline__ int nr_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

static __global__ __launch_bounds__(64) void nearest_merge_kernel(NrArgs a) {
    const int lane = threadIdx.x;
    const long q = blockIdx.x;
    const int words = a.h * a.wd, n = a.splits * a.k;
    nr_u64 lk = NR_NONE;
    unsigned lr = 0;
    for (int b = 0; b < n; b += 64) {
        const bool in = b + lane < n;
        const nr_u64 key = in ? a.ws_keys[q * n + b + lane] : NR_NONE;
        const unsigned rank = in ? a.ws_rank[q * n + b + lane] : 0u;
        nr_insert(lk, lr, key, rank, a.k, lane);
    }
    const unsigned* __restrict__ qp = a.queries + q * words;
    int cells = 0;
    for (int i = lane; i < words; i += 64) cells = __popc(qp[i]) + cells;
    cells = nr_wave_sum(cells);
    if (lane == 0) a.query_cells[q] = cells;
    const int lin0 = a.P * (2 * a.T + 1) + a.T;
    for (int s = 0; s < a.k; ++s) {
        const nr_u64 key = __shfl(lk, s);
        const unsigned rank = __shfl(lr, s);
        const long o = q * a.k + s;
        if (key == NR_NONE) {   // wave-uniform
            if (lane == 0) { a.index[o] = -1; a.distance[o] = -1; a.shift[2 * o] = 0; a.shift[2 * o + 1] = 0; a.intersection[o] = 0; }
            continue;
        }
        const long j = (long)(key & ((1ull << NR_INDEX_BITS) - 1));
        const int lin = nr_lin((int)rank, lin0);
        const int dy = lin / (2 * a.T + 1) - a.P, dt = lin % (2 * a.T + 1) - a.T;
        const int kk = dt >> 5, rr = dt & 31;
        const unsigned* __restrict__ cp = a.rolls + j * words;
        int inter = 0;
        for (int i = lane; i < words; i += 64) {
            const int y = i / a.wd, x = i - y * a.wd, cy = y - dy;
            if (cy < 0 || cy >= a.h) continue;
            const int jl = x - kk, jh = jl - 1;
            const unsigned lo = (jl >= 0 && jl < a.wd) ? __builtin_bswap32(cp[cy * a.wd + jl]) : 0u;
            const unsigned hi = (jh >= 0 && jh < a.wd) ? __builtin_bswap32(cp[cy * a.wd + jh]) : 0u;
            inter = __popc(__builtin_bswap32(qp[i]) & __builtin_amdgcn_alignbit(hi, lo, rr)) + inter;
        }
        inter = nr_wave_sum(inter);
        if (lane == 0) {
            a.index[o] = j; a.distance[o] = (int)(key >> NR_INDEX_BITS); a.shift[2 * o] = dy; a.shift[2 * o + 1] = dt;
            a.intersection[o] = inter;
        }
    }
}
