// Note events out of float pianorolls (include/vae_step.h: vae_extract_notes): hysteresis thresholding, gap bridging, a minimum
// duration, then the surviving runs as (roll, pitch, onset, duration) with their peak, in (roll, pitch, onset) order, and the
// cleaned roll as bit planes.  One wave per row (one pitch of one roll), four rows per workgroup, three launches:
//   note_count_kernel   the row's mask, a walk over its runs, counts[row] (and the cleaned planes when no events are asked for)
//   note_scan_kernel    one workgroup: exclusive prefix of the counts inside tiles of NE_TILE rows (int32, in place), the tiles'
//                       starts (int64) and offsets[0..n]
//   note_emit_kernel    the same mask and walk again, now editing the mask into the cleaned one; then every lane that holds the first
//                       cell of a kept run writes that run's event at (row start + its rank among the row's starts)
// The row's mask lives in LDS, one 64-bit word per 64 time steps.  A chunk's word comes from two ballots: with onm = ballot(x >= on)
// and offm = ballot(!(x >= off)), lane i looks at m = (onm | offm) & (bits 0..i): empty means nothing in this chunk decided yet (the
// state carried in from the previous chunk), otherwise the state is onm's bit at m's highest set bit.  Lanes past the row's end hold
// NaN: off.  Every lane of the wave stores the same word to the same LDS address and reads it back itself, so the order of a row's
// LDS accesses is each lane's own program order: no barrier, and waves never wait for one another.  The walk runs on wave-uniform
// values (the words pass through readfirstlane) from run to run with count-trailing-zeros, not from cell to cell.
// No atomics: a row's position is a prefix sum of integers in row order, an event's position its rank in the row.  Repeated calls
// give the same bits.  Loads are one dword per lane (any 4-byte-aligned base); an event is one 16-byte store where the buffer is
// 16-byte aligned, four dword stores otherwise; a row's cleaned bytes are written by that row's wave alone, one byte per lane.
#pragma once
#include "common.cuh"

constexpr int NE_THREADS = 256;                     // four waves = four rows per workgroup
constexpr int NE_ROWS = NE_THREADS / 64;
constexpr int NE_LOADS = 4;                         // chunks whose loads are in flight together
constexpr int NE_SCAN_THREADS = 1024;
constexpr int NE_SCAN_PER = 16;                     // rows per lane of the scan
constexpr int NE_TILE_LG = 14;
constexpr int NE_TILE = 1 << NE_TILE_LG;            // = NE_SCAN_THREADS * NE_SCAN_PER rows; a tile holds < 2^14 * 2^15 events: int32
constexpr int NE_MAX_W = 65536;
static_assert(NE_TILE == NE_SCAN_THREADS * NE_SCAN_PER, "a scan tile is one pass of the workgroup");
typedef unsigned long long ne_u64;
typedef __attribute__((ext_vector_type(4))) int ne_i32x4;

__device__ __forceinline__ ne_u64 ne_uniform(ne_u64 v) {
    return ((ne_u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// Hysteresis state of the row's w cells into m[0 .. ceil(w/64)); bits past w are 0.
__device__ __forceinline__ void ne_row_mask(const float* __restrict__ row, int w, float on, float off, ne_u64* m, int lane) {
    const int nw = (w + 63) >> 6;
    ne_u64 carry = 0;
    const ne_u64 upto = (2ull << lane) - 1;   // bits 0..lane (lane 63: 2 << 63 is 0, minus 1 all ones)
    for (int c0 = 0; c0 < nw; c0 += NE_LOADS) {
        float v[NE_LOADS];
#pragma unroll
        for (int j = 0; j < NE_LOADS; ++j) {
            const int t = (c0 + j) * 64 + lane;
            v[j] = t < w ? row[t] : __builtin_nanf("");
        }
#pragma unroll
        for (int j = 0; j < NE_LOADS; ++j) {
            if (c0 + j < nw) {   // wave-uniform
                const ne_u64 onm = __ballot(v[j] >= on), offm = __ballot(!(v[j] >= off));
                const ne_u64 mm = (onm | offm) & upto;
                const bool s = mm ? ((onm >> (63 - __builtin_clzll(mm))) & 1) != 0 : carry != 0;
                const ne_u64 word = __ballot(s);
                m[c0 + j] = word;
                carry = word >> 63;
            }
        }
    }
}

// First position >= pos whose mask bit is 1 (zero = false) or 0 (zero = true); w when there is none.  Wave-uniform.  The cursor keeps
// the word last read in registers: a word with many runs costs one LDS round trip, not one per run.
struct NeCursor { int wi; ne_u64 word; };
__device__ __forceinline__ int ne_next(const ne_u64* m, int w, int pos, bool zero, NeCursor& c) {
    while (pos < w) {
        const int wi = pos >> 6;
        if (wi != c.wi) { c.wi = wi; c.word = ne_uniform(m[wi]); }
        const ne_u64 v = (zero ? ~c.word : c.word) >> (pos & 63);
        if (v) return min(w, pos + __builtin_ctzll(v));
        pos = (wi + 1) << 6;
    }
    return w;
}
// Sets or clears the bits [lo, hi), lo < hi.
__device__ __forceinline__ void ne_fill(ne_u64* m, int lo, int hi, bool set) {
    for (int wi = lo >> 6; wi <= (hi - 1) >> 6; ++wi) {
        const int s = max(lo - wi * 64, 0), e = min(hi - wi * 64, 64);
        const ne_u64 bits = (e == 64 ? ~0ull : (1ull << e) - 1) & ~((1ull << s) - 1);
        m[wi] = set ? m[wi] | bits : m[wi] & ~bits;
    }
}
// Walks the runs of ones: a run that starts at most G cells after the open note's end extends it (the gap has a one on both sides by
// construction: it lies between two runs), any other closes it; a closed note shorter than D is dropped.  Returns the number of
// notes kept.  EDIT: the mask becomes the cleaned one - bridged gaps set, dropped notes cleared; both lie behind the walk's position.
template <bool EDIT> __device__ __forceinline__ int ne_walk(ne_u64* m, int w, int D, int G) {
    int count = 0, t0 = 0, t1 = -1;   // the open note [t0, t1); t1 < 0: none
    NeCursor cur{-1, 0};               // (an edit may touch the cursor's word: it is read again afterwards)
    for (int pos = 0;;) {
        const int a = ne_next(m, w, pos, false, cur);
        const int b = a < w ? ne_next(m, w, a, true, cur) : w;
        if (a < w && t1 >= 0 && a - t1 <= G) {
            if (EDIT) { ne_fill(m, t1, a, true); cur.wi = -1; }
        } else {
            if (t1 >= 0) {
                const bool keep = t1 - t0 >= D;
                count += keep;
                if (EDIT && !keep) { ne_fill(m, t0, t1, false); cur.wi = -1; }
            }
            if (a >= w) break;
            t0 = a;
        }
        t1 = b; pos = b;
    }
    return count;
}

// byte bi of a row's planes holds cells 8 bi .. 8 bi + 7, the first in its most significant bit
__device__ __forceinline__ void ne_write_planes(const ne_u64* m, int w, unsigned char* __restrict__ out, int lane) {
    for (int bi = lane; bi < (w >> 3); bi += 64) out[bi] = (unsigned char)(__brev((unsigned)((m[bi >> 3] >> ((bi & 7) * 8)) & 255u)) >> 24);
}

// PLANES: a call that asks for no events gets its cleaned planes here, and no third launch follows.
template <bool PLANES>
static __global__ __launch_bounds__(NE_THREADS) void note_count_kernel(const float* __restrict__ rolls, long nrows, int w, float on, float off,
                                                                       int D, int G, int* __restrict__ counts,
                                                                       unsigned char* __restrict__ cleaned) {
    extern __shared__ ne_u64 ne_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * NE_ROWS + wave;
    if (row >= nrows) return;   // (whole waves leave; nothing below waits for another wave)
    ne_u64* m = ne_lds + wave * ((w + 63) >> 6);
    ne_row_mask(rolls + row * w, w, on, off, m, lane);
    const int c = ne_walk<PLANES>(m, w, D, G);
    if (lane == 0) counts[row] = c;
    if (PLANES) ne_write_planes(m, w, cleaned + row * (w >> 3), lane);
}

// One workgroup, tile after tile in row order: counts[i] becomes the number of events of the rows of i's tile before i, tile_base[t]
// the number before tile t, offsets[r] the number before row r * h, offsets[n] the total.
static __global__ __launch_bounds__(NE_SCAN_THREADS) void note_scan_kernel(int* __restrict__ counts, long nrows, int h,
                                                                           long long* __restrict__ tile_base, long long* __restrict__ offsets,
                                                                           long n) {
    __shared__ int s_wave[NE_SCAN_THREADS / 64];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    long long carry = 0;
    for (long tile0 = 0; tile0 < nrows; tile0 += NE_TILE) {
        const long i0 = tile0 + (long)tid * NE_SCAN_PER;
        // all of a lane's loads are issued before the first is used: four 16-byte loads where its 16 rows exist (the work space is
        // 256-byte aligned and i0 a multiple of 16), loads at a clamped index, the value masked afterwards, in the last lanes
        int v[NE_SCAN_PER], sum = 0;
        if (i0 + NE_SCAN_PER <= nrows) {
#pragma unroll
            for (int q = 0; q < NE_SCAN_PER / 4; ++q) {
                const ne_i32x4 t = *reinterpret_cast<const ne_i32x4*>(counts + i0 + 4 * q);
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < NE_SCAN_PER; ++e) v[e] = counts[min(i0 + e, nrows - 1)];
#pragma unroll
            for (int e = 0; e < NE_SCAN_PER; ++e) v[e] = i0 + e < nrows ? v[e] : 0;
        }
#pragma unroll
        for (int e = 0; e < NE_SCAN_PER; ++e) sum += v[e];
        int inc = sum;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int k = 0; k < NE_SCAN_THREADS / 64; ++k) { const int x = s_wave[k]; wbase += k < wv ? x : 0; total += x; }
        int run = wbase + inc - sum;
        if (tid == 0) tile_base[tile0 >> NE_TILE_LG] = carry;
        if (i0 < nrows) {
            int pre[NE_SCAN_PER];
#pragma unroll
            for (int e = 0; e < NE_SCAN_PER; ++e) { pre[e] = run; run += v[e]; }
            if (i0 + NE_SCAN_PER <= nrows) {
#pragma unroll
                for (int q = 0; q < NE_SCAN_PER / 4; ++q)
                    *reinterpret_cast<ne_i32x4*>(counts + i0 + 4 * q) = ne_i32x4{pre[4 * q], pre[4 * q + 1], pre[4 * q + 2], pre[4 * q + 3]};
            } else {
#pragma unroll
                for (int e = 0; e < NE_SCAN_PER; ++e)
                    if (i0 + e < nrows) counts[i0 + e] = pre[e];
            }
            long roll = i0 / h; int p = (int)(i0 - roll * h);
#pragma unroll
            for (int e = 0; e < NE_SCAN_PER; ++e) {
                if (p == 0 && i0 + e < nrows) offsets[roll] = carry + pre[e];
                if (++p == h) { p = 0; ++roll; }
            }
        }
        carry += total;
        __syncthreads();   // s_wave is rewritten by the next tile
    }
    if (tid == 0) offsets[n] = carry;
}

static __global__ __launch_bounds__(NE_THREADS) void note_emit_kernel(const float* __restrict__ rolls, long nrows, int h, int w, float on, float off,
                                                                      int D, int G, const int* __restrict__ prefix,
                                                                      const long long* __restrict__ tile_base, int* __restrict__ events,
                                                                      float* __restrict__ peaks, long long capacity,
                                                                      unsigned char* __restrict__ cleaned) {
    extern __shared__ ne_u64 ne_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * NE_ROWS + wave;
    if (row >= nrows) return;
    const int nw = (w + 63) >> 6;
    ne_u64* m = ne_lds + wave * nw;
    const float* __restrict__ x = rolls + row * w;
    ne_row_mask(x, w, on, off, m, lane);
    ne_walk<true>(m, w, D, G);
    if (cleaned) ne_write_planes(m, w, cleaned + row * (w >> 3), lane);
    if (!events) return;
    const long long base = tile_base[row >> NE_TILE_LG] + prefix[row];
    const long roll = row / h;
    const int pitch = (int)(row - roll * h);
    const bool vec = (reinterpret_cast<uintptr_t>(events) & 15) == 0;
    int emitted = 0;
    ne_u64 prev = 0;   // the previous chunk's last bit
    for (int c = 0; c < nw; ++c) {
        const ne_u64 k = ne_uniform(m[c]);
        const ne_u64 starts = k & ~((k << 1) | prev);
        prev = k >> 63;
        if (!starts) continue;
        const long long idx = base + emitted + __popcll(starts & ((1ull << lane) - 1));
        if (((starts >> lane) & 1) && idx < capacity) {
            const int onset = c * 64 + lane;
            const ne_u64 z = ~k >> lane;   // (zeros come in at the top: a run that reaches the word's end finds no end here)
            int len;
            if (z) len = __builtin_ctzll(z);
            else {
                len = 64 - lane;
                for (int cc = c + 1; cc < nw; ++cc) {
                    const ne_u64 zz = ~m[cc];   // bits past w are 0 in the mask: the run ends at w at the latest
                    if (zz) { len += __builtin_ctzll(zz); break; }
                    len += 64;
                }
            }
            // x[onset] >= on, never a NaN; fmaxf skips the NaNs of bridged cells.  Eight loads in flight per round trip: a maximum does
            // not mind a cell taken twice, so the last group re-reads the run's last cell instead of branching
            float pk = x[onset];
            const int last = onset + len - 1;
            for (int t = onset + 1; t <= last; t += 8) {
                float u[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) u[j] = x[min(t + j, last)];
#pragma unroll
                for (int j = 0; j < 8; ++j) pk = fmaxf(pk, u[j]);
            }
            if (vec) reinterpret_cast<ne_i32x4*>(events)[idx] = ne_i32x4{(int)roll, pitch, onset, len};
            else { int* e = events + 4 * idx; e[0] = (int)roll; e[1] = pitch; e[2] = onset; e[3] = len; }
            peaks[idx] = pk;
        }
        emitted += __popcll(starts);
    }
}
