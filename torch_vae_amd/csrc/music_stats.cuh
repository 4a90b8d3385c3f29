// Per-roll musical statistics of bit-plane pianorolls (include/vae_music.h: vae_music_roll_stats) and their totals over a set.
//
// Mapping: ONE WAVE PER ROLL, one wave per workgroup (the barriers between the passes then order one wave's LDS traffic and the
// compiler emits no s_barrier for them), at most 32768 workgroups that walk the rolls with a grid stride.  A roll is at most
// 8 KiB, so the wave stages it in LDS once - coalesced dword loads, byte-swapped so that bit 31 of a word is its earliest step,
// stored word column by word column ([w/32][h]) - and makes
// two passes over that image:
//   rows     a lane per pitch row (consecutive lanes read consecutive LDS words) walks the row's words: cells (popcount), onsets
//            m & ~((m >> 1) | (prev << 31)), run lengths across word boundaries (count-leading-zeros / -ones steps) into
//            per-lane 16-bit duration counters packed in three 64-bit registers, the row's pitch class; the onset words are
//            OR-ed across the wave, per word column;
//   columns  a lane per time step adds the step's bit of every row, four rows per 16-byte LDS read when h is a multiple of 4
//            (the 32 lanes of a word column read one address: a broadcast); the polyphony histogram is 16 ballots per 64
//            steps; the gaps between onset steps come from the onset words, 64 words at a time, each lane taking the last
//            onset in front of its word from the nearest lower lane that has one.
// LDS integer atomics remain only where lanes rarely meet: two per row in use (12 pitch classes) and one per gap between onset
// steps; everything else is wave reductions (cells, notes and used rows share one 64-bit sum).  (An LDS atomic per
// note makes all 64 lanes meet on one address: most notes of a roll fall in one duration bucket.)  The feature row leaves as two coalesced
// stores.  All counts are integers: no result depends on an arrival order.  The totals are a second kernel over the [n][76] table
// (a thread per column, 256 rolls per workgroup) that ends in one 64-bit integer atomic per column and workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MS_FEATURES 76
#define MS_WAVES 1                 // rolls (waves) per workgroup of music_roll_stats_kernel
#define MS_MAX_ROLL_BYTES 8192
#define MS_MAX_BLOCKS (32768 / MS_WAVES)
#define MS_TOTAL_ROLLS 256         // rolls per workgroup of music_totals_kernel
#define MS_TOTAL_GROUPS 3          // row groups of 76 threads in its 256
// columns of a feature row (include/vae_music.h)
#define MS_ROLLS 0
#define MS_NONEMPTY 1
#define MS_CELLS 2
#define MS_NOTES 3
#define MS_USED 4
#define MS_LOWEST 5
#define MS_HIGHEST 6
#define MS_SOUNDING 7
#define MS_ONSET_STEPS 8
#define MS_MAX_POLY 9
#define MS_PC_CELLS 10
#define MS_PC_NOTES 22
#define MS_DURATION 34
#define MS_POLYPHONY 46
#define MS_IOI 62

struct MusicArgs {
    const unsigned* planes;   // [n][h][wd] words as stored (numpy.packbits bytes)
    long n;
    int h, wd;                // rows; words per row
    int wd_shift;             // log2(wd) when wd is a power of two, else -1
    int pitch_offset;
    int* features;            // [n][76]
};

// words of LDS one wave needs: the roll, the onset word per word column (each rounded up to 16 bytes), the feature row
__host__ __device__ inline int ms_wave_words(int h, int wd) { return ((h * wd + 3) & ~3) + ((wd + 3) & ~3) + MS_FEATURES; }

__device__ __forceinline__ int ms_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long ms_wave_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned ms_wave_or(unsigned v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int ms_wave_max(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int ms_wave_min(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__host__ __device__ __forceinline__ int ms_clz(unsigned v) { return v ? __builtin_clz(v) : 32; }
__host__ __device__ __forceinline__ int ms_log2_bucket(int v) { const int b = 31 - ms_clz((unsigned)v); return b < 11 ? b : 11; }   // v >= 1

// The notes of one row word m (bit 31 = its earliest step), given `run`, the length of the note that is open at the word's left
// edge (0: none): note(length) for every note that ends inside the word; `run` becomes the length of the note open at its right edge.
template <typename Note> __host__ __device__ __forceinline__ void ms_walk_word(unsigned m, int& run, Note&& note) {
    unsigned x = m;
    int rem = 32;                               // bits of the word still in x, left-aligned
    if (run) {
        const int ones = ms_clz(~x);            // 32 for a full word
        run += ones;
        if (ones == 32) return;
        note(run);
        run = 0;
        x <<= ones;
        rem -= ones;
    }
    while (x) {
        const int z = ms_clz(x);
        x <<= z;
        rem -= z;
        const int ones = ms_clz(~x);
        if (ones == rem) { run = ones; return; }   // the note reaches the end of the word
        note(ones);
        x <<= ones;
        rem -= ones;
    }
}

// The onset steps of one onset word o whose bit 31 is step t0, given p, the onset step in front of it (-1: none): gap(g) for every
// gap between consecutive onset steps; p becomes the last onset step seen.
template <typename Gap> __host__ __device__ __forceinline__ void ms_walk_onsets(unsigned o, int t0, int& p, Gap&& gap) {
    while (o) {
        const int z = ms_clz(o);
        const int t = t0 + z;
        if (p >= 0) gap(t - p);
        p = t;
        o &= ~(0x80000000u >> z);
    }
}

__global__ __launch_bounds__(64 * MS_WAVES) void music_roll_stats_kernel(MusicArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned ms_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = a.h, wd = a.wd, words = h * wd, w = wd * 32;
    unsigned* img = ms_lds + (size_t)wave * ms_wave_words(h, wd);   // [wd][h]: word column j of row r at j * h + r
    unsigned* ons = img + ((words + 3) & ~3);                        // [wd]: OR over the rows of the onset words
    int* feat = reinterpret_cast<int*>(ons + ((wd + 3) & ~3));       // [76]
    // (every wave of a workgroup makes the same number of trips: the barriers below are reached by all of them)
    for (long base = (long)blockIdx.x * MS_WAVES; base < a.n; base += (long)gridDim.x * MS_WAVES) {
        const long roll = base + wave;
        const bool live = roll < a.n;
        if (live) {
            const unsigned* src = a.planes + roll * words;
            for (int i = lane; i < words; i += 64) {
                const unsigned v = __builtin_bswap32(src[i]);
                int r, j;
                if (a.wd_shift >= 0) { r = i >> a.wd_shift; j = i & (wd - 1); }
                else { r = i / wd; j = i - r * wd; }
                img[j * h + r] = v;
            }
            for (int c = lane; c < MS_FEATURES; c += 64) feat[c] = 0;
        }
        __syncthreads();
        if (live) {
            // ---- rows: 64 at a time, a lane each; every lane makes every trip (the onset words are OR-ed across the wave) ----
            int cells = 0, notes = 0, used = 0, lowest = INT32_MAX, highest = -1;
            unsigned long long d0 = 0ull, d1 = 0ull, d2 = 0ull;       // duration buckets 0..3, 4..7, 8..11 in 16-bit fields
            for (int r0 = 0; r0 < h; r0 += 64) {
                const int r = r0 + lane;
                const bool valid = r < h;
                int row_cells = 0, row_notes = 0, run = 0;     // run: length of the note that is open at the word boundary
                unsigned prev = 0u;
                auto note = [&](int length) {
                    const int b = ms_log2_bucket(length);
                    const unsigned long long one = 1ull << ((b & 3) * 16);
                    d0 += b < 4 ? one : 0ull;
                    d1 += (b >= 4 && b < 8) ? one : 0ull;
                    d2 += b >= 8 ? one : 0ull;
                    ++row_notes;
                };
                for (int j = 0; j < wd; ++j) {
                    const unsigned m = valid ? img[j * h + r] : 0u;
                    const unsigned on = ms_wave_or(m & ~((m >> 1) | (prev << 31)));
                    prev = m;
                    if (lane == 0) ons[j] = r0 ? (ons[j] | on) : on;
                    row_cells += __popc(m);
                    ms_walk_word(m, run, note);
                }
                if (run) note(run);
                if (row_cells) {
                    const int pc = (r + a.pitch_offset) % 12;
                    atomicAdd(&feat[MS_PC_CELLS + pc], row_cells);
                    atomicAdd(&feat[MS_PC_NOTES + pc], row_notes);
                    cells += row_cells;
                    notes += row_notes;
                    ++used;
                    lowest = min(lowest, r);
                    highest = max(highest, r);
                }
            }
            // (a roll has at most 65536 cells, 32768 notes and 2048 rows: one 64-bit sum carries the three, and the wave's sum of a
            //  16-bit duration field stays below 2^16)
            const unsigned long long sums = ms_wave_sum64((unsigned long long)cells | ((unsigned long long)notes << 20) | ((unsigned long long)used << 40));
            d0 = ms_wave_sum64(d0);
            d1 = ms_wave_sum64(d1);
            d2 = ms_wave_sum64(d2);
            lowest = ms_wave_min(lowest);
            highest = ms_wave_max(highest);
            cells = (int)(sums & 0xFFFFFu);
            if (lane == 0) {
                feat[MS_ROLLS] = 1;
                feat[MS_NONEMPTY] = cells > 0;
                feat[MS_CELLS] = cells;
                feat[MS_NOTES] = (int)((sums >> 20) & 0xFFFFFu);
                feat[MS_USED] = (int)(sums >> 40);
                feat[MS_LOWEST] = cells > 0 ? lowest : -1;
                feat[MS_HIGHEST] = highest;
            }
            if (lane < 12) {
                const unsigned long long d = lane < 4 ? d0 : (lane < 8 ? d1 : d2);
                feat[MS_DURATION + lane] = (int)((d >> ((lane & 3) * 16)) & 0xFFFFu);
            }
            // ---- columns: cells per time step, a lane per step; the 32 lanes of a word column read the same LDS words ----
            int poly[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) poly[k] = 0;
            int top = 0;
            for (int t0 = 0; t0 < w; t0 += 64) {                // (w is a multiple of 32: the upper half may be past the end)
                const int t = t0 + lane;
                const bool in = t < w;
                int count = 0;
                if (in) {
                    const unsigned* col = img + (t >> 5) * h;
                    const int sh = 31 - (t & 31);
                    if ((h & 3) == 0) {                          // four rows per 16-byte read (j * h is a multiple of 4 then)
                        for (int r = 0; r < h; r += 4) {
                            const uint4 v = *reinterpret_cast<const uint4*>(col + r);
                            count += ((v.x >> sh) & 1u) + ((v.y >> sh) & 1u) + ((v.z >> sh) & 1u) + ((v.w >> sh) & 1u);
                        }
                    } else {
                        for (int r = 0; r < h; ++r) count += (col[r] >> sh) & 1u;
                    }
                }
                top = max(top, count);
                const int kk = in ? min(count, 15) : -1;
#pragma unroll
                for (int k = 0; k < 16; ++k) poly[k] += __popcll(__ballot(kk == k));
            }
            top = ms_wave_max(top);
            if (lane < 16) {
                int mine = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) mine = lane == k ? poly[k] : mine;
                feat[MS_POLYPHONY + lane] = mine;
            }
            if (lane == 0) {
                feat[MS_MAX_POLY] = top;
                feat[MS_SOUNDING] = w - poly[0];
            }
        }
        __syncthreads();      // the onset words are complete
        if (live) {
            // ---- gaps between consecutive onset steps ----
            int onset_steps = 0, last = -1;                     // last: the latest onset step in front of this chunk (wave-uniform)
            for (int j0 = 0; j0 < wd; j0 += 64) {
                const int j = j0 + lane;
                const unsigned o = j < wd ? ons[j] : 0u;
                onset_steps += __popc(o);
                const unsigned long long has = __ballot(o != 0u);
                const int my_last = o ? j * 32 + 31 - (__ffs(o) - 1) : -1;
                const unsigned long long below = has & ((1ull << lane) - 1ull);
                const int from_lane = __shfl(my_last, below ? 63 - __clzll(below) : 0);
                int p = below ? from_lane : last;
                ms_walk_onsets(o, j * 32, p, [&](int g) { atomicAdd(&feat[MS_IOI + ms_log2_bucket(g)], 1); });
                const int chunk_last = __shfl(my_last, has ? 63 - __clzll(has) : 0);
                if (has) last = chunk_last;
            }
            onset_steps = ms_wave_sum(onset_steps);
            if (lane == 0) feat[MS_ONSET_STEPS] = onset_steps;
        }
        __syncthreads();      // the feature row is complete
        if (live) {
            int* dst = a.features + roll * MS_FEATURES;
            for (int c = lane; c < MS_FEATURES; c += 64) dst[c] = feat[c];
        }
        __syncthreads();      // nobody clears what another lane still reads
    }
}

// totals <- the empty value: zeros, lowest -1, highest -1
__global__ void music_totals_init_kernel(long long* totals) {
    const int c = threadIdx.x;
    if (c < MS_FEATURES) totals[c] = (c == MS_LOWEST || c == MS_HIGHEST) ? -1ll : 0ll;
}

// totals (+)= the columns of features [n][76]: sums, but the minimum of `lowest` over the non-empty rolls (-1 = none, the largest
// value as an unsigned word) and the maxima of `highest` and `max_polyphony`.  Thread (g, c) adds column c of every third roll of
// the workgroup's 256; consecutive threads read consecutive words.
__global__ __launch_bounds__(256) void music_totals_kernel(const int* features, long n, long long* totals) {
    __shared__ long long part[MS_TOTAL_GROUPS][MS_FEATURES];
    const int tid = threadIdx.x, g = tid / MS_FEATURES, c = tid - g * MS_FEATURES;
    const bool is_min = c == MS_LOWEST, is_max = c == MS_HIGHEST || c == MS_MAX_POLY;
    if (g < MS_TOTAL_GROUPS) {
        long long acc = is_min ? -1ll : (c == MS_HIGHEST ? -1ll : 0ll);
        for (long first = (long)blockIdx.x * MS_TOTAL_ROLLS; first < n; first += (long)gridDim.x * MS_TOTAL_ROLLS) {
            const long end = first + MS_TOTAL_ROLLS < n ? first + MS_TOTAL_ROLLS : n;
            for (long r = first + g; r < end; r += MS_TOTAL_GROUPS) {
                const long long v = features[r * MS_FEATURES + c];
                if (is_min) acc = (unsigned long long)v < (unsigned long long)acc ? v : acc;
                else if (is_max) acc = v > acc ? v : acc;
                else acc += v;
            }
        }
        part[g][c] = acc;
    }
    __syncthreads();
    if (tid < MS_FEATURES) {
        long long acc = part[0][tid];
        for (int k = 1; k < MS_TOTAL_GROUPS; ++k) {
            const long long v = part[k][tid];
            if (is_min) acc = (unsigned long long)v < (unsigned long long)acc ? v : acc;
            else if (is_max) acc = v > acc ? v : acc;
            else acc += v;
        }
        if (is_min) atomicMin(reinterpret_cast<unsigned long long*>(totals + tid), (unsigned long long)acc);
        else if (is_max) atomicMax(totals + tid, acc);
        else if (acc) atomicAdd(reinterpret_cast<unsigned long long*>(totals + tid), (unsigned long long)acc);
    }
}
