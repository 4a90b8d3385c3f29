// Corruption of a batch of pianorolls for the denoising / infilling objective (include/vae_denoise.h: vae_denoise_corrupt,
// vae_denoise_params): note dropout, a time-span mask and spurious cells, in that order, in ONE launch, with the mask of what was
// hidden.  Pure streaming: the clean batch read, the corrupted one written with 16-byte stores, 1 bit per cell of mask.
//
// A wave owns a row and walks it in chunks of DN_WORDS words of 64 columns.  Pass 1 of a chunk has lane = column: the on-mask of a
// word is a ballot, a note's onset is a set bit whose lower neighbour (the previous word's top bit through carry_on) is clear, the
// onset lane alone hashes the note's draw, and the decision floods the run by ONE 64-bit addition: seeds sit on the lowest bit of
// their runs, so M + X clears exactly the seeded runs (a carry ends in the clear bit above its run and goes no further).  A run that
// crosses into the next word carries its decision in carry_drop, so every cell of a note finds its onset's draw however many words
// the note spans.  Pass 2 has lane = 4 consecutive columns: a 16-byte load of the clean cells (the lines pass 1 just fetched), the
// chunk's masks applied, a 16-byte store.  No atomics, no LDS, nothing read back; every bit is a function of the arguments.
//
// Where it can go wrong, and what guards it (tests/test_denoise_gpu.py sweeps every one past its edge):
//   row guard     r < n * h in the stride loop; a roll's counter, span and pointers are formed from r only
//   column guard  pass 1: t < w, else the lane is off, outside the span and draws nothing; pass 2: t4 < w (w is a multiple of 8, so
//                 a float4 and a mask byte are whole or absent); a word wholly past w is skipped (all its masks are 0)
//   span          (s0, len) drawn or read from spans[b] is INTERSECTED with [0, w) in 64-bit arithmetic: lo = clamp(s0, 0, w),
//                 hi = clamp(s0 + len, lo, w); a negative len hides nothing.  The span only ever enters as the comparison lo <= t < hi
//   word carry    carry_on / carry_drop are bits 63 of M / D: meaningful only after a full word, and a partial word is a row's last
//   seeds         X holds onsets of M, plus bit 0 only where M has bit 0 and the run continues from a dropped one: always the lowest
//                 bit of a run of M, which the flood by addition needs
//   counters      k = counter0 + b * stride and ((k * h + p) * w + t) wrap modulo 2^64 in unsigned arithmetic, as the reference does
//   alignment     clean and out 16-byte aligned (checked by the host), rows are multiples of 32 bytes; hidden is written by bytes
#pragma once
#include "edge_kernels.cuh"

constexpr int DN_STREAM_DROP = 902, DN_STREAM_SPAN = 903, DN_STREAM_ADD = 904;   // counter-generator streams (include/vae_denoise.h)
constexpr int DN_THREADS = 256;        // 4 waves, a row each
constexpr int DN_WORDS = 4;            // words of 64 columns per chunk: pass 2 covers 64 lanes * 4 cells = 256 columns
constexpr int DN_MAX_BLOCKS = 16384;   // capped grid; the rest is a stride loop
typedef unsigned long long dn_u64;

// counter_uniform(i, seed, stream) with the part that does not depend on i taken out: base = dn_base(seed, stream)
__device__ __forceinline__ dn_u64 dn_base(dn_u64 seed, dn_u64 stream) { return splitmix64(splitmix64(seed) ^ (stream * 0xD1342543DE82EF95ULL)); }
__device__ __forceinline__ double dn_uniform(dn_u64 i, dn_u64 base) {
    return (double)(splitmix64(base + i * 0x2545F4914F6CDD1DULL) >> 11) * (1.0 / 9007199254740992.0);
}
// (s0, len) of the roll with counter k: the formulas of vae_denoise_corrupt in include/vae_denoise.h
__device__ __forceinline__ void dn_draw_span(dn_u64 k, dn_u64 base, int w, int span_min, int span_max, int& s0, int& len) {
    s0 = 0; len = 0;
    if (span_max == 0) return;
    len = span_min + (int)(dn_uniform(2 * k, base) * (double)(span_max - span_min + 1));
    s0 = (int)(dn_uniform(2 * k + 1, base) * (double)(w - len + 1));
}

__global__ void denoise_params_kernel(int* __restrict__ spans, long n, int w, int span_min, int span_max, dn_u64 seed, dn_u64 counter0, dn_u64 stride) {
    const dn_u64 base = dn_base(seed, DN_STREAM_SPAN);
    for (long b = blockIdx.x * (long)blockDim.x + threadIdx.x; b < n; b += (long)gridDim.x * blockDim.x) {
        int s0, len;
        dn_draw_span(counter0 + (dn_u64)b * stride, base, w, span_min, span_max, s0, len);
        spans[2 * b] = s0; spans[2 * b + 1] = len;
    }
}

struct CorruptArgs {
    const float* clean; float* out; uint8_t* hidden; long rows; int h, w;
    float thr; double p_drop; int span_min, span_max; double p_add; float add_value;
    const int* spans; dn_u64 seed, counter0, stride;
};

__global__ void __launch_bounds__(DN_THREADS) denoise_corrupt_kernel(const CorruptArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = a.w, wb = w >> 3;
    const bool do_drop = a.p_drop > 0.0, do_add = a.p_add > 0.0;
    const dn_u64 base_drop = dn_base(a.seed, DN_STREAM_DROP), base_span = dn_base(a.seed, DN_STREAM_SPAN), base_add = dn_base(a.seed, DN_STREAM_ADD);
    for (long r = (long)blockIdx.x * (DN_THREADS / 64) + wave; r < a.rows; r += (long)gridDim.x * (DN_THREADS / 64)) {
        const long b = r / a.h; const int p = (int)(r - b * a.h);
        const dn_u64 k = a.counter0 + (dn_u64)b * a.stride;
        int s0, len;
        if (a.spans) { s0 = a.spans[2 * b]; len = a.spans[2 * b + 1]; }
        else dn_draw_span(k, base_span, w, a.span_min, a.span_max, s0, len);
        const int lo = min(max(s0, 0), w);
        const int hi = (int)min(max((long)s0 + (long)len, (long)lo), (long)w);
        const dn_u64 cell0 = (k * (dn_u64)a.h + (dn_u64)p) * (dn_u64)w;   // the counter of cell (p, 0)
        const float* src = a.clean + (size_t)r * w;
        float* dst = a.out + (size_t)r * w;
        uint8_t* hid = a.hidden ? a.hidden + (size_t)r * wb : nullptr;
        dn_u64 carry_on = 0, carry_drop = 0;
        for (int c0 = 0; c0 < w; c0 += 64 * DN_WORDS) {
            dn_u64 Z[DN_WORDS], A[DN_WORDS], Hd[DN_WORDS];   // cells zeroed (dropped or in the span), cells added, cells hidden
#pragma unroll
            for (int q = 0; q < DN_WORDS; ++q) {
                Z[q] = 0; A[q] = 0; Hd[q] = 0;
                if (c0 + 64 * q >= w) continue;   // (wave-uniform)
                const int t = c0 + 64 * q + lane;
                const bool valid = t < w;
                const float v = valid ? src[t] : 0.f;
                const bool on = valid && v >= a.thr;   // (a NaN is off)
                const dn_u64 M = __ballot(on);
                dn_u64 D = 0;
                if (do_drop) {
                    const dn_u64 O = M & ~((M << 1) | carry_on);   // onsets: set, and the cell before (the previous word's last through the carry) clear
                    const bool d = ((O >> lane) & 1) && dn_uniform(cell0 + (dn_u64)t, base_drop) < a.p_drop;
                    const dn_u64 X = __ballot(d) | (carry_on & carry_drop & M & 1);
                    D = M & ~(M + X);
                }
                carry_on = M >> 63; carry_drop = D >> 63;
                const bool in_span = valid && t >= lo && t < hi;
                const dn_u64 S = __ballot(in_span);
                bool add = false;
                if (do_add) add = valid && !on && !in_span && dn_uniform(cell0 + (dn_u64)t, base_add) < a.p_add;
                const dn_u64 Am = __ballot(add);
                const bool zero = ((D | S) >> lane) & 1;
                const float o = zero ? 0.f : add ? a.add_value : v;
                const dn_u64 Mo = __ballot(valid && o >= a.thr);
                Z[q] = D | S; A[q] = Am; Hd[q] = (Mo ^ M) | S;
            }
            // pass 2: lane = cells c0 + 4 lane .. + 3, bits 4 (lane & 15) .. + 3 of word lane >> 4
            const int t4 = c0 + 4 * lane;
            if (t4 < w) {
                const int q = lane >> 4, sh = (lane & 15) * 4;
                const dn_u64 zq = q == 0 ? Z[0] : q == 1 ? Z[1] : q == 2 ? Z[2] : Z[3];
                const dn_u64 aq = q == 0 ? A[0] : q == 1 ? A[1] : q == 2 ? A[2] : A[3];
                const unsigned zn = (unsigned)(zq >> sh) & 15u, an = (unsigned)(aq >> sh) & 15u;
                f32x4 v = *reinterpret_cast<const f32x4*>(src + t4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = ((zn >> e) & 1u) ? 0.f : ((an >> e) & 1u) ? a.add_value : v[e];
                *reinterpret_cast<f32x4*>(dst + t4) = v;
            }
            // the chunk's mask bytes, numpy.packbits order (column 8j is bit 7 of byte j)
            const int bi = (c0 >> 3) + lane;
            if (hid && lane < 8 * DN_WORDS && bi < wb) {
                const int q = lane >> 3;
                const dn_u64 hq = q == 0 ? Hd[0] : q == 1 ? Hd[1] : q == 2 ? Hd[2] : Hd[3];
                hid[bi] = (uint8_t)(__brev((unsigned)((hq >> ((lane & 7) * 8)) & 255u)) >> 24);
            }
        }
    }
}
