"""CPU definition of the corruption kernel (include/vae_denoise.h: vae_denoise_corrupt, vae_denoise_params) in plain numpy: an explicit
loop over rolls and pitch rows, notes found as runs of the thresholded row, every draw from the counter generator of the oracle
(splitmix64 over seed, stream and counter) on streams 902 / 903 / 904, all counter arithmetic modulo 2^64.  Every comparison against
it is exact: the outputs are copied floats, 0.f, add_value, integers and bits."""
import numpy as np

from oracle import vae_oracle as vo

STREAM_DROP, STREAM_SPAN, STREAM_ADD = 902, 903, 904
_M64 = (1 << 64) - 1


def uniform_at(idx, seed, stream):
    """counter_uniform(i, seed, stream) of the library for the counters ``idx`` (Python ints or an array, taken modulo 2^64)."""
    idx = np.array([int(i) & _M64 for i in np.atleast_1d(np.asarray(idx, dtype=object)).ravel()], dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = vo._splitmix64(np.array([int(seed) & _M64], dtype=np.uint64))
        base = vo._splitmix64(base ^ (np.uint64(stream) * np.uint64(0xD1342543DE82EF95)))
        bits = vo._splitmix64(base + idx * np.uint64(0x2545F4914F6CDD1D))
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def roll_counter(b, counter0, counter_stride):
    return (int(counter0) + int(b) * int(counter_stride)) & _M64


def spans_ref(n, w, span_min, span_max, seed, counter0=0, counter_stride=1):
    """int32 [n, 2]: the (s0, len) vae_denoise_params writes; (0, 0) with span_max == 0."""
    out = np.zeros((n, 2), dtype=np.int32)
    if span_max == 0:
        return out
    for b in range(n):
        k = roll_counter(b, counter0, counter_stride)
        u = uniform_at([2 * k, 2 * k + 1], seed, STREAM_SPAN)
        ln = span_min + int(u[0] * (span_max - span_min + 1))
        out[b] = (int(u[1] * (w - ln + 1)), ln)
    return out


def row_runs(on):
    """[(t0, t1)] of the maximal runs of True in a 1-D boolean row."""
    d = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def corrupt_ref(clean, *, threshold=0.5, p_drop=0.0, span=None, p_add=0.0, add_value=1.0, spans=None, seed=0, counter0=0,
                counter_stride=1, info=None):
    """(out float32 [n,h,w], hidden uint8 [n,h,w/8]) of clean float32 [n,h,w].  span: None or (span_min, span_max); spans: integers
    [n, 2] used instead of the draw, intersected with the roll.  ``info`` (a dict) receives the counts notes, dropped, kept,
    crossing_dropped / crossing_kept (notes with cells on both sides of a multiple of 64), added, and the spans used."""
    clean = np.ascontiguousarray(clean, dtype=np.float32)
    n, h, w = clean.shape
    thr = np.float32(threshold)
    smin, smax = (0, 0) if span is None else (int(span[0]), int(span[1]))
    used = np.asarray(spans, dtype=np.int64).reshape(n, 2) if spans is not None else spans_ref(n, w, smin, smax, seed, counter0, counter_stride).astype(np.int64)
    out = clean.copy()
    in_span = np.zeros((n, h, w), dtype=bool)
    counts = dict(notes=0, dropped=0, kept=0, crossing_dropped=0, crossing_kept=0, added=0)
    with np.errstate(invalid="ignore"):
        on = clean >= thr                                   # (a NaN is off)
    for b in range(n):
        k = roll_counter(b, counter0, counter_stride)
        s0, ln = int(used[b, 0]), int(used[b, 1])
        lo = min(max(s0, 0), w)
        hi = min(max(s0 + ln, lo), w)
        in_span[b, :, lo:hi] = True
        for p in range(h):
            cell0 = (k * h + p) * w                          # (Python integers: reduced modulo 2^64 where they are hashed)
            if p_drop > 0.0:
                runs = row_runs(on[b, p])
                u = uniform_at([cell0 + t0 for t0, _ in runs], seed, STREAM_DROP) if runs else []
                for (t0, t1), ui in zip(runs, u):
                    crossing = t0 // 64 != (t1 - 1) // 64
                    counts["notes"] += 1
                    if ui < p_drop:
                        out[b, p, t0:t1] = 0.0
                        counts["dropped"] += 1
                        counts["crossing_dropped"] += crossing
                    else:
                        counts["kept"] += 1
                        counts["crossing_kept"] += crossing
            out[b, p, lo:hi] = 0.0
            if p_add > 0.0:
                cand = np.flatnonzero(~on[b, p] & ~in_span[b, p])
                if cand.size:
                    hit = cand[uniform_at([cell0 + int(t) for t in cand], seed, STREAM_ADD) < p_add]
                    out[b, p, hit] = np.float32(add_value)
                    counts["added"] += int(hit.size)
    with np.errstate(invalid="ignore"):
        hidden = ((out >= thr) != on) | in_span
    if info is not None:
        info.update(counts, spans=used)
    return out, np.packbits(hidden, axis=-1)
