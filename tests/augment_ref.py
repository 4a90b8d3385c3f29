"""Reference for the pianoroll gather / augmentation (include/vae_step.h: vae_gather_rolls, vae_augment_params): plain numpy and
Python, the definition as an explicit loop over (b, y, x) on unpacked cells, and the draws from oracle.counter_uniform on stream
901.  Every comparison against it is exact: the outputs are 0/1, integers times a float32 scale, or copied floats."""
import numpy as np

from oracle import vae_oracle as vo

STREAM = 901


def draws(batch, src_w, w, seed, counter0=0, stride=1, P=0, T=0, crop_mode=1):
    """(dy, c0) int64 [batch, 2] of the samples with counters k = counter0 + b * stride:
    dy = (int)(u(2k) * (2P+1)) - P;  c0 = (int)(u(2k+1) * (s + 2T + 1)) - T (mode 0) or s/2 + (int)(u(2k+1) * (2T+1)) - T (mode 1)."""
    out = np.zeros((batch, 2), np.int64)
    if batch == 0:
        return out
    k = counter0 + stride * np.arange(batch, dtype=np.int64)
    u = vo.counter_uniform(2 * int(k.max()) + 2, seed, STREAM)
    s = src_w - w
    out[:, 0] = (u[2 * k] * (2 * P + 1)).astype(np.int64) - P
    if crop_mode == 0:
        out[:, 1] = (u[2 * k + 1] * (s + 2 * T + 1)).astype(np.int64) - T
    else:
        out[:, 1] = s // 2 + (u[2 * k + 1] * (2 * T + 1)).astype(np.int64) - T
    return out


def gather(cells, index, params, w, scale=None):
    """cells [n_rolls, h, src_w] (unpacked); index [batch] integers (any value); params [batch, 2] (dy, c0) -> float32 [batch,1,h,w]:
    dst[b,0,y,x] = S(i, y - dy, c0 + x) if 0 <= i < n_rolls, 0 <= y - dy < h and 0 <= c0 + x < src_w, else 0, with dy clamped to
    [-h, h] and c0 to [-w, src_w].  scale (float32) multiplies byte cells as a float32 product."""
    cells = np.asarray(cells)
    n_rolls, h, src_w = cells.shape
    S = (cells.astype(np.float32) * np.float32(scale)).astype(np.float32) if scale is not None else cells.astype(np.float32)
    S = S.tolist()
    batch = len(index)
    out = [[[0.0] * w for _ in range(h)] for _ in range(batch)]
    for b in range(batch):
        i = int(index[b])
        dy = min(max(int(params[b][0]), -h), h)
        c0 = min(max(int(params[b][1]), -w), src_w)
        for y in range(h):
            for x in range(w):
                if 0 <= i < n_rolls and 0 <= y - dy < h and 0 <= c0 + x < src_w:
                    out[b][y][x] = S[i][y - dy][c0 + x]
    return np.asarray(out, np.float32).reshape(batch, 1, h, w)


def gather_by_roll(cells, index, params, w, scale=None):
    """The same result from an independent formulation: pad the roll with zeros, np.roll it, slice the window."""
    cells = np.asarray(cells)
    n_rolls, h, src_w = cells.shape
    S = (cells.astype(np.float32) * np.float32(scale)).astype(np.float32) if scale is not None else cells.astype(np.float32)
    out = np.zeros((len(index), 1, h, w), np.float32)
    for b, i in enumerate(index):
        if not 0 <= int(i) < n_rolls:
            continue
        dy = int(np.clip(params[b][0], -h, h))
        c0 = int(np.clip(params[b][1], -w, src_w))
        big = np.zeros((3 * h, src_w + 2 * w), np.float32)     # the roll at rows h..2h-1, columns w..w+src_w-1
        big[h:2 * h, w:w + src_w] = S[int(i)]
        big = np.roll(big, (dy, -c0), axis=(0, 1))             # margins of h rows / w columns: nothing wraps into the window
        out[b, 0] = big[h:2 * h, w:2 * w]
    return out


def unpack_bits(planes, src_w):
    return np.unpackbits(np.asarray(planes, np.uint8), axis=-1)[..., :src_w]
