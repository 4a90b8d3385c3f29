"""The pianoroll gather / augmentation kernel and the device loader on the GPU, against tests/augment_ref.py.  Every comparison is
exact.  In all kernel tests the source is a view into the middle of a larger buffer filled with ones (0xFF bytes, or 1.0f): a
missing or wrong guard shows up as wrong values in the comparison, never as a stray access."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests import augment_ref as ar
from tests.util import make_model
from torch_vae_amd import _lib, data

pytestmark = pytest.mark.gpu

PAD = 4096   # bytes of filler on either side of the source (a multiple of 16: the source keeps the buffer's alignment)


def embed(arr, pinned=False, shift=0):
    """arr (numpy uint8 or float32) as a tensor that views the middle of a larger buffer of ones; `shift` more bytes in front."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if t.dtype == torch.float32:
        assert shift % 4 == 0
        buf = torch.ones(2 * PAD // 4 + shift // 4 + t.numel(), dtype=torch.float32)
        lo = PAD // 4 + shift // 4
    else:
        buf = torch.full((2 * PAD + shift + t.numel(),), 0xFF, dtype=torch.uint8)
        lo = PAD + shift
    buf[lo:lo + t.numel()] = t.reshape(-1)
    buf = buf.pin_memory() if pinned else buf.cuda()
    return buf[lo:lo + t.numel()].view(t.shape), buf


def dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def sweep_params():
    """every (dy, c0) with dy in [-10, 10] and c0 in [-20, 44]: 1365 samples"""
    return np.array([(dy, c0) for dy in range(-10, 11) for c0 in range(-20, 45)], np.int64)


def source(kind, n, h, src_w, seed):
    """(cells [n, h, src_w] unpacked, stored array the kernel reads)"""
    rng = np.random.default_rng(seed)
    if kind == "bits":
        cells = rng.integers(0, 2, (n, h, src_w)).astype(np.uint8)
        return cells, np.packbits(cells, axis=-1)
    if kind == "bytes":
        cells = rng.integers(0, 128, (n, h, src_w)).astype(np.uint8)
        return cells, cells
    cells = rng.standard_normal((n, h, src_w)).astype(np.float32)
    return cells, cells


def run(src, kind, w, index=None, params=None, **kw):
    out = data.gather_rolls(src, kind, w, index=None if index is None else dev(index, torch.int64),
                            params=None if params is None else dev(params, torch.int32), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# 1. bit planes, exhaustive offsets, smallest shapes
@pytest.mark.parametrize("w,src_w", [(16, 40), (8, 8), (24, 24)])
def test_bit_planes_every_offset(w, src_w):
    h, n = 8, 3
    cells, stored = source("bits", n, h, src_w, 1)
    src, _keep = embed(stored)
    params = sweep_params()
    index = np.arange(len(params)) % n
    assert len(params) == 1365
    got = run(src, "bits", w, index=index, params=params)
    assert np.array_equal(got, ar.gather(cells, index, params, w))


# 2. kinds 0 and 2, the same sweep
@pytest.mark.parametrize("kind,scale,shift", [("bytes", 1.0, 0), ("bytes", 1 / 127, 0), ("bytes", 1.0, 3), ("f32", 1.0, 0), ("f32", 1.0, 4)])
def test_bytes_and_floats_every_offset(kind, scale, shift):
    h, n, w, src_w = 8, 3, 16, 40
    cells, stored = source(kind, n, h, src_w, 2)
    src, _keep = embed(stored, shift=shift)     # (shift: a source off the 8- / 16-byte alignment of the wide loads)
    params = sweep_params()
    index = np.arange(len(params)) % n
    got = run(src, kind, w, index=index, params=params, scale=scale)
    want = ar.gather(cells, index, params, w, np.float32(scale) if kind == "bytes" else None)
    assert np.array_equal(got, want)


# 3. index handling
@pytest.mark.parametrize("kind", ["bits", "bytes", "f32"])
def test_index_handling(kind):
    h, n, w, src_w = 8, 6, 16, 40
    cells, stored = source(kind, n, h, src_w, 3)
    src, _keep = embed(stored)
    sc = None if kind != "bytes" else np.float32(1.0)
    # repeats and a reversed order
    index = np.array([5, 4, 3, 2, 1, 0, 0, 0, 3, 3, 5])
    params = np.stack([np.arange(11) % 3 - 1, np.arange(11) * 3 - 4], 1)
    assert np.array_equal(run(src, kind, w, index=index, params=params), ar.gather(cells, index, params, w, sc))
    # no index: rolls first .. first + batch - 1, the last two past the end
    got = run(src, kind, w, first=2, batch=6, params=params[:6])
    assert np.array_equal(got, ar.gather(cells, np.arange(2, 8), params[:6], w, sc))
    assert not got[4:].any()
    # indices outside [0, n) give zero rolls, their neighbours are right
    index = np.array([0, -1, 1, n, 2, 2 ** 40, 3, -2 ** 40, 4, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 5])
    params = np.tile([0, 12], (len(index), 1))
    got = run(src, kind, w, index=index, params=params)
    assert np.array_equal(got, ar.gather(cells, index, params, w, sc))
    for b, i in enumerate(index):
        assert got[b].any() == (0 <= i < n)


# 4. draws
@functools.lru_cache(None)
def draw_case(crop_mode):
    h, n, w, src_w, P, T, B, seed, c0 = 8, 5, 32, 64, 3, 5, 4096, 11, 1000
    cells, stored = source("bits", n, h, src_w, 4)
    index = np.arange(B) % n
    d = ar.draws(B, src_w, w, seed, counter0=c0, P=P, T=T, crop_mode=crop_mode)
    return cells, stored, index, d, ar.gather(cells, index, d, w)


@pytest.mark.parametrize("crop_mode", [0, 1])
def test_draws(crop_mode):
    w, src_w, P, T, B, seed, c0 = 32, 64, 3, 5, 4096, 11, 1000
    cells, stored, index, d, want = draw_case(crop_mode)
    src, _keep = embed(stored)
    kw = dict(seed=seed, counter0=c0, max_pitch_shift=P, max_time_shift=T, crop_mode=crop_mode)
    prm = data.augmentation_params(B, src_w, w, **kw)
    assert prm.dtype == torch.int32 and tuple(prm.shape) == (B, 2)
    assert np.array_equal(prm.cpu().numpy(), d)
    s = src_w - w
    assert set(d[:, 0]) == set(range(-P, P + 1))
    assert set(d[:, 1]) == (set(range(-T, s + T + 1)) if crop_mode == 0 else set(range(s // 2 - T, s // 2 + T + 1)))
    inside = run(src, "bits", w, index=index, **kw)
    given = data.gather_rolls(src, "bits", w, index=dev(index, torch.int64), params=prm).cpu().numpy()
    assert np.array_equal(inside, given)
    assert np.array_equal(inside, want)
    # the same seed gives the same draws, another seed or counter0 other ones
    assert np.array_equal(run(src, "bits", w, index=index, **kw), inside)
    for other in (dict(seed=seed + 1), dict(counter0=c0 + 1)):
        p2 = data.augmentation_params(B, src_w, w, **{**kw, **other}).cpu().numpy()
        assert not np.array_equal(p2, d)
        assert not np.array_equal(run(src, "bits", w, index=index, **{**kw, **other}), inside)
    assert np.array_equal(data.augmentation_params(B - 1, src_w, w, **{**kw, "counter0": c0 + 1}).cpu().numpy(), d[1:])
    # two half batches with counter0 and counter0 + 2048 equal the whole; a stride of 2 takes every other draw
    a = run(src, "bits", w, index=index[:2048], **kw)
    b = run(src, "bits", w, index=index[2048:], **{**kw, "counter0": c0 + 2048})
    assert np.array_equal(np.concatenate([a, b]), inside)
    p2 = data.augmentation_params(2048, src_w, w, **kw, counter_stride=2).cpu().numpy()
    assert np.array_equal(p2, d[::2])
    assert np.array_equal(run(src, "bits", w, index=index[::2], **kw, counter_stride=2), want[::2])


def test_centre_crop_without_shifts_draws_nothing():
    prm = data.augmentation_params(64, 48, 16, seed=5, counter0=9, crop_mode=_lib.CROP_CENTRE).cpu().numpy()
    assert np.array_equal(prm, np.tile([0, 16], (64, 1)))


# 5. agreement with the existing kernel
@pytest.mark.parametrize("B,H", [(8, 32), (4, 128)])
@pytest.mark.parametrize("kind", ["bytes", "bits"])
def test_identity_equals_expand_stimuli(kind, B, H):
    cells, stored = source(kind, B, H, H, 5)
    src, _keep = embed(stored)
    got = data.gather_rolls(src, kind, H, batch=B)
    want = torch.full((B, 1, H, H), 7.0, device="cuda")
    _lib.check(_lib.lib().vae_expand_stimuli(src.data_ptr(), _lib.ROLLS_BITS if kind == "bits" else _lib.ROLLS_BYTES, want.data_ptr(),
                                             B * H * H, torch.cuda.current_stream().cuda_stream), "vae_expand_stimuli")
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy()[:, 0], cells.astype(np.float32))


# 6. the stride loops' second pass: over the samples (grid y), over the rows of a roll (grid x), along a row (the lanes of a tile)
def gather_grid(batch, h, w):
    """(lanes along a row, grid x, grid y) of the launch vae_gather_rolls makes (torch_vae_amd/_lib.py)"""
    tx = 1
    while tx < w // _lib.GATHER_CELLS_PER_LANE and tx < _lib.GATHER_MAX_ROW_LANES:
        tx *= 2
    rows = _lib.GATHER_THREADS // tx
    gx = min(-(-h // rows), _lib.GATHER_MAX_BLOCKS)
    return tx, gx, min(batch, max(1, _lib.GATHER_MAX_BLOCKS // gx))


def test_second_pass_over_the_samples():
    h, w, src_w, n = 1, 8, 16, 7                         # the smallest roll: one workgroup in x, so y takes the whole cap
    B = _lib.GATHER_MAX_BLOCKS + 1                        # one sample more than one pass of the grid's y covers
    assert gather_grid(B, h, w) == (1, 1, B - 1)
    rng = np.random.default_rng(6)
    cells, stored = source("bits", n, h, src_w, 6)
    src, _keep = embed(stored)
    index = rng.integers(-1, n + 1, B)
    params = np.stack([rng.integers(-1, 2, B), rng.integers(-9, 18, B)], 1)
    index[-1], params[-1] = 3, (0, 5)                    # (the one sample of the second pass is not an empty one)
    got = run(src, "bits", w, index=index, params=params)
    want = ar.gather(cells, index, params, w)
    assert want[-1].any()
    assert np.array_equal(got, want)


def test_second_pass_over_the_rows():
    w, src_w, B = 8, 16, 1                                # one lane per row: a workgroup covers the most rows, 256
    h = _lib.GATHER_THREADS * _lib.GATHER_MAX_BLOCKS + 1  # one row more than one pass of the grid's x covers
    assert gather_grid(B, h, w) == (1, _lib.GATHER_MAX_BLOCKS, 1)
    cells, stored = source("bits", 2, h, src_w, 6)
    src, _keep = embed(stored)
    index, params = np.array([1]), np.array([[-1, 3]])   # off the byte grid; up one row, so the last row holds the roll's last
    got = run(src, "bits", w, index=index, params=params)
    want = ar.gather(cells, index, params, w)
    assert want[0, 0, -2:].any()
    assert np.array_equal(got, want)


def test_second_pass_along_a_row():
    h, n, B = 3, 2, 5
    w = _lib.GATHER_CELLS_PER_LANE * (_lib.GATHER_MAX_ROW_LANES + 2)     # two work items more than the lanes along a row
    src_w = w + 16
    assert gather_grid(B, h, w) == (_lib.GATHER_MAX_ROW_LANES, 1, B)
    cells, stored = source("bits", n, h, src_w, 6)
    src, _keep = embed(stored)
    index = np.arange(B) % n
    params = np.array([(0, 0), (1, 5), (-1, 16), (0, 21), (0, -3)])
    got = run(src, "bits", w, index=index, params=params)
    assert np.array_equal(got, ar.gather(cells, index, params, w))


# 7. pinned host source
@pytest.mark.parametrize("kind", ["bytes", "bits"])
def test_pinned_host_source(kind):
    h, n, w, src_w = 8, 3, 16, 40
    cells, stored = source(kind, n, h, src_w, 7)
    on_dev, _k1 = embed(stored)
    on_host, _k2 = embed(stored, pinned=True)
    assert on_host.is_pinned() and not on_host.is_cuda
    params = sweep_params()
    index = np.arange(len(params)) % n
    a = run(on_dev, kind, w, index=index, params=params, scale=0.5)
    b = run(on_host, kind, w, index=index, params=params, scale=0.5, device="cuda")
    assert np.array_equal(a, b)
    assert np.array_equal(a, ar.gather(cells, index, params, w, np.float32(0.5) if kind == "bytes" else None))
    with pytest.raises(_lib.VaeLibError, match="neither device nor pinned host memory"):
        data.gather_rolls(torch.from_numpy(stored.copy()), kind, w, batch=2, device="cuda")


# 8. loader
N, LH, LWS, LW, LB = 37, 16, 48, 16, 8


@functools.lru_cache(None)
def loader_rolls():
    return np.random.default_rng(8).integers(0, 2, (N, LH, LWS)).astype(np.uint8)


def batches_of(loader, with_params=False):
    xs, ps = [], []
    for x, y in loader:
        assert x.dtype == torch.float32 and x.is_cuda and tuple(x.shape[1:]) == (1, LH, LW)
        assert y.shape[0] == x.shape[0]
        xs.append(x.cpu().numpy())
        if with_params:
            ps.append(loader.last_params().cpu().numpy())
    return (xs, ps) if with_params else xs


def test_loader_eval():
    cells = loader_rolls()
    ds = data.PianorollDataset(torch.from_numpy(cells))
    assert ds.storage == "bits" and ds.data.is_cuda
    assert np.array_equal(ds[5].cpu().numpy(), cells[5:6].astype(np.float32))
    ev = data.DevicePianorollLoader(ds, LB, width=LW, train=False, max_pitch_shift=2, max_time_shift=3, rank=0, world=1)
    xs = batches_of(ev)
    assert [len(x) for x in xs] == [8, 8, 8, 8, 5] and len(ev) == 5
    want = cells[:, None, :, 16:32].astype(np.float32)      # the centre window, loader order
    assert np.array_equal(np.concatenate(xs), want)
    assert np.array_equal(np.concatenate(xs), ar.gather(cells, np.arange(N), np.tile([0, 16], (N, 1)), LW))
    ev = data.DevicePianorollLoader(ds, LB, width=LW, train=False, drop_last=True, rank=0, world=1)
    xs = batches_of(ev)
    assert [len(x) for x in xs] == [8, 8, 8, 8] and len(ev) == 4
    assert np.array_equal(np.concatenate(xs), want[:32])


def test_loader_train():
    cells = loader_rolls()
    ds = data.PianorollDataset(torch.from_numpy(cells))
    P, T, seed = 2, 3, 4
    mk = lambda **kw: data.DevicePianorollLoader(ds, LB, width=LW, seed=seed, max_pitch_shift=P, max_time_shift=T, **{"rank": 0, "world": 1, **kw})
    tr = mk()
    xs, ps = batches_of(tr, with_params=True)
    idx = data.epoch_indices(N, seed=seed, epoch=0, shuffle=True, rank=0, world=1, drop_last=False).numpy()
    assert sorted(idx.tolist()) == list(range(N))           # over an epoch every index occurs once
    d = ar.draws(N, LWS, LW, seed, counter0=0, P=P, T=T, crop_mode=0)
    want0 = ar.gather(cells, idx, d, LW)
    assert [len(x) for x in xs] == [8, 8, 8, 8, 5]
    assert np.array_equal(np.concatenate(xs), want0)
    assert np.array_equal(np.concatenate(ps), d)            # last_params()
    assert (d[:, 0] != 0).any() and len(set(d[:, 1])) > 8
    assert np.array_equal(np.concatenate(batches_of(mk())), want0)      # two loaders built alike agree
    # the augmentation does not depend on the batch size
    big = data.DevicePianorollLoader(ds, N, width=LW, seed=seed, max_pitch_shift=P, max_time_shift=T, rank=0, world=1)
    assert np.array_equal(np.concatenate(batches_of(big)), want0)
    # epoch 1: another order and other draws, counters N .. 2N-1
    tr.set_epoch(1)
    x1 = np.concatenate(batches_of(tr))
    assert not np.array_equal(x1, want0)
    idx1 = data.epoch_indices(N, seed=seed, epoch=1, shuffle=True, rank=0, world=1, drop_last=False).numpy()
    assert np.array_equal(x1, ar.gather(cells, idx1, ar.draws(N, LWS, LW, seed, counter0=N, P=P, T=T, crop_mode=0), LW))
    # two ranks partition the (padded) epoch, and every roll gets the augmentation its global position dictates
    total = 38
    for epoch in (0, 2):
        whole = ar.draws(total, LWS, LW, seed, counter0=epoch * total, P=P, T=T, crop_mode=0)
        perm = data.epoch_indices(N, seed=seed, epoch=epoch, shuffle=True, rank=0, world=1, drop_last=False).numpy()
        perm = np.concatenate([perm, perm[:1]])             # DistributedSampler's wrap-around padding
        seen = []
        for rank in (0, 1):
            ld = mk(rank=rank, world=2)
            ld.set_epoch(epoch)
            xr, pr = batches_of(ld, with_params=True)
            assert [len(x) for x in xr] == [8, 8, 3]
            mine = data.epoch_indices(N, seed=seed, epoch=epoch, shuffle=True, rank=rank, world=2, drop_last=False).numpy()
            assert np.array_equal(mine, perm[rank::2])
            assert np.array_equal(np.concatenate(pr), whole[rank::2])
            assert np.array_equal(np.concatenate(pr), ar.draws(19, LWS, LW, seed, counter0=epoch * total + rank, stride=2, P=P, T=T, crop_mode=0))
            assert np.array_equal(np.concatenate(xr), ar.gather(cells, mine, whole[rank::2], LW))
            seen += mine.tolist()
        assert sorted(seen) == sorted(perm.tolist()) and set(seen) == set(range(N))


# 9. through the product
def test_train_one_epoch_and_evaluate_over_the_loader():
    from torch_vae_amd.evaluation import evaluate
    from torch_vae_amd.train import build_optimizer, train_one_epoch
    H, L, B, n, src_w, seed, P, T = 32, 16, 8, 24, 64, 3, 2, 4
    cells = np.random.default_rng(9).integers(0, 2, (n, H, src_w)).astype(np.uint8)
    ds = data.PianorollDataset(torch.from_numpy(cells))
    p = vo.init_params(L, H, 21, False)
    cfg = lambda: Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.0, optimizer="AdamW", scheduler="OneCycle",
                            epochs=2, log_wandb=False, print_interval=1000, log_interval=1000, freeze_encoder=False, global_rank=0, seed=seed,
                            aug_pitch_shift=P, aug_time_shift=T, img_size=H)
    epoch = 1
    idx = data.epoch_indices(n, seed=seed, epoch=epoch, shuffle=True, rank=0, world=1, drop_last=False).numpy()
    want = ar.gather(cells, idx, ar.draws(n, src_w, H, seed, counter0=epoch * n, P=P, T=T, crop_mode=0), H)
    plain = [(torch.from_numpy(want[k:k + B]).cuda(), torch.zeros(B, dtype=torch.long)) for k in range(0, n, B)]

    def train(loader_of):
        c = cfg()
        model = make_model(H, L, False, "f32", p)
        opt, sched = build_optimizer(c, model, steps_per_epoch=3)
        loader = loader_of(c)
        torch.manual_seed(0)                                  # (the reparameterisation noise of the steps)
        res, total_step, seen = train_one_epoch(c, model, opt, sched, model.loss, loader, device="cuda", epoch=epoch)
        assert total_step == 3 and seen == n
        return res["loss"], model.flat_parameters().detach().cpu().numpy().copy(), model

    loss_a, par_a, model_a = train(lambda c: data.DevicePianorollLoader.from_config(c, ds, True, rank=0, world=1))
    loss_b, par_b, _ = train(lambda c: plain)
    assert np.isfinite(loss_a) and loss_a == loss_b
    assert np.array_equal(par_a, par_b)
    # evaluation over the centre-crop loader (torch's device generator, seeded alike, draws the eval forwards' noise)
    ev = data.DevicePianorollLoader.from_config(cfg(), ds, False, rank=0, world=1)
    centre = ar.gather(cells, np.arange(n), np.tile([0, (src_w - H) // 2], (n, 1)), H)
    ref = [(torch.from_numpy(centre[k:k + B]).cuda(), torch.zeros(B, dtype=torch.long)) for k in range(0, n, B)]
    torch.manual_seed(1)
    ra = evaluate(ev, model_a, "cuda", verbosity=0)
    torch.manual_seed(1)
    rb = evaluate(ref, model_a, "cuda", verbosity=0)
    assert ra["count"] == n and rb["count"] == n
    assert ra["mse"] == rb["mse"] and ra["mse"] > 0
