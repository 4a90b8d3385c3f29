"""Host side of the device pianoroll loader (torch_vae_amd/data.py, vae_gather_rolls / vae_augment_params): the numpy reference
pinned against an independent formulation, the draw formula, epoch_indices against DistributedSampler, loader lengths, storage
selection, and the argument refusals of the two entry points (fake, never dereferenced addresses, as in test_refusals_host.py)."""
import numpy as np
import pytest
import torch
from torch.utils.data import DistributedSampler

from tests import augment_ref as ar
from torch_vae_amd import _lib, data

P = 4096          # a fake device address, 16-byte aligned


def test_reference_against_pad_roll_slice():
    rng = np.random.default_rng(0)
    for case in range(12):
        h, w = int(rng.integers(1, 6)), 8 * int(rng.integers(1, 3))
        src_w = w + 8 * int(rng.integers(0, 3))
        n, batch = int(rng.integers(1, 4)), 24
        cells = rng.integers(0, 128, (n, h, src_w)).astype(np.uint8)
        index = rng.integers(-1, n + 1, batch)
        params = np.stack([rng.integers(-h - 2, h + 3, batch), rng.integers(-w - 3, src_w + 4, batch)], 1)
        scale = None if case % 2 else 1 / 127
        got = ar.gather(cells, index, params, w, scale)
        assert got.shape == (batch, 1, h, w) and got.dtype == np.float32
        assert np.array_equal(got, ar.gather_by_roll(cells, index, params, w, scale))
    # a hand-made case: one roll 2 x 8, window 8, up one row and two columns to the left of the roll's start
    cells = np.arange(16, dtype=np.uint8).reshape(1, 2, 8)
    got = ar.gather(cells, [0], [[-1, -2]], 8)[0, 0]
    assert got.tolist() == [[0, 0, 8, 9, 10, 11, 12, 13], [0] * 8]


@pytest.mark.parametrize("crop_mode", [0, 1])
def test_draw_formula(crop_mode):
    src_w, w, Pm, T, n = 64, 32, 3, 5, 4096
    d = ar.draws(n, src_w, w, seed=7, P=Pm, T=T, crop_mode=crop_mode)
    u = ar.vo.counter_uniform(2 * n, 7, 901)
    s = src_w - w
    assert set(d[:, 0]) == set(range(-Pm, Pm + 1))
    lo, hi = (-T, s + T) if crop_mode == 0 else (s // 2 - T, s // 2 + T)
    assert set(d[:, 1]) == set(range(lo, hi + 1))
    for b in (0, 1, 17, n - 1):
        assert d[b, 0] == int(u[2 * b] * (2 * Pm + 1)) - Pm
        want = int(u[2 * b + 1] * (s + 2 * T + 1)) - T if crop_mode == 0 else s // 2 + int(u[2 * b + 1] * (2 * T + 1)) - T
        assert d[b, 1] == want
    # counters: a stride picks every stride-th sample of the sequence, counter0 its start
    assert np.array_equal(ar.draws(100, src_w, w, 7, counter0=5, stride=3, P=Pm, T=T, crop_mode=crop_mode), d[5:305:3])


def test_centre_crop_without_shifts_is_not_random():
    for seed in (0, 1, 99):
        d = ar.draws(64, 48, 16, seed, counter0=seed * 13, P=0, T=0, crop_mode=1)
        assert np.array_equal(d, np.tile([0, 16], (64, 1)))


@pytest.mark.parametrize("n", [1, 7, 64])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_indices_equal_distributed_sampler(n, world, shuffle, drop_last):
    ds = list(range(n))
    for rank in range(world):
        sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle, seed=5, drop_last=drop_last)
        for epoch in (0, 3):
            sampler.set_epoch(epoch)
            got = data.epoch_indices(n, seed=5, epoch=epoch, shuffle=shuffle, rank=rank, world=world, drop_last=drop_last)
            assert got.dtype == torch.int64 and got.device.type == "cpu"
            assert got.tolist() == list(sampler)
            assert len(got) == len(sampler)


def test_epoch_indices_is_pure():
    a = data.epoch_indices(64, seed=1, epoch=2, shuffle=True, rank=0, world=1, drop_last=False)
    torch.manual_seed(123)
    b = data.epoch_indices(64, seed=1, epoch=2, shuffle=True, rank=0, world=1, drop_last=False)
    assert torch.equal(a, b)
    assert not torch.equal(a, data.epoch_indices(64, seed=1, epoch=3, shuffle=True, rank=0, world=1, drop_last=False))


def _host_dataset(rolls, **kw):
    return data.PianorollDataset(rolls, device="cpu", **kw)


def test_loader_length():
    ds = _host_dataset(torch.zeros(37, 16, 48))
    assert len(ds) == 37
    assert len(data.DevicePianorollLoader(ds, 8, width=16, rank=0, world=1)) == 5
    assert len(data.DevicePianorollLoader(ds, 8, width=16, drop_last=True, rank=0, world=1)) == 4
    # two ranks: 19 samples each (one padded)
    assert len(data.DevicePianorollLoader(ds, 8, width=16, rank=1, world=2)) == 3
    assert len(data.DevicePianorollLoader(ds, 8, width=16, drop_last=True, rank=1, world=2)) == 2
    assert len(data.DevicePianorollLoader(ds, 37, rank=0, world=1)) == 1
    ev = data.DevicePianorollLoader(ds, 8, width=16, train=False, max_pitch_shift=3, max_time_shift=4, rank=0, world=1)
    assert (ev.shuffle, ev.max_pitch_shift, ev.max_time_shift, ev.crop_mode) == (False, 0, 0, _lib.CROP_CENTRE)
    tr = data.DevicePianorollLoader(ds, 8, width=16, max_pitch_shift=3, max_time_shift=4, rank=1, world=2)
    assert (tr.shuffle, tr.max_pitch_shift, tr.max_time_shift, tr.crop_mode) == (True, 3, 4, _lib.CROP_RANDOM)
    tr.set_epoch(2)
    assert tr.counter0(5) == 2 * 38 + 1 + 2 * 5
    for bad in (0, 12, 56):
        with pytest.raises(ValueError):
            data.DevicePianorollLoader(ds, 8, width=bad)


def test_loader_from_config():
    class Cfg:
        batch_size_per_gpu, seed, aug_time_shift = 4, 9, 2
    ds = _host_dataset(torch.zeros(10, 8, 32))
    tr = data.DevicePianorollLoader.from_config(Cfg, ds, True, width=16, rank=0, world=1)
    assert (tr.batch_size, tr.seed, tr.max_pitch_shift, tr.max_time_shift, tr.drop_last, tr.width) == (4, 9, 0, 2, True, 16)
    ev = data.DevicePianorollLoader.from_config(Cfg, ds, False, rank=0, world=1)
    assert (ev.drop_last, ev.train, ev.width, ev.max_time_shift) == (False, False, 32, 0)


def test_dataset_storage_selection():
    g = torch.Generator().manual_seed(0)
    bits = torch.randint(0, 2, (5, 1, 8, 16), generator=g)
    for rolls in (bits.bool(), bits.to(torch.uint8), bits.float(), bits.double()):
        ds = _host_dataset(rolls)
        assert (ds.storage, ds.kind, ds.data.dtype, tuple(ds.data.shape)) == ("bits", 1, torch.uint8, (5, 8, 2))
        assert np.array_equal(ar.unpack_bits(ds.data.numpy(), 16), bits[:, 0].numpy())
    vel = torch.randint(0, 128, (5, 8, 16), generator=g).to(torch.uint8)
    ds = _host_dataset(vel)
    assert (ds.storage, ds.kind, ds.data.dtype, tuple(ds.data.shape)) == ("bytes", 0, torch.uint8, (5, 8, 16))
    ds = _host_dataset(torch.rand(5, 8, 16, generator=g))
    assert (ds.storage, ds.kind, ds.data.dtype) == ("f32", 2, torch.float32)
    # forced
    assert _host_dataset(bits, storage="f32").data.dtype == torch.float32
    assert _host_dataset(bits.to(torch.uint8), storage="bytes").kind == 0
    assert _host_dataset(vel, storage="bits").kind == 1
    assert (len(ds), ds.height, ds.width) == (5, 8, 16)


@pytest.mark.parametrize("width", [0, 4, 12, 17])
def test_dataset_refuses_widths_off_8(width):
    with pytest.raises(ValueError, match="multiple of 8"):
        _host_dataset(torch.zeros(3, 8, width))


def test_dataset_refuses_other_shapes_and_names():
    with pytest.raises(ValueError):
        _host_dataset(torch.zeros(3, 2, 8, 16))
    with pytest.raises(ValueError):
        _host_dataset(torch.zeros(3, 8, 16), storage="bf16")
    with pytest.raises(TypeError):
        _host_dataset(torch.zeros(3, 8, 16, dtype=torch.int32))


def gather(L, src=P, kind=1, n_rolls=4, h=8, src_w=16, index=None, params=None, P_=0, T=0, crop=1, scale=1.0, dst=P, batch=2, w=16):
    return L.vae_gather_rolls(src, kind, n_rolls, h, src_w, index, 0, params, 0, 0, 1, P_, T, crop, scale, dst, batch, w, None)


def aug(L, params=P, batch=2, src_w=16, w=16, P_=0, T=0, crop=1):
    return L.vae_augment_params(params, batch, src_w, w, 0, 0, 1, P_, T, crop, None)


W8 = "w and src_w must be positive multiples of 8 (at most 2^30)"
SHIFT = "max_pitch_shift and max_time_shift must be in [0, 2^24]"
CROP = "crop_mode must be 0 (random) or 1 (centre)"
CASES = {
    "gather/null_src": (lambda L: gather(L, src=0), "vae_gather_rolls: null pointer (src, dst)"),
    "gather/null_dst": (lambda L: gather(L, dst=0), "vae_gather_rolls: null pointer (src, dst)"),
    "gather/kind_-1": (lambda L: gather(L, kind=-1), "vae_gather_rolls: kind must be 0 (bytes), 1 (bit planes) or 2 (float32)"),
    "gather/kind_3": (lambda L: gather(L, kind=3), "vae_gather_rolls: kind must be 0 (bytes), 1 (bit planes) or 2 (float32)"),
    "gather/h_0": (lambda L: gather(L, h=0), "vae_gather_rolls: h must be > 0"),
    "gather/batch_-1": (lambda L: gather(L, batch=-1), "vae_gather_rolls: batch must be >= 0"),
    "gather/w_0": (lambda L: gather(L, w=0), "vae_gather_rolls: " + W8),
    "gather/w_12": (lambda L: gather(L, w=12), "vae_gather_rolls: " + W8),
    "gather/src_w_20": (lambda L: gather(L, src_w=20), "vae_gather_rolls: " + W8),
    "gather/src_w_-8": (lambda L: gather(L, src_w=-8), "vae_gather_rolls: " + W8),
    "gather/src_w_below_w": (lambda L: gather(L, src_w=8), "vae_gather_rolls: src_w must be >= w"),
    "gather/n_rolls_0": (lambda L: gather(L, n_rolls=0), "vae_gather_rolls: n_rolls must be > 0 (and the source below 2^62 bytes)"),
    "gather/pitch_shift_-1": (lambda L: gather(L, P_=-1), "vae_gather_rolls: " + SHIFT),
    "gather/time_shift_-1": (lambda L: gather(L, T=-1), "vae_gather_rolls: " + SHIFT),
    "gather/crop_mode_2": (lambda L: gather(L, crop=2), "vae_gather_rolls: " + CROP),
    "gather/crop_mode_-1": (lambda L: gather(L, crop=-1), "vae_gather_rolls: " + CROP),
    "gather/scale_inf": (lambda L: gather(L, kind=0, scale=float("inf")), "vae_gather_rolls: scale must be finite"),
    "gather/scale_nan": (lambda L: gather(L, kind=0, scale=float("nan")), "vae_gather_rolls: scale must be finite"),
    "gather/dst_plus_4": (lambda L: gather(L, dst=P + 4), "vae_gather_rolls: dst must be 16-byte, index 8-byte, params 4-byte aligned"),
    "gather/index_plus_4": (lambda L: gather(L, index=P + 4), "vae_gather_rolls: dst must be 16-byte, index 8-byte, params 4-byte aligned"),
    "params/null": (lambda L: aug(L, params=0), "vae_augment_params: null pointer (params)"),
    "params/batch_-1": (lambda L: aug(L, batch=-1), "vae_augment_params: batch must be >= 0"),
    "params/w_12": (lambda L: aug(L, w=12), "vae_augment_params: " + W8),
    "params/src_w_0": (lambda L: aug(L, src_w=0), "vae_augment_params: " + W8),
    "params/src_w_below_w": (lambda L: aug(L, src_w=8), "vae_augment_params: src_w must be >= w"),
    "params/pitch_shift_-1": (lambda L: aug(L, P_=-1), "vae_augment_params: " + SHIFT),
    "params/time_shift_-1": (lambda L: aug(L, T=-1), "vae_augment_params: " + SHIFT),
    "params/crop_mode_2": (lambda L: aug(L, crop=2), "vae_augment_params: " + CROP),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = CASES[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == want


def test_empty_batch_launches_nothing():
    L = _lib.lib()
    assert gather(L, batch=0) == 0       # fake addresses: returning 0 means nothing looked at them
    assert aug(L, batch=0) == 0


def test_exported():
    L = _lib.lib()
    for name in ("vae_gather_rolls", "vae_augment_params"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.vae_abi_version() == 1
    import torch_vae_amd
    for name in ("PianorollDataset", "DevicePianorollLoader", "epoch_indices", "gather_rolls", "augmentation_params"):
        assert name in torch_vae_amd.__all__ and getattr(torch_vae_amd, name) is getattr(data, name)
