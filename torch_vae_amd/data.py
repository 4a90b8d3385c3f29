"""Device-resident pianoroll data: the dataset lives on the card (or in pinned host memory), and every batch is ONE library launch
(include/vae_step.h: vae_gather_rolls) that picks the rolls, cuts the time window, shifts, transposes and writes the float32 batch
the step reads.  The port of the reference's ``data_transformations.get_transform`` stage (RandomCrop for training, CenterCrop
for evaluation) together with its DataLoader / DistributedSampler epoch and sharding semantics - no host workers, no host link.

Rows of a roll are pitch, columns are time.  A roll's augmentation is a function of (seed, epoch, position in the epoch's global
permutation) only: the sample at global position g of epoch e draws with counter ``e * padded_total + g`` (``padded_total`` the
permutation's padded length, ``g = rank + world * local position``), so it does not depend on the batch size or on how many ranks
share the epoch, and a resumed run that calls ``set_epoch`` continues the sequence."""
from __future__ import annotations

import math

import torch

from . import _lib

_KINDS = {"bytes": _lib.ROLLS_BYTES, "bits": _lib.ROLLS_BITS, "f32": _lib.ROLLS_F32}
_U64 = 0xFFFFFFFFFFFFFFFF


def epoch_indices(n: int, *, seed: int = 0, epoch: int = 0, shuffle: bool = True, rank: int = 0, world: int = 1,
                  drop_last: bool = False) -> torch.Tensor:
    """The indices ``torch.utils.data.DistributedSampler(num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
    drop_last=drop_last)`` yields for a dataset of ``n`` items after ``set_epoch(epoch)``, as an int64 CPU tensor: ``randperm`` from
    a CPU generator seeded ``seed + epoch`` (or 0..n-1), padded by wrap-around to a multiple of ``world`` (or truncated to one
    when ``drop_last``), then ``[rank::world]``.  A pure function; ``world=1`` is the single-process case."""
    n, world, rank = int(n), int(world), int(rank)
    if n < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"need n >= 0, world >= 1 and 0 <= rank < world, got n={n}, world={world}, rank={rank}")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        idx = torch.randperm(n, generator=g)
    else:
        idx = torch.arange(n, dtype=torch.int64)
    total = padded_total(n, world, drop_last)
    if total > n:
        idx = idx.repeat(math.ceil(total / n))[:total] if n else idx
    else:
        idx = idx[:total]
    return idx[rank:total:world].contiguous()


def padded_total(n: int, world: int = 1, drop_last: bool = False) -> int:
    """Length of the epoch's global permutation once DistributedSampler has padded (or, with ``drop_last``, truncated) it."""
    if drop_last and n % world:
        return math.ceil((n - world) / world) * world
    return math.ceil(n / world) * world


def _dist_rank_world(rank, world):
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    return (dist.get_rank() if on else 0) if rank is None else int(rank), (dist.get_world_size() if on else 1) if world is None else int(world)


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def gather_rolls(src: torch.Tensor, kind, width: int, *, index: torch.Tensor | None = None, first: int = 0, batch: int | None = None,
                 params: torch.Tensor | None = None, seed: int = 0, counter0: int = 0, counter_stride: int = 1, max_pitch_shift: int = 0,
                 max_time_shift: int = 0, crop_mode: int = _lib.CROP_CENTRE, scale: float = 1.0, out: torch.Tensor | None = None,
                 device=None) -> torch.Tensor:
    """One augmented float32 batch [B,1,H,width] out of the resident rolls ``src`` ([N,H,Ws] uint8 / float32, or [N,H,Ws/8] uint8 bit
    planes; contiguous, on the GPU or in pinned host memory), through vae_gather_rolls.  ``kind``: "bytes", "bits" or "f32".  The
    rolls are ``index`` (int64 [B] on the GPU; entries outside [0, N) give zero rolls) or ``first .. first + batch - 1``.  ``params``
    (int32 [B,2] on the GPU: pitch shift dy, first source column c0) fixes the augmentation; without it the kernel draws it
    (include/vae_step.h has the formulas; ``crop_mode`` 0 random window, 1 centre window).  For users with their own sampler."""
    k = _KINDS[kind] if isinstance(kind, str) else int(kind)
    if src.dim() != 3 or not src.is_contiguous():
        raise ValueError(f"src must be a contiguous [N, H, columns] tensor, got {tuple(src.shape)}")
    want = torch.float32 if k == _lib.ROLLS_F32 else torch.uint8
    if src.dtype != want:
        raise TypeError(f"kind {kind!r} wants a {want} source, got {src.dtype}")
    n_rolls, h = src.shape[0], src.shape[1]
    src_w = src.shape[2] * (8 if k == _lib.ROLLS_BITS else 1)
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1 or not index.is_cuda or not index.is_contiguous():
            raise ValueError("index must be a contiguous int64 [B] tensor on the GPU")
        batch = index.shape[0] if batch is None else batch
        if batch > index.shape[0]:
            raise ValueError(f"batch {batch} exceeds the {index.shape[0]} indices given")
    if batch is None:
        raise ValueError("give index or batch")
    batch = int(batch)
    if params is not None and (params.dtype != torch.int32 or tuple(params.shape) != (batch, 2) or not params.is_cuda or not params.is_contiguous()):
        raise ValueError(f"params must be a contiguous int32 [{batch}, 2] tensor on the GPU")
    if out is None:
        dev = device if device is not None else (src.device if src.is_cuda else index.device if index is not None else "cuda")
        dev = torch.device(dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty(max(batch, 0), 1, h, int(width), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() != batch * h * int(width):
        raise ValueError(f"out must be a contiguous float32 GPU tensor of {batch}*{h}*{width} cells")
    if batch == 0:
        return out
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().vae_gather_rolls(
            src.data_ptr(), k, n_rolls, h, src_w, _lib.ptr(index), int(first), _lib.ptr(params), int(seed) & _U64, int(counter0) & _U64,
            int(counter_stride) & _U64, int(max_pitch_shift), int(max_time_shift), int(crop_mode), float(scale), out.data_ptr(), batch,
            int(width), _stream(out)), "vae_gather_rolls")
    return out


def augmentation_params(batch: int, src_width: int, width: int, *, seed: int = 0, counter0: int = 0, counter_stride: int = 1,
                        max_pitch_shift: int = 0, max_time_shift: int = 0, crop_mode: int = _lib.CROP_CENTRE, device="cuda") -> torch.Tensor:
    """The (dy, c0) the gather kernel draws for the same arguments, as an int32 [batch, 2] GPU tensor (vae_augment_params)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if int(batch) < 0:
        raise ValueError(f"batch must be >= 0, got {batch}")
    out = torch.empty(int(batch), 2, dtype=torch.int32, device=dev)
    if not out.numel():
        return out
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vae_augment_params(
            out.data_ptr(), int(batch), int(src_width), int(width), int(seed) & _U64, int(counter0) & _U64,
            int(counter_stride) & _U64, int(max_pitch_shift), int(max_time_shift), int(crop_mode), _stream(out)),
            "vae_augment_params")
    return out


def select_storage(rolls: torch.Tensor) -> str:
    """The storage ``PianorollDataset(storage="auto")`` picks: 0/1 data (bool, or uint8 / float holding only 0 and 1) -> "bits";
    other uint8 -> "bytes"; other float -> "f32"."""
    if rolls.dtype == torch.bool:
        return "bits"
    if rolls.dtype == torch.uint8:
        return "bits" if rolls.numel() == 0 or int(rolls.max()) <= 1 else "bytes"
    if rolls.dtype.is_floating_point:
        return "bits" if bool(((rolls == 0) | (rolls == 1)).all()) else "f32"
    raise TypeError(f"rolls must be bool, uint8 or floating point, got {rolls.dtype}")


class PianorollDataset:
    """N pianorolls [N,1,H,Ws] or [N,H,Ws] (pitch by time; Ws a multiple of 8) held where the gather kernel reads them: on
    ``device``, or with ``device="pinned"`` in pinned host memory (read in place over the host link).  Stored as bit planes
    ("bits": 0/1 data, 1/32 of the float32 bytes, through ``train.pack_bits``), bytes ("bytes": uint8 velocities; ``scale``
    multiplies them on the way out, e.g. 1/127) or float32 ("f32"); ``storage="auto"`` chooses by content (``select_storage``).
    ``ds[i]`` is the un-augmented float32 roll [1,H,Ws] on the GPU - for inspection, not for the hot path."""

    def __init__(self, rolls, *, storage: str = "auto", device="cuda", scale: float = 1.0):
        rolls = torch.as_tensor(rolls)
        if rolls.dim() == 4 and rolls.shape[1] == 1:
            rolls = rolls[:, 0]
        if rolls.dim() != 3:
            raise ValueError(f"rolls must be [N,1,H,Ws] or [N,H,Ws], got {tuple(rolls.shape)}")
        if rolls.shape[0] < 1 or rolls.shape[1] < 1:
            raise ValueError(f"need at least one roll and one pitch row, got {tuple(rolls.shape)}")
        if rolls.shape[2] < 8 or rolls.shape[2] % 8:
            raise ValueError(f"the roll width (time steps) must be a positive multiple of 8, got {rolls.shape[2]}")
        if storage == "auto":
            storage = select_storage(rolls)
        if storage not in _KINDS:
            raise ValueError(f"storage must be 'auto', 'bits', 'bytes' or 'f32', got {storage!r}")
        self.storage, self.kind, self.scale = storage, _KINDS[storage], float(scale)
        self.n, self.height, self.width = (int(s) for s in rolls.shape)
        if storage == "bits":
            from .train import pack_bits
            data = pack_bits(rolls)
        elif storage == "bytes":
            data = rolls.to(torch.uint8)
        else:
            data = rolls.to(torch.float32)
        data = data.contiguous()
        self.pinned = device == "pinned"
        self.data = (data.cpu().pin_memory() if self.pinned else data.to(device))

    @classmethod
    def from_stored(cls, stored: torch.Tensor, storage: str, *, scale: float = 1.0) -> "PianorollDataset":
        """Rolls already in their stored form and place - [N,H,Ws/8] uint8 bit planes ("bits"), [N,H,Ws] uint8 ("bytes") or float32
        ("f32"), contiguous, on the GPU or in pinned host memory - wrapped as they are: nothing is unpacked, converted or copied."""
        want = torch.float32 if storage == "f32" else torch.uint8
        if storage not in _KINDS or stored.dim() != 3 or stored.dtype != want or not stored.is_contiguous():
            raise ValueError(f"need storage 'bits', 'bytes' or 'f32' and a contiguous [N,H,columns] {want} tensor")
        ds = cls.__new__(cls)
        ds.storage, ds.kind, ds.scale, ds.data = storage, _KINDS[storage], float(scale), stored
        ds.n, ds.height, ds.width = int(stored.shape[0]), int(stored.shape[1]), int(stored.shape[2]) * (8 if storage == "bits" else 1)
        ds.pinned = not stored.is_cuda
        if ds.n < 1 or ds.height < 1 or ds.width < 8 or ds.width % 8:
            raise ValueError(f"need at least one roll and one row, and a width that is a positive multiple of 8, got {tuple(stored.shape)}")
        return ds

    def __len__(self):
        return self.n

    def __getitem__(self, i: int) -> torch.Tensor:
        i = int(i)
        if not -self.n <= i < self.n:
            raise IndexError(i)
        return gather_rolls(self.data, self.kind, self.width, first=i % self.n, batch=1, scale=self.scale)[0]


class DevicePianorollLoader:
    """Batches ``(stimuli float32 [B,1,H,width] on the GPU, y_true)`` out of a ``PianorollDataset`` - what ``train_one_epoch`` and
    ``evaluation.evaluate`` consume.  ``train=True``: a random window of ``width`` time steps per roll (the reference's RandomCrop),
    shuffled, with a time shift of up to ``max_time_shift`` steps and a transposition of up to ``max_pitch_shift`` rows either way
    (a shift inside a longer roll shows the neighbouring content; what leaves the roll is zero-filled).  ``train=False``: the centre
    window (CenterCrop), loader order, no shifts whatever was passed.  Epoch order and sharding are ``epoch_indices`` (=
    DistributedSampler, padding by wrap-around); ``drop_last`` drops this rank's last partial batch as DataLoader does.
    ``rank`` / ``world`` default to torch.distributed's when it is initialised, else 0 / 1.  At the start of an epoch the rank's
    index tensor goes to the device once; every batch is then one vae_gather_rolls launch with the draws made inside it."""

    def __init__(self, dataset: PianorollDataset, batch_size: int, *, width: int | None = None, train: bool = True, shuffle: bool | None = None,
                 drop_last: bool = False, seed: int = 0, max_pitch_shift: int = 0, max_time_shift: int = 0, rank: int | None = None,
                 world: int | None = None):
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.width = dataset.width if width is None else int(width)
        if self.batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if self.width < 8 or self.width % 8 or self.width > dataset.width:
            raise ValueError(f"width must be a multiple of 8 in [8, {dataset.width}], got {self.width}")
        self.train = bool(train)
        self.shuffle = self.train if shuffle is None else bool(shuffle)
        self.drop_last, self.seed = bool(drop_last), int(seed)
        self.max_pitch_shift = int(max_pitch_shift) if self.train else 0
        self.max_time_shift = int(max_time_shift) if self.train else 0
        if self.max_pitch_shift < 0 or self.max_time_shift < 0:
            raise ValueError("max_pitch_shift and max_time_shift must be >= 0")
        self.crop_mode = _lib.CROP_RANDOM if self.train else _lib.CROP_CENTRE
        self.rank, self.world = _dist_rank_world(rank, world)
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"need 0 <= rank < world, got rank={self.rank}, world={self.world}")
        self.epoch = 0
        self._last = None       # (batch, counter0) of the batch just produced
        self._labels = None

    @classmethod
    def from_config(cls, config, dataset: PianorollDataset, train: bool, **kwargs) -> "DevicePianorollLoader":
        """The loader the reference's DataLoader settings describe (train.py:168-181): ``config.batch_size_per_gpu``, ``config.seed``,
        drop_last for training only; optional ``config.aug_pitch_shift`` / ``config.aug_time_shift`` (default 0) and
        ``config.crop_width`` (default: the model's ``config.img_size`` if set, else the rolls' width)."""
        kw = dict(width=getattr(config, "crop_width", None) or getattr(config, "img_size", None), train=train, drop_last=bool(train),
                  seed=int(getattr(config, "seed", 0) or 0), max_pitch_shift=int(getattr(config, "aug_pitch_shift", 0) or 0),
                  max_time_shift=int(getattr(config, "aug_time_shift", 0) or 0))
        kw.update(kwargs)
        return cls(dataset, config.batch_size_per_gpu, **kw)

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    @property
    def samples_per_rank(self) -> int:
        return padded_total(len(self.dataset), self.world) // self.world

    def __len__(self):
        n = self.samples_per_rank
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def counter0(self, local_position: int, epoch: int | None = None) -> int:
        """Augmentation counter of this rank's sample at ``local_position`` of the epoch (module docstring); stride ``world``."""
        e = self.epoch if epoch is None else int(epoch)
        return e * padded_total(len(self.dataset), self.world) + self.rank + self.world * int(local_position)

    def __iter__(self):
        ds = self.dataset
        idx = epoch_indices(len(ds), seed=self.seed, epoch=self.epoch, shuffle=self.shuffle, rank=self.rank, world=self.world)
        dev = ds.data.device if ds.data.is_cuda else torch.device("cuda", torch.cuda.current_device())
        # the epoch's one host-to-device copy: from pinned memory and asynchronous, so that starting an epoch does not make the host
        # wait for the stream (a blocking copy of a pageable tensor does); the loader keeps the host tensor until the next epoch
        self._index_host = idx.pin_memory()
        index = self._index_host.to(dev, non_blocking=True)
        if self._labels is None or self._labels.device != dev:
            self._labels = torch.zeros(self.batch_size, dtype=torch.long, device=dev)
        for k in range(len(self)):
            lo = k * self.batch_size
            sl = index[lo:lo + self.batch_size]
            c0 = self.counter0(lo)
            x = gather_rolls(ds.data, ds.kind, self.width, index=sl, seed=self.seed, counter0=c0, counter_stride=self.world,
                             max_pitch_shift=self.max_pitch_shift, max_time_shift=self.max_time_shift, crop_mode=self.crop_mode,
                             scale=ds.scale, device=dev)
            self._last = (sl.shape[0], c0, dev)
            yield x, self._labels[:sl.shape[0]]

    def last_params(self) -> torch.Tensor:
        """(dy, c0) of every sample of the batch just produced, int32 [B,2] on the GPU (vae_augment_params: a diagnostic)."""
        if self._last is None:
            raise RuntimeError("last_params() before the first batch")
        b, c0, dev = self._last
        return augmentation_params(b, self.dataset.width, self.width, seed=self.seed, counter0=c0, counter_stride=self.world,
                                   max_pitch_shift=self.max_pitch_shift, max_time_shift=self.max_time_shift, crop_mode=self.crop_mode,
                                   device=dev)
