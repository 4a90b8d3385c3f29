"""vae_music_roll_stats (include/vae_music.h) and its Python layer (evaluation.music_statistics, MusicStatsAccumulator, music_summary,
compare_music, sample_music_stats, evaluate(music_stats=True)) on the GPU against the numpy reference of tests/music_ref.py.
Everything the kernels write is an integer count, so features and totals are compared for exact equality; the host-side float64
numbers of music_summary / compare_music to 1e-12 relative (sums of at most a few hundred terms in [0, 1] over identical
integers).  The reference of every case is computed once (music_ref.gpu_cases) and shared."""
import math

import numpy as np
import pytest
import torch

from tests import music_ref as R
from tests import stream_harness as sh
from tests.stream_harness import Bufs, Case

pytestmark = pytest.mark.gpu

F = R.F
CASE_KEYS = list(R.gpu_cases())       # (h, w, n, pitch_offset): every shape x count x offset, and the 2 x 8192 roll


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from torch_vae_amd import _lib
    return _lib.lib()


def ok(rc, what="vae_music_roll_stats"):
    assert rc == 0, (what, lib().vae_last_error().decode())


def host(t):
    return t.detach().cpu().numpy()


def call(planes, pitch_offset, totals=None, accumulate=0, features=None):
    """vae_music_roll_stats on numpy planes [n, h, w/8] -> (features, totals) device tensors"""
    n, h, wb = planes.shape
    d = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    if features is None:
        features = torch.full((n, F), -7, dtype=torch.int32, device="cuda")
    ok(lib().vae_music_roll_stats(d.data_ptr(), n, h, wb * 8, pitch_offset, features.data_ptr(), 0 if totals is None else totals.data_ptr(),
                                  accumulate, st()))
    return features, totals


def garbage_totals():
    return torch.full((F,), 123456789, dtype=torch.int64, device="cuda")


# ---- the kernel against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASE_KEYS, ids=str)
def test_features_and_totals(key):
    h, w, n, off = key
    planes, want = R.gpu_cases()[key]
    feats, totals = call(planes, off, garbage_totals())
    got = host(feats)
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), f"first differences (roll, column): {bad[:8].tolist()} got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"
    assert got.dtype == np.int32
    assert np.array_equal(host(totals), R.totals(want))


def test_the_cases_reach_every_column():
    """Over the whole case set every live column is non-zero in some roll THE DEVICE computed, and the last duration / polyphony /
    ioi buckets are hit: a column stuck at 0 cannot pass."""
    feats = np.concatenate([host(call(planes, key[3])[0]) for key, (planes, _) in R.gpu_cases().items()])
    assert [c for c in range(74) if not feats[:, c].any()] == []
    assert not feats[:, 74:].any()
    for name in ("duration", "polyphony", "ioi"):
        assert feats[:, R.COL[name] + R.WIDTH[name] - 1].any(), name


@pytest.mark.parametrize("key", [(128, 128, 67, 21), (5, 288, 67, 0), (256, 256, 3, 0)], ids=str)
def test_accumulate_over_halves(key):
    h, w, n, off = key
    planes, want = R.gpu_cases()[key]
    whole = R.totals(want)
    for cut in (1, n // 2):          # (roll 0 of these cases is the all-zero roll: cut = 1 is a first half of only empty rolls)
        t = garbage_totals()
        f1, _ = call(planes[:cut], off, t, accumulate=0)
        if cut == 1:
            assert not want[0, R.COL["cells"]] and np.array_equal(host(t), R.totals(want[:1]))
            assert host(t)[R.COL["lowest"]] == -1 and host(t)[R.COL["highest"]] == -1
        f2, _ = call(planes[cut:], off, t, accumulate=1)
        assert np.array_equal(host(t), whole)
        assert np.array_equal(np.concatenate([host(f1), host(f2)]), want)
    # an all-empty call on top of totals that hold something changes only the counts of rolls and of empty steps
    t = torch.from_numpy(whole).cuda()
    call(planes[:1], off, t, accumulate=1)
    assert np.array_equal(host(t), R.totals(want[:1], into=whole))


def test_no_rolls():
    planes = torch.zeros(4, 4, dtype=torch.uint8, device="cuda")
    feats = torch.full((4, F), -7, dtype=torch.int32, device="cuda")
    t = garbage_totals()
    L = lib()
    ok(L.vae_music_roll_stats(planes.data_ptr(), 0, 4, 32, 0, feats.data_ptr(), t.data_ptr(), 1, st()))
    assert (host(t) == 123456789).all()                      # accumulate: nothing to add
    ok(L.vae_music_roll_stats(planes.data_ptr(), 0, 4, 32, 0, feats.data_ptr(), t.data_ptr(), 0, st()))
    assert np.array_equal(host(t), R.empty_totals())         # overwrite: the empty value
    ok(L.vae_music_roll_stats(planes.data_ptr(), 0, 4, 32, 0, feats.data_ptr(), 0, 0, st()))
    assert (host(feats) == -7).all()


def test_without_totals_and_repeated_calls():
    key = (128, 128, 67, 0)
    planes, want = R.gpu_cases()[key]
    first, _ = call(planes, 0)
    assert np.array_equal(host(first), want)
    t1, t2 = garbage_totals(), garbage_totals()
    a, _ = call(planes, 0, t1)
    b, _ = call(planes, 0, t2)
    assert sh.same_bits(a, b) and sh.same_bits(a, first) and sh.same_bits(t1, t2)


@pytest.mark.parametrize("key", [(13, 64, 67, 21), (128, 128, 3, 0), (1, 32, 1, 0)], ids=str)
def test_nothing_outside_the_feature_table_is_written(key):
    h, w, n, off = key
    planes, want = R.gpu_cases()[key]
    guard = 64
    buf = torch.full((guard + n * F + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    call(planes, off, garbage_totals(), features=buf[guard:guard + n * F])
    got = host(buf)
    assert (got[:guard] == 0x5A5A5A5A).all() and (got[guard + n * F:] == 0x5A5A5A5A).all()
    assert np.array_equal(got[guard:guard + n * F].reshape(n, F), want)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def close(got, want, path=""):
    """dicts / lists / numbers: equal keys, integers equal, floats to 1e-12 relative, nan where nan"""
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), (path, sorted(got), sorted(want))
        for k in want:
            close(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            close(g, w, f"{path}[{i}]")
    elif isinstance(want, float) and math.isnan(want):
        assert isinstance(got, float) and math.isnan(got), (path, got)
    else:
        print(path, got, want)
        assert abs(got - want) <= 1e-12 * abs(want), (path, got, want)


def test_the_three_input_kinds_agree():
    from torch_vae_amd.data import PianorollDataset
    from torch_vae_amd.evaluation import MUSIC_COLUMNS, music_statistics
    key = (13, 64, 67, 21)
    planes, want = R.gpu_cases()[key]
    cells = torch.from_numpy(R.unpack(planes).astype(np.float32)).cuda()
    d = torch.from_numpy(planes).cuda()
    results = [music_statistics(d, pitch_offset=21), music_statistics(cells, pitch_offset=21),
               music_statistics(cells[:, None] * 0.75, pitch_offset=21, threshold=0.7),
               music_statistics(PianorollDataset(cells.cpu(), storage="bits"), pitch_offset=21),
               music_statistics(PianorollDataset.from_stored(d, "bits"), pitch_offset=21)]
    for r in results:
        assert r["features"].dtype == torch.int32 and r["totals"].dtype == torch.int64 and r["features"].is_cuda and r["totals"].is_cuda
        assert np.array_equal(host(r["features"]), want) and np.array_equal(host(r["totals"]), R.totals(want))
        assert (r["height"], r["width"], r["pitch_offset"]) == (13, 64, 21) and r["columns"] == MUSIC_COLUMNS
        assert np.array_equal(host(r["features"][:, r["columns"]["duration"]]), want[:, 34:46])
    cut = music_statistics(cells * 0.75, threshold=0.8)              # nothing reaches the threshold
    assert int(cut["totals"][2]) == 0 and int(cut["totals"][5]) == -1
    none = music_statistics(d[:0])
    assert none["features"].shape == (0, F) and np.array_equal(host(none["totals"]), R.empty_totals())


def test_accumulator_over_batches_of_five():
    from torch_vae_amd.evaluation import MusicStatsAccumulator, music_statistics
    key = (128, 128, 67, 1000003 % (1 << 20))
    planes, want = R.gpu_cases()[key]
    d = torch.from_numpy(planes).cuda()
    acc = MusicStatsAccumulator(pitch_offset=key[3])
    for first in range(0, 67, 5):
        acc.update(d[first:first + 5])
    acc.update(d[:0])
    got, one_call = acc.compute(), music_statistics(d, pitch_offset=key[3])
    assert sh.same_bits(got["features"], one_call["features"]) and sh.same_bits(got["totals"], one_call["totals"])
    assert np.array_equal(host(got["features"]), want) and (got["height"], got["width"]) == (128, 128)
    acc.update(d[:2])                                                  # compute() does not close the accumulator
    assert np.array_equal(host(acc.compute()["totals"]), R.totals(want[:2], into=R.totals(want)))
    with pytest.raises(ValueError, match="holds 128x128"):
        acc.update(d[:, :64].contiguous())


def test_summary_and_compare_against_numpy():
    from torch_vae_amd.evaluation import compare_music, music_statistics, music_summary
    (pa, fa), (pb, fb) = R.gpu_cases()[(128, 128, 67, 21)], R.gpu_cases()[(128, 128, 3, 21)]
    a, b = music_statistics(torch.from_numpy(pa).cuda(), pitch_offset=21), music_statistics(torch.from_numpy(pb).cuda(), pitch_offset=21)
    close(music_summary(a), R.summary(fa, 128, 128), "summary_a")
    close(music_summary(b), R.summary(fb, 128, 128), "summary_b")
    close(compare_music(a, b), R.compare(fa, fb), "compare")
    same = compare_music(a, a)
    for name in R.DISTRIBUTIONS:
        assert same[f"js_{name}"] == 0.0 and abs(same[f"overlap_{name}"] - 1.0) <= 1e-15
    for name in R.SCALARS:
        assert same[f"w1_{name}"] == 0.0
    # the nan rules: an all-empty set, and a set of no rolls
    empty = music_statistics(torch.zeros(2, 128, 16, dtype=torch.uint8, device="cuda"), pitch_offset=21)
    close(music_summary(empty), R.summary(R.features(np.zeros((2, 128, 16), np.uint8)), 128, 128), "summary_empty")
    close(compare_music(empty, a), R.compare(R.features(np.zeros((2, 128, 16), np.uint8)), fa), "compare_empty")
    none = music_statistics(torch.zeros(0, 128, 16, dtype=torch.uint8, device="cuda"))
    close(music_summary(none), R.summary(np.zeros((0, F), np.int32), 128, 128), "summary_none")
    close(compare_music(a, none), R.compare(fa, np.zeros((0, F), np.int32)), "compare_none")


def tiny_model(dtype="f32"):
    from tests.util import make_model, perturbed_params
    return make_model(32, 16, False, dtype, perturbed_params(16, 32, 31, False))


def tiny_rolls(n, width, seed=23):
    rng = np.random.default_rng(seed)
    return np.stack([R.random_runs(rng, 32, width, 0.08) for _ in range(n)])


def test_sample_music_stats():
    from torch_vae_amd.data import DevicePianorollLoader, PianorollDataset
    from torch_vae_amd.evaluation import sample_music_stats
    from torch_vae_amd.mixture import LatentMixture, encode_dataset
    model = tiny_model()
    cells = tiny_rolls(40, 32)
    ds = PianorollDataset(torch.from_numpy(cells.astype(np.float32)), storage="bits")
    want_data = R.summary(R.features(R.pack(cells), 21), 32, 32)
    mu, _ = encode_dataset(model, DevicePianorollLoader(ds, 40, train=False))
    mix = LatentMixture.fit(mu, 2, covariance="diag", iters=3)
    for prior in (None, mix):
        kw = dict(seed=5, prior=prior, pitch_offset=21, max_notes=4096, onset_threshold=0.5)
        r = sample_music_stats(model, ds, 12, **kw)
        assert sorted(r) == ["dataset", "gap", "samples"]
        close(r["dataset"], want_data, "dataset")
        assert r["samples"]["rolls"] == 12 and r["dataset"]["rolls"] == 40
        for name in R.DISTRIBUTIONS:
            both = not math.isnan(sum(r["samples"][name])) and not math.isnan(sum(r["dataset"][name]))
            assert math.isfinite(r["gap"][f"js_{name}"]) == both, name
        assert math.isfinite(r["gap"]["js_polyphony"]) and math.isfinite(r["gap"]["w1_notes"])
        again = sample_music_stats(model, ds, 12, **kw)
        close(again, r, "again")
    # the samples' statistics are those of the cleaned planes sample_notes gives
    notes = model.sample_notes(12, seed=5, cleaned=True, max_notes=4096)
    close(sample_music_stats(model, ds, 12, seed=5, pitch_offset=21, max_notes=4096)["samples"],
          R.summary(R.features(host(notes["cleaned"]), 21), 32, 32), "samples")
    # a dataset stored wider than the model: the centre window of the model's width
    wide = tiny_rolls(40, 64, seed=29)
    r = sample_music_stats(model, PianorollDataset(torch.from_numpy(wide.astype(np.float32)), storage="bits"), 12, seed=5, batch_size=16,
                           max_notes=4096)
    close(r["dataset"], R.summary(R.features(R.pack(wide[:, :, 16:48])), 32, 32), "wide")
    with pytest.raises(ValueError, match="'bits' storage"):
        sample_music_stats(model, PianorollDataset(torch.from_numpy(cells.astype(np.float32) * 0.5), storage="f32"), 4)
    with pytest.raises(ValueError, match="the model's 32x32"):
        sample_music_stats(model, PianorollDataset(torch.from_numpy(tiny_rolls(4, 32)[:, :16].astype(np.float32)), storage="bits"), 4)


def test_evaluate_with_music_stats():
    from torch_vae_amd.data import DevicePianorollLoader, PianorollDataset
    from torch_vae_amd.evaluation import evaluate
    from torch_vae_amd.generation import binarize_rolls
    model = tiny_model()
    cells = tiny_rolls(40, 32)
    ds = PianorollDataset(torch.from_numpy(cells.astype(np.float32)), storage="bits")
    loader = DevicePianorollLoader(ds, 16, train=False)

    def run(**kw):
        torch.manual_seed(3)          # the eval forward draws eps from torch's device generator
        return evaluate(loader, model, "cuda", verbosity=0, **kw)

    plain, with_music = run(note_thresholds=0.5), run(note_thresholds=0.5, music_stats=True)
    extra = sorted(k for k in with_music if k not in plain)
    assert extra and all(k.startswith("music_") for k in extra) and list(with_music)[:len(plain)] == list(plain)
    for k, v in plain.items():
        assert with_music[k] == v and type(with_music[k]) is type(v), k
    # against the reference on the reconstructions themselves
    torch.manual_seed(3)
    with torch.no_grad():
        rec = torch.cat([model(x)["output"] for x, _ in loader])
    want = R.compare(R.features(host(binarize_rolls(rec.float().contiguous(), 0.5))), R.features(R.pack(cells)))
    close({k[len("music_"):]: with_music[k] for k in extra}, want, "music")
    bare, second = run(), run(music_stats=True)          # the path without note_thresholds
    close({k: second[k] for k in extra}, {k: with_music[k] for k in extra}, "second")
    assert {k: second[k] for k in bare} == bare and list(second)[:len(bare)] == list(bare)
    assert not [k for k in bare if k.startswith("music_")]


# ---- the stream contract (include/vae_step.h, first paragraph) on the new entry point -------------------------------------------------
SKEY = (13, 64, 67, 21)


def _make_stats():
    planes, _ = R.gpu_cases()[SKEY]
    b = Bufs()
    b.inp("planes", torch.from_numpy(planes), poison=0xFF)
    b.outp("features", 67, F, dtype=torch.int32)
    b.outp("totals", F, dtype=torch.int64)
    b.outp("features_only", 67, F, dtype=torch.int32)
    return b


def _stats(b):
    ok(lib().vae_music_roll_stats(b["planes"].data_ptr(), 67, 13, 64, 21, b["features"].data_ptr(), b["totals"].data_ptr(), 0, st()))
    ok(lib().vae_music_roll_stats(b["planes"].data_ptr(), 67, 13, 64, 21, b["features_only"].data_ptr(), 0, 0, st()))


def _make_accumulate():
    planes, want = R.gpu_cases()[SKEY]
    b = Bufs()
    b.inp("planes", torch.from_numpy(planes), poison=0xFF)
    b.inp("totals", torch.from_numpy(R.totals(want[:30])), inout=True, poison=-12345)
    b.outp("features", 37, F, dtype=torch.int32)
    return b


def _accumulate(b):
    ok(lib().vae_music_roll_stats(b["planes"][30:].data_ptr(), 37, 13, 64, 21, b["features"].data_ptr(), b["totals"].data_ptr(), 1, st()))


STREAM_CASES = [
    Case("music_roll_stats", ("vae_music_roll_stats",), _make_stats, _stats),
    Case("music_roll_stats_accumulate", ("vae_music_roll_stats",), _make_accumulate, _accumulate),
]


def _make_python():
    planes, _ = R.gpu_cases()[SKEY]
    b = Bufs()
    b.inp("planes", torch.from_numpy(planes), poison=0xFF)
    b.inp("rolls", torch.from_numpy(R.unpack(planes[:20]).astype(np.float32)))
    return b


def _python(b):
    from torch_vae_amd.evaluation import MusicStatsAccumulator, music_statistics
    s = music_statistics(b["planes"], pitch_offset=21)
    b.out["features"], b.out["totals"] = s["features"], s["totals"]
    f = music_statistics(b["rolls"], pitch_offset=21)
    b.out["float_features"], b.out["float_totals"] = f["features"], f["totals"]
    acc = MusicStatsAccumulator(pitch_offset=21)
    for first in range(0, 67, 25):
        acc.update(b["planes"][first:first + 25])
    acc.update(b["rolls"])
    got = acc.compute()
    b.out["acc_features"], b.out["acc_totals"] = got["features"], got["totals"]


PY_STREAM_CASES = [
    Case("python/music_statistics+accumulator", ("vae_music_roll_stats",), _make_python, _python, warmups=2),
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_stream_contract(case):
    sh.check_case(case)
    if case.name == "music_roll_stats_accumulate":      # and what it accumulated is right
        b = case.make()
        sh.stage(b)
        case.run(b)
        assert np.array_equal(host(b["totals"]), R.totals(R.gpu_cases()[SKEY][1]))


@pytest.mark.parametrize("case", PY_STREAM_CASES, ids=repr)
def test_stream_contract_python_layer(case):
    sh.check_case(case)
