"""Note-level reconstruction metrics on the GPU (vae_recon_metrics, evaluation.reconstruction_metrics, ReconMetricsAccumulator,
evaluate(..., note_thresholds=...)) against the numpy f64 restatement in tests/test_recon_metrics_host.py, which that file checks
against torch's binary_cross_entropy and a brute-force count.

Gates: every count and range exactly equal; se / ae within 1e-12 relative (the same doubles, another summation order); bce within
1e-6 relative (non-negative terms; the device logf and the f32 products of the term are within a few f32 ulp of the f64 ones)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.test_loglik_gpu import model_for
from tests.test_recon_metrics_host import SPECIAL_XHAT, recon_metrics_reference, synthetic_rolls

pytestmark = pytest.mark.gpu

SUM_RTOL, BCE_RTOL = 1e-12, 1e-6
T1 = (0.5,)
T8 = (0.5, 0.0, 0.25, 0.3, 1.0, 0.3, 0.9, 0.05)          # unsorted, one repeated, the equalities of SPECIAL_XHAT among them
COUNT_KEYS = ("n_cells", "positives", "tp", "fp", "fn", "roll_positives", "roll_tp", "roll_fp")
TOTAL_KEYS = ("se", "ae", "bce", "n_cells", "positives", "tp", "fp", "fn", "xhat_range", "target_range")


@functools.lru_cache(maxsize=None)
def _case(shape, seed, velocity, thresholds, tt):
    x, t = synthetic_rolls(shape, seed, velocity)
    x.reshape(-1)[: len(SPECIAL_XHAT)] = SPECIAL_XHAT[: x.size]        # every special value at least once where there is room
    ref = recon_metrics_reference(x, t, thresholds, tt)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t, ref


def _rel(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if err.size and err.max() > 0 else 0.0
    print(f"{what}: max relative difference {worst:.3g} (gate {tol:g})")
    assert np.isfinite(got).all() and (err <= tol * np.abs(ref)).all(), (what, worst)


def _compare(out, ref, tag, keys=None):
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k in host if keys is None else keys:
        if k in COUNT_KEYS:
            assert host[k].dtype == np.int64, k
            np.testing.assert_array_equal(host[k], np.asarray(ref[k]), err_msg=f"{tag} {k}")
        elif k.endswith("_range"):
            np.testing.assert_array_equal(host[k], ref[k], err_msg=f"{tag} {k}")
        else:
            assert host[k].dtype == np.float64, k
            _rel(host[k], ref[k], BCE_RTOL if k.endswith("bce") else SUM_RTOL, f"{tag} {k}")


def _offset_view(a, off):
    """The array on the GPU as a contiguous view whose base pointer is 4 * off bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 4, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a)))
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


SHAPES = [(1, 1), (1, 3), (3, 1023), (2, 1024), (5, 1025), (2, 4100), (257, 64), (1, 65536), (4, 1, 32, 32), (2, 1, 128, 128)]


@pytest.mark.parametrize("thresholds", [T1, T8], ids=["T1", "T8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_reference(shape, thresholds):
    from torch_vae_amd.evaluation import reconstruction_metrics
    x, t, ref = _case(shape, 100 + len(shape) + shape[0], False, thresholds, 0.5)
    out = reconstruction_metrics(torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(t)).cuda(), thresholds)
    assert out["roll_tp"].shape == (shape[0], len(thresholds)) and out["tp"].shape == (len(thresholds),)
    _compare(out, ref, f"{shape} T{len(thresholds)}")


@pytest.mark.parametrize("shape", [(5, 1025), (4, 1, 32, 32)], ids=["5x1025", "4x1x32x32"])
def test_velocity_targets(shape):
    from torch_vae_amd.evaluation import reconstruction_metrics
    x, t, ref = _case(shape, 31, True, T8, 0.3)
    assert 0 < ref["positives"] < int((np.asarray(t) > 0).sum())          # the threshold cuts through the velocities
    out = reconstruction_metrics(torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(t)).cuda(), T8, target_threshold=0.3)
    _compare(out, ref, f"velocity {shape}")


@pytest.mark.parametrize("offsets", [(1, 1), (1, 0), (0, 3), (2, 3)], ids=lambda o: f"x{o[0]}t{o[1]}")
@pytest.mark.parametrize("shape", [(1, 3), (5, 1025), (2, 4100)], ids=["1x3", "5x1025", "2x4100"])
def test_unaligned_views(shape, offsets):
    """Base pointers 4-byte but not 16-byte aligned, alike and differently for the two tensors (odd roll lengths move every later
    roll's base as well)."""
    from torch_vae_amd.evaluation import reconstruction_metrics
    x, t, ref = _case(shape, 100 + len(shape) + shape[0], False, T8, 0.5)
    out = reconstruction_metrics(_offset_view(x, offsets[0]), _offset_view(t, offsets[1]), T8)
    _compare(out, ref, f"{shape} offsets {offsets}")


def test_nan_output_is_never_a_note():
    from torch_vae_amd.evaluation import reconstruction_metrics
    x, t = (np.array(a) for a in _case((3, 1023), 106, False, T8, 0.5)[:2])
    x[1, 5] = x[1, 1000] = np.nan
    ref = recon_metrics_reference(x, t, T8, 0.5)
    out = {k: v.cpu().numpy() for k, v in reconstruction_metrics(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), T8).items()}
    for k in COUNT_KEYS:
        np.testing.assert_array_equal(out[k], np.asarray(ref[k]), err_msg=k)
    for k in ("se", "ae", "bce"):
        assert np.isnan(out[k]) and np.isnan(out["roll_" + k][1]) and np.isfinite(out["roll_" + k][[0, 2]]).all(), k
    np.testing.assert_array_equal(out["xhat_range"], ref["xhat_range"])


def test_repeated_calls_are_bit_identical():
    from torch_vae_amd.evaluation import reconstruction_metrics
    for shape in ((5, 1025), (2, 4100), (257, 64)):
        x, t, _ = _case(shape, 100 + len(shape) + shape[0], False, T8, 0.5)
        xd, td = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(t)).cuda()
        a, b = reconstruction_metrics(xd, td, T8), reconstruction_metrics(xd, td, T8)
        for k in a:
            assert torch.equal(a[k], b[k]), (shape, k)          # finite values: equal means the same bits


def test_accumulator_split_matches_one_call():
    from torch_vae_amd.evaluation import ReconMetricsAccumulator, reconstruction_metrics
    x, t, _ = _case((19, 4100), 77, False, T8, 0.5)
    xd, td = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(t)).cuda()
    xd[:8] = xd[:8] * 0.5 + 0.25            # the ranges grow after the first batch (xhat) and in the last one (target's maximum)
    td[:16] = td[:16] * 0.75
    xh, th = xd.cpu().numpy(), td.cpu().numpy()
    ref = recon_metrics_reference(xh, th, T8, 0.5)
    one = reconstruction_metrics(xd, td, T8)
    acc = ReconMetricsAccumulator(T8)
    for a, b in ((0, 8), (8, 16), (16, 19)):
        acc.update(xd[a:b], td[a:b])
    tot = acc.totals()
    for k in TOTAL_KEYS:
        if k in ("se", "ae", "bce"):
            _rel(tot[k].cpu(), one[k].cpu().numpy(), SUM_RTOL, "split vs one call " + k)
        else:
            assert torch.equal(tot[k], one[k]), k
    _compare(tot, ref, "accumulated", TOTAL_KEYS)
    got = acc.compute()
    n = xh.size
    assert got["count_cells"] == n and got["note_density"] == ref["positives"] / n
    assert got["xhat_range"] == tuple(ref["xhat_range"]) and got["target_range"] == tuple(ref["target_range"])
    for k in ("mse", "mae"):
        _rel(got[k], ref[k[1:]] / n, SUM_RTOL, "compute " + k)
    _rel(got["bce"], ref["bce"] / n, BCE_RTOL, "compute bce")
    tp, fp, fn = (ref[k].astype(np.float64) for k in ("tp", "fp", "fn"))
    _rel(got["precision"], tp / (tp + fp), 1e-15, "precision")
    _rel(got["recall"], tp / (tp + fn), 1e-15, "recall")
    _rel(got["f1"], 2 * tp / (2 * tp + fp + fn), 1e-15, "f1")
    _rel(got["pred_density"], (tp + fp) / n, 1e-15, "pred_density")
    _rel(got["accuracy"], (n - fp - fn) / n, 1e-15, "accuracy")
    acc.reset()
    cleared = acc.compute()
    assert cleared["count_cells"] == 0 and cleared["mse"] == 0.0 and cleared["bce"] == 0.0 and cleared["recall"] == [0.0] * 8
    acc.update(xd[16:], td[16:])            # after reset() the ranges start again: nothing of the first pass is left
    last = reconstruction_metrics(xd[16:], td[16:], T8)
    for k in TOTAL_KEYS:
        assert torch.equal(acc.totals()[k], last[k]), k


def _raw_call(x, t, rolls, roll_len, thresholds, tt, rs, rc, tot, cnt, accumulate):
    from torch_vae_amd import _lib
    ptr = lambda a: None if a is None else a.data_ptr()
    thr = None if thresholds is None else (ctypes.c_float * max(len(thresholds), 1))(*thresholds)
    n = 0 if thresholds is None else len(thresholds)
    return _lib.lib().vae_recon_metrics(ptr(x), ptr(t), rolls, roll_len, thr, n, tt, ptr(rs), ptr(rc), ptr(tot), ptr(cnt), accumulate,
                                        torch.cuda.current_stream().cuda_stream)


def test_zero_rolls_zeroes_or_keeps_the_totals():
    from torch_vae_amd.evaluation import reconstruction_metrics
    tot = torch.full((8,), 3.5, device="cuda", dtype=torch.float64)
    cnt = torch.full((5,), 7, device="cuda", dtype=torch.int64)
    assert _raw_call(None, None, 0, 16, (0.5, 0.3), 0.5, None, None, tot, cnt, 1) == 0
    assert bool((tot == 3.5).all()) and bool((cnt == 7).all())
    assert _raw_call(None, None, 0, 16, (0.5, 0.3), 0.5, None, None, tot, cnt, 0) == 0
    assert bool((tot == 0).all()) and bool((cnt == 0).all())
    out = reconstruction_metrics(torch.empty(0, 5, device="cuda"), torch.empty(0, 5, device="cuda"), (0.5, 0.3))
    assert int(out["n_cells"]) == 0 and float(out["se"]) == 0.0 and out["tp"].tolist() == [0, 0] and out["roll_tp"].shape == (0, 2)


def test_argument_errors_through_the_c_abi():
    from torch_vae_amd import _lib
    x = torch.rand(2, 16, device="cuda")
    t = torch.zeros(2, 16, device="cuda")
    rs = torch.zeros(2, 3, device="cuda", dtype=torch.float64)
    rc = torch.zeros(2, 17, device="cuda", dtype=torch.int64)
    tot = torch.full((8,), 3.5, device="cuda", dtype=torch.float64)
    cnt = torch.full((17,), 7, device="cuda", dtype=torch.int64)
    ok = (x, t, 2, 16, (0.5,), 0.5, rs, rc, tot, cnt, 0)

    def bad(**kw):
        names = ("x", "t", "rolls", "roll_len", "thresholds", "tt", "rs", "rc", "tot", "cnt", "accumulate")
        args = [kw.get(n, v) for n, v in zip(names, ok)]
        assert _raw_call(*args) != 0, kw
        msg = _lib.lib().vae_last_error().decode()
        assert "vae_recon_metrics" in msg, msg
        return msg

    for name in ("x", "t", "rs", "rc", "tot", "cnt", "thresholds"):
        assert "null" in bad(**{name: None})
    assert "n_thresholds" in bad(thresholds=())
    assert "n_thresholds" in bad(thresholds=(0.5,) * 9)
    assert "finite" in bad(thresholds=(0.5, float("nan")))
    assert "finite" in bad(thresholds=(float("inf"),))
    assert "finite" in bad(tt=float("nan"))
    assert "roll_len" in bad(roll_len=0)
    assert "rolls" in bad(rolls=-1)
    torch.cuda.synchronize()
    assert bool((tot == 3.5).all()) and bool((cnt == 7).all())          # a refused call touches nothing
    assert _raw_call(*ok) == 0


def test_update_does_not_synchronise_with_the_host():
    from torch_vae_amd.evaluation import ReconMetricsAccumulator
    x, t, _ = _case((4, 1, 32, 32), 105, False, T1, 0.5)
    xd, td = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(t)).cuda()
    acc = ReconMetricsAccumulator((0.5, 0.3))
    acc.update(xd, td)                       # the library is loaded and the state allocated before the mode is switched on
    one = torch.ones(1, device="cuda")
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            one.item()
            probe = False
        except RuntimeError:
            probe = True
        if probe:
            acc.update(xd, td)
            acc.update(xd[:3], td[:3])       # another batch size: the per-roll work space is replaced, still without a sync
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not probe:
        print("torch.cuda.set_sync_debug_mode('error') does not catch .item() on this build: the no-synchronisation assertion is skipped")
    assert acc.compute()["count_cells"] == (11 if probe else 4) * 1024


class _Loader(list):
    pass


@functools.lru_cache(maxsize=None)
def _eval_setup():
    H, L = 32, 16
    m = model_for(H, L, False, "f32", "bce")
    rolls = torch.from_numpy(vo.synth_pianoroll(19, H, 4242).astype(np.float32))
    loader = _Loader((rolls[a:b], torch.zeros(b - a, dtype=torch.long)) for a, b in ((0, 8), (8, 16), (16, 19)))
    return m, loader


def test_evaluate_default_path_is_unchanged():
    from torch_vae_amd.evaluation import evaluate
    m, loader = _eval_setup()
    torch.manual_seed(5)
    res = evaluate(loader, m, "cuda", verbosity=0)
    assert list(res) == ["count", "cross-entropy", "mse", "mae"] and res["count"] == 19 and res["cross-entropy"] == 0.0
    torch.manual_seed(5)
    assert evaluate(loader, m, "cuda", verbosity=0, note_thresholds=None) == res


def test_evaluate_note_thresholds(capsys):
    from torch_vae_amd.evaluation import evaluate
    m, loader = _eval_setup()
    torch.manual_seed(5)
    base = evaluate(loader, m, "cuda", verbosity=1)
    out_base = capsys.readouterr().out
    torch.manual_seed(5)
    res = evaluate(loader, m, "cuda", verbosity=1, note_thresholds=(0.5, 0.3))
    printed = capsys.readouterr().out
    assert list(res) == ["count", "cross-entropy", "mse", "mae", "bce", "precision", "recall", "f1", "note_density", "best_f1",
                         "best_threshold"]
    assert res["count"] == 19 and res["cross-entropy"] == 0.0
    _rel(res["mse"], base["mse"], SUM_RTOL, "evaluate mse")
    _rel(res["mae"], base["mae"], SUM_RTOL, "evaluate mae")
    assert printed.splitlines()[:2] == out_base.splitlines()[:2]                 # the two range lines
    for k in ("bce", "precision", "recall", "f1", "note_density", "best_f1", "best_threshold"):
        assert sum(line.strip().startswith(k + " .") for line in printed.splitlines()) == 1, k
    line = lambda k: next(l for l in printed.splitlines() if l.strip().startswith(k + " ."))
    assert line("bce").endswith(" nat") and line("f1").endswith(" %") and line("best_threshold").strip()[-1].isdigit()
    # the same eps again: the model's own outputs, batch by batch in loader order, through the restatement
    torch.manual_seed(5)
    m.eval()
    with torch.no_grad():
        rec = np.concatenate([m(x.cuda())["output"].cpu().numpy() for x, _ in loader])
    ref = recon_metrics_reference(rec, np.concatenate([x.numpy() for x, _ in loader]), (0.5, 0.3), 0.5)
    n = ref["n_cells"]
    tp, fp, fn = (ref[k].astype(np.float64) for k in ("tp", "fp", "fn"))
    f1 = 2 * tp / np.maximum(2 * tp + fp + fn, 1)
    _rel(res["bce"], ref["bce"] / n, BCE_RTOL, "evaluate bce")
    _rel(res["precision"], 100 * tp[0] / max(tp[0] + fp[0], 1), SUM_RTOL, "evaluate precision")
    _rel(res["recall"], 100 * tp[0] / max(tp[0] + fn[0], 1), SUM_RTOL, "evaluate recall")
    _rel(res["f1"], 100 * f1[0], SUM_RTOL, "evaluate f1")
    _rel(res["note_density"], 100 * ref["positives"] / n, SUM_RTOL, "evaluate note_density")
    _rel(res["best_f1"], 100 * f1.max(), SUM_RTOL, "evaluate best_f1")
    assert res["best_threshold"] == float(np.float32((0.5, 0.3)[int(f1.argmax())]))
    assert ref["positives"] > 0 and 0.0 < res["note_density"] < 100.0
    # one threshold, given as a float: no best_* keys
    torch.manual_seed(5)
    single = evaluate(loader, m, "cuda", verbosity=0, note_thresholds=0.3)
    assert list(single) == list(res)[:-2]
    _rel(single["f1"], 100 * f1[1], SUM_RTOL, "evaluate f1 at 0.3")


def test_evaluate_note_thresholds_composes(capsys):
    from torch_vae_amd.evaluation import evaluate
    m, loader = _eval_setup()
    c0 = m._ll_count
    torch.manual_seed(6)
    plain = evaluate(loader, m, "cuda", verbosity=0, nll_samples=2, latent_rolls=8)
    m._ll_count = c0                         # the same likelihood seeds again
    torch.manual_seed(6)
    both = evaluate(loader, m, "cuda", verbosity=0, nll_samples=2, latent_rolls=8, note_thresholds=(0.5, 0.3))
    for k in ("count", "cross-entropy", "nll", "elbo", "kl", "active_units", "mi", "tc", "dwkl"):
        assert both[k] == plain[k], k
    assert set(both) - set(plain) == {"bce", "precision", "recall", "f1", "note_density", "best_f1", "best_threshold"}
    assert capsys.readouterr().out == ""
    _rel(both["mse"], plain["mse"], SUM_RTOL, "composed mse")
