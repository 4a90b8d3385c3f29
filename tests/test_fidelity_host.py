"""Host side (no GPU) of the fidelity tests: the numpy reference (tests/fidelity_ref.py) against identities and closed forms, the
conditions the inputs of the GPU tests must meet (checked here, before anything is sent to a device), the refusals of
include/vae_fidelity.h through fake, never dereferenced pointers, the header / export bookkeeping and the argument checks of the
Python layer."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import fidelity_ref as R
from tests import test_fidelity_gpu as gpu_cases
from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_fidelity.h")
P = 4096          # a fake device address, 16-byte aligned


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_identical_sets():
    x = R.gpu_cases()[("gaussian", 16, 193, 131)]["a"]
    for k in R.KS:
        p = R.prdc(x, x, k)
        assert p["precision"] == p["recall"] == p["coverage"] == 1.0 and p["density"] >= 1.0
    assert R.frechet_distance(x, x) == pytest.approx(0.0, abs=1e-12)
    idx, best, _ = R.nearest(R.d2(x, x))
    assert np.array_equal(idx, np.arange(193)) and not best.any()
    assert (R.mmd2(x, x) < 0).all()                        # the unbiased estimator of a set with itself


def test_far_apart_clusters():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((50, 4)).astype(np.float32)
    b = (rng.standard_normal((40, 4)) + 100.0).astype(np.float32)
    p = R.prdc(a, b, 3)
    assert p["precision"] == p["recall"] == p["density"] == p["coverage"] == 0.0
    assert R.mmd2(a, b, [1.0])[0] > 0.05      # no cross term: the two within-set means, about 2 * 5^-2 for unit Gaussians in 4-D


def test_frechet_of_diagonal_gaussians_in_closed_form():
    m1, m2 = np.array([0.5, -1.0, 2.0]), np.array([0.0, 1.0, 2.5])
    v1, v2 = np.array([0.3, 2.0, 1.0]), np.array([1.2, 0.5, 1.0])
    want = ((m1 - m2) ** 2).sum() + ((np.sqrt(v1) - np.sqrt(v2)) ** 2).sum()
    assert R.frechet(m1, np.diag(v1), m2, np.diag(v2)) == pytest.approx(want, abs=1e-9)
    from torch_vae_amd.fidelity import frechet_from_moments
    assert frechet_from_moments(m1, np.diag(v1), m2, np.diag(v2)) == pytest.approx(want, abs=1e-9)
    x, y = R.frechet_cases()[0]
    assert frechet_from_moments(*R.moments(x), *R.moments(y)) == R.frechet_distance(x, y)


def test_mmd2_by_hand():
    """x = {0, 1}, y = {0, 3} on the line, gamma = 1: K_xx' = 2 e^-1, K_yy' = 2 e^-9, K_xy = 1 + e^-9 + e^-1 + e^-4"""
    x, y = np.array([[0.0], [1.0]], np.float32), np.array([[0.0], [3.0]], np.float32)
    e = math.exp
    want = 2 * e(-1) / 2 + 2 * e(-9) / 2 - 2 * (1 + e(-9) + e(-1) + e(-4)) / 4
    assert R.mmd2(x, y, [1.0])[0] == pytest.approx(want, rel=1e-14)
    assert R.mmd2(x, x, [1.0])[0] == pytest.approx(2 * e(-1) - 2 * (2 + 2 * e(-1)) / 4, rel=1e-14)     # = e^-1 - 1
    assert R.kernel_sums(R.d2(x, y), [])[0] == 0 + 9 + 1 + 4


def test_radii_two_ways_and_special_values():
    c = R.gpu_cases()[("lattice", 3, 193, 131)]
    for k in R.KS:
        assert np.array_equal(R.radii(c["a"], k), R.radii_by_exclusion(c["a"], k))      # a duplicate is a neighbour at 0 either way
    assert (R.radii(c["a"], 1) == 0).any()
    x = np.array([[0.0], [1.0], [np.nan], [np.inf], [3.0]], np.float32)
    assert R.radii(x, 1).tolist() == [1.0, 1.0, np.inf, np.inf, 4.0] and R.radii(x, 3).tolist() == [np.inf] * 5
    idx, best, _ = R.nearest(R.d2(x, x), exclude=True)
    assert idx.tolist() == [1, 0, -1, -1, 1] and best.tolist() == [1.0, 1.0, np.inf, np.inf, 4.0]
    rad = np.array([1.0, 0.5, np.inf, np.inf, 100.0])
    assert R.counts(R.d2(x, x), rad).tolist() == [3, 4, 0, 0, 2]      # +inf <= +inf counts; NaN (row 2, and inf - inf) never does


# ---- what the GPU cases must be (the conditions of the issue on the inputs) ---------------------------------------------------------------
def test_gpu_cases_cover_the_shapes():
    cases = R.gpu_cases()
    assert list(cases) == gpu_cases.CASE_KEYS
    assert {k[1] for k in cases} == {1, 3, 16, 67, 128} and {k[2:] for k in cases} == {(193, 131), (65, 64), (7, 300), (2, 1)}
    assert gpu_cases.SPLITS == (1, 2, 5, 64) and R.KS == (1, 3, 8)
    for (kind, D, n, m), c in cases.items():
        assert c["a"].shape == (n, D) and c["b"].shape == (m, D) and c["a"].dtype == c["b"].dtype == np.float32
        assert sorted(c["radii"]) == [k for k in R.KS if k < n] and len(c["gammas"]) == 8


def test_lattice_cases_are_exact_and_hold_ties():
    for key, c in R.gpu_cases().items():
        if key[0] != "lattice":
            continue
        for x in (c["a"], c["b"]):
            assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x * 8).max() <= 16
        assert (c["ab"] * 64 == np.round(c["ab"] * 64)).all() and c["ab"].max() * 64 < 2 ** 24       # exact in f32, in any order
        if key[2] >= 7 and key[3] > 1:
            assert (c["ab"] == 0).any()                                                             # duplicates across the sets
            on_boundary = sum(int((R.counts(c["ab"], c["ball_radii"][k].astype(np.float64))
                                   - R.counts(c["ab"], c["ball_radii"][k].astype(np.float64), strict=True)).sum()) for k in R.KS)
            assert on_boundary > 0                                                                  # d2 == radius2: <= must count them
        if key[2] >= 65:
            assert (c["nearest"][1] == c["nearest"][2]).any()                                       # ties for the nearest reference
            assert (c["radii"][1] == 0).any()                                                       # duplicates within a set


@pytest.mark.parametrize("key", [k for k in R.gpu_cases() if k[0] == "gaussian"], ids=str)
def test_undecided_pairs_of_the_gaussian_cases(key):
    c = R.gpu_cases()[key]
    for k in R.KS:
        assert R.undecided(c, k) <= R.UNDECIDED_CAP * c["n"] * c["m"], (k, R.undecided(c, k))
    if key == gpu_cases.PKEY:          # the Python-layer case: precision, recall, density and coverage are exact
        for k in (1, 5):
            for real, fake in ((c["a"], c["b"]), (c["b"], c["a"])):
                rad = R.radii(real, k).astype(np.float32).astype(np.float64)
                dist = R.d2(fake, real)
                assert not (np.abs(dist - rad[None, :]) <= R.tol(16) * rad[None, :]).any()
            rad = R.radii(c["a"], k)
            best = R.nearest(c["ab"])[1]
            assert not (np.abs(best - rad) <= 2 * R.tol(16) * rad).any()                            # coverage: both sides are rounded


@pytest.mark.parametrize("D", R.DIMS)
def test_consistency_sets_have_the_gap(D):
    x = R.consistency_set(D)
    assert x.shape == (R.CONSISTENCY_N, D) and R.consistency_gap_ok(x, D)


def test_frechet_cases_are_well_conditioned():
    for x, y in R.frechet_cases():
        assert x.shape == y.shape == (512, 16)
        assert R.frechet_distance(x, y) > 1.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def knn(L, x=P, n=10, D=4, k=3, splits=0, radii2=P):
    return L.vae_fidelity_knn_radii(x, n, D, k, splits, radii2, None)


def balls(L, q=P, m=10, r=P, n=12, D=4, radii2=P, exclude=0, splits=0, counts=P, nearest=P, nearest_d2=P):
    return L.vae_fidelity_balls(q, m, r, n, D, radii2, exclude, splits, counts, nearest, nearest_d2, None)


def ksums(L, a=P, n=10, b=P, m=12, D=4, gammas=P, G=2, exclude=0, splits=0, sums=P):
    return L.vae_fidelity_kernel_sums(a, n, b, m, D, gammas, G, exclude, splits, sums, None)


BIG = (1 << 22) + 1
KNN, BALLS, SUMS = "vae_fidelity_knn_radii", "vae_fidelity_balls", "vae_fidelity_kernel_sums"
REFUSALS = {
    "knn_null_x": (KNN, lambda L: knn(L, x=None), "null pointer (x, radii2)"),
    "knn_null_radii2": (KNN, lambda L: knn(L, radii2=None), "null pointer (x, radii2)"),
    "knn_D_0": (KNN, lambda L: knn(L, D=0), "D must be in 1..128"),
    "knn_D_129": (KNN, lambda L: knn(L, D=129), "D must be in 1..128"),
    "knn_n_0": (KNN, lambda L: knn(L, n=0), "set sizes must be in 1..2^22"),
    "knn_n_above_2^22": (KNN, lambda L: knn(L, n=BIG), "set sizes must be in 1..2^22"),
    "knn_splits_negative": (KNN, lambda L: knn(L, splits=-1), "splits must be in 0..64"),
    "knn_splits_65": (KNN, lambda L: knn(L, splits=65), "splits must be in 0..64"),
    "knn_k_0": (KNN, lambda L: knn(L, k=0), "k must be in 1..8"),
    "knn_k_9": (KNN, lambda L: knn(L, k=9, n=100), "k must be in 1..8"),
    "knn_k_equals_n": (KNN, lambda L: knn(L, k=3, n=3), "k must be < n"),
    "knn_one_point": (KNN, lambda L: knn(L, k=1, n=1), "k must be < n"),
    "knn_partials": (KNN, lambda L: knn(L, n=(1 << 20) + 1, splits=64), "splits * queries must stay within 2^26"),
    "knn_x_plus_2": (KNN, lambda L: knn(L, x=P + 2), "x and radii2 must be 4-byte aligned"),
    "knn_radii2_plus_1": (KNN, lambda L: knn(L, radii2=P + 1), "x and radii2 must be 4-byte aligned"),
    "balls_null_q": (BALLS, lambda L: balls(L, q=None), "null pointer (q, r, nearest, nearest_d2)"),
    "balls_null_r": (BALLS, lambda L: balls(L, r=None), "null pointer (q, r, nearest, nearest_d2)"),
    "balls_null_nearest": (BALLS, lambda L: balls(L, nearest=None), "null pointer (q, r, nearest, nearest_d2)"),
    "balls_null_nearest_d2": (BALLS, lambda L: balls(L, nearest_d2=None), "null pointer (q, r, nearest, nearest_d2)"),
    "balls_D_129": (BALLS, lambda L: balls(L, D=129), "D must be in 1..128"),
    "balls_m_0": (BALLS, lambda L: balls(L, m=0), "set sizes must be in 1..2^22"),
    "balls_n_above_2^22": (BALLS, lambda L: balls(L, n=BIG), "set sizes must be in 1..2^22"),
    "balls_splits_65": (BALLS, lambda L: balls(L, splits=65), "splits must be in 0..64"),
    "balls_counts_without_radii2": (BALLS, lambda L: balls(L, radii2=None), "counts needs radii2"),
    "balls_partials": (BALLS, lambda L: balls(L, m=(1 << 21) + 1, splits=32), "splits * queries must stay within 2^26"),
    "balls_q_plus_1": (BALLS, lambda L: balls(L, q=P + 1), "every pointer must be 4-byte aligned"),
    "balls_counts_plus_2": (BALLS, lambda L: balls(L, counts=P + 2), "every pointer must be 4-byte aligned"),
    "balls_radii2_plus_2": (BALLS, lambda L: balls(L, radii2=P + 2), "every pointer must be 4-byte aligned"),
    "sums_null_a": (SUMS, lambda L: ksums(L, a=None), "null pointer (a, b, sums)"),
    "sums_null_b": (SUMS, lambda L: ksums(L, b=None), "null pointer (a, b, sums)"),
    "sums_null_sums": (SUMS, lambda L: ksums(L, sums=None), "null pointer (a, b, sums)"),
    "sums_D_0": (SUMS, lambda L: ksums(L, D=0), "D must be in 1..128"),
    "sums_m_0": (SUMS, lambda L: ksums(L, m=0), "set sizes must be in 1..2^22"),
    "sums_n_above_2^22": (SUMS, lambda L: ksums(L, n=BIG), "set sizes must be in 1..2^22"),
    "sums_splits_65": (SUMS, lambda L: ksums(L, splits=65), "splits must be in 0..64"),
    "sums_G_negative": (SUMS, lambda L: ksums(L, G=-1), "G must be in 0..8"),
    "sums_G_9": (SUMS, lambda L: ksums(L, G=9), "G must be in 0..8"),
    "sums_null_gammas": (SUMS, lambda L: ksums(L, gammas=None, G=1), "null gammas with G > 0"),
    "sums_partials": (SUMS, lambda L: ksums(L, n=(1 << 22), splits=17), "splits * queries must stay within 2^26"),
    "sums_gammas_plus_4": (SUMS, lambda L: ksums(L, gammas=P + 4), "a and b must be 4-byte, gammas and sums 8-byte aligned"),
    "sums_sums_plus_4": (SUMS, lambda L: ksums(L, sums=P + 4), "a and b must be 4-byte, gammas and sums 8-byte aligned"),
    "sums_a_plus_2": (SUMS, lambda L: ksums(L, a=P + 2), "a and b must be 4-byte, gammas and sums 8-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_message(case):
    L = _lib.lib()
    entry, call, want = REFUSALS[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == f"{entry}: {want}"


def test_every_refusal_of_the_header_is_tested():
    text = open(HEADER).read()
    for entry, _, want in REFUSALS.values():
        assert entry in text
    listed = {want for _, _, want in REFUSALS.values()}
    source = open(os.path.join(ROOT, "torch_vae_amd", "csrc", "vae_fidelity.hip")).read()
    in_source = set(re.findall(r'"([^"]+)"', "".join(line for line in source.splitlines(True) if "vae_set_error(what" in line or "return \"" in line or "? \"" in line)))
    in_source = {s for s in in_source if " " in s}
    assert in_source == listed, in_source ^ listed


def test_limits_are_accepted_up_to_the_refusal():
    """Nothing can be launched here, so a call at every limit at once is given one misaligned pointer: it must get past every other
    check and be refused for that pointer alone (alignment is checked last)."""
    L = _lib.lib()
    top = 1 << 22
    assert knn(L, x=P + 2, n=top, D=128, k=8, splits=16) == -1
    assert L.vae_last_error().decode() == "vae_fidelity_knn_radii: x and radii2 must be 4-byte aligned"
    assert knn(L, x=P + 2, n=9, D=1, k=8, splits=64) == -1 and L.vae_last_error().decode().endswith("4-byte aligned")
    assert knn(L, x=P + 2, n=2, D=1, k=1, splits=0) == -1 and L.vae_last_error().decode().endswith("4-byte aligned")
    assert balls(L, q=P + 2, m=top, n=top, D=128, splits=16) == -1 and L.vae_last_error().decode().endswith("every pointer must be 4-byte aligned")
    assert balls(L, q=P + 2, m=1, n=1, D=1, splits=64, radii2=None, counts=None) == -1 and L.vae_last_error().decode().endswith("4-byte aligned")
    assert ksums(L, sums=P + 4, n=top, m=top, D=128, G=8, splits=16) == -1 and L.vae_last_error().decode().endswith("8-byte aligned")
    assert ksums(L, sums=P + 4, n=1, m=1, D=1, G=0, gammas=None, splits=64) == -1 and L.vae_last_error().decode().endswith("8-byte aligned")


# ---- the header, the exports and the stream-case table ------------------------------------------------------------------------------
def _header(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def test_header_declares_exactly_the_fidelity_exports():
    declared = set(re.findall(r"\b(vae_[a-z0-9_]+)\s*\(", _header(HEADER)))
    assert declared == set(_lib.FIDELITY_EXPORTS) == {KNN, BALLS, SUMS}
    assert all(n.startswith("vae_fidelity_") for n in _lib.FIDELITY_EXPORTS)
    L = _lib.lib()
    assert not [n for n in _lib.FIDELITY_EXPORTS if not hasattr(L, n)]
    assert not set(_lib.FIDELITY_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.MIXTURE_EXPORTS) | set(_lib.MUSIC_EXPORTS))
    assert L.vae_abi_version() == 1
    raw = open(HEADER).read()
    for name, value in (("VAE_FID_MAX_DIM", _lib.FID_MAX_DIM), ("VAE_FID_MAX_K", _lib.FID_MAX_K), ("VAE_FID_MAX_BANDWIDTHS", _lib.FID_MAX_BANDWIDTHS),
                        ("VAE_FID_MAX_SPLITS", _lib.FID_MAX_SPLITS)):
        assert int(re.search(rf"#define {name} (\d+)", raw).group(1)) == value
    assert re.search(r"#define VAE_FID_MAX_POINTS \(1 << 22\)", raw) and _lib.FID_MAX_POINTS == 1 << 22


def test_the_other_headers_declare_no_fidelity_function():
    for name in ("vae_step.h", "vae_mixture.h", "vae_music.h"):
        assert "vae_fidelity_" not in _header(os.path.join(ROOT, "include", name)), name


def test_every_stream_entry_point_of_the_header_has_a_stream_case():
    names = [m.group(1) for m in re.finditer(r"\b(vae_\w+)\s*\(([^;{}]*?)\)\s*;", _header(HEADER)) if re.search(r"\bvae_stream_t\b", m.group(2))]
    assert sorted(names) == sorted(_lib.FIDELITY_EXPORTS)
    covered = set()
    for c in gpu_cases.STREAM_CASES:
        assert c.sync_free and c.reads_back is None, c.name
        covered |= set(c.covers)
    assert sorted(covered) == sorted(names)
    called = set(re.findall(r"lib\(\)\.(vae_\w+)\(", inspect.getsource(gpu_cases)))
    for c in gpu_cases.STREAM_CASES:
        assert not [n for n in c.covers if n not in called], c.name
    all_names = [c.name for c in gpu_cases.STREAM_CASES + gpu_cases.PY_STREAM_CASES]
    assert len(set(all_names)) == len(all_names)
    for c in gpu_cases.PY_STREAM_CASES:
        assert c.sync_free and c.reads_back is None, c.name      # nothing of the device-side Python layer reads back
        assert set(_lib.FIDELITY_EXPORTS) <= set(c.covers)


# ---- Python argument checks (all raised before anything touches a device) ------------------------------------------------------------
def test_python_argument_checks():
    from torch_vae_amd import fidelity as F
    import torch_vae_amd
    assert torch_vae_amd.compare_encodings is F.compare_encodings and torch_vae_amd.sample_fidelity is F.sample_fidelity
    assert "compare_encodings" in torch_vae_amd.__all__ and "sample_fidelity" in torch_vae_amd.__all__
    x = torch.zeros(10, 4)
    for call in (lambda: F.knn_radii(x), lambda: F.ball_membership(x, x), lambda: F.kernel_sums(x, x, [1.0]), lambda: F.mmd2(x, x),
                 lambda: F.precision_recall(x, x), lambda: F.frechet_distance(x, x), lambda: F.compare_encodings(x, x)):
        with pytest.raises(ValueError, match="must be on the GPU"):
            call()
    for bad, word in ((x.numpy(), "must be a tensor"), (torch.zeros(10), r"\[n, D\]"), (torch.zeros(10, 4, dtype=torch.float64), "float32"),
                      (torch.zeros(10, 4, dtype=torch.float16), "float32")):
        with pytest.raises(ValueError, match=word):
            F.knn_radii(bad)
        with pytest.raises(ValueError, match=word):
            F.kernel_sums(bad, bad, None)
    with pytest.raises(TypeError, match="PianorollDataset"):
        F.sample_fidelity(None, x, 4)


def test_python_checks_that_need_device_tensors():
    """the checks behind the device check, on meta tensors that claim to be on the GPU: none of them reaches the library"""
    from torch_vae_amd import fidelity as F

    class OnGpu(torch.Tensor):
        device = torch.device("cuda", 0)

    def fake(*shape, dtype=torch.float32):
        t = torch.zeros(*shape, dtype=dtype).as_subclass(OnGpu)
        t.detach = lambda: t
        t.contiguous = lambda: t
        return t

    x, y = fake(10, 4), fake(12, 4)
    for k in (0, 9, 1.0, True, "3"):
        with pytest.raises(ValueError, match="k must be an integer in 1..8"):
            F.knn_radii(x, k)
    with pytest.raises(ValueError, match="k must be below the number of points"):
        F.knn_radii(fake(5, 4), 5)
    with pytest.raises(ValueError, match="k must be below the number of points"):
        F.precision_recall(x, fake(3, 4), 3)
    for s in (-1, 65, 1.0):
        with pytest.raises(ValueError, match="splits must be an integer in 0..64"):
            F.knn_radii(x, 3, splits=s)
    with pytest.raises(ValueError, match="1..128 columns"):
        F.knn_radii(fake(10, 129))
    with pytest.raises(ValueError, match="1..128 columns"):
        F.frechet_distance(fake(10, 129), fake(10, 129))
    with pytest.raises(ValueError, match=r"1..2\^22 rows"):
        F.knn_radii(fake(0, 4))
    with pytest.raises(ValueError, match="same number of columns"):
        F.ball_membership(x, fake(12, 5))
    with pytest.raises(ValueError, match="radii2 must be a float32 tensor"):
        F.ball_membership(x, y, radii2=fake(10))
    with pytest.raises(ValueError, match="at least 2 points a side"):
        F.mmd2(fake(1, 4), y)
    with pytest.raises(ValueError, match="at least 2 points a side"):
        F.compare_encodings(x, fake(1, 4))
    with pytest.raises(ValueError, match="at least 2 points"):
        F.frechet_distance(fake(1, 4), y)
    with pytest.raises(ValueError, match="gammas must be finite"):
        F.kernel_sums(x, y, [1.0, -1.0])
    with pytest.raises(ValueError, match="gammas must be finite"):
        F.kernel_sums(x, y, [float("inf")])
    with pytest.raises(ValueError, match="finite positive gammas"):
        F.mmd2(x, y, bandwidths=[0.0])
    with pytest.raises(ValueError, match="finite positive gammas"):
        F.mmd2(x, y, bandwidths=[1.0] * 9)
