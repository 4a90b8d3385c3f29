"""The set-level fidelity metrics (include/vae_fidelity.h: vae_fidelity_knn_radii, vae_fidelity_balls, vae_fidelity_kernel_sums) and
their Python layer (torch_vae_amd/fidelity.py) on the GPU against the numpy float64 reference of tests/fidelity_ref.py.  Lattice
inputs (integers over 8: every d2 is exact in float32) must match exactly; Gaussian inputs within the bounds derived in DESIGN.md
("Set-level fidelity"), which fidelity_ref states: TOL(D) = 2 (D + 2) u relative for an order statistic, ((D + 3) / e + 4) u
absolute for a mean kernel value, (D + 3) u relative for the distance sum.  The cases are generated once and shared
(fidelity_ref.gpu_cases)."""
import math

import numpy as np
import pytest
import torch

from tests import fidelity_ref as R
from tests import stream_harness as sh
from tests.stream_harness import Bufs, Case

pytestmark = pytest.mark.gpu

CASE_KEYS = list(R.gpu_cases())                 # (kind, D, n, m)
LATTICE = [k for k in CASE_KEYS if k[0] == "lattice"]
GAUSSIAN = [k for k in CASE_KEYS if k[0] == "gaussian"]
SPLITS = (1, 2, 5, 64)
# device against reference on the two pairs of fidelity_ref.frechet_cases(), relative, as measured on an MI355X (1.220e-08 and
# 5.406e-09; DESIGN.md, "Set-level fidelity"; tools/diag/gpu_fidelity_cost.py measures it again); the gate is 8 times that and
# never above 1e-4
FRECHET_MEASURED = 1.22e-8
FRECHET_GATE = min(8 * FRECHET_MEASURED, 1e-4)


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from torch_vae_amd import _lib
    return _lib.lib()


def ok(rc, what):
    assert rc == 0, (what, lib().vae_last_error().decode())


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def knn(x, k, splits=0, out=None):
    n, D = x.shape
    out = torch.full((n,), -7.0, device="cuda") if out is None else out
    ok(lib().vae_fidelity_knn_radii(x.data_ptr(), n, D, k, splits, out.data_ptr(), st()), "vae_fidelity_knn_radii")
    return out


def balls(q, r, rad=None, exclude=0, splits=0, outs=None):
    m, n, D = q.shape[0], r.shape[0], q.shape[1]
    if outs is None:
        outs = (torch.full((m,), -7, dtype=torch.int32, device="cuda") if rad is not None else None,
                torch.full((m,), -7, dtype=torch.int32, device="cuda"), torch.full((m,), -7.0, device="cuda"))
    counts, nearest, nd2 = outs
    ok(lib().vae_fidelity_balls(q.data_ptr(), m, r.data_ptr(), n, D, 0 if rad is None else rad.data_ptr(), exclude, splits,
                                0 if counts is None else counts.data_ptr(), nearest.data_ptr(), nd2.data_ptr(), st()), "vae_fidelity_balls")
    return outs


def sums(a, b, gammas, exclude=0, splits=0, out=None):
    G = 0 if gammas is None else gammas.shape[0]
    out = torch.full((G + 1,), -7.0, dtype=torch.float64, device="cuda") if out is None else out
    ok(lib().vae_fidelity_kernel_sums(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], gammas.data_ptr() if G else 0, G, exclude,
                                      splits, out.data_ptr(), st()), "vae_fidelity_kernel_sums")
    return out


def within(got, want, rel, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err[(got == want)] = 0.0
    print(f"{what}: worst relative error {err.max():.3e}, bound {rel:.3e}")
    assert (err <= rel).all(), (what, float(err.max()), rel)


# ---- lattice inputs: exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", LATTICE, ids=str)
def test_lattice_is_exact(key):
    c = R.gpu_cases()[key]
    a, b = dev(c["a"]), dev(c["b"])
    for k in R.KS:
        if k < c["n"]:
            got = host(knn(a, k))
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), c["radii"][k]), (k, "radii2")
        counts, near, nd2 = balls(a, b, dev(c["ball_radii"][k]))
        assert np.array_equal(host(counts), c["counts"][k]), (k, "counts")
        assert np.array_equal(host(near), c["nearest"][0]) and np.array_equal(host(nd2).astype(np.float64), c["nearest"][1]), (k, "nearest")
        if k in c["self_counts"]:
            counts, near, nd2 = balls(a, a, dev(c["radii"][k], torch.float32), exclude=1)
            assert np.array_equal(host(counts), c["self_counts"][k]), (k, "counts without the diagonal")
            assert np.array_equal(host(near), c["nearest_self"][0]) and np.array_equal(host(nd2).astype(np.float64), c["nearest_self"][1])
    _, near, nd2 = balls(a, b)                                   # without radii: no counts, the same nearest
    assert np.array_equal(host(near), c["nearest"][0]) and np.array_equal(host(nd2).astype(np.float64), c["nearest"][1])


# ---- Gaussian inputs: within the bounds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", GAUSSIAN, ids=str)
def test_gaussian_within_bounds(key):
    c = R.gpu_cases()[key]
    D, t = c["D"], R.tol(c["D"])
    a, b = dev(c["a"]), dev(c["b"])
    for k in R.KS:
        if k < c["n"]:
            within(host(knn(a, k)), c["radii"][k], t, f"radii2 k={k}")
        rb = c["ball_radii"][k].astype(np.float64)
        counts, near, nd2 = balls(a, b, dev(c["ball_radii"][k]))
        lo, hi = R.counts(c["ab"], rb, scale=1 - t, strict=True), R.counts(c["ab"], rb, scale=1 + t)
        got = host(counts)
        assert ((lo <= got) & (got <= hi)).all(), (k, "counts")
        if R.undecided(c, k) == 0:
            assert np.array_equal(got, c["counts"][k])
        idx, best, second = c["nearest"]
        within(host(nd2), best, t, f"nearest_d2 k={k}")
        clear = (second - best) > t * second
        assert np.array_equal(host(near)[clear], idx[clear])
        if k in c["self_counts"]:
            ra = R._f32(c["radii"][k]).astype(np.float64)
            counts, near, nd2 = balls(a, a, dev(c["radii"][k], torch.float32), exclude=1)
            lo, hi = R.counts(c["aa"], ra, True, 1 - t, True), R.counts(c["aa"], ra, True, 1 + t)
            assert ((lo <= host(counts)) & (host(counts) <= hi)).all()
            idx, best, second = c["nearest_self"]
            within(host(nd2), best, t, "nearest_d2 without the diagonal")
            clear = (second - best) > t * second
            assert np.array_equal(host(near)[clear], idx[clear])


@pytest.mark.parametrize("key", CASE_KEYS, ids=str)
def test_kernel_sums_within_bounds(key):
    c = R.gpu_cases()[key]
    D, n, m = c["D"], c["n"], c["m"]
    a, b = dev(c["a"]), dev(c["b"])
    g = dev(np.array(c["gammas"]))
    for name, other, rows, exclude in (("sums", b, m, 0), ("sums_self", a, n, 1)):
        pairs = R.pairs(n, rows, exclude)
        if pairs == 0:
            continue
        want = c[name]
        got = host(sums(a, other, g, exclude))
        err = np.abs(got[:8] - want[:8]) / pairs
        print(f"{name}: worst mean kernel error {err.max():.3e}, bound {R.kernel_bound(D):.3e}")
        assert (err <= R.kernel_bound(D)).all(), (name, err.max())
        within(got[8:], want[8:], R.dist_sum_bound(D), name + " distances")
        few = host(sums(a, other, g[:5], exclude))                 # G = 5 and G = 0 read the same pairs
        assert (np.abs(few[:5] - want[:5]) / pairs <= R.kernel_bound(D)).all() and few[5] == got[8]
        assert host(sums(a, other, None, exclude))[0] == got[8]
        if key[0] == "lattice":
            assert got[8] == want[8]                                # the distances are exact, and so is their f64 sum


# ---- one distance function behind the three entry points ------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.DIMS)
def test_every_point_is_in_k_plus_one_balls(D):
    """counts[i] over q = r = A with A's own radii: point j's ball holds j and its k nearest, so the counts add up to n (k + 1) -
    exactly, if d2 has the same bits in vae_fidelity_knn_radii and vae_fidelity_balls and d2(a, b) == d2(b, a)."""
    x = dev(R.consistency_set(D))
    n = x.shape[0]
    for k in R.KS:
        counts, near, nd2 = balls(x, x, knn(x, k))
        assert int(counts.sum()) == n * (k + 1), (D, k)
        assert np.array_equal(host(near), np.arange(n)) and not host(nd2).any()      # everybody's nearest is itself, at 0


# ---- splits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in CASE_KEYS if k[2] == 193 and k[1] in (3, 67, 128)], ids=str)
def test_splits_change_no_bit_of_the_order_statistics(key):
    c = R.gpu_cases()[key]
    a, b = dev(c["a"]), dev(c["b"])
    g, rb = dev(np.array(c["gammas"])), dev(c["ball_radii"][3])
    first = None
    for s in SPLITS:
        got = dict(radii=knn(a, 3, s), sums=sums(a, b, g, 0, s), sums_self=sums(a, a, g, 1, s))
        got["counts"], got["nearest"], got["nearest_d2"] = balls(a, b, rb, 0, s)
        got["self_counts"], got["self_nearest"], got["self_d2"] = balls(a, a, knn(a, 3, s), 1, s)
        again = dict(radii=knn(a, 3, s), sums=sums(a, b, g, 0, s), sums_self=sums(a, a, g, 1, s))
        again["counts"], again["nearest"], again["nearest_d2"] = balls(a, b, rb, 0, s)
        for name in again:
            assert sh.same_bits(got[name], again[name]), (s, name, "two calls differ")
        if first is None:
            first = got
            continue
        for name in got:
            if name.startswith("sums"):
                within(host(got[name]), host(first[name]), 1e-12, f"{name} splits={s}")
            else:
                assert sh.same_bits(got[name], first[name]), (s, name)
    auto = knn(a, 3, 0)
    assert sh.same_bits(auto, first["radii"])


# ---- special values, and nothing outside the outputs ----------------------------------------------------------------------------------------
def guarded(n, dtype, pattern):
    guard = 64
    buf = torch.full((guard + n + guard,), pattern, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n], guard


def untouched(buf, n, guard, pattern):
    got = host(buf)
    return (got[:guard] == pattern).all() and (got[guard + n:] == pattern).all()


@pytest.mark.parametrize("D,splits", [(5, 1), (5, 5), (67, 2), (128, 0)])
def test_special_values_and_guards(D, splits):
    rng = np.random.default_rng(9 + D)
    n, k = 70, 3
    x = rng.standard_normal((n, D)).astype(np.float32)
    x[7] = np.nan
    x[11, D // 2] = np.inf
    # the inputs sit inside NaN: a read past either end would surface in the results
    xin = torch.full((64 + n * D + 64,), float("nan"), device="cuda")
    xin[64:64 + n * D] = dev(x).reshape(-1)
    xd = xin[64:64 + n * D].view(n, D)
    want_r = R.radii(x, k)
    assert np.isinf(want_r[7]) and np.isinf(want_r[11]) and np.isfinite(np.delete(want_r, [7, 11])).all()
    rbuf, rview, guard = guarded(n, torch.float32, -7.0)
    knn(xd, k, splits, rview)
    got_r = host(rview)
    assert untouched(rbuf, n, guard, -7.0)
    assert np.array_equal(np.isinf(got_r), np.isinf(want_r)) and (got_r[np.isinf(got_r)] > 0).all()
    fin = np.isfinite(want_r)
    within(got_r[fin], want_r[fin], R.tol(D), "radii2 beside a NaN row and an inf coordinate")
    # balls over the same set, the diagonal left out; the radii are the reference's (+inf for rows 7 and 11)
    rad = R._f32(want_r)
    dist = R.d2(x, x)
    cbuf, cview, _ = guarded(n, torch.int32, 0x5A5A5A5A)
    ibuf, iview, _ = guarded(n, torch.int32, 0x5A5A5A5A)
    dbuf, dview, _ = guarded(n, torch.float32, -7.0)
    balls(xd, xd, dev(rad), 1, splits, (cview, iview, dview))
    assert untouched(cbuf, n, guard, 0x5A5A5A5A) and untouched(ibuf, n, guard, 0x5A5A5A5A) and untouched(dbuf, n, guard, -7.0)
    t = R.tol(D)
    lo, hi = R.counts(dist, rad.astype(np.float64), True, 1 - t, True), R.counts(dist, rad.astype(np.float64), True, 1 + t)
    got_c = host(cview)
    assert ((lo <= got_c) & (got_c <= hi)).all()
    assert got_c[7] == 0                                   # a NaN distance is in no ball
    assert got_c[0] >= 1                                   # +inf <= +inf: every finite point is in the ball of row 11
    idx, best, second = R.nearest(dist, exclude=True)
    got_i, got_d = host(iview), host(dview)
    assert got_i[7] == -1 and got_i[11] == -1 and np.isposinf(got_d[7]) and np.isposinf(got_d[11])
    assert (idx[[7, 11]] == -1).all()
    rest = np.isfinite(best)
    within(got_d[rest], best[rest], t, "nearest_d2")
    with np.errstate(invalid="ignore"):
        clear = rest & ((second - best) > t * second)
    assert np.array_equal(got_i[clear], idx[clear])
    # sums: +inf distances vanish from the kernel sums and make the distance sum +inf; a NaN row makes everything NaN
    g = dev(np.array([0.5 / D, 2.0 / D]))
    sbuf, sview, _ = guarded(3, torch.float64, -7.0)
    y = np.delete(x, 7, axis=0)
    sums(dev(y), dev(y), g, 1, splits, sview)
    assert untouched(sbuf, 3, guard, -7.0)
    want = R.kernel_sums(R.d2(y, y), [0.5 / D, 2.0 / D], True)
    got = host(sview)
    assert (np.abs(got[:2] - want[:2]) / R.pairs(n - 1, n - 1, True) <= R.kernel_bound(D)).all() and np.isposinf(got[2]) and np.isposinf(want[2])
    assert np.isnan(host(sums(xd, xd, g, 1, splits))).all()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
PKEY = ("gaussian", 16, 193, 131)


def test_wrappers_match_the_entry_points():
    from torch_vae_amd import fidelity as F
    c = R.gpu_cases()[PKEY]
    a, b = dev(c["a"]), dev(c["b"])
    assert sh.same_bits(F.knn_radii(a, 3), knn(a, 3)) and sh.same_bits(F.knn_radii(a, 3, splits=5), knn(a, 3))
    rb = dev(c["ball_radii"][3])
    for got, want in zip(F.ball_membership(a, b, rb), balls(a, b, rb)):
        assert sh.same_bits(got, want)
    counts, near, nd2 = F.ball_membership(a, a, exclude_self=True)
    assert counts is None and np.array_equal(host(near), c["nearest_self"][0])
    g = dev(np.array(c["gammas"]))
    assert sh.same_bits(F.kernel_sums(a, b, g), sums(a, b, g)) and sh.same_bits(F.kernel_sums(a, b, c["gammas"]), sums(a, b, g))
    assert sh.same_bits(F.kernel_sums(a, a, None, True), sums(a, a, None, 1))
    # a non-contiguous view is made contiguous, not misread
    wide = torch.cat([a, a], dim=1)
    assert sh.same_bits(F.knn_radii(wide[:, :16], 3), knn(a, 3))


def test_mmd2_and_precision_recall_against_the_reference():
    from torch_vae_amd import fidelity as F
    c = R.gpu_cases()[PKEY]
    D, n, m = PKEY[1:]
    a, b = dev(c["a"]), dev(c["b"])
    values, mean = F.mmd2(a, b)
    assert values.dtype == torch.float64 and values.is_cuda and tuple(values.shape) == (5,) and mean.is_cuda
    want = R.mmd2(c["a"], c["b"])
    # three means of kernel values, each within the kernel bound (the cross term counts twice); the default gammas come from the
    # device's own distance sum, (D + 3) u relative off, which moves a kernel value by at most that times t e^-t <= 1 / e
    bound = 4 * (R.kernel_bound(D) + R.dist_sum_bound(D) / math.e)
    err = np.abs(host(values) - want)
    print(f"mmd2 {host(values)}, reference {want}, worst error {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all() and abs(float(mean) - want.mean()) <= bound
    fixed, _ = F.mmd2(a, b, bandwidths=[0.02, 0.1])
    assert (np.abs(host(fixed) - R.mmd2(c["a"], c["b"], [0.02, 0.1])) <= 4 * R.kernel_bound(D)).all()
    for k in (1, 5):
        # exact where no pair sits within TOL of a boundary: checked for this case in tests/test_fidelity_host.py
        got, ref = F.precision_recall(a, b, k), R.prdc(c["a"], c["b"], k)
        for name in ("precision", "recall", "density", "coverage"):
            assert got[name].dtype == torch.float64 and got[name].is_cuda and got[name].dim() == 0
            assert abs(float(got[name]) - ref[name]) <= 1e-15, (k, name, float(got[name]), ref[name])


def test_a_set_against_itself():
    from torch_vae_amd import fidelity as F
    a = dev(R.consistency_set(16))
    r = F.compare_encodings(a, a, k=3)
    assert r["precision"] == r["recall"] == r["coverage"] == 1.0 and r["real"] == r["fake"] == R.CONSISTENCY_N
    # every ball holds its centre and the centre's 3 nearest (this set has no tie at a boundary): n (k + 1) memberships over k n
    assert r["density"] == pytest.approx(4 / 3, abs=1e-15)
    bound = 4 * R.kernel_bound(16)
    assert all(v <= bound for v in r["mmd2_per_bandwidth"]) and r["mmd2"] < 0        # the unbiased estimator of identical sets
    assert len(r["gammas"]) == 5 and abs(r["frechet"]) <= 1e-9
    assert all(isinstance(v, float) for k, v in r.items() if k not in ("mmd2_per_bandwidth", "gammas", "real", "fake"))


def test_compare_encodings_is_the_sum_of_its_parts():
    from torch_vae_amd import fidelity as F
    c = R.gpu_cases()[PKEY]
    a, b = dev(c["a"]), dev(c["b"])
    r = F.compare_encodings(a, b, k=3)
    prdc = F.precision_recall(a, b, 3)
    for name in prdc:
        assert r[name] == float(prdc[name])
    values, mean = F.mmd2(a, b)
    assert r["mmd2_per_bandwidth"] == host(values).tolist() and r["mmd2"] == pytest.approx(float(mean), rel=1e-12)
    assert r["frechet"] == F.frechet_distance(a, b)


def test_moments_against_float64():
    """the gates of tests/test_mixture_gpu.py::test_mstep: |dm_d| <= 1e-6 sqrt(S_dd + m_d^2), |dS_ij| <= 5e-6 sqrt(S_ii S_jj), S symmetric"""
    from torch_vae_amd import fidelity as F
    for x in R.frechet_cases()[0]:
        mean, cov = (host(t) for t in F._moments(dev(x)))
        want_m, want_c = R.moments(x)
        var = np.diag(want_c)
        e_m = (np.abs(mean - want_m) / np.sqrt(var + want_m ** 2)).max()
        e_S = (np.abs(cov - want_c) / np.sqrt(var[:, None] * var[None, :])).max()
        print(f"mean {e_m:.2e} (1e-6)  cov {e_S:.2e} (5e-6)")
        assert e_m <= 1e-6 and e_S <= 5e-6 and np.array_equal(cov, cov.T)


@pytest.mark.parametrize("which", [0, 1])
def test_frechet_distance(which):
    from torch_vae_amd import fidelity as F
    x, y = R.frechet_cases()[which]
    for s in (x, y):
        w = np.linalg.eigvalsh(R.moments(s)[1])
        assert 0.15 < w.min() and w.max() < 6.0                      # the sample covariances of eigenvalues drawn in [0.25, 4]
    got, want = F.frechet_distance(dev(x), dev(y)), R.frechet_distance(x, y)
    err = abs(got - want) / want
    print(f"frechet {got!r}, reference {want!r}, relative error {err:.3e}, gate {FRECHET_GATE:.3e}")
    assert want > 1.0 and err <= FRECHET_GATE
    assert abs(F.frechet_distance(dev(x), dev(x))) <= 1e-9 * np.trace(R.moments(x)[1])


def test_sample_fidelity_smoke():
    from tests.util import make_model, perturbed_params
    from torch_vae_amd.data import DevicePianorollLoader, PianorollDataset
    from torch_vae_amd.fidelity import sample_fidelity
    from torch_vae_amd.mixture import LatentMixture, encode_dataset
    model = make_model(64, 16, True, "f32", perturbed_params(16, 64, 31, True))
    rng = np.random.default_rng(41)
    cells = (rng.random((64, 64, 64)) < 0.06).astype(np.float32)
    ds = PianorollDataset(torch.from_numpy(cells), storage="bits")
    mu, _ = encode_dataset(model, DevicePianorollLoader(ds, 64, train=False))
    mix = LatentMixture.fit(mu, 2, covariance="diag", iters=3)
    for prior in (None, mix):
        r = sample_fidelity(model, ds, 32, prior=prior, seed=5, batch_size=48)
        assert r["real"] == 64 and r["fake"] == 32
        for name in ("precision", "recall", "coverage"):
            assert 0.0 <= r[name] <= 1.0, (name, r[name])
        for name in ("density", "mmd2", "frechet"):
            assert math.isfinite(r[name]), (name, r[name])
        assert r["density"] >= 0.0 and all(math.isfinite(v) for v in r["mmd2_per_bandwidth"] + r["gammas"])
        assert sample_fidelity(model, ds, 32, prior=prior, seed=5, batch_size=48) == r
    assert sample_fidelity(model, ds, 32, seed=5, max_rolls=40, k=3)["real"] == 40


# ---- the stream contract (include/vae_step.h, first paragraph) on the new entry points -----------------------------------------------------
SKEY = ("gaussian", 67, 193, 131)


def _make_knn():
    b = Bufs()
    b.inp("x", torch.from_numpy(R.gpu_cases()[SKEY]["a"]))
    b.outp("radii", 193)
    b.outp("radii_split", 193)
    return b


def _knn(b):
    ok(lib().vae_fidelity_knn_radii(b["x"].data_ptr(), 193, 67, 3, 0, b["radii"].data_ptr(), st()), "vae_fidelity_knn_radii")
    ok(lib().vae_fidelity_knn_radii(b["x"].data_ptr(), 193, 67, 8, 5, b["radii_split"].data_ptr(), st()), "vae_fidelity_knn_radii")


def _make_balls():
    c = R.gpu_cases()[SKEY]
    b = Bufs()
    b.inp("q", torch.from_numpy(c["a"]))
    b.inp("r", torch.from_numpy(c["b"]))
    b.inp("radii", torch.from_numpy(c["ball_radii"][3]))
    for tag in ("", "_split"):
        b.outp("counts" + tag, 193, dtype=torch.int32)
        b.outp("nearest" + tag, 193, dtype=torch.int32)
        b.outp("nearest_d2" + tag, 193)
    return b


def _balls(b):
    for tag, splits in (("", 1), ("_split", 5)):
        ok(lib().vae_fidelity_balls(b["q"].data_ptr(), 193, b["r"].data_ptr(), 131, 67, b["radii"].data_ptr(), 0, splits,
                                    b["counts" + tag].data_ptr(), b["nearest" + tag].data_ptr(), b["nearest_d2" + tag].data_ptr(), st()),
           "vae_fidelity_balls")


def _make_sums():
    c = R.gpu_cases()[SKEY]
    b = Bufs()
    b.inp("a", torch.from_numpy(c["a"]))
    b.inp("b", torch.from_numpy(c["b"]))
    b.inp("gammas", torch.from_numpy(np.array(c["gammas"])))
    b.outp("sums", 9, dtype=torch.float64)
    b.outp("sums_self", 9, dtype=torch.float64)
    return b


def _sums(b):
    ok(lib().vae_fidelity_kernel_sums(b["a"].data_ptr(), 193, b["b"].data_ptr(), 131, 67, b["gammas"].data_ptr(), 8, 0, 0, b["sums"].data_ptr(),
                                      st()), "vae_fidelity_kernel_sums")
    ok(lib().vae_fidelity_kernel_sums(b["a"].data_ptr(), 193, b["a"].data_ptr(), 193, 67, b["gammas"].data_ptr(), 8, 1, 5,
                                      b["sums_self"].data_ptr(), st()), "vae_fidelity_kernel_sums")


STREAM_CASES = [
    Case("fidelity_knn_radii", ("vae_fidelity_knn_radii",), _make_knn, _knn),
    Case("fidelity_balls", ("vae_fidelity_balls",), _make_balls, _balls),
    Case("fidelity_kernel_sums", ("vae_fidelity_kernel_sums",), _make_sums, _sums),
]


def _make_python():
    c = R.gpu_cases()[SKEY]
    b = Bufs()
    b.inp("real", torch.from_numpy(c["a"]))
    b.inp("fake", torch.from_numpy(c["b"]))
    return b


def _python(b):
    from torch_vae_amd import fidelity as F
    b.out["radii"] = F.knn_radii(b["real"], 5)
    b.out["counts"], b.out["nearest"], b.out["nearest_d2"] = F.ball_membership(b["fake"], b["real"], b.out["radii"])
    b.out["distance_sum"] = F.kernel_sums(b["real"], b["fake"], None)
    b.out["mmd2"], b.out["mmd2_mean"] = F.mmd2(b["real"], b["fake"])
    for name, v in F.precision_recall(b["real"], b["fake"], 5).items():
        b.out[name] = v
    b.out["mean"], b.out["covariance"] = F._moments(b["real"])


PY_STREAM_CASES = [
    Case("python/fidelity", ("vae_fidelity_knn_radii", "vae_fidelity_balls", "vae_fidelity_kernel_sums", "vae_mixture_mstep"), _make_python,
         _python, warmups=2),
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_stream_contract(case):
    sh.check_case(case)


@pytest.mark.parametrize("case", PY_STREAM_CASES, ids=repr)
def test_stream_contract_python_layer(case):
    sh.check_case(case)
