"""Host side (no GPU) of the latent-mixture tests: the numpy reference (tests/mixture_ref.py) against direct numpy.linalg formulas,
the conditions the EM shapes must meet for the device comparison to mean something, the float32-emulation gaps the GPU gates are
built from, the refusals of include/vae_mixture.h through fake, never dereferenced pointers, the header / export bookkeeping and
the argument checks of torch_vae_amd.mixture."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mixture_ref as R
from tests import test_mixture_gpu as gpu_cases
from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_mixture.h")
P = 4096          # a fake device address, 16-byte aligned


# ---- the reference against numpy.linalg ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.SHAPES), ids=R.shape_id)
def test_reference_matches_linalg(shape):
    n, L, K, kind = shape
    c = R.case(shape)
    x, pi, m, S = c["x"].astype(np.float64), c["pi"], c["m"], c["S"]
    assert not c["status"].any()
    lp = np.empty((n, K))
    for k in range(K):
        Sk = np.diag(S[k]) if kind == "diag" else S[k]
        d = x - m[k]
        sign, logabs = np.linalg.slogdet(Sk)
        assert sign > 0
        lp[:, k] = np.log(pi[k]) - 0.5 * (L * R.LOG2PI + logabs + np.einsum("ni,ij,nj->n", d, np.linalg.inv(Sk), d))
        np.testing.assert_allclose(c["logdet"][k], -0.5 * logabs, rtol=1e-10, atol=1e-10)
        Ck = np.diag(c["C"][k]) if kind == "diag" else c["C"][k]
        np.testing.assert_allclose(Ck, np.linalg.cholesky(Sk), rtol=1e-10, atol=1e-10 * np.abs(Ck).max())
    mx = lp.max(1)
    want = mx + np.log(np.exp(lp - mx[:, None]).sum(1))
    np.testing.assert_allclose(c["log_prob"], want, rtol=1e-10)
    np.testing.assert_allclose(c["log_resp"], lp - want[:, None], rtol=1e-10, atol=1e-10)
    # one M-step from the exact responsibilities, against the textbook sums
    r = np.exp(c["log_resp"])
    pi2, m2, S2 = R.mstep(c["log_resp"], c["x"], R.REG, kind)
    N = r.sum(0)
    np.testing.assert_allclose(pi2, N / n, rtol=1e-10)
    np.testing.assert_allclose(m2, (r.T @ x) / N[:, None], rtol=1e-10, atol=1e-10)
    for k in range(K):
        d = x - m2[k]
        full = (r[:, k, None] * d).T @ d / N[k] + R.REG * np.eye(L)
        np.testing.assert_allclose(S2[k], np.diag(full) if kind == "diag" else full, rtol=1e-10, atol=1e-10 * np.abs(full).max())


def test_reference_sample_and_pick():
    pi = np.array([0.2, 0.5, 0.3])
    u = np.array([0.0, 0.19999, 0.2, 0.69, 0.7, 0.999999, 1.0])
    comp, cum = R.pick(pi, u)
    assert comp.tolist() == [0, 0, 1, 1, 2, 2, 2]          # the last component takes the remainder, u = 1.0 included
    c = R.case((257, 3, 2, "full"))
    rng = np.random.default_rng(3)
    u, eps = rng.random(50), rng.standard_normal((50, 3)).astype(np.float32)
    z, comp, _ = R.sample(c["pi"], c["m"], c["C"], "full", 0.7, u, eps)
    for i in range(50):
        np.testing.assert_allclose(z[i], c["m"][comp[i]] + 0.7 * np.linalg.cholesky(c["S"][comp[i]]) @ eps[i].astype(np.float64), rtol=1e-10)


@pytest.mark.parametrize("shape", R.EM_SHAPES, ids=R.shape_id)
def test_em_shapes_are_well_conditioned(shape):
    """The device EM is compared with the reference's trajectory; that only means something where the trajectory is stable: the mean
    log-likelihood never decreases and no component starves."""
    c = R.case(shape)
    steps = np.diff(c["hist"])
    print(R.shape_id(shape), "ll history", c["hist"], "min weight", c["min_weight"])
    assert (steps >= -1e-12 * np.abs(c["hist"][:-1])).all(), steps
    assert c["min_weight"] >= 0.04


@pytest.mark.parametrize("shape", list(R.SHAPES), ids=R.shape_id)
def test_emulation_gaps_are_the_recorded_ones(shape):
    """The gaps G between the reference's float32 emulation and its float64 run, printed, and held against the constants the GPU
    gates are built from (tests/test_mixture_gpu.py: GAPS, produced by `python -m tests.mixture_ref`)."""
    g, rec = R.case(shape)["gaps"], gpu_cases.GAPS[shape]
    print(R.shape_id(shape), {k: f"{v:.2e}" for k, v in g.items()})
    for k, v in g.items():
        # (a fresh measurement moves with the BLAS that numpy runs on; gaps at the 1e-12 level are rounding noise of the float64 run)
        assert v <= 1.5 * rec[k] + 1e-11 and rec[k] <= 1.5 * v + 1e-11, (k, v, rec[k])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def factor(L, cov=P, K=3, dim=16, kind=0, status=P):
    return L.vae_mixture_factor(cov, K, dim, kind, P, P, P, P, status, None)


def log_prob(L, x=P, n=100, dim=16, K=3, kind=0, mean=P):
    return L.vae_mixture_log_prob(x, n, dim, K, kind, P, P, P, P, P, None, mean, None)


def mstep(L, lr=P, n=100, dim=16, K=3, kind=0, reg=1e-6):
    return L.vae_mixture_mstep(lr, P, n, dim, K, kind, reg, P, P, P, None)


def sample(L, n=10, dim=16, K=3, kind=0, t=1.0, z=P):
    return L.vae_mixture_sample(n, dim, K, kind, P, P, P, t, 0, None, None, z, P, None)


def em(L, x=P, n=100, dim=16, K=3, kind=0, iters=2, reg=1e-6, hist=P):
    return L.vae_mixture_em(x, n, dim, K, kind, iters, reg, P, P, P, P, P, P, P, P, hist, None)


NULL_EM = "vae_mixture_em: null pointer (x, weights, means, covariances, chol, winv, winv32, logdet, status, ll_history)"
REFUSALS = {
    "factor/0_components": (lambda L: factor(L, K=0), "vae_mixture_factor: components must be in 1..64"),
    "factor/65_components": (lambda L: factor(L, K=65), "vae_mixture_factor: components must be in 1..64"),
    "factor/full_dim_129": (lambda L: factor(L, dim=129), "vae_mixture_factor: latent_dim must be in 1..128 for full covariances"),
    "factor/diag_dim_4097": (lambda L: factor(L, dim=4097, kind=1), "vae_mixture_factor: latent_dim must be in 1..4096 for diagonal covariances"),
    "factor/dim_0": (lambda L: factor(L, dim=0), "vae_mixture_factor: latent_dim must be in 1..128 for full covariances"),
    "factor/kind_2": (lambda L: factor(L, kind=2), "vae_mixture_factor: kind must be 0 (full) or 1 (diag)"),
    "factor/null_covariances": (lambda L: factor(L, cov=None), "vae_mixture_factor: null pointer (covariances, chol, winv, winv32, logdet, status)"),
    "factor/null_status": (lambda L: factor(L, status=None), "vae_mixture_factor: null pointer (covariances, chol, winv, winv32, logdet, status)"),
    "factor/status_plus_2": (lambda L: factor(L, status=P + 2), "vae_mixture_factor: f64 pointers must be 8-byte, winv32 and status 4-byte aligned"),
    "log_prob/0_components": (lambda L: log_prob(L, K=0), "vae_mixture_log_prob: components must be in 1..64"),
    "log_prob/65_components": (lambda L: log_prob(L, K=65), "vae_mixture_log_prob: components must be in 1..64"),
    "log_prob/full_dim_129": (lambda L: log_prob(L, dim=129), "vae_mixture_log_prob: latent_dim must be in 1..128 for full covariances"),
    "log_prob/n_below_components": (lambda L: log_prob(L, n=2), "vae_mixture_log_prob: n must be >= components"),
    "log_prob/n_above_2^30": (lambda L: log_prob(L, n=(1 << 30) + 1), "vae_mixture_log_prob: n must be <= 2^30"),
    "log_prob/kind_2": (lambda L: log_prob(L, kind=2), "vae_mixture_log_prob: kind must be 0 (full) or 1 (diag)"),
    "log_prob/null_x": (lambda L: log_prob(L, x=None), "vae_mixture_log_prob: null pointer (x, weights, means, winv32, logdet, log_prob, mean_log_prob)"),
    "log_prob/null_mean": (lambda L: log_prob(L, mean=None), "vae_mixture_log_prob: null pointer (x, weights, means, winv32, logdet, log_prob, mean_log_prob)"),
    "mstep/65_components": (lambda L: mstep(L, K=65), "vae_mixture_mstep: components must be in 1..64"),
    "mstep/full_dim_129": (lambda L: mstep(L, dim=129), "vae_mixture_mstep: latent_dim must be in 1..128 for full covariances"),
    "mstep/n_below_components": (lambda L: mstep(L, n=2), "vae_mixture_mstep: n must be >= components"),
    "mstep/kind_2": (lambda L: mstep(L, kind=2), "vae_mixture_mstep: kind must be 0 (full) or 1 (diag)"),
    "mstep/null_log_resp": (lambda L: mstep(L, lr=None), "vae_mixture_mstep: null pointer (log_resp, x, weights, means, covariances)"),
    "mstep/negative_reg_covar": (lambda L: mstep(L, reg=-1e-9), "vae_mixture_mstep: reg_covar must be finite and >= 0"),
    "mstep/nan_reg_covar": (lambda L: mstep(L, reg=float("nan")), "vae_mixture_mstep: reg_covar must be finite and >= 0"),
    "mstep/inf_reg_covar": (lambda L: mstep(L, reg=float("inf")), "vae_mixture_mstep: reg_covar must be finite and >= 0"),
    "sample/0_components": (lambda L: sample(L, K=0), "vae_mixture_sample: components must be in 1..64"),
    "sample/full_dim_129": (lambda L: sample(L, dim=129), "vae_mixture_sample: latent_dim must be in 1..128 for full covariances"),
    "sample/kind_2": (lambda L: sample(L, kind=2), "vae_mixture_sample: kind must be 0 (full) or 1 (diag)"),
    "sample/negative_n": (lambda L: sample(L, n=-1), "vae_mixture_sample: n must be in 0..2^30"),
    "sample/null_z": (lambda L: sample(L, z=None), "vae_mixture_sample: null pointer (weights, means, chol, z, component)"),
    "sample/nan_temperature": (lambda L: sample(L, t=float("nan")), "vae_mixture_sample: temperature must be finite"),
    "sample/inf_temperature": (lambda L: sample(L, t=float("-inf")), "vae_mixture_sample: temperature must be finite"),
    "em/0_components": (lambda L: em(L, K=0), "vae_mixture_em: components must be in 1..64"),
    "em/65_components": (lambda L: em(L, K=65), "vae_mixture_em: components must be in 1..64"),
    "em/full_dim_129": (lambda L: em(L, dim=129), "vae_mixture_em: latent_dim must be in 1..128 for full covariances"),
    "em/n_below_components": (lambda L: em(L, n=2), "vae_mixture_em: n must be >= components"),
    "em/kind_2": (lambda L: em(L, kind=2), "vae_mixture_em: kind must be 0 (full) or 1 (diag)"),
    "em/null_x": (lambda L: em(L, x=None), NULL_EM),
    "em/null_ll_history": (lambda L: em(L, hist=None), NULL_EM),
    "em/0_iters": (lambda L: em(L, iters=0), "vae_mixture_em: iters must be >= 1"),
    "em/negative_reg_covar": (lambda L: em(L, reg=-1.0), "vae_mixture_em: reg_covar must be finite and >= 0"),
    "em/nan_reg_covar": (lambda L: em(L, reg=float("nan")), "vae_mixture_em: reg_covar must be finite and >= 0"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = REFUSALS[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == want


# ---- the header, the exports and the stream-case table ------------------------------------------------------------------------------
def _header(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def test_header_declares_exactly_the_mixture_exports():
    declared = set(re.findall(r"\b(vae_[a-z0-9_]+)\s*\(", _header(HEADER)))
    assert declared == set(_lib.MIXTURE_EXPORTS) and len(_lib.MIXTURE_EXPORTS) == 5
    L = _lib.lib()
    assert not [n for n in _lib.MIXTURE_EXPORTS if not hasattr(L, n)]
    assert not set(_lib.MIXTURE_EXPORTS) & set(_lib.EXPORTS)
    assert L.vae_abi_version() == 1


def test_vae_step_h_declares_no_mixture_function():
    assert "vae_mixture_" not in _header(os.path.join(ROOT, "include", "vae_step.h"))


def stream_entry_points():
    found = [m.group(1) for m in re.finditer(r"\b(vae_\w+)\s*\(([^;{}]*?)\)\s*;", _header(HEADER)) if re.search(r"\bvae_stream_t\b", m.group(2))]
    assert len(found) == len(set(found))
    return found


def test_every_stream_entry_point_of_the_header_has_a_stream_case():
    """The rule of tests/test_streams_host.py on the new header and its own case table: every function of include/vae_mixture.h that
    takes a stream is called by a sync-free case of tests/test_mixture_gpu.py, and `covers` names calls the module really makes."""
    names = stream_entry_points()
    assert sorted(names) == sorted(_lib.MIXTURE_EXPORTS)
    covered = set()
    for c in gpu_cases.STREAM_CASES:
        assert c.sync_free and c.reads_back is None, c.name
        covered |= set(c.covers)
    assert not [n for n in names if n not in covered]
    assert not [n for n in covered if n not in names]
    called = {a or b for a, b in re.findall(r"lib\(\)\.(vae_\w+)\(|L_\.(vae_\w+)\(", inspect.getsource(gpu_cases))}
    for c in gpu_cases.STREAM_CASES:
        assert not [n for n in c.covers if n not in called], c.name
    all_names = [c.name for c in gpu_cases.STREAM_CASES + gpu_cases.PY_STREAM_CASES]
    assert len(set(all_names)) == len(all_names)
    for c in gpu_cases.PY_STREAM_CASES:
        assert c.reads_back is None or (not c.sync_free and len(c.reads_back.split()) >= 5), c.name


# ---- Python argument checks (all raised before anything touches a device) ------------------------------------------------------------
def test_python_argument_checks():
    from torch_vae_amd.mixture import LatentMixture, encode_dataset
    z = torch.zeros(20, 4)
    with pytest.raises(ValueError, match="must be on the GPU"):
        LatentMixture.fit(z, 2)
    with pytest.raises(TypeError, match="float32"):
        LatentMixture.fit(z.double(), 2)
    with pytest.raises(ValueError, match=r"\[n, latent_dim\]"):
        LatentMixture.fit(z[0], 2)
    with pytest.raises(TypeError, match="tensor"):
        LatentMixture.fit(z.numpy(), 2)
    with pytest.raises(TypeError, match="float64 tensor on the GPU"):
        LatentMixture(torch.ones(2, dtype=torch.float64) / 2, torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="'full' or 'diag'"):
        LatentMixture(None, None, None, "tied")
    with pytest.raises(ValueError, match="max_rolls"):
        encode_dataset(None, [], max_rolls=0)


def test_python_shape_checks():
    from torch_vae_amd import mixture
    for K, L, cov, word in ((0, 4, "full", "components"), (65, 4, "full", "components"), (2, 129, "full", "latent_dim"),
                            (2, 4097, "diag", "latent_dim"), (2, 0, "diag", "latent_dim"), (2, 4, "tied", "covariance")):
        with pytest.raises(ValueError, match=word):
            mixture._checked_shape(K, L, cov)
    mixture._checked_shape(64, 128, "full")
    mixture._checked_shape(1, 4096, "diag")
    for bad in (True, 1.5, -1, "3"):
        with pytest.raises(ValueError, match="integer"):
            mixture._integer(bad, "components", 0)
