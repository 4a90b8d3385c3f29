"""Latent diagnostics (evaluation.latent_statistics, vae_latent_stats): the numpy f64 restatement of the definitions that
tests/test_latent_stats_gpu.py scores the kernels with, checked here against a brute-force torch.logsumexp, and the host-side
argument handling (no GPU needed)."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

LOG_2PI = math.log(2.0 * math.pi)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def form_z(eps, mu, lv):
    """z[s,i,d] = eps * exp(0.5 lv) + mu in f32 as the kernels form it: sd rounded to f32, then one fused multiply-add (the f64
    product of two f32 values is exact, the sum is rounded once more to f32).  eps [S,N,L]; mu, lv [N,L]."""
    eps, mu, lv = (np.asarray(a, np.float32) for a in (eps, mu, lv))
    sd = np.exp(np.float32(0.5) * lv)
    return (eps.astype(np.float64) * sd.astype(np.float64) + mu.astype(np.float64)).astype(np.float32)


def _lse(a, axis):
    m = a.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def latent_stats_reference(mu, lv, eps=None, z=None, chunk_elems=1 << 24):
    """The definitions in f64: mu, lv [N,L]; z [S,N,L] (or formed from eps with form_z).  Returns a dict with the keys of
    LatentStatsOutput (numpy, active_units at threshold 0.01) plus log_qz_prod [S,N]."""
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    N, L = mu.shape
    if z is None:
        z = form_z(eps, mu, lv)
    z = np.asarray(z, np.float64)
    S = z.shape[0]
    zq = z.reshape(S * N, L)
    iv, c = np.exp(-lv), -0.5 * (LOG_2PI + lv)
    log_qz = np.empty(S * N)
    log_qz_dims = np.empty((S * N, L))
    cq = max(1, chunk_elems // (N * L))
    for q0 in range(0, S * N, cq):
        a = c[None] - 0.5 * (zq[q0:q0 + cq, None, :] - mu[None]) ** 2 * iv[None]     # [cq, N, L]: log N(z_qd; mu_jd, sigma_jd^2)
        log_qz[q0:q0 + cq] = _lse(a.sum(-1), 1) - math.log(N)
        log_qz_dims[q0:q0 + cq] = _lse(a, 1) - math.log(N)
    log_qz_prod = log_qz_dims.sum(-1)
    kl_i = 0.5 * (mu * mu + np.exp(lv) - 1.0 - lv)
    negent = -0.5 * (LOG_2PI + 1.0 + lv).sum(-1)
    xent = -0.5 * (LOG_2PI + mu * mu + np.exp(lv)).sum(-1)
    var_mu = ((mu - mu.mean(0)) ** 2).mean(0)
    return dict(
        kl=kl_i.sum(-1).mean(), mi=negent.mean() - log_qz.mean(), tc=log_qz.mean() - log_qz_prod.mean(),
        dwkl=log_qz_prod.mean() - xent.mean(), kl_per_dim=kl_i.mean(0), var_mu=var_mu,
        dwkl_per_dim=log_qz_dims.mean(0) + (0.5 * (LOG_2PI + mu * mu + np.exp(lv))).mean(0),
        active_units=int((var_mu > 0.01).sum()), log_qz=log_qz.reshape(S, N), log_qz_dims=log_qz_dims.reshape(S, N, L),
        log_qz_prod=log_qz_prod.reshape(S, N))


def synthetic_posteriors(N, L, seed, kind="normal"):
    rng = np.random.default_rng(seed)
    if kind == "far":        # means 10^3 apart, sigma = e^-5: every component but the query's own underflows
        mu = 1000.0 * np.arange(N)[:, None] + rng.standard_normal((N, L))
        lv = np.full((N, L), -10.0)
    elif kind == "mixed":    # very broad and very narrow posteriors side by side
        # narrow means stay small: z is formed in f32 from an f32 sigma the host cannot round exactly as the device's expf
        # does, and one ulp of a mean of 3 is already 2e-4 sigma at sigma = e^-7
        narrow = rng.random((N, L)) < 0.5
        mu = np.where(narrow, 0.02 * rng.standard_normal((N, L)), 3.0 * rng.standard_normal((N, L)))
        lv = np.where(narrow, rng.uniform(-14.0, -10.0, (N, L)), rng.uniform(4.0, 6.0, (N, L)))
    else:
        mu = rng.standard_normal((N, L)) * rng.uniform(0.05, 2.0, L)
        lv = rng.uniform(-3.0, 1.0, (N, L))
    return mu.astype(np.float32), lv.astype(np.float32)


def _brute(mu, lv, z):
    """torch f64, the whole [S*N, N, L] tensor at once, torch.logsumexp."""
    mu, lv, z = (torch.from_numpy(np.asarray(a, np.float64)) for a in (mu, lv, z))
    N, L = mu.shape
    zq = z.reshape(-1, 1, L)
    a = -0.5 * (LOG_2PI + lv + (zq - mu) ** 2 * torch.exp(-lv))
    return (torch.logsumexp(a.sum(-1), 1) - math.log(N)).numpy(), (torch.logsumexp(a, 1) - math.log(N)).numpy()


@pytest.mark.parametrize("N,L,S,kind", [(1, 1, 1, "normal"), (7, 10, 3, "normal"), (33, 16, 2, "mixed"), (12, 5, 1, "far"),
                                        (50, 3, 1, "normal")])
def test_reference_matches_torch_logsumexp(N, L, S, kind):
    mu, lv = synthetic_posteriors(N, L, 3 + N, kind)
    eps = np.random.default_rng(N).standard_normal((S, N, L)).astype(np.float32)
    ref = latent_stats_reference(mu, lv, eps, chunk_elems=64)     # small chunks: the chunking itself is exercised
    lq, lqd = _brute(mu, lv, form_z(eps, mu, lv))
    np.testing.assert_allclose(ref["log_qz"].ravel(), lq, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(ref["log_qz_dims"].reshape(-1, L), lqd.reshape(-1, L), rtol=1e-12, atol=1e-9)
    assert np.isfinite(ref["log_qz"]).all() and np.isfinite(ref["log_qz_dims"]).all()


@pytest.mark.parametrize("kind", ["normal", "mixed", "far"])
def test_kl_decomposes_into_mi_tc_dwkl(kind):
    mu, lv = synthetic_posteriors(40, 6, 9, kind)
    eps = np.random.default_rng(1).standard_normal((2, 40, 6)).astype(np.float32)
    r = latent_stats_reference(mu, lv, eps)
    assert abs(r["kl"] - (r["mi"] + r["tc"] + r["dwkl"])) <= 1e-9 * max(1.0, abs(r["kl"]))
    assert abs(r["dwkl"] - r["dwkl_per_dim"].sum()) <= 1e-9 * max(1.0, abs(r["dwkl"]))
    assert abs(r["kl"] - r["kl_per_dim"].sum()) <= 1e-12 * max(1.0, abs(r["kl"]))


def test_far_apart_reference_is_own_term():
    """Every other component is thousands of sigma away: log q(z) is the query's own log-density minus log N."""
    N, L = 12, 5
    mu, lv = synthetic_posteriors(N, L, 2, "far")
    eps = np.random.default_rng(0).standard_normal((1, N, L)).astype(np.float32)
    z = form_z(eps, mu, lv).astype(np.float64)[0]
    mu64, lv64 = mu.astype(np.float64), lv.astype(np.float64)
    own = (-0.5 * (LOG_2PI + lv64 + (z - mu64) ** 2 * np.exp(-lv64)))
    r = latent_stats_reference(mu, lv, eps)
    np.testing.assert_allclose(r["log_qz"][0], own.sum(-1) - math.log(N), rtol=1e-12)
    np.testing.assert_allclose(r["log_qz_dims"][0], own - math.log(N), rtol=1e-12)


def test_collapsed_posteriors_have_no_active_units():
    mu, lv = np.zeros((9, 4), np.float32), np.zeros((9, 4), np.float32)
    r = latent_stats_reference(mu, lv, np.ones((1, 9, 4), np.float32))
    assert r["active_units"] == 0 and (r["kl_per_dim"] == 0).all() and (r["var_mu"] == 0).all()
    assert abs(r["mi"]) < 1e-12 and abs(r["tc"]) < 1e-12


# -- argument handling: raised before any library call, so no GPU is needed --------------------------------------------

def _cpu(N=5, L=3):
    return torch.zeros(N, L), torch.zeros(N, L)


def test_rejects_bad_shapes_and_dtypes():
    from torch_vae_amd.evaluation import latent_statistics
    mu, lv = _cpu()
    with pytest.raises(ValueError, match=r"\[N, L\]"):
        latent_statistics(mu.reshape(-1), lv.reshape(-1))
    with pytest.raises(ValueError, match=r"\[N, L\]"):
        latent_statistics(mu, torch.zeros(5, 4))
    with pytest.raises(ValueError, match="L <= 4096"):
        latent_statistics(torch.zeros(2, 4097), torch.zeros(2, 4097))
    with pytest.raises(ValueError, match="N >= 1"):
        latent_statistics(torch.zeros(0, 3), torch.zeros(0, 3))
    with pytest.raises(TypeError, match="float32"):
        latent_statistics(mu.double(), lv.double())


@pytest.mark.parametrize("draws", [0, -1, 1.5])
def test_rejects_bad_draws(draws):
    from torch_vae_amd.evaluation import latent_statistics
    with pytest.raises(ValueError, match="draws"):
        latent_statistics(*_cpu(), draws=draws)


def test_rejects_bad_eps():
    from torch_vae_amd.evaluation import latent_statistics
    mu, lv = _cpu()
    with pytest.raises(ValueError, match=r"eps must be \[2,5,3\]"):
        latent_statistics(mu, lv, draws=2, eps=torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match="eps must be"):
        latent_statistics(mu, lv, eps=torch.zeros(5, 3))
    with pytest.raises(TypeError, match="eps must be float32"):
        latent_statistics(mu, lv, eps=torch.zeros(1, 5, 3, dtype=torch.float64))


def test_rejects_host_tensors():
    from torch_vae_amd.evaluation import latent_statistics
    with pytest.raises(ValueError, match="GPU"):
        latent_statistics(*_cpu(), eps=torch.zeros(1, 5, 3))


def test_evaluate_signature_gains_latent_rolls():
    from torch_vae_amd.evaluation import evaluate
    p = inspect.signature(evaluate).parameters
    assert p["latent_rolls"].default == 0 and p["latent_rolls"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["nll_samples"].default == 0


def test_latent_statistics_signature_and_output_keys():
    from torch_vae_amd.evaluation import latent_statistics
    from torch_vae_amd.types_helpers import LatentStatsOutput
    p = inspect.signature(latent_statistics).parameters
    assert [k for k in p] == ["mu", "log_var", "draws", "eps", "seed", "active_threshold"]
    assert (p["draws"].default, p["eps"].default, p["seed"].default, p["active_threshold"].default) == (1, None, 0, 0.01)
    assert set(LatentStatsOutput.__annotations__) == {"kl", "mi", "tc", "dwkl", "active_units", "kl_per_dim", "var_mu",
                                                      "dwkl_per_dim", "log_qz", "log_qz_dims"}


def test_abi_declares_latent_stats():
    from torch_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vae_step.h")).read()
    assert "int vae_latent_stats(" in hdr and "vae_latent_stats" in _lib.EXPORTS
