"""Importance-weighted log-likelihood and per-sample ELBO (VanillaVAE.log_likelihood, vae_log_likelihood): the numpy
restatement of the f64 combine that tests/test_loglik_gpu.py scores the kernels with, checked here against torch, and the
host-side argument handling (no GPU needed)."""
import inspect
import math

import numpy as np
import pytest
import torch

LOG_PI = math.log(math.pi)


def combine_reference(lpx, lat, mu, lv):
    """lpx, lat [K, B]: log p(x|z_k) and log p(z_k) - log q(z_k|x); mu, lv [B, L].  Returns (log_w [K,B], log p(x) [B],
    elbo [B]) in f64: max-shifted logsumexp over k minus log K, and mean_k log p(x|z_k) minus the analytic KL."""
    lpx = np.asarray(lpx, np.float64)
    log_w = lpx + np.asarray(lat, np.float64)
    K = log_w.shape[0]
    mx = log_w.max(axis=0)
    ll = mx + np.log(np.exp(log_w - mx).sum(axis=0)) - math.log(K)
    mu, lv = np.asarray(mu, np.float64), np.asarray(lv, np.float64)
    kl = -0.5 * (1.0 + lv - mu * mu - np.exp(lv)).sum(axis=1)
    return log_w, ll, lpx.mean(axis=0) - kl


def latent_terms(eps, mu, lv):
    """z = eps * exp(lv/2) + mu and log p(z) - log q(z|x) = sum_l (-z^2/2 + eps^2/2 + lv/2) (the 2 pi terms cancel).
    eps [K, B, L]; mu, lv [B, L]; f64."""
    eps, mu, lv = (np.asarray(a, np.float64) for a in (eps, mu, lv))
    z = eps * np.exp(0.5 * lv) + mu
    return z, (-0.5 * z * z + 0.5 * eps * eps + 0.5 * lv).sum(axis=-1)


def _torch_reference(log_w):
    t = torch.from_numpy(log_w)
    return (torch.logsumexp(t, dim=0) - math.log(t.shape[0])).numpy()


@pytest.mark.parametrize("case", ["random", "large_negative", "k1", "ties", "spread"])
def test_combine_matches_torch_logsumexp(case):
    rng = np.random.default_rng(3)
    K, B, L = 7, 5, 4
    lpx = -1000.0 + 30.0 * rng.standard_normal((K, B))
    lat = rng.standard_normal((K, B))
    if case == "large_negative":
        lpx = lpx - 1e6              # exp() of the unshifted weights underflows to 0: the shift must carry it
    elif case == "k1":
        lpx, lat = lpx[:1], lat[:1]
    elif case == "ties":
        lpx[:] = lpx[0]
        lat[:] = lat[0]
    elif case == "spread":
        lpx[0] += 800.0              # one draw dominates by far
    mu, lv = 0.3 * rng.standard_normal((B, L)), 0.2 * rng.standard_normal((B, L))
    log_w, ll, elbo = combine_reference(lpx, lat, mu, lv)
    np.testing.assert_allclose(ll, _torch_reference(log_w), rtol=1e-14, atol=0)
    assert np.all(np.isfinite(ll))
    if case == "k1":
        np.testing.assert_array_equal(ll, log_w[0])
    if case == "ties":
        np.testing.assert_allclose(ll, log_w[0], rtol=1e-15)
    assert np.all(ll >= log_w.mean(axis=0) - 1e-9 * np.abs(log_w.mean(axis=0)))   # Jensen: IWAE bound >= mean log-weight
    kl = 0.5 * (mu ** 2 + np.exp(lv) - 1 - lv).sum(axis=1)
    np.testing.assert_allclose(elbo, lpx.mean(axis=0) - kl, rtol=1e-14)


def test_latent_terms_are_log_prior_minus_log_posterior():
    rng = np.random.default_rng(4)
    K, B, L = 3, 2, 6
    eps, mu, lv = rng.standard_normal((K, B, L)), rng.standard_normal((B, L)), 0.5 * rng.standard_normal((B, L))
    z, lat = latent_terms(eps, mu, lv)
    sd = torch.from_numpy(np.exp(0.5 * lv))
    prior = torch.distributions.Normal(0.0, 1.0).log_prob(torch.from_numpy(z)).sum(-1)
    post = torch.distributions.Normal(torch.from_numpy(mu), sd).log_prob(torch.from_numpy(z)).sum(-1)
    np.testing.assert_allclose(lat, (prior - post).numpy(), rtol=1e-12, atol=1e-12)


def test_gaussian_likelihood_constant():
    """MSE: log p(x|z) = -sum (xhat - t)^2 - (H*W/2) log(pi) is the Gaussian log-density with variance 1/2."""
    rng = np.random.default_rng(5)
    xh, t = rng.uniform(size=64), rng.uniform(size=64)
    want = torch.distributions.Normal(torch.from_numpy(xh), math.sqrt(0.5)).log_prob(torch.from_numpy(t)).sum().item()
    np.testing.assert_allclose(-((xh - t) ** 2).sum() - 64 / 2 * LOG_PI, want, rtol=1e-13)


def test_argument_validation_without_gpu():
    from torch_vae_amd.models import VanillaVAE
    m = VanillaVAE(1, 16, 32, compute_dtype="f32")
    x = torch.zeros(3, 1, 32, 32)
    with pytest.raises(ValueError):
        m.log_likelihood(x, 0)
    with pytest.raises(ValueError):
        m.log_likelihood(x, 4, chunk=0)
    with pytest.raises(ValueError):
        m.log_likelihood(x, 4, eps=torch.zeros(4, 3, 15))
    with pytest.raises(ValueError):
        m.log_likelihood(x, 4, eps=torch.zeros(3, 4, 16))
    with pytest.raises(RuntimeError):        # valid arguments: the model is not on a HIP device (there is no CPU path)
        m.log_likelihood(x, 4)


def test_evaluate_signature_and_output_type():
    from torch_vae_amd import evaluation, types_helpers
    sig = inspect.signature(evaluation.evaluate)
    p = sig.parameters["nll_samples"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0
    assert list(sig.parameters)[:5] == ["dataloader", "model", "device", "partition_name", "verbosity"]
    assert set(types_helpers.LikelihoodOutput.__annotations__) == {"log_likelihood", "elbo", "log_weights"}


def test_library_exports_the_entry_point():
    from torch_vae_amd import _lib
    assert "vae_log_likelihood" in _lib.EXPORTS
