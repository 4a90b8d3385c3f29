"""Latent diagnostics on the GPU (evaluation.latent_statistics, vae_latent_stats, evaluate(..., latent_rolls=R)) against the numpy
f64 restatement of the definitions in tests/test_latent_stats_host.py, which that file checks against torch.logsumexp."""
import math

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.test_latent_stats_host import form_z, latent_stats_reference, synthetic_posteriors
from tests.test_loglik_gpu import cpu_state, model_for, ref_encode

pytestmark = pytest.mark.gpu

# Per query: |log_qz - ref| <= Q_ATOL + Q_RTOL |ref| (likewise log_qz_prod and each log_qz_dims element).  The joint sum over d runs
# in f32 in the kernel (its magnitude grows with L), everything after the logsumexp in f64.
Q_ATOL, Q_RTOL = 1e-4, 1e-6
# The four scalars and the per-dimension arrays: 1e-4 nats, plus f64 rounding where they are differences of terms of order |ref|
# (means 10^3 apart make E log p(z) ~ 1e12 nats, one f64 ulp of which is 2e-4).
S_ATOL, S_RTOL = 1e-4, 1e-15


def _close(got, ref, atol, rtol, what, slack=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    worst = float((err / (atol + rtol * np.abs(ref) + slack)).max())
    print(f"{what}: max |d| {err.max():.3g}, max |d|/|ref| {float((err / np.maximum(np.abs(ref), 1e-30)).max()):.3g}, "
          f"worst / tolerance {worst:.3g}")
    assert worst <= 1.0, (what, float(err.max()), worst)


def _run(mu, lv, S, eps=None, seed=0):
    from torch_vae_amd.evaluation import latent_statistics
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    return latent_statistics(t(mu), t(lv), draws=S, eps=None if eps is None else t(eps), seed=seed)


def _compare(out, ref, tag, slack=None):
    sl = lambda k: 0.0 if slack is None else slack[k]
    _close(out["log_qz"].cpu(), ref["log_qz"], Q_ATOL, Q_RTOL, tag + " log_qz", sl("log_qz"))
    _close(out["log_qz_dims"].cpu(), ref["log_qz_dims"], Q_ATOL, Q_RTOL, tag + " log_qz_dims", sl("log_qz_dims"))
    _close(out["log_qz_dims"].sum(-1).cpu(), ref["log_qz_prod"], Q_ATOL, Q_RTOL, tag + " log_qz_prod", sl("log_qz_prod"))
    for k in ("kl_per_dim", "var_mu", "dwkl_per_dim"):
        _close(out[k].cpu(), ref[k], S_ATOL, S_RTOL, f"{tag} {k}", sl(k))
    for k in ("kl", "mi", "tc", "dwkl"):
        _close(float(out[k]), ref[k], S_ATOL, S_RTOL, f"{tag} {k}", sl(k))
    assert out["active_units"] == ref["active_units"]
    for k in ("kl", "mi", "tc", "dwkl", "kl_per_dim", "var_mu", "dwkl_per_dim", "log_qz", "log_qz_dims"):
        assert out[k].dtype == torch.float64, k
    s = out
    assert abs(float(s["kl"]) - float(s["mi"] + s["tc"] + s["dwkl"])) <= 1e-9 * max(1.0, abs(float(s["kl"])))


@pytest.mark.parametrize("N,L,S", [(1, 1, 1), (1, 128, 3), (7, 1, 3), (7, 10, 1), (7, 128, 3), (1000, 16, 3), (1000, 128, 1),
                                   (4099, 1, 3), (4099, 10, 1), (4099, 16, 1),
                                   # a partial second dimension tile of the dims kernel (65..127: tiles of 64), partial second and
                                   # later dimension stages of the joint kernel (> 128: stages of 128), the largest latent size
                                   (33, 65, 2), (130, 100, 1), (9, 129, 3), (70, 200, 1), (5, 4096, 2)])
def test_synthetic_explicit_eps(N, L, S):
    mu, lv = synthetic_posteriors(N, L, 100 + N + L)
    eps = np.random.default_rng(N * L + S).standard_normal((S, N, L)).astype(np.float32)
    _compare(_run(mu, lv, S, eps), latent_stats_reference(mu, lv, eps), f"N{N} L{L} S{S}")


@pytest.mark.parametrize("N,L", [(64, 16), (300, 128)])
def test_far_apart_posteriors(N, L):
    mu, lv = synthetic_posteriors(N, L, 5, "far")
    eps = np.random.default_rng(7).standard_normal((1, N, L)).astype(np.float32)
    out = _run(mu, lv, 1, eps)
    ref = latent_stats_reference(mu, lv, eps)
    _compare(out, ref, f"far N{N} L{L}")
    z = form_z(eps, mu, lv).astype(np.float64)[0]
    m64, l64 = mu.astype(np.float64), lv.astype(np.float64)
    own = (-0.5 * (math.log(2 * math.pi) + l64 + (z - m64) ** 2 * np.exp(-l64))).sum(-1) - math.log(N)
    _close(out["log_qz"][0].cpu(), own, Q_ATOL, Q_RTOL, "far own term")


@pytest.mark.parametrize("N,L,S", [(500, 16, 2), (2000, 10, 1)])
def test_mixed_scales(N, L, S):
    """A broad posterior's draw can land within a few sigma of a narrow one's mean, whose term then dominates log q(z_d) and
    moves by (dz / sigma_narrow) when z moves by one f32 ulp.  z is formed with the device's expf, which the host cannot
    reproduce to the last bit, so the reference is known only to within its change under a one-ulp change of sigma: that
    spread (measured 2.8e-4 nats at most per element here) is added to the tolerances."""
    mu, lv = synthetic_posteriors(N, L, 11, "mixed")
    eps = np.random.default_rng(3).standard_normal((S, N, L)).astype(np.float32)
    ref = latent_stats_reference(mu, lv, eps)
    sd = np.exp(np.float32(0.5) * lv)
    slack = {k: 0.0 for k in ref}
    for to in (np.float32(np.inf), np.float32(0.0)):
        z = (eps.astype(np.float64) * np.nextafter(sd, to).astype(np.float64) + mu.astype(np.float64)).astype(np.float32)
        alt = latent_stats_reference(mu, lv, z=z)
        for k in slack:
            if k != "active_units":
                slack[k] = np.maximum(slack[k], np.abs(np.asarray(alt[k]) - np.asarray(ref[k])))
    _compare(_run(mu, lv, S, eps), ref, f"mixed N{N} L{L}", slack)


def test_device_generator_is_stream_7():
    N, L, S, seed = 300, 16, 2, 1234
    mu, lv = synthetic_posteriors(N, L, 21)
    dev = _run(mu, lv, S, None, seed)
    eps7 = vo.counter_normal(S * N * L, seed, 7).reshape(S, N, L).astype(np.float32)
    given = _run(mu, lv, S, eps7)
    _close(dev["log_qz"].cpu(), given["log_qz"].cpu().numpy(), Q_ATOL, Q_RTOL, "generator log_qz")
    _close(dev["log_qz_dims"].cpu(), given["log_qz_dims"].cpu().numpy(), Q_ATOL, Q_RTOL, "generator log_qz_dims")
    for k in ("mi", "tc", "dwkl"):
        _close(float(dev[k]), float(given[k]), S_ATOL, 0.0, "generator " + k)
    _compare(dev, latent_stats_reference(mu, lv, eps7), "generator vs reference")
    other_seed = _run(mu, lv, S, None, seed + 1)
    eps6 = vo.counter_normal(S * N * L, seed, 6).reshape(S, N, L).astype(np.float32)
    other_stream = _run(mu, lv, S, eps6)
    for o in (other_seed, other_stream):
        assert float((o["log_qz"] - dev["log_qz"]).abs().max()) > 1e-2


def test_default_seed_is_fixed_and_calls_are_bit_identical():
    mu, lv = synthetic_posteriors(2500, 16, 8)
    a, b = _run(mu, lv, 2), _run(mu, lv, 2)
    for k in ("kl", "mi", "tc", "dwkl", "kl_per_dim", "var_mu", "dwkl_per_dim", "log_qz", "log_qz_dims"):
        assert torch.equal(a[k], b[k]), k
    assert a["active_units"] == b["active_units"]


def _rolls(n, H, seed):
    return torch.from_numpy(vo.synth_pianoroll(n, H, seed).astype(np.float32))


def test_collapsed_encoder_has_no_active_units():
    m = model_for(32, 16, False, "f32", "bce")
    with torch.no_grad():
        for name in ("fc_mu", "fc_var"):
            getattr(m, name).weight.zero_()
            getattr(m, name).bias.zero_()
    m.eval()
    enc = m.encode(_rolls(12, 32, 4).cuda())
    from torch_vae_amd.evaluation import latent_statistics
    out = latent_statistics(enc["mu"], enc["log_var"])
    assert out["active_units"] == 0
    assert bool((out["kl_per_dim"] == 0).all()) and float(out["kl"]) == 0.0 and bool((out["var_mu"] == 0).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_evaluate_latent_rolls(dtype, capsys):
    from torch_vae_amd.evaluation import evaluate, latent_statistics
    from torch_vae_amd.train import SyntheticPianorollLoader
    H, L, R = 32, 16, 10
    m = model_for(H, L, False, dtype, "bce")
    loader = SyntheticPianorollLoader(4, H, 3, seed=9)
    torch.manual_seed(0)
    base = evaluate(loader, m, "cuda", verbosity=1)
    out_base = capsys.readouterr().out
    torch.manual_seed(0)
    res = evaluate(loader, m, "cuda", verbosity=1, latent_rolls=R)
    printed = capsys.readouterr().out
    assert {k: res[k] for k in base} == base
    assert list(res)[len(base):] == ["kl", "active_units", "mi", "tc", "dwkl"]
    assert printed.startswith(out_base.rstrip("\n")) and printed.count(" nat") == out_base.count(" nat") + 4
    assert "active_units" in printed
    m.eval()
    xs = [x for x, _ in loader]
    mus, lvs = [], []
    with torch.no_grad():
        for x in xs:
            e = m.encode(x.cuda())
            mus.append(e["mu"])
            lvs.append(e["log_var"])
    mu, lv = torch.cat(mus)[:R], torch.cat(lvs)[:R]
    direct = latent_statistics(mu, lv)
    for k in ("kl", "mi", "tc", "dwkl"):
        assert res[k] == float(direct[k]), k
    assert res["active_units"] == direct["active_units"]
    if dtype == "f32":
        # the torch f64 CPU encoder, the same draws (stream 7, default seed 0): the f32 encoder moves mu / log_var by ~1e-6
        mu_r, lv_r = ref_encode(cpu_state(m), torch.cat(xs)[:R].cpu().double())
        eps = vo.counter_normal(R * L, 0, 7).reshape(1, R, L)
        ref = latent_stats_reference(mu_r.numpy(), lv_r.numpy(), z=eps * np.exp(0.5 * lv_r.numpy()) + mu_r.numpy())
        for k in ("kl", "mi", "tc", "dwkl"):
            _close(res[k], ref[k], 1e-3, 0.0, "evaluate f32 vs torch f64 encoder " + k)
