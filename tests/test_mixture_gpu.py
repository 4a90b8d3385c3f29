"""The latent Gaussian mixture on the device (include/vae_mixture.h, torch_vae_amd/mixture.py) against the numpy float64 reference
(tests/mixture_ref.py), at the smallest shapes at which something can go wrong:
    (64, 1, 1) L = K = 1 | (257, 3, 2) n no multiple of any block, L below every tile | (300, 16, 5) the default latent size |
    (515, 33, 4) L just past a tile edge | (400, 128, 3) maximal L, reg_covar carries the factor | (70, 5, 64) maximal K, n barely
    above K, nearly empty components | diag (300, 16, 5) | diag (130, 200, 3) L above 128.

GAPS.  log_prob and log_resp cannot be bounded tightly a priori; G is the distance between the reference's float32 emulation and
its float64 run at the shape, measured on the CPU by `python -m tests.mixture_ref` (tests/test_mixture_host.py holds the constants
below to a fresh measurement).  The gate on log_prob / log_resp is 4 G + 1e-6 |ref|: the device's FMA chains and lane trees differ
from the emulation's sequential order, and both obey the same first-order bound.  EM is compared with the reference's float64
trajectory from the same initial state at 10 x the measured distance between the emulated and the float64 trajectories (iterations
compound the difference), plus 1e-12 on the weights, whose measured gap is exactly zero where the clusters do not overlap.

CASES of the stream contract at the end; the tables are collected without touching the GPU (tests/test_mixture_host.py)."""
import io

import numpy as np
import pytest
import torch

from tests import mixture_ref as R
from tests import stream_harness as sh
from tests.stream_harness import Bufs, Case

pytestmark = pytest.mark.gpu

# python -m tests.mixture_ref   (max over the shape's elements of |float32 emulation - float64|; em_mean in standard deviations,
# em_cov relative to sqrt(S_ii S_jj))
GAPS = {
    (64, 1, 1, "full"): dict(log_prob=3.894e-07, log_resp=0.000e+00, em_ll=1.431e-08, em_pi=0.000e+00, em_mean=1.030e-09, em_cov=3.030e-07),
    (257, 3, 2, "full"): dict(log_prob=1.513e-06, log_resp=2.652e-05, em_ll=7.203e-08, em_pi=2.432e-12, em_mean=1.581e-07, em_cov=8.988e-08),
    (300, 16, 5, "full"): dict(log_prob=2.771e-06, log_resp=4.005e-05, em_ll=1.296e-07, em_pi=2.295e-11, em_mean=1.116e-07, em_cov=7.643e-08),
    (515, 33, 4, "full"): dict(log_prob=7.205e-06, log_resp=6.237e-05, em_ll=1.168e-07, em_pi=0.000e+00, em_mean=1.201e-07, em_cov=8.004e-08),
    (400, 128, 3, "full"): dict(log_prob=3.872e-04, log_resp=3.591e+00, em_ll=2.892e-03, em_pi=0.000e+00, em_mean=1.618e-07, em_cov=1.135e-07),
    (70, 5, 64, "full"): dict(log_prob=3.820e-06, log_resp=6.566e-02, em_ll=4.544e-08, em_pi=1.227e-08, em_mean=1.974e-06, em_cov=1.690e-06),
    (300, 16, 5, "diag"): dict(log_prob=3.363e-06, log_resp=1.438e-05, em_ll=1.303e-07, em_pi=9.055e-10, em_mean=1.455e-07, em_cov=1.195e-07),
    (130, 200, 3, "diag"): dict(log_prob=5.033e-05, log_resp=3.055e-04, em_ll=1.123e-06, em_pi=0.000e+00, em_mean=3.137e-07, em_cov=1.681e-07),
}
KIND = {"full": 0, "diag": 1}
U24 = 2.0 ** -24


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from torch_vae_amd import _lib
    return _lib.lib()


def ok(rc, what=""):
    assert rc == 0, (what, lib().vae_last_error().decode())


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def device_mixture(c, kind):
    from torch_vae_amd.mixture import LatentMixture
    return LatentMixture.from_state_dict(dict(covariance=kind, weights=dev(c["pi"]), means=dev(c["m"]), covariances=dev(c["S"]),
                                              log_likelihood_history=torch.empty(0, dtype=torch.float64)))


def factor_call(S, kind):
    """vae_mixture_factor on covariances [K, L, L] (or [K, L]) -> chol, winv, winv32, logdet, status"""
    K, L = S.shape[0], S.shape[1]
    S = dev(S)
    chol, winv, w32 = torch.empty_like(S), torch.empty_like(S), torch.empty(S.shape, dtype=torch.float32, device="cuda")
    logdet, status = torch.empty(K, dtype=torch.float64, device="cuda"), torch.empty(K, dtype=torch.int32, device="cuda")
    ok(lib().vae_mixture_factor(S.data_ptr(), K, L, KIND[kind], chol.data_ptr(), winv.data_ptr(), w32.data_ptr(), logdet.data_ptr(),
                                status.data_ptr(), st()), "vae_mixture_factor")
    return chol, winv, w32, logdet, status


# ---- factor -------------------------------------------------------------------------------------------------------------------------
def spd(L, K, seed):
    rng = np.random.default_rng(seed)
    S = np.empty((K, L, L))
    for k in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((L, L)))
        lam = 10.0 ** rng.uniform(-2, 2, L)
        lam[0], lam[-1] = 1e-2, 1e2                      # the whole range at every L (L = 1: 1e2)
        S[k] = (Q * lam) @ Q.T
        S[k] = 0.5 * (S[k] + S[k].T)
    return S


@pytest.mark.parametrize("L", [1, 3, 16, 33, 128])
def test_factor_full(L):
    K = 3
    S = spd(L, K, 40 + L)
    chol, winv, w32, logdet, status = (host(t) for t in factor_call(S, "full"))
    assert status.tolist() == [0] * K
    eye = np.eye(L)
    for k in range(K):
        Ck, Wk = chol[k], winv[k]
        assert not np.triu(Ck, 1).any() and not np.triu(Wk, 1).any()
        e_c = np.linalg.norm(Ck @ Ck.T - S[k]) / np.linalg.norm(S[k])
        e_w = np.abs(Wk @ Ck - eye).max()
        want = 0.5 * np.linalg.slogdet(S[k])[1]
        print(f"L {L} k {k}: |CC^T - S|_F / |S|_F {e_c:.2e}  max|WC - I| {e_w:.2e}  logdet {-logdet[k]:.12g} vs {want:.12g}")
        assert e_c <= 1e-12
        assert e_w <= 1e-10
        assert abs(-logdet[k] - want) <= 1e-12 * max(1.0, abs(want))
        assert np.array_equal(w32[k], Wk.astype(np.float32))


def test_factor_flags_a_matrix_that_is_not_positive_definite():
    L = 16
    S = spd(L, 3, 7)
    rng = np.random.default_rng(8)
    Q, _ = np.linalg.qr(rng.standard_normal((L, L)))
    lam = np.linspace(1.0, 2.0, L)
    lam[5] = -0.5
    S[1] = (Q * lam) @ Q.T
    S[1] = 0.5 * (S[1] + S[1].T)
    want = R.factor(S)[3]
    assert want[0] == 0 and want[1] > 0 and want[2] == 0
    chol, winv, w32, logdet, status = (host(t) for t in factor_call(S, "full"))
    assert status.tolist() == want.tolist()
    for a in (chol, winv, w32, logdet):
        assert np.isfinite(a).all()
    # diagonal kind: the first variance that is not > 0
    var = np.abs(rng.standard_normal((3, 300))) + 0.1
    var[2, 137], var[2, 250] = 0.0, -1.0
    chol, winv, w32, logdet, status = (host(t) for t in factor_call(var, "diag"))
    assert status.tolist() == [0, 0, 138]
    for a in (chol, winv, w32, logdet):
        assert np.isfinite(a).all()
    np.testing.assert_allclose(chol[:2], np.sqrt(var[:2]), rtol=1e-15)
    np.testing.assert_allclose(logdet[:2], -0.5 * np.log(var[:2]).sum(1), rtol=1e-12)


# ---- log_prob, log_resp --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.SHAPES), ids=R.shape_id)
def test_log_prob_and_log_resp(shape):
    n, L, K, kind = shape
    c, g = R.case(shape), GAPS[shape]
    mix = device_mixture(c, kind)
    x = dev(c["x"])
    lp, lr = host(mix.log_prob(x)), host(mix.log_responsibilities(x)).astype(np.float64)
    gate_p = 4 * g["log_prob"] + 1e-6 * np.abs(c["log_prob"])
    gate_r = 4 * g["log_resp"] + 1e-6 * np.abs(c["log_resp"])
    e_p, e_r = np.abs(lp - c["log_prob"]), np.abs(lr - c["log_resp"])
    print(f"{R.shape_id(shape)}: log_prob max err {e_p.max():.3e} (G {g['log_prob']:.3e}, worst err/gate {(e_p / gate_p).max():.3f}); "
          f"log_resp max err {e_r.max():.3e} (G {g['log_resp']:.3e}, worst err/gate {np.nanmax(e_r / np.maximum(gate_r, 1e-300)):.3f})")
    assert (e_p <= gate_p).all()
    assert (e_r <= gate_r).all()
    # the mean, and bit-identical repeats
    mean = torch.empty((), dtype=torch.float64, device="cuda")
    lp2 = torch.empty(n, dtype=torch.float64, device="cuda")
    ok(lib().vae_mixture_log_prob(x.data_ptr(), n, L, K, KIND[kind], mix.weights.data_ptr(), mix.means.data_ptr(), mix._winv32.data_ptr(),
                                  mix._logdet.data_ptr(), lp2.data_ptr(), 0, mean.data_ptr(), st()), "vae_mixture_log_prob")
    assert np.array_equal(host(lp2), lp)
    assert abs(float(mean) - c["mean"]) <= 4 * g["log_prob"] + 1e-6 * abs(c["mean"])
    assert abs(float(mean) - lp.mean()) <= 1e-12 * np.abs(lp).max()


# ---- M-step --------------------------------------------------------------------------------------------------------------------------
def mstep_call(lr32, x, K, kind, reg=R.REG):
    n, L = x.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    pi, m = torch.empty(K, **f64), torch.empty(K, L, **f64)
    S = torch.empty((K, L, L) if kind == "full" else (K, L), **f64)
    ok(lib().vae_mixture_mstep(lr32.data_ptr(), x.data_ptr(), n, L, K, KIND[kind], reg, pi.data_ptr(), m.data_ptr(), S.data_ptr(), st()),
       "vae_mixture_mstep")
    return pi, m, S


@pytest.mark.parametrize("shape", list(R.SHAPES), ids=R.shape_id)
def test_mstep(shape):
    """From the reference's own float32 log_resp.  pi to 1e-12; |dS_ij| <= 5e-6 sqrt(S_ii S_jj): at most 8 roundings per f32 product
    plus the 64-term f32 accumulation is 72 * 2^-24 = 4.3e-6, and Cauchy-Schwarz bounds the sum; |dm_d| <= 1e-6 sqrt(S_dd + m_d^2)."""
    n, L, K, kind = shape
    c = R.case(shape)
    lr32 = c["log_resp32"]
    pi_w, m_w, S_w = R.mstep(lr32, c["x"], R.REG, kind)
    pi, m, S = (host(t) for t in mstep_call(dev(lr32), dev(c["x"]), K, kind))
    var = np.einsum("kdd->kd", S_w) if kind == "full" else S_w
    e_pi = np.abs(pi - pi_w).max()
    e_m = (np.abs(m - m_w) / np.sqrt(var + m_w ** 2)).max()
    scale = np.sqrt(var[:, :, None] * var[:, None, :]) if kind == "full" else var
    e_S = (np.abs(S - S_w) / scale).max()
    print(f"{R.shape_id(shape)}: pi {e_pi:.2e} (1e-12)  mean {e_m:.2e} (1e-6)  cov {e_S:.2e} (5e-6)")
    assert e_pi <= 1e-12
    assert e_m <= 1e-6
    assert e_S <= 5e-6
    if kind == "full":
        assert np.array_equal(S, S.transpose(0, 2, 1))


# ---- EM ------------------------------------------------------------------------------------------------------------------------------
def em_call(x, init, kind, iters, reg=R.REG):
    pi0, m0, S0 = init
    n, L = x.shape
    K = len(pi0)
    pi, m, S = dev(pi0), dev(m0), dev(S0)
    chol, winv, w32 = torch.empty_like(S), torch.empty_like(S), torch.empty(S.shape, dtype=torch.float32, device="cuda")
    logdet, status = torch.empty(K, dtype=torch.float64, device="cuda"), torch.empty(K, dtype=torch.int32, device="cuda")
    hist = torch.empty(iters, dtype=torch.float64, device="cuda")
    ok(lib().vae_mixture_em(x.data_ptr(), n, L, K, KIND[kind], iters, reg, pi.data_ptr(), m.data_ptr(), S.data_ptr(), chol.data_ptr(),
                            winv.data_ptr(), w32.data_ptr(), logdet.data_ptr(), status.data_ptr(), hist.data_ptr(), st()), "vae_mixture_em")
    return dict(pi=pi, m=m, S=S, chol=chol, winv=winv, w32=w32, logdet=logdet, status=status, hist=hist)


@pytest.mark.parametrize("shape", R.EM_SHAPES, ids=R.shape_id)
def test_em_against_the_reference_trajectory(shape):
    n, L, K, kind = shape
    c, g = R.case(shape), GAPS[shape]
    x = dev(c["x"])
    got = em_call(x, c["init"], kind, c["iters"])
    again = em_call(x, c["init"], kind, c["iters"])
    for k in got:
        assert sh.same_bits(got[k], again[k]), k                     # two calls, identical bits
    out = {k: host(v) for k, v in got.items()}
    assert not out["status"].any()
    sd = np.sqrt(np.einsum("kdd->kd", c["S"]) if kind == "full" else c["S"])
    sc = sd[:, :, None] * sd[:, None, :] if kind == "full" else c["S"]
    e = dict(em_ll=np.abs(out["hist"] - c["hist"]).max(), em_pi=np.abs(out["pi"] - c["pi"]).max(),
             em_mean=(np.abs(out["m"] - c["m"]) / sd).max(), em_cov=(np.abs(out["S"] - c["S"]) / sc).max())
    tol = {k: 10 * g[k] + (1e-12 if k == "em_pi" else 0.0) for k in e}
    print(f"{R.shape_id(shape)}: " + "  ".join(f"{k} {e[k]:.2e} (tol {tol[k]:.2e})" for k in e))
    for k in e:
        assert e[k] <= tol[k], k
    # the mean log-likelihood never falls by more than twice the log_prob gate
    gate = 4 * g["log_prob"] + 1e-6 * np.abs(c["hist"]).max()
    assert (np.diff(out["hist"]) >= -2 * gate).all(), out["hist"]
    # the factors returned belong to the final covariances
    chol = host(factor_call(out["S"], kind)[0])
    assert np.array_equal(chol, out["chol"])


def test_fit_is_the_documented_sequence_of_calls():
    """LatentMixture.fit = the epoch-0 permutation's first K points, one M-step with a single component and log_resp = 0, uniform
    weights, then one EM call: bit for bit, and within the EM tolerances of the reference's fit."""
    from torch_vae_amd.data import epoch_indices
    from torch_vae_amd.mixture import LatentMixture
    shape = (300, 16, 5, "full")
    n, L, K, kind = shape
    c = R.case(shape)
    x = dev(c["x"])
    mix = LatentMixture.fit(x, K, iters=c["iters"], seed=0)
    _, _, S1 = mstep_call(torch.zeros(n, 1, device="cuda"), x, 1, kind)
    first = epoch_indices(n, seed=0, epoch=0)[:K]
    init = (np.full(K, 1.0 / K), c["x"][first.numpy()].astype(np.float64), np.repeat(host(S1), K, axis=0))
    want = em_call(x, init, kind, c["iters"])
    for name, t in (("pi", mix.weights), ("m", mix.means), ("S", mix.covariances), ("chol", mix.cholesky), ("hist", mix.log_likelihood_history)):
        assert sh.same_bits(t, want[name]), name
    assert mix.log_likelihood_history.shape == (c["iters"],) and mix.weights.dtype == torch.float64
    # (N_k sums exp of the float32 log_resp, each 2^-24 |log r| off in relative terms: the weights add up to 1 only that closely)
    np.testing.assert_allclose(host(mix.weights).sum(), 1.0, rtol=1e-6)
    # a different seed starts elsewhere
    other = LatentMixture.fit(x, K, iters=1, seed=1)
    assert not sh.same_bits(other.log_likelihood_history[:1], mix.log_likelihood_history[:1])
    # the diagonal kind through the same door
    d = LatentMixture.fit(x, 3, covariance="diag", iters=2)
    assert d.covariances.shape == (3, L) and d.cholesky.shape == (3, L) and torch.isfinite(d.log_likelihood_history).all()


def test_fit_reports_a_failed_pivot():
    from torch_vae_amd.mixture import LatentMixture
    x = torch.zeros(40, 4, device="cuda")
    x[:, 0] = torch.arange(40, device="cuda")          # three constant columns: singular without reg_covar
    with pytest.raises(RuntimeError, match=r"component \d+ .*not positive definite"):
        LatentMixture.fit(x, 2, iters=2, reg_covar=0.0)


# ---- sample --------------------------------------------------------------------------------------------------------------------------
def sample_call(mix_arrays, kind, n, t, seed=0, u=None, eps=None):
    pi, m, chol = mix_arrays
    K, L = m.shape
    z = torch.empty(n, L, device="cuda")
    comp = torch.empty(n, dtype=torch.int32, device="cuda")
    ok(lib().vae_mixture_sample(n, L, K, KIND[kind], pi.data_ptr(), m.data_ptr(), chol.data_ptr(), t, seed, 0 if u is None else u.data_ptr(),
                                0 if eps is None else eps.data_ptr(), z.data_ptr(), comp.data_ptr(), st()), "vae_mixture_sample")
    return z, comp


@pytest.mark.parametrize("shape", [(257, 3, 2, "full"), (515, 33, 4, "full"), (400, 128, 3, "full"), (70, 5, 64, "full"), (130, 200, 3, "diag")],
                         ids=R.shape_id)
def test_sample_with_explicit_draws(shape):
    """Components equal the reference's exactly; |z - ref| <= (L + 2) 2^-24 (|m_d| + t sum_j |C_dj eps_j|)."""
    n, L, K, kind = shape
    c = R.case(shape)
    rng = np.random.default_rng(60 + L)
    n_draws, t = 203, 0.8
    u = rng.random(n_draws)
    u[:3] = [0.0, np.nextafter(1.0, 0.0), np.cumsum(c["pi"])[0]]          # the ends, and a cumulative weight itself (not exceeded)
    eps = rng.standard_normal((n_draws, L)).astype(np.float32)
    z_w, comp_w, scale = R.sample(c["pi"], c["m"], c["C"], kind, t, u, eps)
    z, comp = sample_call((dev(c["pi"]), dev(c["m"]), dev(c["C"])), kind, n_draws, t, u=dev(u), eps=dev(eps))
    assert host(comp).tolist() == comp_w.tolist()
    err = np.abs(host(z).astype(np.float64) - z_w)
    print(f"{R.shape_id(shape)}: worst err / bound {(err / ((L + 2) * U24 * scale)).max():.3f}")
    assert (err <= (L + 2) * U24 * scale).all()


def test_sample_with_generated_draws():
    shape = (300, 16, 5, "full")
    n, L, K, kind = shape
    c = R.case(shape)
    mix = device_mixture(c, kind)
    n_draws, t = 500, 1.3
    cum = np.cumsum(c["pi"])
    for seed in (0, 1, 12345):
        u, eps = R.generated_draws(n_draws, L, seed)
        assert np.abs(u[:, None] - cum[None, :]).min() > 1e-12      # no draw on a boundary: the choice is unambiguous
        z_w, comp_w, scale = R.sample(c["pi"], c["m"], c["C"], kind, t, u, eps)
        z, comp = mix.sample(n_draws, temperature=t, seed=seed, return_components=True)
        assert comp.dtype == torch.int32 and host(comp).tolist() == comp_w.tolist()
        # (the device's normals are the float32 roundings of its own float64 Box-Muller: one more unit in the last place of every eps_j
        #  beside the bound of the explicit draws)
        err = np.abs(host(z).astype(np.float64) - z_w)
        assert (err <= (L + 4) * U24 * scale).all()
        z2, comp2 = mix.sample(n_draws, temperature=t, seed=seed, return_components=True)
        assert sh.same_bits(z, z2) and sh.same_bits(comp, comp2)
    assert not sh.same_bits(mix.sample(n_draws, seed=0), mix.sample(n_draws, seed=1))
    assert mix.sample(0).shape == (0, L)


def test_sample_frequencies():
    shape = (257, 3, 2, "full")
    c = R.case(shape)
    pi = np.array([0.5, 0.2, 0.3])
    mix_arrays = (dev(pi), dev(np.repeat(c["m"][:1], 3, 0)), dev(np.repeat(c["C"][:1], 3, 0)))
    n = 20000
    _, comp = sample_call(mix_arrays, "full", n, 1.0, seed=9)
    freq = np.bincount(host(comp), minlength=3) / n
    print("frequencies", freq, "weights", pi)
    assert (np.abs(freq - pi) <= 4 * np.sqrt(pi * (1 - pi) / n)).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_end_to_end(dtype):
    from tests.util import make_model, perturbed_params
    from torch_vae_amd.data import DevicePianorollLoader, PianorollDataset
    from torch_vae_amd.evaluation import sample_novelty
    from torch_vae_amd.mixture import LatentMixture, encode_dataset
    H, L = 32, 16
    model = make_model(H, L, False, dtype, perturbed_params(L, H, 31, False))
    rng = np.random.default_rng(23)
    ds = PianorollDataset(torch.from_numpy((rng.random((96, H, H)) < 0.1).astype(np.float32)), storage="bits")
    loader = DevicePianorollLoader(ds, 40, train=False)
    mu, log_var = encode_dataset(model, loader)
    assert mu.shape == (96, L) and log_var.shape == (96, L) and mu.dtype == torch.float32 and mu.is_cuda
    with torch.no_grad():
        first = model.encode(next(iter(loader))[0])
    assert sh.same_bits(mu[:40], first["mu"])
    assert encode_dataset(model, loader, max_rolls=50)[0].shape == (50, L)
    mix = LatentMixture.fit(mu, 3, iters=5)
    assert torch.isfinite(mix.log_likelihood_history).all()
    # the prior hook: sample_notes(prior=mix) decodes exactly mix.sample
    notes = model.sample_notes(6, prior=mix, seed=1, temperature=0.9, return_rolls=True)
    with torch.no_grad():
        want = model.decode(mix.sample(6, temperature=0.9, seed=1))
    assert sh.same_bits(notes["rolls"], want)
    assert sh.same_bits(model.sample(6, 0, prior=mix, temperature=0.9, seed=1), want)
    # and without one, today's draw
    plain = model.sample_notes(6, seed=1, temperature=0.9, return_rolls=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    z = 0.9 * torch.randn(6, L, generator=g, device="cuda", dtype=torch.float32)
    with torch.no_grad():
        assert sh.same_bits(plain["rolls"], model.decode(z))
    assert not sh.same_bits(plain["rolls"], notes["rolls"])
    summary, near, ev = sample_novelty(model, ds, 6, seed=1, prior=mix, max_notes=512)
    assert isinstance(summary, dict) and near["index"].shape[0] == 6 and "cleaned" in ev
    # state_dict round trip through torch.save keeps log_prob bits
    buf = io.BytesIO()
    torch.save(mix.state_dict(), buf)
    buf.seek(0)
    back = LatentMixture.from_state_dict(torch.load(buf))
    assert sh.same_bits(back.log_prob(mu), mix.log_prob(mu))
    assert sh.same_bits(back.cholesky, mix.cholesky)


# ---- the stream contract (include/vae_step.h, first paragraph) on the mixture's entry points ---------------------------------------------
SN, SL, SK = 20, 5, 3


def _stream_state():
    rng = np.random.default_rng(77)
    x = R.make_data(SN, SL, SK)
    pi, m, S = R.initial_state(x, SK)
    pi, m, S, _ = R.em(x, pi, m, S, "full", 2)
    C_, W, logdet, _ = R.factor(S)
    lr = R.log_prob(x, pi, m, W, logdet, "full", f32=True)[1]
    return dict(x=x, pi=pi, m=m, S=S, C=C_, W32=W.astype(np.float32), logdet=logdet, lr=lr, u=rng.random(SN),
                eps=rng.standard_normal((SN, SL)).astype(np.float32))


def _b(names, outs):
    s, b = _stream_state(), Bufs()
    for name in names:
        b.inp(name, torch.from_numpy(np.array(s[name])))
    for name, shape, dtype in outs:
        b.outp(name, *shape, dtype=dtype)
    return b


F64, F32, I32 = torch.float64, torch.float32, torch.int32
KLL = (SK, SL, SL)


def _make_factor():
    return _b(["S"], [("chol", KLL, F64), ("winv", KLL, F64), ("w32", KLL, F32), ("logdet", (SK,), F64), ("status", (SK,), I32)])


def _factor(b):
    ok(lib().vae_mixture_factor(b["S"].data_ptr(), SK, SL, 0, b["chol"].data_ptr(), b["winv"].data_ptr(), b["w32"].data_ptr(),
                                b["logdet"].data_ptr(), b["status"].data_ptr(), st()), "vae_mixture_factor")


def _make_log_prob():
    return _b(["x", "pi", "m", "W32", "logdet"], [("log_prob", (SN,), F64), ("log_resp", (SN, SK), F32), ("mean", (1,), F64)])


def _log_prob(b):
    ok(lib().vae_mixture_log_prob(b["x"].data_ptr(), SN, SL, SK, 0, b["pi"].data_ptr(), b["m"].data_ptr(), b["W32"].data_ptr(),
                                  b["logdet"].data_ptr(), b["log_prob"].data_ptr(), b["log_resp"].data_ptr(), b["mean"].data_ptr(), st()),
       "vae_mixture_log_prob")


def _make_mstep():
    return _b(["lr", "x"], [("pi_out", (SK,), F64), ("m_out", (SK, SL), F64), ("S_out", KLL, F64)])


def _mstep(b):
    ok(lib().vae_mixture_mstep(b["lr"].data_ptr(), b["x"].data_ptr(), SN, SL, SK, 0, 1e-6, b["pi_out"].data_ptr(), b["m_out"].data_ptr(),
                               b["S_out"].data_ptr(), st()), "vae_mixture_mstep")


def _make_sample():
    return _b(["pi", "m", "C", "u", "eps"], [("z", (SN, SL), F32), ("component", (SN,), I32), ("z_gen", (SN, SL), F32), ("component_gen", (SN,), I32)])


def _sample(b):
    ok(lib().vae_mixture_sample(SN, SL, SK, 0, b["pi"].data_ptr(), b["m"].data_ptr(), b["C"].data_ptr(), 0.9, 3, b["u"].data_ptr(),
                                b["eps"].data_ptr(), b["z"].data_ptr(), b["component"].data_ptr(), st()), "vae_mixture_sample")
    ok(lib().vae_mixture_sample(SN, SL, SK, 0, b["pi"].data_ptr(), b["m"].data_ptr(), b["C"].data_ptr(), 0.9, 3, 0, 0, b["z_gen"].data_ptr(),
                                b["component_gen"].data_ptr(), st()), "vae_mixture_sample")


def _make_em():
    s, b = _stream_state(), Bufs()
    pi, m, S = R.initial_state(s["x"], SK)
    b.inp("x", torch.from_numpy(np.array(s["x"])))
    b.inp("pi", torch.from_numpy(pi), inout=True); b.inp("m", torch.from_numpy(m), inout=True); b.inp("S", torch.from_numpy(S), inout=True)
    for name, shape, dtype in [("chol", KLL, F64), ("winv", KLL, F64), ("w32", KLL, F32), ("logdet", (SK,), F64), ("status", (SK,), I32),
                               ("hist", (3,), F64)]:
        b.outp(name, *shape, dtype=dtype)
    return b


def _em(b):
    ok(lib().vae_mixture_em(b["x"].data_ptr(), SN, SL, SK, 0, 3, 1e-6, b["pi"].data_ptr(), b["m"].data_ptr(), b["S"].data_ptr(),
                            b["chol"].data_ptr(), b["winv"].data_ptr(), b["w32"].data_ptr(), b["logdet"].data_ptr(), b["status"].data_ptr(),
                            b["hist"].data_ptr(), st()), "vae_mixture_em")


STREAM_CASES = [
    Case("mixture_factor", ("vae_mixture_factor",), _make_factor, _factor),
    Case("mixture_log_prob", ("vae_mixture_log_prob",), _make_log_prob, _log_prob),
    Case("mixture_mstep", ("vae_mixture_mstep",), _make_mstep, _mstep),
    Case("mixture_sample", ("vae_mixture_sample",), _make_sample, _sample),
    Case("mixture_em", ("vae_mixture_em",), _make_em, _em),
]


def _make_fit():
    b = Bufs()
    b.inp("x", torch.from_numpy(np.array(R.make_data(SN, SL, SK))))
    return b


def _fit(b):
    from torch_vae_amd.mixture import LatentMixture
    mix = LatentMixture.fit(b["x"], SK, iters=3)
    b.out["weights"], b.out["means"], b.out["covariances"] = mix.weights, mix.means, mix.covariances
    b.out["history"] = mix.log_likelihood_history
    b.out["z"], b.out["component"] = mix.sample(SN, seed=4, return_components=True)
    b.out["log_prob"] = mix.log_prob(b["x"])


PY_STREAM_CASES = [
    Case("python/mixture_fit+sample", ("vae_mixture_mstep", "vae_mixture_em", "vae_mixture_sample", "vae_mixture_log_prob"), _make_fit, _fit,
         sync_free=False, warmups=2, reads_back="LatentMixture.fit ends with one read of the factorisation status, by design"),
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_stream_contract(case):
    sh.check_case(case)


@pytest.mark.parametrize("case", PY_STREAM_CASES, ids=repr)
def test_stream_contract_python_layer(case):
    sh.check_case(case)
