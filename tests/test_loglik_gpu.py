"""Importance-weighted log-likelihood and per-sample ELBO on the GPU (VanillaVAE.log_likelihood, vae_log_likelihood).
Yardsticks: a torch f64 eval-mode restatement on the CPU (f32 mode), the model's own eval decoder scored per sample in f64
(16-bit modes, kernel-local), and the numpy oracle's 16-bit storage emulation.  The combine is restated in
tests/test_loglik_host.py (combine_reference), which checks it against torch.logsumexp."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from tests.test_loglik_host import LOG_PI, combine_reference, latent_terms
from tests.util import load_params, make_model, perturbed_params

pytestmark = pytest.mark.gpu

# max |log_w - oracle| / |oracle| of the 16-bit modes against vo.forward(train=False, storage=...): the oracle rounds where the
# kernels store, but sums in another order, so a stored value can land on the other side of a rounding step.  Measured on
# MI355X (64x64, L 16, B 3, K 4, perturbed running statistics): bf16 5.2e-7 (BCE) / 4.6e-7 (MSE), f16 1.0e-6 / 1.8e-7.
STORAGE_TOL = {"bf16": 5e-6, "f16": 5e-6}
# Chunking and batch composition change the batch the decoder kernels run on, and with it how they tile the work: log_w moves
# at the rounding level.  Measured on MI355X (64x64, L 16): f32 8.9e-9, f16 7.1e-8 relative at most, bf16 bit-identical in
# these cases (not guaranteed).  Repeats with the same chunking are bit-identical in every mode.
BATCH_RTOL = {"bf16": 5e-7, "f16": 5e-7, "f32": 1e-7}


def perturb_running_stats(model, seed):
    """Running statistics away from 0 / 1, so eval-mode BatchNorm is not the identity."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in model._bn_modules():
            C = bn.running_mean.numel()
            bn.running_mean.copy_(0.2 * torch.randn(C, generator=g, dtype=torch.float64))
            bn.running_var.copy_(0.5 + torch.rand(C, generator=g, dtype=torch.float64))


def rolls(B, H, seed, recon):
    x = vo.synth_pianoroll(B, H, seed).astype(np.float64)
    if recon == "mse":                      # velocity-valued targets for the Gaussian likelihood
        x = x * np.random.default_rng(seed).uniform(0.2, 1.0, x.shape)
    return x.astype(np.float32)


def model_for(H, L, gen, dtype, recon, seed=61, max_batch=None):
    from torch_vae_amd.models import VanillaVAE
    p = perturbed_params(L, H, seed, gen)
    m = VanillaVAE(1, L, H, generalised=gen, compute_dtype=dtype, recon_loss=recon, max_batch=max_batch).cuda()
    load_params(m, p)
    perturb_running_stats(m, seed + 1)
    return m


def cpu_state(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


def ref_encode(sd, x):
    a = x
    for i in range(4):
        n = f"encoder.{i}"
        a = F.conv2d(a, sd[n + ".0.weight"], sd[n + ".0.bias"], stride=2, padding=1)
        a = F.batch_norm(a, sd[n + ".1.running_mean"], sd[n + ".1.running_var"], sd[n + ".1.weight"], sd[n + ".1.bias"],
                         training=False, eps=1e-5)
        a = F.leaky_relu(a, 0.01)
    pre = a.flatten(1)
    return F.linear(pre, sd["fc_mu.weight"], sd["fc_mu.bias"]), F.linear(pre, sd["fc_var.weight"], sd["fc_var.bias"])


def ref_decode(sd, z, s):
    def bn(a, n):
        return F.leaky_relu(F.batch_norm(a, sd[n + ".running_mean"], sd[n + ".running_var"], sd[n + ".weight"], sd[n + ".bias"],
                                         training=False, eps=1e-5), 0.01)
    a = F.linear(z, sd["decoder_input.weight"], sd["decoder_input.bias"]).view(-1, 256, s, s)
    for i in range(3):
        n = f"decoder.{i}"
        a = bn(F.conv_transpose2d(a, sd[n + ".0.weight"], sd[n + ".0.bias"], stride=2, padding=1, output_padding=1), n + ".1")
    a = bn(F.conv_transpose2d(a, sd["final_layer.0.weight"], sd["final_layer.0.bias"], stride=2, padding=1, output_padding=1),
           "final_layer.1")
    return torch.sigmoid(F.conv2d(a, sd["final_layer.3.weight"], sd["final_layer.3.bias"], padding=1))


def score(xhat, t, recon):
    """log p(x|z) per sample, f64: Bernoulli (ATen's BCE, logs clamped at -100) or Gaussian with variance 1/2."""
    xhat, t = torch.as_tensor(xhat).double(), torch.as_tensor(t).double()
    if recon == "bce":
        return -F.binary_cross_entropy(xhat, t, reduction="none").sum((1, 2, 3)).numpy()
    return (-((xhat - t) ** 2).sum((1, 2, 3)) - xhat[0].numel() / 2 * LOG_PI).numpy()


def torch_reference(model, x, eps, recon):
    sd = cpu_state(model)
    s = model.img_size // 16 if model.generalised else 2
    K, B, L = eps.shape
    mu, lv = ref_encode(sd, torch.from_numpy(x).double())
    z, lat = latent_terms(eps, mu.numpy(), lv.numpy())
    xhat = ref_decode(sd, torch.from_numpy(z.reshape(K * B, L)), s)
    lpx = score(xhat, torch.from_numpy(x).double().repeat(K, 1, 1, 1), recon).reshape(K, B)
    return combine_reference(lpx, lat, mu.numpy(), lv.numpy())


def run(model, x, K, **kw):
    if "eps" in kw and isinstance(kw["eps"], np.ndarray):
        kw["eps"] = torch.from_numpy(kw["eps"]).cuda()
    out = model.log_likelihood(torch.from_numpy(x).cuda(), K, **kw)
    torch.cuda.synchronize()
    assert all(v.dtype == torch.float64 and v.device.type == "cuda" for v in out.values())
    return out["log_weights"].cpu().numpy(), out["log_likelihood"].cpu().numpy(), out["elbo"].cpu().numpy()


@pytest.mark.parametrize("recon", ["bce", "mse"])
@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 4, False), (64, 16, 3, True), (128, 16, 2, True), (32, 1024, 3, False)])
def test_f32_against_torch_f64(H, L, B, gen, recon):
    m = model_for(H, L, gen, "f32", recon)
    x = rolls(B, H, 62, recon)
    for K in (1, 5):
        eps = vo.counter_normal(K * B * L, 70 + K, 6).reshape(K, B, L).astype(np.float32)
        got = run(m, x, K, eps=eps)
        want = torch_reference(m, x, eps, recon)
        assert got[0].shape == (K, B) and got[1].shape == (B,) and got[2].shape == (B,)
        for name, g, w in zip(("log_w", "log_likelihood", "elbo"), got, want):
            np.testing.assert_allclose(g, w, rtol=1e-5, err_msg=f"{name} K={K}")


@pytest.mark.parametrize("recon", ["bce", "mse"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16bit_kernel_local_and_storage_emulation(dtype, recon):
    H, L, B, gen, K = 64, 16, 3, True, 4
    m = model_for(H, L, gen, dtype, recon)
    x = rolls(B, H, 63, recon)
    eps = vo.counter_normal(K * B * L, 64, 6).reshape(K, B, L).astype(np.float32)
    log_w, _, _ = run(m, x, K, eps=eps)
    # kernel-local: the same z through the model's own eval-mode decoder, scored per sample in f64
    m.eval()
    with torch.no_grad():
        enc = m(torch.from_numpy(x).cuda())["encoded"]
    mu, lv = enc["mu"].cpu().numpy(), enc["log_var"].cpu().numpy()
    sd = torch.exp(0.5 * enc["log_var"]).cpu().numpy()                          # expf(0.5f * lv), as the latent kernel
    z = (eps.astype(np.float64) * sd.astype(np.float64) + mu.astype(np.float64)).astype(np.float32)   # its fused multiply-add
    xhat = m.decode(torch.from_numpy(z.reshape(K * B, L)).cuda()).cpu()
    lpx = score(xhat, torch.from_numpy(x).repeat(K, 1, 1, 1), recon).reshape(K, B)
    _, lat = latent_terms(eps, mu, lv)
    np.testing.assert_allclose(log_w, lpx + lat, rtol=1e-5)
    # against the oracle's 16-bit storage emulation, one draw at a time
    p = {k: v.detach().cpu().double().numpy() for k, v in m.named_parameters()}
    bn = {k: v.detach().cpu().double().numpy() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    want = np.empty((K, B))
    for k in range(K):
        c = vo.forward(p, x.astype(np.float64), eps[k].astype(np.float64), bn, train=False, storage=dtype)
        _, lat_k = latent_terms(eps[k:k + 1], c["mu"], c["lv"])
        want[k] = score(torch.from_numpy(c["output"]), torch.from_numpy(x), recon) + lat_k[0]
    err = float(np.max(np.abs(log_w - want) / np.abs(want)))
    print(f"{dtype} {recon}: max relative |log_w - oracle(storage)| = {err:.3e}")
    assert err < STORAGE_TOL[dtype], err


def same(a, b, dtype, msg=""):
    np.testing.assert_allclose(a, b, rtol=BATCH_RTOL[dtype], atol=0, err_msg=msg)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_chunking_repeats_and_device_noise(dtype):
    H, L, B, gen, K = 64, 16, 3, True, 5
    m = model_for(H, L, gen, dtype, "bce", max_batch=K * B)
    x = rolls(B, H, 65, "bce")
    base = run(m, x, K, seed=1234)
    for chunk in (1, 3, K):
        got = run(m, x, K, seed=1234, chunk=chunk)
        for g, b in zip(got, base):
            same(g, b, dtype, f"chunk={chunk}")
    # repeats and the device generator against its numpy restatement: bit-identical in every mode (same chunking)
    again = run(m, x, K, seed=1234)
    eps = vo.counter_normal(K * B * L, 1234, 6).reshape(K, B, L).astype(np.float32)
    explicit = run(m, x, K, eps=eps)
    for g, e, b in zip(again, explicit, base):
        np.testing.assert_array_equal(g, b)
        np.testing.assert_array_equal(e, b)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_batch_independence(dtype):
    H, L, B, gen, K = 64, 16, 4, True, 3
    m = model_for(H, L, gen, dtype, "bce")
    x = rolls(B, H, 66, "bce")
    eps = vo.counter_normal(K * B * L, 67, 6).reshape(K, B, L).astype(np.float32)
    full = run(m, x, K, eps=eps)
    for i in range(B):
        one = run(m, x[i:i + 1], K, eps=np.ascontiguousarray(eps[:, i:i + 1]))
        same(one[0][:, 0], full[0][:, i], dtype)
        same(one[1][0], full[1][i], dtype)
        same(one[2][0], full[2][i], dtype)


def test_bounds():
    H, L, B, gen = 32, 16, 6, False
    m = model_for(H, L, gen, "bf16", "bce")
    x = rolls(B, H, 68, "bce")
    log_w, ll, _ = run(m, x, 8, seed=5)
    mean = log_w.mean(axis=0)
    assert np.all(ll >= mean - 1e-12 * np.abs(mean)), (ll, mean)
    log_w1, ll1, _ = run(m, x, 1, seed=5)
    np.testing.assert_array_equal(ll1, log_w1[0])


def test_no_side_effects():
    from torch_vae_amd import _lib
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen = 32, 16, 4, False
    m1 = model_for(H, L, gen, "bf16", "bce", max_batch=16)
    m2 = model_for(H, L, gen, "bf16", "bce", max_batch=16)
    x = torch.from_numpy(rolls(B, H, 69, "bce")).cuda()
    m1.train()
    before = (m1._flat.clone(), m1._bnflat.clone(), m1._nbt.clone())
    m1.log_likelihood(x, 4)
    torch.cuda.synchronize()
    assert m1.training and m1._fwd_count == 0 and m1._last is None
    for a, b in zip(before, (m1._flat, m1._bnflat, m1._nbt)):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError):
        m1._run_backward(None, None, None, None, None, None)
    st = torch.cuda.current_stream().cuda_stream
    out3 = torch.empty(3, device="cuda")
    assert _lib.lib().vae_loss(m1._ctx.handle, 1.0, out3.data_ptr(), st) != 0
    assert _lib.lib().vae_backward(m1._ctx.handle, x.data_ptr(), m1._flat.data_ptr(), m1._gnew.data_ptr(), 0, 0, 0, 0, 0, 0,
                                   1.0, 1, st) != 0
    outs = []
    for m in (m1, m2):
        opt = FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
        o3, _ = m.fused_train_step(opt, x)
        outs.append(o3.cpu().numpy().copy())
    np.testing.assert_array_equal(outs[0], outs[1])


def test_evaluate_nll_on_synthetic_loader(capsys):
    from torch_vae_amd.evaluation import evaluate
    from torch_vae_amd.train import SyntheticPianorollLoader
    m = model_for(32, 16, False, "bf16", "bce")
    loader = SyntheticPianorollLoader(4, 32, 3, seed=9)
    torch.manual_seed(0)
    today = evaluate(loader, m, "cuda", verbosity=1)
    out_today = capsys.readouterr().out
    torch.manual_seed(0)
    zero = evaluate(loader, m, "cuda", verbosity=1, nll_samples=0)
    assert zero == today and capsys.readouterr().out == out_today
    assert list(zero) == ["count", "cross-entropy", "mse", "mae"]
    c0 = m._ll_count
    torch.manual_seed(0)
    res = evaluate(loader, m, "cuda", verbosity=1, nll_samples=8)
    printed = capsys.readouterr().out
    assert {k: res[k] for k in today} == today
    assert "nll" in printed and printed.count(" nat") == 3
    m._ll_count = c0                         # the same seeds again
    lls, elbos = [], []
    for x, _ in loader:
        o = m.log_likelihood(x, 8)
        lls.append(o["log_likelihood"].cpu().numpy())
        elbos.append(o["elbo"].cpu().numpy())
    np.testing.assert_allclose(res["nll"], -np.concatenate(lls).mean(), rtol=1e-12)
    np.testing.assert_allclose(res["elbo"], np.concatenate(elbos).mean(), rtol=1e-12)
    assert math.isfinite(res["nll"]) and res["nll"] > 0
