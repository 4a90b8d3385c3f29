"""KL control, host side (no GPU): KLSchedule values, validation of the VanillaVAE keywords, the C-ABI declarations, and the
torch f64 yardstick the GPU tests (tests/test_kl_control_gpu.py) compare against.

The yardstick is torch autograd on the CPU, in float64, of
    recon + beta * torch.clamp(kl_d, min=lambda).sum()        (free bits)
    recon + beta * (KL - C).abs()                             (capacity)
over oracle.torch_cpu_step.TorchCpuStep.forward - never the code under test."""
import math
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from oracle.torch_cpu_step import TorchCpuStep
from tests.util import perturbed_params
from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_step.h")
NEW = ("vae_set_kl_objective", "vae_elbo_generic_kl", "vae_kl_per_dim")
MARGIN = 1e-2          # smallest |kl_d - lambda| / lambda a test accepts (the f32 path's error is four orders below)


# ---- yardstick helpers (imported by the GPU file) ------------------------------------------------------------------------
def kl_terms(mu, lv):
    """kl_d [L] (batch mean per dimension) and KL = sum_d kl_d of torch tensors mu, log_var [B, L]."""
    kl_bd = -0.5 * (1 + lv - mu ** 2 - torch.exp(lv))
    kl_d = kl_bd.mean(dim=0)
    return kl_d, kl_d.sum()


def choose_lambda(kl_d):
    """The fixed rule: sort kl_d, take the widest gap between neighbours within the middle half of the sorted list, lambda =
    its midpoint.  Asserts the two preconditions every test needs (dimensions on each side, relative margin >= MARGIN)."""
    s = np.sort(np.asarray(kl_d, np.float64))
    n = len(s)
    lo, hi = n // 4, n - n // 4                       # the middle half: s[lo:hi]
    assert hi - lo >= 2, "latent too small for the rule"
    gaps = s[lo + 1:hi] - s[lo:hi - 1]
    i = lo + int(np.argmax(gaps))
    lam = 0.5 * (s[i] + s[i + 1])
    check_lambda(kl_d, lam)
    return float(lam)


def check_lambda(kl_d, lam):
    k = np.asarray(kl_d, np.float64)
    below, above = int((k < lam).sum()), int((k > lam).sum())
    assert below > 0 and above > 0, (below, above)
    margin = float(np.abs(k - lam).min() / lam)
    assert margin >= MARGIN, margin
    return below, above, margin


def shaped_term(mu, lv, objective, param):
    """T of the objective on torch tensors (differentiable), and the raw KL."""
    kl_d, kl = kl_terms(mu, lv)
    if objective == "free_bits":
        return torch.clamp(kl_d, min=param).sum(), kl
    if objective == "capacity":
        return (kl - param).abs(), kl
    assert objective == "plain"
    return kl, kl


def resolve_param(kl_d, kl, objective, rule):
    """The objective's parameter from the yardstick's own kl_d / KL: free bits by the lambda rule; capacity 'lo' / 'hi' = 0.5 / 1.5 KL."""
    if objective == "free_bits":
        return choose_lambda(kl_d.detach().numpy()) if rule is None else float(rule)
    if objective == "capacity":
        return {"lo": 0.5, "hi": 1.5}[rule] * float(kl.detach()) if isinstance(rule, str) else float(rule)
    return 0.0


def cpu_kl_step(p, x, eps, beta, objective, rule=None, recon="bce"):
    """One forward + backward of the yardstick.  Returns dict(out3 = [loss, recon, -KL], xhat, grads, kl_d, kl, param, mu, lv)."""
    st = TorchCpuStep(p, kld_weight=beta, dtype=torch.float64)
    xt = torch.from_numpy(np.asarray(x, np.float64))
    xhat, mu, lv, _ = st.forward(xt, torch.from_numpy(np.asarray(eps, np.float64)))
    kl_d, kl = kl_terms(mu, lv)
    param = resolve_param(kl_d, kl, objective, rule)
    rec = F.binary_cross_entropy(xhat, xt) if recon == "bce" else F.mse_loss(xhat, xt)
    T, _ = shaped_term(mu, lv, objective, param)
    loss = rec + beta * T
    loss.backward()
    return dict(out3=[float(loss.detach()), float(rec.detach()), float(-kl.detach())], xhat=xhat.detach().numpy(), grads={k: v.grad.numpy() for k, v in st.p.items()},
                kl_d=kl_d.detach().numpy(), kl=float(kl.detach()), param=param, mu=mu.detach().numpy(), lv=lv.detach().numpy())


class KlCpuStep(TorchCpuStep):
    """TorchCpuStep whose step takes the KL weight of the step and a free-bits floor (the CPU side of the train_one_epoch test)."""

    def step(self, x, eps, beta, free_bits):
        xhat, mu, lv, z = self.forward(x, eps)
        self.opt.zero_grad()
        recon = F.binary_cross_entropy(xhat, x)
        T, kl = shaped_term(mu, lv, "free_bits", free_bits)
        loss = recon + beta * T
        loss.backward()
        self.opt.step()
        self.sched.step()
        return (float(loss.detach()), float(recon.detach()), float(-kl.detach())), kl_terms(mu.detach(), lv.detach())[0].numpy()


def synth_inputs(B, H, L, seed):
    x = vo.synth_pianoroll(B, H, seed)
    eps = vo.counter_normal(B * L, seed, 5).reshape(B, L).astype(np.float32)
    return x, eps


# ---- 1. KLSchedule ---------------------------------------------------------------------------------------------------------
def test_kl_schedule_values():
    from torch_vae_amd.train import KLSchedule
    c = KLSchedule("constant", beta=4.0)
    assert [c.value(t) for t in (0, 1, 10 ** 6)] == [4.0, 4.0, 4.0] and c.capacity(5) is None
    lin = KLSchedule("linear", beta=4.0, warmup_steps=8)
    assert lin.value(0) == 0.0 and lin.value(2) == 1.0 and lin.value(7) == 3.5
    assert lin.value(8) == 4.0 and lin.value(9) == 4.0 and lin.value(10 ** 6) == 4.0      # the step where the ramp ends, and after
    cyc = KLSchedule("cyclical", beta=2.0, period=10, ratio=0.5)
    assert cyc.value(0) == 0.0 and cyc.value(1) == pytest.approx(0.4) and cyc.value(4) == pytest.approx(1.6)
    assert cyc.value(5) == 2.0 and cyc.value(9) == 2.0                                    # flat second half of the cycle
    assert cyc.value(10) == 0.0 and cyc.value(11) == pytest.approx(0.4) and cyc.value(25) == 2.0   # cycle boundary: restart
    full = KLSchedule("cyclical", beta=2.0, period=4, ratio=1.0)
    assert [full.value(t) for t in range(5)] == [0.0, 0.5, 1.0, 1.5, 0.0]
    cap = KLSchedule("constant", beta=100.0, capacity_max=25.0, capacity_steps=1000)
    assert cap.capacity(0) == 0.0 and cap.capacity(100) == 2.5 and cap.capacity(1000) == 25.0 and cap.capacity(5000) == 25.0
    assert cap.value(123) == 100.0
    # a resumed run: a schedule built afresh from the same settings continues at total_step = t with the uninterrupted values
    for make in (lambda: KLSchedule("linear", beta=4.0, warmup_steps=8), lambda: KLSchedule("cyclical", beta=2.0, period=10),
                 lambda: KLSchedule("constant", beta=1.0, capacity_max=5.0, capacity_steps=7)):
        a = make()
        run = [(a.value(t), a.capacity(t)) for t in range(30)]
        b = make()
        assert [(b.value(t), b.capacity(t)) for t in range(13, 30)] == run[13:]


def test_kl_schedule_validation_and_config():
    from torch_vae_amd.models import VanillaVAE
    from torch_vae_amd.train import KLSchedule
    for kw in (dict(kind="cosine"), dict(kind="linear", warmup_steps=0), dict(kind="cyclical", period=0),
               dict(kind="cyclical", period=10, ratio=0.0), dict(kind="cyclical", period=10, ratio=1.5), dict(beta=-1.0),
               dict(beta=float("nan")), dict(capacity_max=-1.0, capacity_steps=10), dict(capacity_max=5.0, capacity_steps=0)):
        with pytest.raises(ValueError):
            KLSchedule(**kw)
    m = VanillaVAE(1, 16, 32, kld_weight=4.0)
    assert KLSchedule.from_config(Namespace(), m) is None                 # none of the fields: no schedule
    cfg = Namespace(kl_schedule="linear", kl_warmup_steps=10)
    s = KLSchedule.from_config(cfg, m)
    assert cfg.kl_beta == 4.0 and s.value(5) == 2.0                       # the target is stored on first use ...
    m.kld_weight = s.value(5)
    assert KLSchedule.from_config(cfg, m).value(10) == 4.0                # ... so a later epoch ramps towards the same value
    s = KLSchedule.from_config(Namespace(kl_capacity_max=8.0, kl_capacity_steps=4, kl_beta=50.0), m)
    assert s.kind == "constant" and s.value(3) == 50.0 and s.capacity(1) == 2.0


# ---- 2. constructor keywords ----------------------------------------------------------------------------------------------
def test_constructor_keywords_validate():
    from torch_vae_amd.models import VanillaVAE, _kl_objective
    m = VanillaVAE(1, 16, 32)
    assert m.kl_free_bits == 0.0 and m.kl_capacity is None
    assert _kl_objective(m.kl_free_bits, m.kl_capacity) == (_lib.KL_PLAIN, 0.0)
    assert _kl_objective(0.25, None) == (_lib.KL_FREE_BITS, 0.25) and _kl_objective(0.0, 3.0) == (_lib.KL_CAPACITY, 3.0)
    assert _kl_objective(0, 0.0) == (_lib.KL_CAPACITY, 0.0)
    m = VanillaVAE(1, 16, 32, kl_free_bits=0.5)
    assert m.kl_free_bits == 0.5
    assert VanillaVAE(1, 16, 32, kl_capacity=2.0).kl_capacity == 2.0
    for kw in (dict(kl_free_bits=0.5, kl_capacity=1.0), dict(kl_free_bits=-0.1), dict(kl_free_bits=float("nan")),
               dict(kl_free_bits=float("inf")), dict(kl_capacity=-1.0), dict(kl_capacity=float("nan")), dict(kl_free_bits="0.5")):
        with pytest.raises(ValueError):
            VanillaVAE(1, 16, 32, **kw)
    with pytest.raises(TypeError):
        VanillaVAE(1, 16, 32, None, 1.0, False, None, "bf16", "bce", None, 0.5)   # keyword-only, like recon_loss
    m.kl_capacity = 1.0                                                   # plain attributes: a bad pair is refused when it is read
    with pytest.raises(ValueError):
        _kl_objective(m.kl_free_bits, m.kl_capacity)


# ---- 3. C ABI --------------------------------------------------------------------------------------------------------------
def declared_params(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", open(HEADER).read())
    assert m, f"{name} is not declared in include/vae_step.h"
    return [re.sub(r"\s*\b\w+$", "", " ".join(p.split())).replace(" *", "*") for p in m.group(1).split(",")]


def test_new_symbols_declared_exported_and_bound():
    L = _lib.lib()
    for name in NEW:
        declared_params(name)
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(declared_params(name)), name
    hdr = open(HEADER).read()
    for macro, value in (("VAE_KL_PLAIN", _lib.KL_PLAIN), ("VAE_KL_FREE_BITS", _lib.KL_FREE_BITS), ("VAE_KL_CAPACITY", _lib.KL_CAPACITY)):
        assert re.search(r"#define " + macro + r" (\d+)", hdr).group(1) == str(value)
    assert (_lib.KL_PLAIN, _lib.KL_FREE_BITS, _lib.KL_CAPACITY) == (0, 1, 2)
    ex, kl = declared_params("vae_elbo_generic_ex"), declared_params("vae_elbo_generic_kl")
    i = ex.index("int", 8) + 1                              # behind `recon`
    assert kl[:i] == ex[:i] and kl[i:i + 2] == ["int", "double"] and kl[i + 2:] == ex[i:]
    assert declared_params("vae_set_kl_objective") == ["vae_ctx*", "int", "double"]
    assert declared_params("vae_kl_per_dim") == ["vae_ctx*", "double*", "vae_stream_t"]


def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _lib.lib()
    assert L.vae_set_kl_objective(None, _lib.KL_PLAIN, 0.0) == -1 and b"null ctx" in L.vae_last_error()
    assert L.vae_kl_per_dim(None, 4096, None) == -1 and b"vae_kl_per_dim" in L.vae_last_error()
    # fake, never dereferenced device addresses: refused before anything is enqueued
    for kind, param in ((7, 1.0), (_lib.KL_FREE_BITS, 0.0), (_lib.KL_FREE_BITS, -1.0), (_lib.KL_FREE_BITS, float("nan")),
                        (_lib.KL_CAPACITY, -0.5), (_lib.KL_CAPACITY, float("inf")), (_lib.KL_CAPACITY, float("nan"))):
        rc = L.vae_elbo_generic_kl(4096, 4096, 4096, 4096, 64, 4, 16, 1.0, _lib.RECON_BCE, kind, param, 4096, 4096, 4096, 4096, None)
        assert rc == -1 and L.vae_last_error().decode().startswith("vae_elbo_generic_kl: "), (kind, param)


# ---- 4. the yardstick itself -------------------------------------------------------------------------------------------------
def test_lambda_rule():
    lam = choose_lambda([0.01, 0.02, 0.03, 0.10, 0.11, 0.30, 0.31, 0.9])     # middle half: 0.03 .. 0.30; widest gap 0.11 -> 0.30
    assert lam == pytest.approx(0.205)
    with pytest.raises(AssertionError):
        check_lambda([0.1, 0.2, 0.3], 0.05)                                   # nothing below
    with pytest.raises(AssertionError):
        check_lambda([0.1, 0.2, 0.3], 0.2005)                                 # a tie within the margin


@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 4, False), (32, 10, 8, False)])
def test_free_bits_gradient_identity_of_the_yardstick(H, L, B, gen):
    """grad_plain(fc_mu.bias)_d - grad_fb(fc_mu.bias)_d = beta * mean_b mu_bd for dimensions below lambda and 0 above; the
    same with 0.5 (e^lv - 1) for fc_var.bias.  (The decoder-side part of both gradients is the same graph.)"""
    beta = 2.0
    p = perturbed_params(L, H, 51, gen)
    x, eps = synth_inputs(B, H, L, 52)
    plain = cpu_kl_step(p, x, eps, beta, "plain")
    fb = cpu_kl_step(p, x, eps, beta, "free_bits")
    below = plain["kl_d"] < fb["param"]
    assert 0 < below.sum() < L
    d_mu = plain["grads"]["fc_mu.bias"] - fb["grads"]["fc_mu.bias"]
    d_lv = plain["grads"]["fc_var.bias"] - fb["grads"]["fc_var.bias"]
    want_mu = np.where(below, beta * plain["mu"].mean(axis=0), 0.0)
    want_lv = np.where(below, beta * (0.5 * (np.exp(plain["lv"]) - 1.0)).mean(axis=0), 0.0)
    np.testing.assert_allclose(d_mu, want_mu, rtol=0, atol=1e-13)
    np.testing.assert_allclose(d_lv, want_lv, rtol=0, atol=1e-13)
    # T and the reported scalars
    assert fb["out3"][2] == plain["out3"][2] and fb["out3"][1] == plain["out3"][1]
    T = np.maximum(plain["kl_d"], fb["param"]).sum()
    assert fb["out3"][0] == pytest.approx(fb["out3"][1] + beta * T, rel=1e-14)
    for rule, sign in (("lo", 1.0), ("hi", -1.0)):
        cap = cpu_kl_step(p, x, eps, beta, "capacity", rule)
        np.testing.assert_allclose(cap["grads"]["fc_mu.bias"] - fb["grads"]["fc_mu.bias"],
                                   beta * plain["mu"].mean(axis=0) * (sign - np.where(below, 0.0, 1.0)), rtol=0, atol=1e-13)
        assert cap["out3"][0] == pytest.approx(cap["out3"][1] + beta * abs(plain["kl"] - cap["param"]), rel=1e-14)


def test_lambda_rule_holds_on_the_gpu_test_shapes():
    """The precondition (dimensions on both sides, margin >= 1e-2) on the yardstick's kl_d at the cheap GPU-test shapes."""
    for H, L, B, gen in ((32, 16, 32, False), (32, 10, 8, False), (32, 16, 4, False)):
        x, eps = synth_inputs(B, H, L, 52)
        st = TorchCpuStep(perturbed_params(L, H, 51, gen), dtype=torch.float64)
        with torch.no_grad():
            _, mu, lv, _ = st.forward(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(eps.astype(np.float64)))
        kl_d, kl = kl_terms(mu, lv)
        lam = choose_lambda(kl_d.numpy())
        assert math.isfinite(lam) and 0 < lam < float(kl)
