"""Differentiable encode / decode / eval-mode forwards and x.grad on the GPU (vae_encode, vae_decode, vae_backward_ex).
Yardstick: torch f64 autograd on the CPU, on the same state dict (perturbed BatchNorm affine values and running statistics)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from tests.test_loglik_gpu import model_for
from tests.path_local import LOSS_SCALE, upstream_weights
from tests.util import PRE_BN_BIAS, profile_sequence, rel_l2

pytestmark = pytest.mark.gpu

GRAD_TOL = {"f32": 5e-3, "bf16": 0.28, "f16": 0.14}   # per-tensor gradient rel-L2 against f64 (the gates of test_parity_gpu.py)
LOSS_TOL = 1e-4
# the latent-infilling trajectory (10 Adam steps on z, f32 kernels against the f64 run): max |z - z_f64| / max |z_f64|, measured
# 1.8e-6 on MI355X
INFILL_TOL = 2e-4


def _bn(a, sd, bufs, n, train):
    return F.leaky_relu(F.batch_norm(a, bufs[n + ".running_mean"], bufs[n + ".running_var"], sd[n + ".weight"], sd[n + ".bias"],
                                     training=train, momentum=0.1, eps=1e-5), 0.01)


def ref_encode(sd, bufs, x, train):
    a = x
    for i in range(4):
        n = f"encoder.{i}"
        a = _bn(F.conv2d(a, sd[n + ".0.weight"], sd[n + ".0.bias"], stride=2, padding=1), sd, bufs, n + ".1", train)
    pre = a.flatten(1)
    return F.linear(pre, sd["fc_mu.weight"], sd["fc_mu.bias"]), F.linear(pre, sd["fc_var.weight"], sd["fc_var.bias"]), pre


def ref_decode(sd, bufs, z, s, train):
    a = F.linear(z, sd["decoder_input.weight"], sd["decoder_input.bias"]).view(-1, 256, s, s)
    for n in ("decoder.0", "decoder.1", "decoder.2", "final_layer"):
        k = n + ".0" if n != "final_layer" else "final_layer.0"
        a = _bn(F.conv_transpose2d(a, sd[k + ".weight"], sd[k + ".bias"], stride=2, padding=1, output_padding=1), sd, bufs,
                n + ".1", train)
    return torch.sigmoid(F.conv2d(a, sd["final_layer.3.weight"], sd["final_layer.3.bias"], padding=1))


def ref_state(model):
    """(parameters as f64 leaves requiring grad, f64 copies of the BatchNorm buffers, bottleneck side)"""
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    params = {n: sd[n].clone().requires_grad_(True) for n, _ in model.named_parameters()}
    bufs = {k: v.clone() for k, v in sd.items() if "running" in k}
    return params, bufs, (model.img_size // 16 if model.generalised else 2)


def ref_elbo(xhat, x, mu, lv, kw):
    kld = torch.mean(-0.5 * torch.sum(1 + lv - mu ** 2 - lv.exp(), dim=1), dim=0)
    return F.binary_cross_entropy(xhat, x) + kw * kld


def grads_of(model):
    return {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in model.named_parameters()}


def bn_buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


def check_grads(got, ref_params, tol, names=None, tag="", train=False):
    for n, p in ref_params.items():
        if names is not None and n not in names:
            continue
        assert got[n] is not None, (tag, n)
        want = p.grad.numpy()
        if train and n in PRE_BN_BIAS:      # conv biases in front of a train-mode BatchNorm: analytically zero
            assert np.abs(got[n]).max() < 1e-6 and np.abs(want).max() < 1e-9, (tag, n)
            continue
        gap = rel_l2(got[n], want)
        assert gap < tol, (tag, n, gap)


def inputs(B, H, L, seed):
    x = torch.from_numpy(vo.synth_pianoroll(B, H, seed))
    eps = torch.from_numpy(vo.counter_normal(B * L, seed, 5).reshape(B, L)).float()
    return x, eps


DEC = ("decoder_input", "decoder", "final_layer")


@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 1, False), (32, 16, 5, False), (64, 16, 3, True),
                                       (32, 300, 3, False)])   # L >= 288: decin_wgrad_kernel, latent_dz over dense slabs, fc_dgrad passes
def test_eval_backward_and_input_gradient_match_torch(H, L, B, gen):
    m = model_for(H, L, gen, "f32", "bce", seed=80 + B)
    m.kld_weight = 2.0
    x, eps = inputs(B, H, L, 81 + B)
    m.eval()
    before = bn_buffers(m)
    # a grad-enabled eval forward gives the no-grad forward's outputs bit for bit
    m.set_next_eps(eps.cuda())
    with torch.no_grad():
        o0 = m(x.cuda())
    xg = x.cuda().requires_grad_(True)
    m.set_next_eps(eps.cuda())
    out = m(xg)
    assert out["output"].grad_fn is not None
    for a, b in ((o0["output"], out["output"]), (o0["encoded"]["mu"], out["encoded"]["mu"]),
                 (o0["encoded"]["log_var"], out["encoded"]["log_var"]), (o0["latents"], out["latents"])):
        assert torch.equal(a, b)
    lo = m.loss(out)["loss"]
    lo.backward()
    torch.cuda.synchronize()
    P, bufs, s = ref_state(m)
    xr = x.double().requires_grad_(True)
    mu, lv, _ = ref_encode(P, bufs, xr, False)
    z = eps.double() * torch.exp(0.5 * lv) + mu
    want = ref_elbo(ref_decode(P, bufs, z, s, False), x.double(), mu, lv, 2.0)
    want.backward()
    assert abs(lo.item() - want.item()) <= LOSS_TOL * abs(want.item())
    check_grads(grads_of(m), P, GRAD_TOL["f32"], tag="eval")
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < GRAD_TOL["f32"]
    after = bn_buffers(m)
    for k in before:
        assert torch.equal(before[k], after[k]), k


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 5, False), (64, 16, 3, True), (32, 300, 3, False)])
def test_every_upstream_gradient_and_a_loss_scale_match_torch(mode, H, L, B, gen):
    """The upstream-gradient arguments of the C ABI end to end (g_xhat, g_mu, g_lv, g_z on latents, g_pre on pre_latents in the
    reference's NCHW-flatten order, gscale != 1): the ELBO plus a random-weighted sum on each of the five outputs, times a scale that
    is no power of two, against torch f64 autograd of the same loss.  eval: x.requires_grad (vae_backward_ex, dx compared);
    train: plain vae_backward.  (tests/test_grad_paths_local_gpu.py checks the same kernels layer by layer, with formulas it shares
    with their authors; this check shares none.)"""
    train = mode == "train"
    m = model_for(H, L, gen, "f32", "bce", seed=160 + B)
    m.kld_weight = 2.5
    m.train(train)
    x, eps = inputs(B, H, L, 161 + B)
    P, bufs, s = ref_state(m)
    w = {k: torch.from_numpy(v).float() for k, v in upstream_weights("forward", H, L, B, 256 * s * s, 162).items()}

    def composite(out, elbo, cast):
        enc = out["encoded"]
        t = {"output": out["output"], "mu": enc["mu"], "log_var": enc["log_var"], "latents": out["latents"], "pre_latents": enc["pre_latents"]}
        return LOSS_SCALE * (elbo + sum((t[k] * cast(w[k])).sum() for k in w))

    xg = x.cuda().requires_grad_(not train)
    m.set_next_eps(eps.cuda())
    out = m(xg)
    lo = composite(out, m.loss(out)["loss"], lambda v: v.cuda())
    lo.backward()
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    mu, lv, pre = ref_encode(P, bufs, xr, train)
    z = eps.double() * torch.exp(0.5 * lv) + mu
    xh = ref_decode(P, bufs, z, s, train)
    ref_out = {"output": xh, "latents": z, "encoded": {"mu": mu, "log_var": lv, "pre_latents": pre}}
    want = composite(ref_out, ref_elbo(xh, x.double(), mu, lv, 2.5), lambda v: v.double())
    want.backward()
    assert abs(lo.item() - want.item()) <= LOSS_TOL * abs(want.item())
    check_grads(grads_of(m), P, GRAD_TOL["f32"], tag=mode, train=train)
    if not train:
        assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < GRAD_TOL["f32"]


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("H,B,gen,L", [(32, 3, False, 16), (64, 7, True, 16), (32, 5, False, 600)],
                         ids=["32-3-False", "64-7-True", "32-5-False-L600"])   # (L 600: decin_fwd_kernel's two z passes, decin_wgrad_kernel)
def test_decode_is_differentiable(mode, H, B, gen, L):
    m = model_for(H, L, gen, "f32", "bce", seed=90 + B)
    m.train(mode == "train")
    P, bufs, s = ref_state(m)
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, L, generator=g)
    w = torch.rand(B, 1, H, H, generator=g) - 0.3          # an arbitrary upstream gradient on xhat
    zg = z.cuda().requires_grad_(True)
    xh = m.decode(zg)
    assert xh.grad_fn is not None
    (xh * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    zr = z.double().requires_grad_(True)
    xr = ref_decode(P, bufs, zr, s, mode == "train")
    (xr * w.double()).sum().backward()
    assert rel_l2(xh.detach().cpu().numpy(), xr.detach().numpy()) < 1e-4
    assert rel_l2(zg.grad.cpu().numpy(), zr.grad.numpy()) < GRAD_TOL["f32"]
    got = grads_of(m)
    check_grads(got, P, GRAD_TOL["f32"], names={n for n in P if n.startswith(DEC)}, tag=mode, train=mode == "train")
    assert all(got[n] is None for n in P if not n.startswith(DEC))
    # train mode updates the decoder's running statistics once, as torch does; eval mode writes nothing
    sd = m.state_dict()
    for k, v in bufs.items():
        assert np.allclose(sd[k].cpu().numpy(), v.numpy(), rtol=1e-5, atol=1e-6), k
    nbt = int(sd["decoder.0.1.num_batches_tracked"])
    assert nbt == (1 if mode == "train" else 0) and int(sd["encoder.0.1.num_batches_tracked"]) == 0


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_encode_is_encoder_only_and_differentiable(mode):
    H, L, B, gen = 64, 16, 5, True
    m = model_for(H, L, gen, "f32", "bce", seed=100)
    m2 = model_for(H, L, gen, "f32", "bce", seed=100)
    for mm in (m, m2):
        mm.train(mode == "train")
    x, eps = inputs(B, H, L, 101)
    P, bufs, s = ref_state(m)
    with torch.no_grad():
        m2.set_next_eps(eps.cuda())
        full = m2(x.cuda())["encoded"]
    xg = x.cuda().requires_grad_(True)
    m._context(B)
    seq = profile_sequence(m, lambda: m.encode(x.cuda()))
    assert seq and not any(("@decoder" in e or "@final_layer" in e or "decin" in e) for e in seq), seq
    enc = m.encode(xg)
    assert torch.equal(enc["mu"], full["mu"]) and torch.equal(enc["log_var"], full["log_var"])
    g = torch.Generator().manual_seed(3)
    w1, w2 = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    ((enc["mu"] * w1.cuda()).sum() + (enc["log_var"] * w2.cuda()).sum()).backward()
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    mu, lv, _ = ref_encode(P, bufs, xr, mode == "train")
    ((mu * w1.double()).sum() + (lv * w2.double()).sum()).backward()
    got = grads_of(m)
    check_grads(got, P, GRAD_TOL["f32"], names={n for n in P if not n.startswith(DEC)}, tag=mode, train=mode == "train")
    assert all(got[n] is None for n in P if n.startswith(DEC))
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < GRAD_TOL["f32"]


def test_train_forward_input_gradient_and_unchanged_step():
    H, L, B, gen = 32, 16, 6, False
    m = model_for(H, L, gen, "f32", "bce", seed=110)
    x, eps = inputs(B, H, L, 111)
    P, bufs, s = ref_state(m)
    xg = x.cuda().requires_grad_(True)
    m.set_next_eps(eps.cuda())
    lo = m.loss(m(xg))["loss"]
    lo.backward()
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    mu, lv, _ = ref_encode(P, bufs, xr, True)
    want = ref_elbo(ref_decode(P, bufs, eps.double() * torch.exp(0.5 * lv) + mu, s, True), x.double(), mu, lv, 1.0)
    want.backward()
    check_grads(grads_of(m), P, GRAD_TOL["f32"], tag="train", train=True)
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < GRAD_TOL["f32"]
    # without x.requires_grad the input-gradient kernel is never launched
    seq = profile_sequence(m, lambda: m.loss(m(x.cuda()))["loss"].backward())
    assert any("conv1_wgrad" in e for e in seq) and not any("conv1_dgrad" in e for e in seq)
    seq = profile_sequence(m, lambda: m.fused_forward_backward(x.cuda()))
    assert not any("conv1_dgrad" in e for e in seq)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16bit_eval_decode_and_encode_gradients(dtype):
    H, L, B, gen = 64, 16, 3, True
    m = model_for(H, L, gen, dtype, "bce", seed=120)
    m.eval()
    x, eps = inputs(B, H, L, 121)
    P, bufs, s = ref_state(m)
    xg = x.cuda().requires_grad_(True)
    m.set_next_eps(eps.cuda())
    m.loss(m(xg))["loss"].backward()
    xr = x.double().requires_grad_(True)
    mu, lv, _ = ref_encode(P, bufs, xr, False)
    ref_elbo(ref_decode(P, bufs, eps.double() * torch.exp(0.5 * lv) + mu, s, False), x.double(), mu, lv, 1.0).backward()
    check_grads(grads_of(m), P, GRAD_TOL[dtype], tag=dtype)
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < GRAD_TOL[dtype]
    # decode with a sum-reduced loss: finite, within the gate
    m.zero_grad(set_to_none=True)
    P, bufs, s = ref_state(m)
    z = torch.randn(B, L, generator=torch.Generator().manual_seed(5))
    zg = z.cuda().requires_grad_(True)
    F.binary_cross_entropy(m.decode(zg), x.cuda(), reduction="sum").backward()
    zr = z.double().requires_grad_(True)
    F.binary_cross_entropy(ref_decode(P, bufs, zr, s, False), x.double(), reduction="sum").backward()
    got = grads_of(m)
    assert all(np.isfinite(v).all() for v in got.values() if v is not None) and torch.isfinite(zg.grad).all()
    check_grads(got, P, GRAD_TOL[dtype], names={n for n in P if n.startswith(DEC)}, tag=dtype + " decode")
    assert rel_l2(zg.grad.cpu().numpy(), zr.grad.numpy()) < GRAD_TOL[dtype]


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_f16_full_size_decode_is_finite_and_agrees_with_f32(reduction):
    H, L, B = 128, 16, 4
    ms = {d: model_for(H, L, True, d, "bce", seed=130) for d in ("f32", "f16")}
    x, _ = inputs(B, H, L, 131)
    z = torch.randn(B, L, generator=torch.Generator().manual_seed(7)).cuda()
    got = {}
    for d, m in ms.items():
        m.eval()
        zg = z.clone().requires_grad_(True)
        F.binary_cross_entropy(m.decode(zg), x.cuda(), reduction=reduction).backward()
        got[d] = (zg.grad.cpu().numpy(), grads_of(m))
    assert np.isfinite(got["f16"][0]).all()
    assert rel_l2(got["f16"][0], got["f32"][0]) < GRAD_TOL["f16"]
    for n, g in got["f32"][1].items():
        if g is not None:
            assert np.isfinite(got["f16"][1][n]).all(), n
            assert rel_l2(got["f16"][1][n], g) < GRAD_TOL["f16"], n


def test_latent_infilling_with_a_frozen_eval_model():
    H, L, B, gen = 32, 16, 3, False
    m = model_for(H, L, gen, "f32", "bce", seed=140)
    m.eval()
    m.requires_grad_(False)
    before = bn_buffers(m)
    P, bufs, s = ref_state(m)
    P = {k: v.detach() for k, v in P.items()}
    x, _ = inputs(B, H, L, 141)
    mask = torch.zeros(B, 1, H, H)
    mask[..., : H // 2] = 1.0                                # the left half of the roll is known
    z0 = 0.5 * torch.randn(B, L, generator=torch.Generator().manual_seed(9))

    def run(decode, z, xt, mk):
        opt = torch.optim.Adam([z], lr=0.05)
        traj = []
        for _ in range(10):
            opt.zero_grad()
            xh = decode(z)
            (F.binary_cross_entropy(xh, xt, reduction="none") * mk).sum().div(mk.sum()).backward()
            opt.step()
            traj.append(z.detach().cpu().double().numpy().copy())
        return np.stack(traj)

    zg = z0.clone().cuda().requires_grad_(True)
    got = run(m.decode, zg, x.cuda(), mask.cuda())
    zr = z0.clone().double().requires_grad_(True)
    want = run(lambda z: ref_decode(P, bufs, z, s, False), zr, x.double(), mask.double())
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"latent infilling: max |z - z_f64| / max |z_f64| = {err:.3e}")
    assert err < INFILL_TOL, err
    assert all(p.grad is None for p in m.parameters())
    after = bn_buffers(m)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_stale_decode_graph_raises():
    H, L, B = 32, 16, 2
    m = model_for(H, L, False, "f32", "bce", seed=150)
    m.eval()
    z = torch.randn(B, L, device="cuda", requires_grad=True)
    xh = m.decode(z)
    m(torch.from_numpy(vo.synth_pianoroll(B, H, 3)).cuda())
    with pytest.raises(RuntimeError, match="no longer the model's last"):
        xh.sum().backward()
