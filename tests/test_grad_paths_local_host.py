"""The CPU side of the layer-local check of vae_backward_ex (tests/test_grad_paths_local_gpu.py), without a GPU: the eval-mode
BatchNorm backward of the oracle against torch f64 autograd, and the layer-local recomputation itself fed with the tensors an f64
reference run stores - the proof that the reference alone stays far inside the gate it imposes on the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo
from tests.test_grad_paths_gpu import ref_decode, ref_elbo, ref_encode
from tests.path_local import LAYERS, LOSS_SCALE, path_local_gaps, path_local_recompute, path_params, upstream_of, upstream_weights
from tests.util import PRE_BN_BIAS, perturbed_params, rel_l2

SELF_TOL = 1e-10        # recomputation on the reference's own stored tensors against those tensors
AUTOGRAD_TOL = 1e-9     # assembled gradients against torch f64 autograd over ref_encode / ref_decode


@pytest.mark.parametrize("shape", [(2, 5, 4, 4), (3, 32, 8, 8), (1, 7, 1, 1)])
def test_bn_eval_bwd_matches_torch_autograd(shape):
    """bn_eval_bwd against autograd of conv bias -> F.batch_norm(training=False): dy, dgamma, dbeta and the bias of the conv in front
    (non-zero in eval mode only)."""
    g = torch.Generator().manual_seed(shape[1])
    B, C = shape[:2]
    y0 = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
    cb = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    rm = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    rv = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    dz = torch.randn(shape, generator=g, dtype=torch.float64)
    y = y0 + cb.view(1, -1, 1, 1)
    y.retain_grad()
    out = F.batch_norm(y, rm.clone(), rv.clone(), gamma, beta, training=False, eps=1e-5)
    (out * dz).sum().backward()
    dy, dgam, dbet, dcb = vo.bn_eval_bwd(dz.numpy(), y.detach().numpy(), gamma.detach().numpy(), rm.numpy(), rv.numpy())
    for got, want in ((dy, y.grad), (dgam, gamma.grad), (dbet, beta.grad), (dcb, cb.grad)):
        assert rel_l2(got, want.numpy()) < 1e-13
    # the forward it differentiates is the oracle's own
    assert rel_l2(vo.bn_eval_fwd(y.detach().numpy(), gamma.detach().numpy(), beta.detach().numpy(), rm.numpy(), rv.numpy()),
                  out.detach().numpy()) < 1e-13
    assert np.abs(dcb).max() > 0


def reference_state(H, L, gen, seed):
    p = perturbed_params(L, H, seed, gen)
    rng = np.random.default_rng(seed + 1)
    bn = {}
    for i, n in enumerate(LAYERS):
        C = p[n + ".1.weight"].shape[0]
        bn[n + ".1.running_mean"] = 0.2 * rng.standard_normal(C)
        bn[n + ".1.running_var"] = 0.5 + rng.uniform(size=C)
    return p, bn


def captured_run(kind, train, P, bufs, s, x, eps, z_in, weights, kld_weight, recon):
    """The path in torch f64 with every tensor the device stores kept: y_l, the gradient on each BatchNorm output (dz_l), d0 / dd0,
    the total gradient on mu | log_var (dlat), dx, dz.  Returns (dev, loss)."""
    Y, ZB = {}, {}

    def block(i, a):
        n = LAYERS[i]
        if i < 4:
            y = F.conv2d(a, P[n + ".0.weight"], P[n + ".0.bias"], stride=2, padding=1)
        else:
            y = F.conv_transpose2d(a, P[n + ".0.weight"], P[n + ".0.bias"], stride=2, padding=1, output_padding=1)
        zb = F.batch_norm(y, bufs[n + ".1.running_mean"], bufs[n + ".1.running_var"], P[n + ".1.weight"], P[n + ".1.bias"],
                          training=train, momentum=0.1, eps=1e-5)
        y.retain_grad(); zb.retain_grad()
        Y[i], ZB[i] = y, zb
        return F.leaky_relu(zb, 0.01)

    W = {k: torch.from_numpy(v) for k, v in weights.items()}
    t = {}
    loss = 0.0
    if kind != "decode":
        a = x
        for i in range(4):
            a = block(i, a)
        t["pre_latents"] = a.flatten(1)
        t["mu"] = F.linear(t["pre_latents"], P["fc_mu.weight"], P["fc_mu.bias"])
        t["log_var"] = F.linear(t["pre_latents"], P["fc_var.weight"], P["fc_var.bias"])
        t["mu"].retain_grad(); t["log_var"].retain_grad()
        z = None
        if kind == "forward":
            z = t["latents"] = eps * torch.exp(0.5 * t["log_var"]) + t["mu"]
    else:
        z = z_in
    if kind != "encode":
        d0 = F.linear(z, P["decoder_input.weight"], P["decoder_input.bias"])
        d0.retain_grad()
        a = d0.view(-1, 256, s, s)
        for i in range(4, 8):
            a = block(i, a)
        xhat = torch.sigmoid(F.conv2d(a, P["final_layer.3.weight"], P["final_layer.3.bias"], padding=1))
        t["output"] = t["xhat"] = xhat
    if kind == "forward":
        kld = torch.mean(-0.5 * torch.sum(1 + t["log_var"] - t["mu"] ** 2 - t["log_var"].exp(), dim=1), dim=0)
        rec = F.mse_loss(xhat, x.detach()) if recon == "mse" else F.binary_cross_entropy(xhat, x.detach())
        loss = rec + kld_weight * kld
    loss = LOSS_SCALE * (loss + sum((t[k] * w).sum() for k, w in W.items()))
    loss.backward()
    n64 = lambda v: v.detach().numpy().astype(np.float64)    # noqa: E731
    dev = {"Y": {i: n64(v) for i, v in Y.items()}, "DZ": {i: n64(v.grad) for i, v in ZB.items()}}
    if kind != "decode":
        dev.update(x=n64(x), dx=n64(x.grad), mu=n64(t["mu"]), lv=n64(t["log_var"]),
                   dlat=np.concatenate([n64(t["mu"].grad), n64(t["log_var"].grad)], axis=1))
    if kind != "encode":
        dev.update(d0=n64(d0).reshape(-1, 256, s, s), dd0=n64(d0.grad).reshape(-1, 256, s, s), z=n64(z), xhat=n64(xhat))
    if kind == "forward":
        dev["eps"] = n64(eps)
    if kind == "decode":
        dev["dz"] = n64(z_in.grad)
    return dev, loss


@pytest.mark.parametrize("H,L,B,gen", [(32, 16, 3, False), (64, 5, 2, True)])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("kind,recon", [("forward", "bce"), ("forward", "mse"), ("encode", "bce"), ("decode", "bce")])
def test_layer_local_recomputation_is_exact_on_the_reference(kind, recon, train, H, L, B, gen):
    """path_local_recompute with storage=None on the tensors an f64 reference run stores, for every path and mode with every
    upstream gradient present: each recomputed tensor within 1e-10 of the stored one, and the assembled parameter gradients, dx and
    dz within 1e-9 of torch f64 autograd over ref_encode / ref_decode.  Measured: worst 6.2e-14 / 6.2e-14 (train mode; 2.4e-15 in eval mode)."""
    p, bn = reference_state(H, L, gen, 7)
    s = H // 16 if gen else 2
    Fdim = 256 * s * s
    kw = 2.5
    x = vo.synth_pianoroll(B, H, 31).astype(np.float64)
    if recon == "mse":
        x = x * np.random.default_rng(3).uniform(0.2, 1.0, x.shape)
    eps = vo.counter_normal(B * L, 31, 5).reshape(B, L)
    zin = np.random.default_rng(5).standard_normal((B, L))
    weights = upstream_weights(kind, H, L, B, Fdim, 11)
    leaves = lambda: ({k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in p.items()},       # noqa: E731
                      {k: torch.from_numpy(v.copy()) for k, v in bn.items()},
                      torch.from_numpy(x.copy()).requires_grad_(True), torch.from_numpy(zin.copy()).requires_grad_(True))
    P, bufs, xt, zt = leaves()
    dev, loss = captured_run(kind, train, P, bufs, s, xt, torch.from_numpy(eps), zt, weights, kw, recon)
    grads = {k: (None if v.grad is None else v.grad.numpy()) for k, v in P.items()}
    want = path_local_recompute(kind, train, p, bn, dev, upstream_of(weights, LOSS_SCALE, kind == "forward"), H, L, B, gen,
                                kld_weight=kw, recon=recon)
    names = path_params(kind)
    assert len(names) == (40 if kind == "forward" else 20) and all(n in want for n in names)
    assert all(grads[n] is None for n in p if n not in names)
    gaps, zero = path_local_gaps(kind, train, want, dev, grads)
    assert len(gaps) + len(zero) == len(want)
    worst = max(gaps, key=gaps.get)
    print(f"{kind} train={train}: worst self-consistency gap {gaps[worst]:.2e} ({worst})")
    assert gaps[worst] < SELF_TOL, {k: v for k, v in gaps.items() if not v < SELF_TOL}
    assert len(zero) == (0 if not train else 8 if kind == "forward" else 4) and all(v < 1e-9 for v in zero.values()), zero   # (torch's own cancellation residue)
    # the same loss through ref_encode / ref_decode: the assembled gradients are torch autograd's
    P2, bufs2, x2, z2 = leaves()
    W = {k: torch.from_numpy(v) for k, v in weights.items()}
    if kind == "decode":
        l2 = LOSS_SCALE * (ref_decode(P2, bufs2, z2, s, train) * W["xhat"]).sum()
    else:
        mu, lv, pre = ref_encode(P2, bufs2, x2, train)
        l2 = (mu * W["mu"]).sum() + (lv * W["log_var"]).sum() + (pre * W["pre_latents"]).sum()
        if kind == "forward":
            z = torch.from_numpy(eps) * torch.exp(0.5 * lv) + mu
            xh = ref_decode(P2, bufs2, z, s, train)
            if recon == "mse":
                kld = torch.mean(-0.5 * torch.sum(1 + lv - mu ** 2 - lv.exp(), dim=1), dim=0)
                elbo = F.mse_loss(xh, x2.detach()) + kw * kld
            else:
                elbo = ref_elbo(xh, x2.detach(), mu, lv, kw)
            l2 = l2 + elbo + (xh * W["output"]).sum() + (z * W["latents"]).sum()
        l2 = LOSS_SCALE * l2
    l2.backward()
    assert abs(l2.item() - loss.item()) <= 1e-12 * abs(loss.item())
    auto = {n: rel_l2(want[n], P2[n].grad.numpy()) for n in names if not (train and n in PRE_BN_BIAS)}
    auto["dz" if kind == "decode" else "dx"] = (rel_l2(want["dz"], z2.grad.numpy()) if kind == "decode"
                                                 else rel_l2(want["dx"], x2.grad.numpy()))
    worst = max(auto, key=auto.get)
    print(f"{kind} train={train}: worst gap to torch autograd {auto[worst]:.2e} ({worst})")
    assert auto[worst] < AUTOGRAD_TOL, {k: v for k, v in auto.items() if not v < AUTOGRAD_TOL}


def test_a_misrouted_upstream_gradient_is_far_outside_the_gate():
    """The weights of upstream_weights make every upstream gradient count: dropping any one of them, or reading g_pre in the
    kernels' NHWC order instead of the reference's NCHW-flatten order, moves the tensor it enters by more than 100x the 5e-4 gate."""
    H, L, B, gen, kw = 32, 16, 3, False, 2.5
    p, bn = reference_state(H, L, gen, 7)
    s, Fdim = 2, 1024
    x = vo.synth_pianoroll(B, H, 31).astype(np.float64)
    eps = vo.counter_normal(B * L, 31, 5).reshape(B, L)
    weights = upstream_weights("forward", H, L, B, Fdim, 11)
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in p.items()}
    bufs = {k: torch.from_numpy(v.copy()) for k, v in bn.items()}
    dev, _ = captured_run("forward", False, P, bufs, s, torch.from_numpy(x).requires_grad_(True), torch.from_numpy(eps), None,
                          weights, kw, "bce")
    grads = {k: v.grad.numpy() for k, v in P.items()}
    up = upstream_of(weights, LOSS_SCALE, True)
    hit = {"g_xhat": "dz7", "g_mu": "dlat", "g_lv": "dlat", "g_z": "dlat", "g_pre": "dz3", "gscale": "dlat"}
    for k, tensor in hit.items():
        bad = dict(up)
        bad[k] = None if k != "gscale" else 1.0
        gaps, _ = path_local_gaps("forward", False, path_local_recompute("forward", False, p, bn, dev, bad, H, L, B, gen, kld_weight=kw),
                                  dev, grads)
        assert gaps[tensor] > 0.05, (k, gaps[tensor])
    bad = dict(up)
    bad["g_pre"] = up["g_pre"].reshape(B, 256, s * s).transpose(0, 2, 1).reshape(B, Fdim)      # NHWC order
    gaps, _ = path_local_gaps("forward", False, path_local_recompute("forward", False, p, bn, dev, bad, H, L, B, gen, kld_weight=kw),
                              dev, grads)
    assert gaps["dz3"] > 0.05, gaps["dz3"]
