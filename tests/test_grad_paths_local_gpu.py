"""Layer-local parity of the backwards outside the training step (vae_encode / vae_decode / vae_backward_ex after a forward in train
or eval mode, and vae_backward with every upstream gradient): each stored gradient and each parameter gradient recomputed on the CPU
from the tensors the device stored one layer earlier (tests/util.py: path_local_recompute, proven exact on an f64 reference run in
tests/test_grad_paths_local_host.py), at the gates of test_every_kernel_against_oracle_on_its_own_inputs."""
import math

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.test_grad_paths_gpu import bn_buffers, grads_of
from tests.test_loglik_gpu import model_for, rolls
from tests.test_parity_gpu import KERNEL_VARIANTS, report
from tests.path_local import LOSS_SCALE, layer_shapes, path_local_gaps, path_local_recompute, path_params, upstream_of, upstream_weights
from tests.util import fetch_debug_tensor

pytestmark = pytest.mark.gpu

GATE = {"f32": 1e-5, "bf16": 5e-4, "f16": 5e-4}     # relative L2 per tensor: the layer-local gates of test_parity_gpu.py, unchanged
ZERO_GATE = 1e-6                                    # max |gradient| of a conv bias in front of a train-mode BatchNorm (the kernels write 0)
KLD_WEIGHT = 2.5


def _f16_upstream_exponent(up, B, H):
    """The second power of two of VanillaVAE._run_backward_ex (f16 storage), restated from its documented rule: the upstream
    gradients are multiplied by 2^-e, e = ceil(log2(the largest upstream magnitude relative to the standard ELBO's)) - a gradient on
    xhat weighted by B*H*W, one on a latent tensor by B, the loss scale by 1."""
    npix = float(B * H * H)
    # (the products in f32, as the model forms them on the device: next to a power of two an f64 product could land on its other side)
    mags = [np.abs(np.asarray(up[k], np.float32)).max() * np.float32(f) for k, f in (("g_xhat", npix), ("g_mu", B), ("g_lv", B), ("g_z", B), ("g_pre", B))
            if up.get(k) is not None]
    if up.get("gscale") is not None:
        mags.append(np.abs(np.float32(up["gscale"])))
    m = float(max(mags))
    return int(math.ceil(math.log2(m))) if m > 0 and math.isfinite(m) else 0


def _path_local_gaps(kind, train, dtype, H, L, B, gen, recon="bce", opts=None, warm=None, seed=71):
    """One pass of `kind` ("forward" / "encode" / "decode") through the model's Python surface (m(x), m.encode, m.decode, autograd,
    x.requires_grad) in train or eval mode on perturbed parameters and running statistics, with a loss that puts a gradient on every
    output of the path (tests/util.py: upstream_weights) times a scale that is no power of two; then every tensor the backward stored
    (vae_debug_tensor 0..18) and wrote against its layer-local recomputation.  Returns ({tensor: relative L2 gap}, {train-mode pre-BN
    conv bias: max |gradient|}).  warm: batch of a larger pass run first, so the context is sized for more than B."""
    from torch_vae_amd import _lib
    m = model_for(H, L, gen, dtype, recon, seed=seed)
    m.kld_weight = KLD_WEIGHT
    for k, v in (opts or {}).items():
        _lib.check(_lib.lib().vae_set_option(m._context(max(B, warm or 0)).handle, k.encode(), v), "set " + k)
    shapes, s = layer_shapes(H, B, gen)
    Fdim = 256 * s * s
    if warm:
        assert warm > B
        with torch.no_grad():
            m.eval()
            if kind == "decode":
                m.decode(torch.randn(warm, L, generator=torch.Generator().manual_seed(1)).cuda())
            else:
                m(torch.from_numpy(rolls(warm, H, seed + 1, recon)).cuda())
    m.train(train)
    p = {n: v.detach().cpu().double().numpy() for n, v in m.named_parameters()}
    before = bn_buffers(m)
    bn = {k: v.double().cpu().numpy() for k, v in before.items() if "running" in k}
    x = rolls(B, H, seed + 2, recon)
    eps = vo.counter_normal(B * L, seed + 2, 5).reshape(B, L).astype(np.float32)
    zin = np.random.default_rng(seed + 3).standard_normal((B, L)).astype(np.float32)
    weights = {k: v.astype(np.float32) for k, v in upstream_weights(kind, H, L, B, Fdim, seed + 4).items()}
    W = {k: torch.from_numpy(v).cuda() for k, v in weights.items()}
    dev = {}
    # ---- the pass and its backward, through the model's own surface
    want_dx = kind == "encode" or (kind == "forward" and not train)     # train-mode forward: plain vae_backward, no input gradient
    if kind == "decode":
        zg = torch.from_numpy(zin).cuda().requires_grad_(True)
        xh = m.decode(zg)
        (LOSS_SCALE * (xh * W["xhat"]).sum()).backward()
        dev.update(z=zin, xhat=xh.detach())
    else:
        xg = torch.from_numpy(x).cuda().requires_grad_(want_dx)
        if kind == "encode":
            enc = m.encode(xg)
            terms = {"mu": enc["mu"], "log_var": enc["log_var"], "pre_latents": enc["pre_latents"]}
            loss = sum((terms[k] * W[k]).sum() for k in W)
        else:
            m.set_next_eps(torch.from_numpy(eps).cuda())
            out = m(xg)
            enc = out["encoded"]
            terms = {"output": out["output"], "mu": enc["mu"], "log_var": enc["log_var"], "latents": out["latents"],
                     "pre_latents": enc["pre_latents"]}
            loss = m.loss(out)["loss"] + sum((terms[k] * W[k]).sum() for k in W)
            dev.update(eps=eps, z=out["latents"].detach(), xhat=out["output"].detach())
        (LOSS_SCALE * loss).backward()
        dev.update(x=x, mu=enc["mu"].detach(), lv=enc["log_var"].detach())
    torch.cuda.synchronize()
    if warm:
        assert m._ctx.key[2] == warm
    up = upstream_of(weights, np.float32(LOSS_SCALE), kind == "forward")
    up = {k: (None if v is None else np.asarray(v, np.float32).astype(np.float64)) for k, v in up.items()}     # (what autograd hands over, in f32)
    # ---- what the device stored
    gs = 1.0
    if dtype == "f16":
        gs = vo.f16_grad_scale(B, H)
        if not (kind == "forward" and train):           # vae_backward_ex: the upstream rescaling of _run_backward_ex on top
            gs *= 2.0 ** -_f16_upstream_exponent(up, B, H)
    layers = {"forward": range(8), "encode": range(4), "decode": range(4, 8)}[kind]
    dev["Y"] = {i: fetch_debug_tensor(m, i, shapes[i]) for i in layers}
    dev["DZ"] = {i: fetch_debug_tensor(m, 8 + i, shapes[i], gs) for i in layers}
    if kind != "encode":
        dev["d0"], dev["dd0"] = fetch_debug_tensor(m, 16, (B, 256, s, s)), fetch_debug_tensor(m, 17, (B, 256, s, s), gs)
    if kind != "decode":
        dev["dlat"] = fetch_debug_tensor(m, 18, (B, 2 * L), gs)
        dev["dx"] = xg.grad if want_dx else None
    else:
        dev["dz"] = zg.grad
    dev = {k: (v.double().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v)
           for k, v in dev.items()}
    grads = grads_of(m)
    # ---- untouched state: parameters the path does not write, BatchNorm buffers in eval mode
    names = path_params(kind)
    assert all(grads[n] is not None for n in names) and all(grads[n] is None for n in p if n not in names)
    if not train:
        after = bn_buffers(m)
        for k in before:
            assert torch.equal(before[k], after[k]), k
    store = None if dtype == "f32" else dtype
    want = path_local_recompute(kind, train, p, bn, dev, up, H, L, B, gen, storage=store, fma=dtype, gscale_store=gs,
                                kld_weight=KLD_WEIGHT, recon=recon)
    gaps, zero = path_local_gaps(kind, train, want, dev, grads)
    n_stored = {"forward": 8 + 2 + int(want_dx), "encode": 4 + 2, "decode": 4 + 2}[kind]      # dz_l, (dd0, dlat) / (dd0, dz), dx
    assert len(gaps) + len(zero) == len(names) + n_stored and len(zero) == (len(names) // 5 if train else 0)
    return gaps, zero


def _check(tag, kind, train, dtype, H, L, B, gen, **kw):
    gaps, zero = _path_local_gaps(kind, train, dtype, H, L, B, gen, **kw)
    worst = max(gaps, key=gaps.get)
    print(f"{tag} {kind} {'train' if train else 'eval'} {dtype} {H}x{H} L{L} B{B}: worst {gaps[worst]:.3e} ({worst}), "
          f"zero-gradient biases {max(zero.values(), default=0.0):.1e}")
    report(test=tag, kind=kind, train=train, dtype=dtype, img=H, latent=L, batch=B, worst=worst, worst_gap=gaps[worst], gaps=gaps,
           zero=zero, **{k: v for k, v in kw.items() if k != "seed"})
    bad = {k: v for k, v in gaps.items() if not v < GATE[dtype]}
    assert not bad, bad
    assert all(v < ZERO_GATE for v in zero.values()), zero


BOTH = ("bf16", "f16")
# eval-mode forward: the ELBO (kld_weight 2.5) plus a weighted sum on each of output, mu, log_var, latents and pre_latents, times 1.7,
# with x.requires_grad - vae_backward_ex with g_xhat, gscale, g_mu, g_lv, g_z, g_pre and dx all present
FWD_EVAL = ([(d, H, L, B, gen, "bce") for d in ("bf16", "f16", "f32") for H, L, B, gen in ((32, 16, 6, False), (64, 16, 5, True), (128, 16, 3, True))]
            # one image at every size; ragged batches
            + [(d, H, 16, B, gen, "bce") for d in BOTH for H, B, gen in ((32, 1, False), (128, 1, True), (256, 1, True), (32, 33, False), (64, 48, True))]
            # latent sizes across the fc_dgrad8 / fc_dgrad / MFMA switch (64, 128), the weight-gradient switches (144, 287) and the
            # multi-pass staging (256, 512), up to the largest the library takes: g_pre enters a different kernel on each side
            + [(d, 32, L, B, False, "bce") for d in BOTH for L, B in ((1, 3), (3, 9), (40, 6), (65, 5), (145, 7), (288, 5), (600, 3), (4096, 2))]
            # conv1_dgrad_kernel with more than 2048 iterations: its grid-stride loop
            + [(d, H, 16, B, True, "bce") for d in BOTH for H, B in ((128, 40), (256, 9))]
            + [("bf16", 64, 16, 5, True, "mse")])


@pytest.mark.parametrize("dtype,H,L,B,gen,recon", FWD_EVAL)
def test_eval_forward_backward_kernels_on_their_own_inputs(dtype, H, L, B, gen, recon):
    """51 tensors per case - dz_0..7, dd0, the latent gradient, dx and all 40 parameter gradients (the eight pre-BN conv biases
    included: non-zero in eval mode) - each within 5e-4 (16-bit) / 1e-5 (f32) relative L2 of the recomputation on the device's own
    stored inputs; the BatchNorm buffers bit-unchanged.  Measured on MI355X over the 40 cases: worst 1.5e-4 (16-bit: dz3, bf16 latent 4096) / 6.1e-7 (f32: dd0); the f32-output kernels far
    below - dx 1.1e-7, the latent gradient 7.0e-8, the eval-mode conv biases 1.7e-7."""
    _check("path_local_eval_forward", "forward", False, dtype, H, L, B, gen, recon=recon)


@pytest.mark.parametrize("dtype,H,L,B,gen", [("bf16", 64, 16, 5, True), ("f16", 128, 16, 3, True), ("f32", 32, 16, 6, False),
                                             ("bf16", 32, 300, 7, False)])
def test_train_forward_backward_with_every_upstream_gradient(dtype, H, L, B, gen):
    """The same loss on a train-mode forward without x.requires_grad: plain vae_backward with all five upstream gradients and a
    loss scale.  50 tensors; the eight pre-BN conv biases by their absolute bound.  Measured on MI355X: worst 3.1e-4 (16-bit: dz1,
    bf16 latent 300 batch 7) / 5.1e-7 (f32: dd0); the biases exactly 0."""
    _check("path_local_train_forward", "forward", True, dtype, H, L, B, gen)


ENCODE = ([(d, H, L, B, gen) for d in BOTH for H, L, B, gen in ((64, 16, 5, True), (32, 145, 3, False))]
          + [("f32", 64, 16, 5, True), ("bf16", 128, 16, 1, True), ("f16", 128, 16, 1, True)])


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("dtype,H,L,B,gen", ENCODE)
def test_encode_backward_kernels_on_their_own_inputs(dtype, H, L, B, gen, train):
    """m.encode with terms on mu, log_var and pre_latents and x.requires_grad: dz_0..3, the latent gradient, dx and the 20 encoder /
    fc parameter gradients; the decoder's parameters keep grad None.  Measured on MI355X: eval worst 3.2e-5 (16-bit: dz0) / 4.3e-7
    (f32), train 7.5e-5 (dz0) / 4.8e-7; dx at most 1.1e-7."""
    _check("path_local_encode", "encode", train, dtype, H, L, B, gen)


DECODE = ([(d, H, L, B, gen) for d in BOTH for H, L, B, gen in ((64, 16, 7, True), (128, 16, 1, True), (32, 600, 5, False))]
          + [("f32", 64, 16, 7, True)])


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("dtype,H,L,B,gen", DECODE)
def test_decode_backward_kernels_on_their_own_inputs(dtype, H, L, B, gen, train):
    """m.decode(z) with an O(1)-weighted sum on xhat (in the f16 mode the upstream rescaling of _run_backward_ex is at work: 2^-e
    with e around 13 .. 16): dz_4..7, dd0, dz and the 20 decoder parameter gradients; the encoder's parameters keep grad None.
    Measured on MI355X: eval worst 2.7e-5 (16-bit: dz4) / 5.9e-7 (f32: dd0), train 7.3e-5 (dd0, f16 latent 600) / 5.7e-7; dz at
    most 6.4e-7."""
    _check("path_local_decode", "decode", train, dtype, H, L, B, gen)


@pytest.mark.parametrize("dtype", BOTH)
def test_decode_backward_at_the_largest_latent_size(dtype):
    """latent 4096 in eval mode: decin_wgrad_kernel and latent_dz_kernel over the widest slabs.  Measured on MI355X: worst 3.4e-6 (bf16) /
    2.1e-5 (f16)."""
    _check("path_local_decode", "decode", False, dtype, 32, 4096, 2, False)


def test_decode_backward_on_a_context_sized_for_a_larger_batch():
    """A decode of 3 after a decode of 40 on the same model: the backward's launch plans follow the batch of the pass, not the
    context's capacity.  Measured on MI355X: worst 1.5e-5 (dz6)."""
    _check("path_local_decode_reused_context", "decode", False, "f16", 64, 16, 3, True, warm=40)


PATH_VARIANTS = [o for o in KERNEL_VARIANTS if o in ({"use_fused_wgrad": 0}, {"use_pipelined": 0}, {"use_latent_mfma": 0, "use_fc_dgrad8": 0},
                                                    {"use_latent_mfma": 15}, {"use_side_stream": 0, "use_fused_bn": 0})]


@pytest.mark.parametrize("vi", range(len(PATH_VARIANTS)), ids=["+".join(f"{k}={v}" for k, v in o.items()) for o in PATH_VARIANTS])
def test_eval_forward_backward_kernel_variants(vi):
    """The eval forward's backward with the library switched to the alternative kernels that take the BNF_NONE coefficient route or
    g_pre differently: separate input / weight gradient kernels, one tile per workgroup, the latent block on the VALU kernels and
    on the exact-f32 MFMA, one stream with standalone BatchNorm finalisation.  Measured on MI355X: worst 3.1e-5 (dd0) over the five."""
    assert len(PATH_VARIANTS) == 5
    _check("path_local_eval_forward_variant", "forward", False, "bf16", 128, 16, 9, True, opts=PATH_VARIANTS[vi])
