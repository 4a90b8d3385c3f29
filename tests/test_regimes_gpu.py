"""The layer-local gate (tests/test_parity_gpu.py: _layer_local_gaps, 54 tensors per case) outside the data every other GPU test
uses: velocity-valued rolls with a silent and a full image (fractional BCE targets, an x no 16-bit type holds exactly),
trained-like parameters (negative and dead BatchNorm gammas, channels on one LeakyReLU branch, conv rows 32x apart, fc_var biases
down to -8), the reference's shipped kld_weight 0.00025 and 0 - and, after every step, the ELBO scalars recomputed in f64 from the
GPU's own x_hat / mu / log_var and the padding of the flat buffers, which must stay exactly zero.  tests/test_regimes_host.py
pins the regimes (oracle against torch f64, conditioning) and shows on three wrong kernels restated on the oracle that these cases
can fail where the default data cannot.

Measured on MI355X, worst of the 54 tensors over the four shapes (gate 1e-5 for f32, 5e-4 for the 16-bit modes):
    regime             f32                          bf16                 f16
    velocity           1.0e-6 (encoder.0.0.weight)  5.05e-4 (dz2) *      5.3e-5 (y3)
    trained            6.6e-6 (encoder.0.0.weight)  6.25e-4 (dz2) *      6.1e-5 (y3)
    velocity+trained   5.3e-6 (encoder.0.0.weight)  1.2e-4 (dz1)         6.4e-5 (dz2)
    the three variants on velocity+trained: 1.2e-4 (bf16, dz1), 6.4e-5 (f16, dz2); kld_weight 0.00025 / 0: 8.6e-5 / 1.9e-4 (bf16),
    3.6e-5 / 3.9e-5 (f16), 5.5e-7 (f32).  ELBO scalars within 8.5e-8 of the f64 recomputation in every case; the padding exactly 0
    in every case.  Every tensor of every case: profiles/regime_layer_local_parity.txt.

The two figures above the gate, dz2 in bf16 at 32x32 / latent 3 / batch 9, are one staged operand each.  dz2 is what encoder.3's
input-gradient kernel stores; its operand dy = dz*k0 + (y*k1 + k2) is formed in f32 and rounded to bf16, the emulation rounds the
f64 value.  On the GPU's own stored inputs, dy[2, 186, 0, 0] (velocity) lies 7.3e-8 relative from a bf16 tie and dy[2, 74, 0, 1]
(trained) 2.1e-8 - inside the f32 evaluation's error bound, the f32 formula lands exactly on the tie in the second case - and the
kernel rounds to the other neighbour.  Rounding that one operand the other way in the emulation reproduces the GPU's dz2 to 2 resp.
1 of 18432 elements (118 resp. 232 differed before).  One operand weighs this much because the tensor is tiny and image 2 carries
the largest gradient; the same flip on the default data is worth 1.9e-4.  So the arithmetic is legitimate, and per the rule for
such cases that one tensor, in those two cases only, is gated at twice the f32 restatement's own gap: restated_f32_gap_dz2 flips,
one at a time, every operand whose rounding f32 does not determine and takes the largest move of dz2 - 5.15e-4 (velocity) and
6.25e-4 (trained), so the gates are 1.03e-3 and 1.25e-3.  It runs on the CPU from the kernel's stored inputs, never from the GPU's dz2.
"""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from tests.regimes import REGIMES, SHAPES, padding_mask, regime_inputs
from tests.test_parity_gpu import KERNEL_VARIANTS, _layer_local_gaps, report
from tests.util import make_model, perturbed_params

pytestmark = pytest.mark.gpu
GATE = {"f32": 1e-5, "bf16": 5e-4, "f16": 5e-4}          # the layer-local gate
ELBO_TOL = {"f32": 1e-5, "bf16": 2e-4, "f16": 2e-4}      # test_full_size_properties' tolerances for the recomputed scalars
# The one tensor whose gate is not the project's: dz2 in these two cases is gated at twice the f32 restatement's own gap
# (restated_f32_gap_dz2, evaluated at run time on the kernel's stored inputs; 5.15e-4 and 6.25e-4 - see the module docstring).
RESTATED_DZ2 = {("velocity", "bf16", 32, 3, 9), ("trained", "bf16", 32, 3, 9)}


def _optimised_norm(m):
    """f64 norm of the gradients FusedAdamW updates (encoder and decoder), over the tensors alone: no padding."""
    from torch_vae_amd import _lib
    g = m.flat_grads().double().cpu().numpy()
    sq = [float((g[o:o + n] ** 2).sum()) for nm, o, n in zip(_lib.PARAM_NAMES, m._offs, m._sizes) if nm.startswith(("encoder.", "decoder."))]
    assert len(sq) == 28
    return math.sqrt(sum(sq))


def restated_f32_gap_dz2(p, stored, B):
    """How far dz2 moves when ONE operand of encoder.3's input-gradient product rounds the other way - for the operands whose
    rounding the kernel's f32 arithmetic does not determine.  The kernel stages dy = dz*k0 + (y*k1 + k2) (common.cuh,
    bn_fused_channel: f32 coefficients rounded from doubles, two f32 fmas) rounded to bf16; the emulation rounds the f64 value.
    Where the f64 value lies within the f32 evaluation's error bound of a bf16 tie - 2^-24 (|dz k0| + |y k1| + |k2|) for the
    rounded coefficients plus as much for the two fma results - either neighbour is a correct f32 result.  Computed from the
    stored inputs of that kernel on the CPU alone (never from the GPU's dz2).  Returns the largest relative L2 move of dz2 over
    those operands, one flipped at a time, and their number."""
    P = lambda k: p[k].astype(np.float64)                                    # noqa: E731
    rs = lambda v: vo.round_storage(v, "bf16")                               # noqa: E731
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)             # noqa: E731
    R = lambda a: a.reshape(1, -1, 1, 1)                                     # noqa: E731
    Y3, DZ3, Z2, CA3 = stored["Y"][3], stored["DZ"][3], stored["Z"][2], stored["CA"][3]
    gamma = P("encoder.3.1.weight")
    dy, dgam, dbet = vo.bn_train_bwd(DZ3, gamma, CA3)
    cnt = DZ3.shape[0] * DZ3.shape[2] * DZ3.shape[3]
    inv, mean = f32(CA3[1]), CA3[2]
    s = gamma * inv
    k0, k1, k2 = f32(s), f32(-s * dgam / cnt * inv), f32(-s * dbet / cnt + s * dgam / cnt * mean * inv)
    a = np.abs(dy)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(a, 1e-300))) - 7)
    lo = np.floor(a / ulp) * ulp
    bound = 2 * 2.0 ** -24 * (np.abs(DZ3 * R(k0)) + np.abs(Y3 * R(k1)) + np.abs(R(k2)))
    undetermined = np.argwhere((np.abs(a - (lo + ulp / 2)) <= bound) & (a > 0))
    w = rs(P("encoder.3.0.weight"))
    dyr = rs(dy)
    want = rs(vo.lrelu_bwd(Z2, vo.conv_dgrad(dyr, w, 2, Z2.shape[2:])))
    norm = max(np.sqrt((want ** 2).sum()), 1e-30)
    worst = 0.0
    for b, c, yy, xx in undetermined:
        alt = dyr[b:b + 1].copy()
        other = lo[b, c, yy, xx] + ulp[b, c, yy, xx] if abs(dyr[b, c, yy, xx]) == lo[b, c, yy, xx] else lo[b, c, yy, xx]
        alt[0, c, yy, xx] = np.sign(dy[b, c, yy, xx]) * other
        moved = rs(vo.lrelu_bwd(Z2[b:b + 1], vo.conv_dgrad(alt, w, 2, Z2.shape[2:])))
        worst = max(worst, float(np.sqrt(((moved - want[b:b + 1]) ** 2).sum()) / norm))
    return worst, len(undetermined)


def _check_case(test, dtype, H, L, B, gen, regime="default", kld_weight=1.0, opts=None, **tags):
    x, p = regime_inputs(regime, H, L, B, gen) if regime != "default" else (None, None)
    keep = {}
    exact = (opts or {}).get("use_mfma_convout", 1) == 0
    gaps = _layer_local_gaps(dtype, H, L, B, gen, opts=opts, kld_weight=kld_weight, exact_convout=exact, keep=keep, x=x, params=p)
    worst = max(gaps, key=gaps.get)
    # the three ELBO scalars in f64 from the GPU's own x_hat, mu and log_var
    if x is None:
        x = vo.synth_pianoroll(B, H, 21).astype(np.float64)
    last = keep["last"]
    lo = vo.loss({"output": last["xhat"], "x": x, "mu": last["mu"], "lv": last["lv"]}, kld_weight)
    want = np.array([float(lo["loss"]), float(lo["reconstruction_loss"]), float(lo["kld_loss"])])
    got = np.array(keep["out3"].tolist())
    # the padding between the tensors of the flat gradient
    m = keep["model"]
    pad = padding_mask(m._offs, m._sizes, keep["grads"].numel())
    stray = keep["grads"].cpu().numpy()[pad]
    report(test=test, regime=regime, dtype=dtype, img=H, latent=L, batch=B, kld_weight=kld_weight, worst=worst, worst_gap=gaps[worst],
           elbo_rel=float(np.abs(got / want - 1).max()), padding=int(pad.sum()), padding_nonzero=int(np.count_nonzero(stray)),
           gaps=gaps, **tags)
    assert len(gaps) == 54
    gates = dict.fromkeys(gaps, GATE[dtype])
    if (regime, dtype, H, L, B) in RESTATED_DZ2:
        restated, n = restated_f32_gap_dz2(p, keep["stored"], B)
        report(test=test + "_restated", regime=regime, dtype=dtype, img=H, latent=L, batch=B, tensor="dz2", restated_f32_gap=restated,
               undetermined_operands=n, measured=gaps["dz2"])
        gates["dz2"] = max(GATE[dtype], 2 * restated)
    bad = {k: v for k, v in gaps.items() if not v < gates[k]}
    assert not bad, bad
    np.testing.assert_allclose(got, want, rtol=ELBO_TOL[dtype])
    assert pad.sum() > 0 and not stray.any(), np.flatnonzero(pad)[np.flatnonzero(stray)][:8]


@pytest.mark.parametrize("H,L,B,gen", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("regime", REGIMES)
def test_every_kernel_on_its_own_inputs_in_every_regime(regime, dtype, H, L, B, gen):
    """All 54 tensors of the layer-local check with BCE and the default objective, per regime and storage mode at the smallest
    shapes that reach each kernel family (tests/regimes.py: SHAPES)."""
    _check_case("layer_local_regime", dtype, H, L, B, gen, regime=regime)


@pytest.mark.parametrize("dtype,H,L,B", [("bf16", 128, 16, 3), ("f16", 64, 16, 5)])
@pytest.mark.parametrize("vi", [0, 2, 18], ids=["tiled", "separate-wgrad", "valu-convout"])
def test_kernel_variants_on_velocity_rolls_and_trained_like_weights(vi, dtype, H, L, B):
    """Velocity rolls with trained-like parameters on the tiled forms of the streaming kernels, the separate input / weight
    gradient kernels and the VALU output conv."""
    _check_case("layer_local_regime_variant", dtype, H, L, B, True, regime="velocity+trained", opts=KERNEL_VARIANTS[vi], variant=vi)


@pytest.mark.parametrize("dtype,H,L,B,gen", [("bf16", 128, 16, 3, True), ("f16", 64, 16, 5, True), ("f32", 32, 16, 6, False)])
@pytest.mark.parametrize("kw", [0.00025, 0.0])
def test_every_kernel_on_its_own_inputs_at_small_kld_weights(kw, dtype, H, L, B, gen):
    """kld_weight 0.00025 (the reference's shipped configuration) and 0 on the default data."""
    _check_case("layer_local_kld_weight", dtype, H, L, B, gen, kld_weight=kw)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("L", [1, 3, 10, 40])
def test_one_call_step_keeps_the_padding_zero(L, dtype, clip):
    """Two one-call training steps at 32x32, batch 5, at latent sizes whose tensors end inside a 64-float slot (and inside the 16- and
    32-wide tiles of the kernels that write their gradients): the padding of the gradients, the parameters and both AdamW moments
    is exactly 0 - the all-reduce, the gradient norm and the update all run over whole ranges - and the reported gradient norm is
    the f64 norm over the tensors alone."""
    from torch_vae_amd.train import build_optimizer, fused_step
    H, B = 32, 5
    m = make_model(H, L, False, dtype, perturbed_params(L, H, 41, False))
    cfg = Namespace(batch_size_per_gpu=B, world_size=1, lr_relative=0.01, weight_decay=0.01, optimizer="AdamW", scheduler="OneCycle", epochs=1,
                    freeze_encoder=False)
    if clip:                                  # a quarter of the first step's gradient norm: the clip is active
        probe = make_model(H, L, False, dtype, perturbed_params(L, H, 41, False))
        probe.fused_forward_backward(torch.from_numpy(vo.synth_pianoroll(B, H, 31)).cuda(),
                                     eps=torch.from_numpy(vo.counter_normal(B * L, 31, 5).reshape(B, L)).float().cuda())
        cfg.max_grad_norm = 0.25 * _optimised_norm(probe)
    opt, sched = build_optimizer(cfg, m, steps_per_epoch=10)
    opt._bind()
    pad = padding_mask(m._offs, m._sizes, m.flat_parameters().numel())
    assert pad.sum() > 0 and pad.size % 64 == 0
    for step in (1, 2):
        x = torch.from_numpy(vo.synth_pianoroll(B, H, 30 + step)).cuda()
        eps = torch.from_numpy(vo.counter_normal(B * L, 30 + step, 5).reshape(B, L)).float().cuda()
        fused_step(m, opt, x, eps=eps)
        sched.step()
        torch.cuda.synchronize()
        g = m.flat_grads().double().cpu().numpy()
        for name, buf in (("grad", g), ("param", m.flat_parameters().cpu().numpy()), ("exp_avg", opt._m.cpu().numpy()),
                          ("exp_avg_sq", opt._v.cpu().numpy())):
            assert not buf[pad].any(), (step, name, np.flatnonzero(pad)[np.flatnonzero(buf[pad])][:8])
        if opt.last_grad_norm is not None:
            norm = _optimised_norm(m)
            assert abs(float(opt.last_grad_norm) - norm) <= 1e-12 * norm, (float(opt.last_grad_norm), norm)
            assert norm > 1.1 * cfg.max_grad_norm
    assert (opt.last_grad_norm is not None) == clip
