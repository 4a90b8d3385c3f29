"""The layer-local recomputation of the backwards outside the training step, shared by its host proof
(tests/test_grad_paths_local_host.py) and the GPU check (tests/test_grad_paths_local_gpu.py), and the seeded upstream-gradient
weights those tests and the end-to-end check of tests/test_grad_paths_gpu.py compose their losses from."""
import numpy as np

from oracle import vae_oracle as vo
from tests.util import PRE_BN_BIAS, rel_l2

LAYERS = ["encoder.0", "encoder.1", "encoder.2", "encoder.3", "decoder.0", "decoder.1", "decoder.2", "final_layer"]
LAYER_CH = [32, 64, 128, 256, 128, 64, 32, 32]


def layer_shapes(H, B, gen):
    """(shapes [B, C, h, w] of the eight stored y_l / dz_l, bottleneck side s)"""
    s = H // 16 if gen else 2
    hw = [H // 2, H // 4, H // 8, s, 2 * s, 4 * s, 8 * s, 16 * s]
    return [(B, LAYER_CH[i], hw[i], hw[i]) for i in range(8)], s


def path_params(kind):
    """Names of the parameters whose gradients a backward of `kind` ("forward" / "encode" / "decode") writes."""
    dec = ("decoder_input", "decoder", "final_layer")
    names = list(vo.param_shapes(1))
    if kind == "forward":
        return names
    return [n for n in names if n.startswith(dec) == (kind == "decode")]


def path_local_recompute(kind, train, p, bn, dev, up, H, L, B, gen, *, storage=None, fma=None, gscale_store=1.0,
                         kld_weight=1.0, recon="bce"):
    """The backward of a forward / encode / decode pass (train or eval mode), LAYER BY LAYER ON THE TENSORS THE DEVICE STORED: every
    stored gradient and every parameter gradient is recomputed in f64 from what was stored one layer earlier, so a gap is one kernel's.

    p: f64 parameters; bn: {"<bn name>.running_mean" / ".running_var": f64} as the forward read them (eval mode only).
    dev ("the tensors the device stored", f64, NCHW): Y[i], DZ[i] (dicts over the path's layers; DZ without the f16 scale), d0, dd0,
      dlat [B, 2L], mu, lv, z, xhat, x, eps - whichever the path has.
    up: upstream gradients g_xhat, g_mu, g_lv, g_z, g_pre ([B, F], the reference's NCHW-flatten order), each an array or None,
      and gscale: the factor on the standard ELBO (None: no ELBO term, only explicit upstream gradients).
    storage ("bf16" / "f16" / None): where a kernel stores or stages 16 bits the value is rounded (gradients on the grid scaled by
      gscale_store); fma (anything but None): the pre-activation is the kernels' single f32 fused multiply-add (also the f32 mode).
    Returns {name: recomputed tensor}: dz0..dz7, dd0, dlat, dx (when dev holds one) / dz, and the path's parameter gradients."""
    rs = lambda v: vo.round_storage(v, storage)                  # noqa: E731
    rg = lambda v: vo.round_storage(v, storage, gscale_store)    # noqa: E731
    P = lambda k: np.asarray(p[k], np.float64)                   # noqa: E731
    layers = {"forward": range(8), "encode": range(4), "decode": range(4, 8)}[kind]
    Y, DZ = dev["Y"], dev["DZ"]
    want = {}
    Z, CA = {}, {}
    for i in layers:
        n = LAYERS[i] + ".1"
        if train:
            Z[i], CA[i] = vo.bn_train_fwd_stored(Y[i], P(n + ".weight"), P(n + ".bias"), fma)
        else:
            Z[i] = vo.bn_eval_fwd_stored(Y[i], P(n + ".weight"), P(n + ".bias"), bn[n + ".running_mean"], bn[n + ".running_var"], fma)
    A = {i: rs(vo.lrelu(Z[i])) for i in layers}          # staged operands LeakyReLU(BN(y_l)) as the next kernel rounds them

    def bn_bwd(i):
        n = LAYERS[i]
        if train:
            dy, dgam, dbet = vo.bn_train_bwd(DZ[i], P(n + ".1.weight"), CA[i])
            dcb = np.zeros_like(dbet)                    # the conv bias in front of a train-mode BatchNorm: analytically zero
        else:
            dy, dgam, dbet, dcb = vo.bn_eval_bwd(DZ[i], Y[i], P(n + ".1.weight"), bn[n + ".1.running_mean"], bn[n + ".1.running_var"])
        want[n + ".1.weight"], want[n + ".1.bias"], want[n + ".0.bias"] = dgam, dbet, dcb
        return dy

    if kind != "encode":
        # ---- output conv from the device's xhat and the combined dlogit, then the decoder stack
        xh = dev["xhat"]
        dlogit = np.zeros_like(xh)
        if up.get("gscale") is not None:
            x = dev["x"]
            if recon == "mse":
                dlogit = dlogit + up["gscale"] * (xh - x) * 2.0 / xh.size * (1 - xh) * xh
            else:
                dlogit = dlogit + up["gscale"] * (xh - x) / np.maximum(xh * (1 - xh), 1e-12) / xh.size * xh * (1 - xh)
        if up.get("g_xhat") is not None:
            dlogit = dlogit + up["g_xhat"] * xh * (1 - xh)
        dl_op = rg(dlogit)                               # the MFMA operand of the output conv's gradient products
        wo = rs(P("final_layer.3.weight"))
        dw, _ = vo.conv_wgrad(A[7], dl_op, 1)
        want["final_layer.3.weight"], want["final_layer.3.bias"] = dw, dlogit.sum(axis=(0, 2, 3))
        want["dz7"] = rg(vo.lrelu_bwd(Z[7], vo.conv_dgrad(dl_op, wo, 1, (H, H))))
        ins = {4: dev["d0"], 5: A.get(4), 6: A.get(5), 7: A.get(6)}
        for i in (7, 6, 5, 4):
            n = LAYERS[i]
            dyr = rg(bn_bwd(i))
            dx, dw, _ = vo.convT_bwd(ins[i], rs(P(n + ".0.weight")), dyr)
            want[n + ".0.weight"] = dw
            if i == 4:
                want["dd0"] = rg(dx)
            else:
                want[f"dz{i - 1}"] = rg(vo.lrelu_bwd(Z[i - 1], dx))
        # ---- decoder_input on the device's dd0
        f = dev["dd0"].reshape(B, -1)
        want["decoder_input.weight"] = f.T @ dev["z"]
        want["decoder_input.bias"] = f.sum(axis=0)
        dzl = f @ rs(P("decoder_input.weight"))
        if kind == "decode":
            want["dz"] = dzl                             # (f32 sums of the split-K slabs: nothing is rounded to 16 bits)
            return want
    # ---- latent block: reparameterisation + KL backward, every upstream gradient
    z0 = np.zeros((B, L))
    opt = lambda k: z0 if up.get(k) is None else np.asarray(up[k], np.float64)   # noqa: E731
    mu, lv = dev["mu"], dev["lv"]
    if kind == "forward":
        d = dzl + opt("g_z")                             # the gradient on z: decoder_input's plus the upstream one, BEFORE eps * std
        dmu, dlv = d.copy(), d * dev["eps"] * np.exp(0.5 * lv) * 0.5
        if up.get("gscale") is not None:
            k = up["gscale"] * kld_weight / B
            dmu, dlv = dmu + k * mu, dlv + k * 0.5 * (np.exp(lv) - 1)
    else:
        dmu, dlv = z0.copy(), z0.copy()
    dmu, dlv = dmu + opt("g_mu"), dlv + opt("g_lv")
    want["dlat"] = np.concatenate([dmu, dlv], axis=1)
    # ---- fc heads on the device's dlat (f32: read unrounded)
    dmu, dlv = dev["dlat"][:, :L], dev["dlat"][:, L:]
    act3 = vo.lrelu(Z[3]).reshape(B, -1)                 # (unrounded: the fc weight gradient reads it in f32)
    want["fc_mu.weight"], want["fc_var.weight"] = dmu.T @ act3, dlv.T @ act3
    want["fc_mu.bias"], want["fc_var.bias"] = dmu.sum(axis=0), dlv.sum(axis=0)
    dpre = dmu @ rs(P("fc_mu.weight")) + dlv @ rs(P("fc_var.weight"))
    if up.get("g_pre") is not None:
        dpre = dpre + np.asarray(up["g_pre"], np.float64)   # (pre_latents is the NCHW flatten of encoder.3's activation: same order)
    want["dz3"] = rg(vo.lrelu_bwd(Z[3], dpre.reshape(Z[3].shape)))
    # ---- encoder stack
    x = dev["x"]
    for i in (3, 2, 1, 0):
        n = LAYERS[i]
        dy = bn_bwd(i)
        if i == 0:      # conv1_wgrad / conv1_dgrad: f32 weights, unrounded gradient operand
            want[n + ".0.weight"], _ = vo.conv_wgrad(x, dy, 2)
            if dev.get("dx") is not None:               # (a backward that was asked for the input gradient)
                want["dx"] = vo.conv_dgrad(dy, P(n + ".0.weight"), 2, (H, H))
            continue
        dyr = rg(dy)
        dw, _ = vo.conv_wgrad(A[i - 1], dyr, 2)
        want[n + ".0.weight"] = dw
        want[f"dz{i - 1}"] = rg(vo.lrelu_bwd(Z[i - 1], vo.conv_dgrad(dyr, rs(P(n + ".0.weight")), 2, A[i - 1].shape[2:])))
    return want


def path_local_gaps(kind, train, want, dev, grads):
    """Relative L2 gap of every tensor path_local_recompute returned against what the device holds: stored gradients from `dev`
    (DZ, dd0, dlat, dx, dz), parameter gradients from `grads`.  The conv biases in front of a train-mode BatchNorm are analytically
    zero: they come back in the second dict as max |gradient| (an absolute bound, never a skip)."""
    gaps, zero = {}, {}
    for k, w in want.items():
        if k.startswith("dz") and k != "dz":
            got = dev["DZ"][int(k[2:])]
        elif k in ("dd0", "dlat", "dx", "dz"):
            got = dev[k]
        else:
            got = grads[k]
            assert got is not None, k
        got = np.asarray(got, np.float64).reshape(np.shape(w))
        if train and k in PRE_BN_BIAS:
            assert np.abs(w).max() == 0.0
            zero[k] = float(np.abs(got).max())
        else:
            gaps[k] = rel_l2(got, w)
    return gaps, zero


def upstream_weights(kind, H, L, B, F, seed):
    """Seeded weights of the random-weighted sums a test adds to its loss, one per output of the path: distinct per element and of
    a different magnitude per tensor, each of the order of the standard ELBO's own gradient on that output (1/(B*H*W) per pixel,
    1/B per latent), so a swapped, dropped or mis-indexed upstream gradient moves the result by its own size.  decode: O(1) weights
    on xhat, a sum-reduced loss (in the f16 mode far above the range the library's gradient scale was chosen for)."""
    rng = np.random.default_rng(seed)
    if kind == "decode":
        return {"xhat": rng.uniform(-0.3, 0.7, (B, 1, H, H))}
    w = {"mu": 0.5 / B * rng.standard_normal((B, L)), "log_var": 0.3 / B * rng.standard_normal((B, L)),
         "pre_latents": 0.08 / B * rng.standard_normal((B, F))}
    if kind == "forward":
        w["output"] = 0.7 / (B * H * H) * rng.standard_normal((B, 1, H, H))
        w["latents"] = 0.8 / B * rng.standard_normal((B, L))
    return w


LOSS_SCALE = 1.7        # not a power of two: the loss scale reaches the kernels as gscale != 1
UP_KEYS = {"output": "g_xhat", "xhat": "g_xhat", "mu": "g_mu", "log_var": "g_lv", "latents": "g_z", "pre_latents": "g_pre"}


def upstream_of(weights, scale, with_elbo):
    """The `up` argument of path_local_recompute for the loss scale * ([ELBO] + sum_k (w_k * out_k).sum())."""
    up = {UP_KEYS[k]: scale * v for k, v in weights.items()}
    up["gscale"] = scale if with_elbo else None
    return up
