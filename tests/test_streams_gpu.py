"""The stream contract of include/vae_step.h on a NON-default stream: every entry point that takes a stream, enqueued behind a
50 ms chain of matrix products on a stream of its own with every live buffer poisoned in front of the chain, against the same
calls on the synchronised default stream (tests/stream_harness.py has the procedure).  A launch, memset or copy on stream 0, a
side stream forked before its event or never joined, a read-back on the wrong stream or a Python helper that fetches the stream
at the wrong moment all give stale or NaN results here and right ones on a synchronised default stream.  The host must also have
enqueued the whole case while the stream was still held up (`pending`): a host wait inside the library fails the case.

CASES is collected without touching torch.cuda (tests/test_streams_host.py holds it against the header)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import stream_harness as sh
from tests.stream_harness import Bufs, Case

pytestmark = pytest.mark.gpu

# Entry points that may make the host wait on the per-call path, each with the sentence of include/vae_step.h that allows it.
# After the warm-up of the harness none of the listed cases needs one.
EXEMPT = {}

# Exported functions with a vae_stream_t parameter that no case calls, each with the reason.
NOT_COVERED = {
    "vae_selftest_tr16": "a hardware probe of the transposed LDS read that synchronises by design and returns its verdict to the host",
    "vae_broadcast_state": "needs two ranks to move anything: with the one rank a single GPU can form it leaves every buffer as it was",
}

SEED = 7
LR, B1, B2, AEPS, WD = 3e-3, 0.9, 0.999, 1e-8, 0.01


def st():
    """The stream pointer every call passes: the CURRENT stream, fetched at the call."""
    return torch.cuda.current_stream().cuda_stream


def lib():
    from torch_vae_amd import _lib
    return _lib.lib()


def ok(rc, what=""):
    assert rc == 0, (what, lib().vae_last_error().decode())


@functools.lru_cache(maxsize=None)
def _params(H, L, gen):
    from tests.util import perturbed_params
    return perturbed_params(L, H, 31, gen)


@functools.lru_cache(maxsize=None)
def _inputs(H, L, B):
    from oracle import vae_oracle as vo
    rng = np.random.default_rng(5)
    return dict(x=torch.from_numpy(vo.synth_pianoroll(B, H, 32)).float(),
                eps=torch.from_numpy(vo.counter_normal(B * L, 32, 5).reshape(B, L)).float(),
                z=torch.from_numpy(rng.standard_normal((B, L))).float(),
                g_xhat=torch.from_numpy(rng.standard_normal((B, 1, H, H)) / (B * H * H)).float(),
                g_mu=torch.from_numpy(rng.standard_normal((B, L)) / B).float())


# ---- the network cases: a model's context handle with caller-owned tensors --------------------------------------------------------
class Net:
    """Fresh model and context plus the buffers of one batch, registered in a Bufs.  cfg = (dtype, H, L, B, generalised)."""

    def __init__(self, cfg, eps=True, kl=None, opts=(), max_batch=None, comm=False, inf=False):
        from tests.util import make_model
        dtype, H, L, B, gen = cfg
        self.cfg, self.H, self.L, self.B = cfg, H, L, B
        self.m = m = make_model(H, L, gen, dtype, _params(H, L, gen))
        if kl == "free_bits":
            m.kl_free_bits = 0.05
        elif kl == "tc":
            m.tc_weight = 3.0
        if comm:
            from torch_vae_amd.train import enable_library_allreduce
            assert enable_library_allreduce(m)
        self.h = m._context(max_batch or B).handle
        for name, value in opts:
            ok(lib().vae_set_option(self.h, name, value), name)
        if comm:
            assert m.library_comm_world() == 1
        self.b = b = Bufs()
        b.keep.append(self)
        inp = _inputs(H, L, B)
        x = inp["x"].clone()
        if inf:
            x[0, 0, 3, 5] = float("inf")            # one non-finite cell: every gradient follows, the clipped step skips
        b.inp("x", x)
        self.eps = b.inp("eps", inp["eps"]) if eps else None
        b.adopt("params", m._flat, inout=True)
        b.adopt("bn_running", m._bnflat, inout=True)
        b.adopt("num_batches_tracked", m._nbt, inout=True, poison=0)
        b.adopt("grads", m._gflat, inout=True)
        b.outp("xhat", B, 1, H, H); b.outp("mu", B, L); b.outp("log_var", B, L); b.outp("z", B, L); b.outp("out3", 3)
        enc, dec = m.group_range("encoder"), m.group_range("decoder")
        self.offs, self.sizes = (C.c_int64 * 2)(enc[0], dec[0]), (C.c_int64 * 2)(enc[1], dec[1])
        self.lrs, self.b1s = (C.c_double * 2)(LR, 0.5 * LR), (C.c_double * 2)(B1, 0.85)
        self.dec = ((C.c_int64 * 1)(dec[0]), (C.c_int64 * 1)(dec[1]))

    def moments(self):
        rng = np.random.default_rng(9)
        n = self.m._flat.numel()
        self.b.inp("exp_avg", torch.from_numpy(1e-3 * rng.standard_normal(n)).float(), inout=True)
        self.b.inp("exp_avg_sq", torch.from_numpy(1e-6 * rng.random(n)).float(), inout=True)

    def clip_state(self):
        b = self.b
        b.inp("step", torch.tensor(3, dtype=torch.int64), inout=True, poison=0)
        b.inp("skipped", torch.tensor(1, dtype=torch.int64), inout=True, poison=5)
        b.outp("norm", 1, dtype=torch.float64)
        self.scratch = torch.empty(8192, dtype=torch.uint8, device="cuda")

    # the calls
    def forward(self, train):
        b = self.b
        ok(lib().vae_forward(self.h, b["x"].data_ptr(), self.B, b["params"].data_ptr(), b["bn_running"].data_ptr(), b["num_batches_tracked"].data_ptr(),
                             0 if self.eps is None else self.eps.data_ptr(), SEED, train, b["xhat"].data_ptr(), b["mu"].data_ptr(),
                             b["log_var"].data_ptr(), b["z"].data_ptr(), st()), "vae_forward")

    def encode(self, train=1):
        b = self.b
        ok(lib().vae_encode(self.h, b["x"].data_ptr(), self.B, b["params"].data_ptr(), b["bn_running"].data_ptr(), b["num_batches_tracked"].data_ptr(),
                            0 if self.eps is None else self.eps.data_ptr(), SEED, train, b["mu"].data_ptr(), b["log_var"].data_ptr(),
                            b["z"].data_ptr(), st()), "vae_encode")

    def decode(self, train=1):
        b = self.b
        ok(lib().vae_decode(self.h, b["z_in"].data_ptr(), self.B, b["params"].data_ptr(), b["bn_running"].data_ptr(), b["num_batches_tracked"].data_ptr(),
                            train, b["xhat"].data_ptr(), st()), "vae_decode")

    def loss(self):
        ok(lib().vae_loss(self.h, 1.0, self.b["out3"].data_ptr(), st()), "vae_loss")

    def loss_deferred(self):
        ok(lib().vae_loss_deferred(self.h, 1.0, self.b["out3"].data_ptr(), st()), "vae_loss_deferred")

    def _bwd_args(self, use_std=1, g_xhat=None, g_mu=None):
        b = self.b
        return (self.h, b["x"].data_ptr(), b["params"].data_ptr(), b["grads"].data_ptr(), 0 if g_xhat is None else g_xhat.data_ptr(), 0,
                0 if g_mu is None else g_mu.data_ptr(), 0, 0, 0, 1.0, use_std)

    def backward(self):
        ok(lib().vae_backward(*self._bwd_args(), st()), "vae_backward")

    def backward_part(self, part):
        ok(lib().vae_backward_part(*self._bwd_args(), part, st()), "vae_backward_part")

    def backward_ex(self, use_std, g_xhat=None, g_mu=None, dx=None, dz=None):
        ok(lib().vae_backward_ex(*self._bwd_args(use_std, g_xhat, g_mu), 0 if dx is None else dx.data_ptr(), 0 if dz is None else dz.data_ptr(),
                                 st()), "vae_backward_ex")

    def _step_head(self):
        b = self.b
        return (self.h, b["x"].data_ptr(), self.B, b["params"].data_ptr(), b["grads"].data_ptr(), b["exp_avg"].data_ptr(), b["exp_avg_sq"].data_ptr(),
                b["bn_running"].data_ptr(), b["num_batches_tracked"].data_ptr(), 0 if self.eps is None else self.eps.data_ptr(), SEED, 1.0, 2,
                self.offs, self.sizes, self.lrs, self.b1s, B2, AEPS, WD)

    def _step_tail(self):
        b = self.b
        return (b["xhat"].data_ptr(), b["mu"].data_ptr(), b["log_var"].data_ptr(), b["z"].data_ptr(), b["out3"].data_ptr(), st())

    def train_step(self):
        ok(lib().vae_train_step(*self._step_head(), 4, *self._step_tail()), "vae_train_step")

    def train_step_fused(self, exchange=0):
        ok(lib().vae_train_step_fused(*self._step_head(), 1.0, 4, exchange, *self._step_tail()), "vae_train_step_fused")

    def train_step_fused_clipped(self, exchange=0):
        b = self.b
        ok(lib().vae_train_step_fused_clipped(*self._step_head(), 1.0, 0.05, 1, b["step"].data_ptr(), b["norm"].data_ptr(), b["skipped"].data_ptr(),
                                              self.scratch.data_ptr(), exchange, *self._step_tail()), "vae_train_step_fused_clipped")


def net_case(name, covers, cfg, body, setup=None, **net_kw):
    """A network case: setup(net) adds buffers, body(net) makes the calls."""
    def make():
        n = Net(cfg, **net_kw)
        if setup is not None:
            setup(n)
        return n.b

    def run(b):
        return body(b.keep[0])
    return Case(name, covers, make, run, dtype=cfg[0])


def _fwd_loss_bwd(n):
    n.forward(1); n.loss(); n.backward()


def _fwd_loss_parts(n):
    n.forward(1); n.loss(); n.backward_part(1); n.backward_part(2)


def _fwd2_deferred_bwd(n):
    n.forward(2); n.loss_deferred(); n.backward()


def _eval_fwd_bwd_ex(n):
    n.forward(0); n.loss(); n.backward_ex(1, dx=n.b["dx"])


def _encode_bwd_ex(n):
    n.encode(1); n.backward_ex(0, g_mu=n.b["g_mu"], dx=n.b["dx"])


def _decode_bwd_ex(n):
    n.decode(1); n.backward_ex(0, g_xhat=n.b["g_xhat"], dz=n.b["dz"])


def _setup_dx(n):
    n.b.outp("dx", n.B, 1, n.H, n.H)


def _setup_encode(n):
    n.b.outp("dx", n.B, 1, n.H, n.H)
    n.b.inp("g_mu", _inputs(n.H, n.L, n.B)["g_mu"])


def _setup_decode(n):
    n.b.inp("z_in", _inputs(n.H, n.L, n.B)["z"])
    n.b.inp("g_xhat", _inputs(n.H, n.L, n.B)["g_xhat"])
    n.b.outp("dz", n.B, n.L)


def _setup_clipped(n):
    n.moments(); n.clip_state()


# (name, entry points, body, setup, needs 16-bit storage, takes eps / a KL objective, extra Net arguments)
STEP_BODIES = [
    ("fwd_loss_bwd", ("vae_forward", "vae_loss", "vae_backward"), _fwd_loss_bwd, None, False, True, {}),
    ("fwd_loss_parts", ("vae_forward", "vae_loss", "vae_backward_part"), _fwd_loss_parts, None, False, True, {}),
    ("fwd2_deferred_bwd", ("vae_forward", "vae_loss_deferred", "vae_backward"), _fwd2_deferred_bwd, None, True, True, {}),
    ("train_step", ("vae_train_step",), Net.train_step, Net.moments, False, True, {}),
    ("train_step_fused", ("vae_train_step_fused",), Net.train_step_fused, Net.moments, False, True, {}),
    ("fused_clipped", ("vae_train_step_fused_clipped",), Net.train_step_fused_clipped, _setup_clipped, False, True, {}),
    ("fused_clipped_inf", ("vae_train_step_fused_clipped",), Net.train_step_fused_clipped, _setup_clipped, False, True, {"inf": True}),
    ("eval_fwd_bwd_ex_dx", ("vae_forward", "vae_loss", "vae_backward_ex"), _eval_fwd_bwd_ex, _setup_dx, False, True, {}),
    ("encode_bwd_ex", ("vae_encode", "vae_backward_ex"), _encode_bwd_ex, _setup_encode, False, True, {}),
    ("decode_bwd_ex_dz", ("vae_decode", "vae_backward_ex"), _decode_bwd_ex, _setup_decode, False, False, {}),
]
R32 = (32, 16, 4, False)          # the reference model: 32x32, latent 16, batch 4
G128 = (128, 16, 3, True)         # row-streaming kernels, deferred output conv, fused input + weight gradient kernels
STEP_CONFIGS = [("f32",) + R32, ("bf16",) + R32, ("bf16",) + G128, ("f16",) + G128]
# each body once more on the bf16 reference model: noise drawn on the device (a side stream, knob_lean bit 0), a KL objective whose
# reduction runs on a side stream and is ordered in by ev_kl, and everything on the caller's stream
STEP_VARIANTS = [("eps_null", dict(eps=False)), ("free_bits", dict(kl="free_bits")), ("tc", dict(kl="tc")),
                 ("no_side_stream", dict(opts=((b"use_side_stream", 0),)))]


def _step_cases():
    out = []
    for name, covers, body, setup, sixteen, latent, kw in STEP_BODIES:
        for cfg in STEP_CONFIGS:
            if sixteen and cfg[0] == "f32":
                continue
            out.append(net_case(f"{name}/{cfg[0]}_h{cfg[1]}", covers, cfg, body, setup, **kw))
        for vname, vkw in STEP_VARIANTS:
            if not latent and vname != "no_side_stream":
                continue
            out.append(net_case(f"{name}/bf16_h32/{vname}", covers, ("bf16",) + R32, body, setup, **kw, **vkw))
    return out


# ---- read-backs after a forward, nothing in between --------------------------------------------------------------------------------
def debug_tensor(n, which, out):
    """vae_debug_tensor into a caller's buffer on the current stream, with no synchronisation (tests/util.fetch_debug_tensor has one)."""
    ok(lib().vae_debug_tensor(n.h, which, out.data_ptr(), out.numel(), st()), f"vae_debug_tensor {which}")


def _setup_readbacks(n):
    b, B, L, H = n.b, n.B, n.L, n.H
    flat = n.m.flattened_size
    b.outp("pre_latents", B, flat); b.outp("last_eps", B, L); b.outp("kl_per_dim", L, dtype=torch.float64); b.outp("tc", 1, dtype=torch.float64)
    b.outp("y0", B * 32 * (H // 2) * (H // 2)); b.outp("dz0", B * 32 * (H // 2) * (H // 2))
    b.outp("dec_in", B * flat); b.outp("g_dec_in", B * flat); b.outp("g_latent", B * 2 * L); b.outp("g_tc", B * 2 * L)


def _readbacks(n):
    b, L_ = n.b, lib()
    n.forward(1)
    ok(L_.vae_pre_latents(n.h, b["pre_latents"].data_ptr(), st()), "vae_pre_latents")
    ok(L_.vae_last_eps(n.h, b["last_eps"].data_ptr(), st()), "vae_last_eps")
    ok(L_.vae_kl_per_dim(n.h, b["kl_per_dim"].data_ptr(), st()), "vae_kl_per_dim")
    ok(L_.vae_last_total_correlation(n.h, b["tc"].data_ptr(), st()), "vae_last_total_correlation")
    debug_tensor(n, 0, b["y0"]); debug_tensor(n, 16, b["dec_in"]); debug_tensor(n, 20, b["g_tc"])
    n.loss(); n.backward()
    debug_tensor(n, 8, b["dz0"]); debug_tensor(n, 17, b["g_dec_in"]); debug_tensor(n, 18, b["g_latent"])


READBACK_COVERS = ("vae_forward", "vae_pre_latents", "vae_last_eps", "vae_kl_per_dim", "vae_last_total_correlation", "vae_debug_tensor",
                   "vae_loss", "vae_backward")


def _readback_cases():
    return [net_case(f"readbacks/{d}{'/' + v if v else ''}", READBACK_COVERS, (d,) + R32, _readbacks, _setup_readbacks, **kw)
            for d, v, kw in (("f32", "", {}), ("bf16", "", {}), ("bf16", "eps_null", dict(eps=False)), ("bf16", "free_bits", dict(kl="free_bits")),
                             ("bf16", "tc", dict(kl="tc")))]


# ---- log-likelihood ------------------------------------------------------------------------------------------------------------------
def _setup_loglik(n):
    n.b.outp("log_w", 4, n.B, dtype=torch.float64); n.b.outp("log_likelihood", n.B, dtype=torch.float64); n.b.outp("elbo", n.B, dtype=torch.float64)


def _loglik(n):
    b = n.b
    ok(lib().vae_log_likelihood(n.h, b["x"].data_ptr(), n.B, b["params"].data_ptr(), b["bn_running"].data_ptr(), 4, 2, 0, 9, b["log_w"].data_ptr(),
                                b["log_likelihood"].data_ptr(), b["elbo"].data_ptr(), st()), "vae_log_likelihood")


# ---- the optimiser (no context) ------------------------------------------------------------------------------------------------------
N_OPT = 5000
OPT_OFFS, OPT_SIZES = (C.c_int64 * 2)(0, 3008), (C.c_int64 * 2)(3000, 1992)      # two ranges with a gap between them (never written)
OPT_LRS, OPT_B1S = (C.c_double * 2)(LR, 0.5 * LR), (C.c_double * 2)(B1, 0.85)


def _make_opt(clipped):
    b = Bufs()
    rng = np.random.default_rng(3)
    b.inp("params", torch.from_numpy(rng.standard_normal(N_OPT)).float(), inout=True)
    b.inp("grads", torch.from_numpy(rng.standard_normal(N_OPT)).float(), inout=True)
    b.inp("exp_avg", torch.from_numpy(0.1 * rng.standard_normal(N_OPT)).float(), inout=True)
    b.inp("exp_avg_sq", torch.from_numpy(0.01 * rng.random(N_OPT)).float(), inout=True)
    if clipped:
        b.inp("step", torch.tensor(3, dtype=torch.int64), inout=True, poison=0)
        b.inp("skipped", torch.tensor(1, dtype=torch.int64), inout=True, poison=5)
        b.outp("norm", 1, dtype=torch.float64)
        b.outp("norm_only", 1, dtype=torch.float64)
        b.keep.append(torch.empty(8192, dtype=torch.uint8, device="cuda"))
    return b


def _adamw(b):
    ok(lib().vae_adamw_step(b["params"].data_ptr(), b["grads"].data_ptr(), b["exp_avg"].data_ptr(), b["exp_avg_sq"].data_ptr(), 2, OPT_OFFS, OPT_SIZES,
                            OPT_LRS, OPT_B1S, B2, AEPS, WD, 0.5, 4, st()), "vae_adamw_step")


def _adamw_clipped(b):
    ok(lib().vae_grad_norm(b["grads"].data_ptr(), 2, OPT_OFFS, OPT_SIZES, 0.5, b["norm_only"].data_ptr(), b.keep[0].data_ptr(), st()), "vae_grad_norm")
    ok(lib().vae_adamw_step_clipped(b["params"].data_ptr(), b["grads"].data_ptr(), b["exp_avg"].data_ptr(), b["exp_avg_sq"].data_ptr(), 2, OPT_OFFS,
                                    OPT_SIZES, OPT_LRS, OPT_B1S, B2, AEPS, WD, 0.5, 1.0, 1, b["step"].data_ptr(), b["norm"].data_ptr(),
                                    b["skipped"].data_ptr(), b.keep[0].data_ptr(), st()), "vae_adamw_step_clipped")


# ---- context-free kernels, each at the smallest shape of its own test file -----------------------------------------------------------
def _make_elbo():
    b = Bufs()
    rng = np.random.default_rng(11)
    n, B, L = 4 * 32 * 32, 4, 16
    b.inp("xhat", torch.from_numpy(rng.uniform(0.02, 0.98, n)).float())
    b.inp("target", torch.from_numpy((rng.random(n) < 0.1).astype(np.float32)))
    b.inp("mu", torch.from_numpy(rng.standard_normal((B, L))).float())
    b.inp("log_var", torch.from_numpy(0.3 * rng.standard_normal((B, L))).float())
    b.outp("out3", 3); b.outp("g_xhat", n); b.outp("g_mu", B, L); b.outp("g_log_var", B, L)
    return b


def _elbo(which):
    from torch_vae_amd import _lib

    def run(b):
        head = (b["xhat"].data_ptr(), b["target"].data_ptr(), b["mu"].data_ptr(), b["log_var"].data_ptr(), 4 * 32 * 32, 4, 16, 0.7)
        tail = (b["out3"].data_ptr(), b["g_xhat"].data_ptr(), b["g_mu"].data_ptr(), b["g_log_var"].data_ptr(), st())
        if which == "generic":
            ok(lib().vae_elbo_generic(*head, *tail), which)
        elif which == "ex":
            ok(lib().vae_elbo_generic_ex(*head, _lib.RECON_MSE, *tail), which)
        elif which == "kl":
            ok(lib().vae_elbo_generic_kl(*head, _lib.RECON_BCE, _lib.KL_FREE_BITS, 0.05, *tail), which)
        else:
            ok(lib().vae_elbo_generic_w(*head, _lib.RECON_WBCE, 4.0, _lib.KL_FREE_BITS, 0.05, *tail), which)
    return run


def _make_tc():
    b = Bufs()
    rng = np.random.default_rng(12)
    B, L = 5, 7
    for name, scale in (("mu", 1.0), ("log_var", 0.3), ("eps", 1.0)):
        b.inp(name, torch.from_numpy(scale * rng.standard_normal((B, L))).float())
    b.outp("tc", 1, dtype=torch.float64); b.outp("g_mu", B, L); b.outp("g_log_var", B, L)
    return b


def _tc(b):
    ok(lib().vae_total_correlation(b["mu"].data_ptr(), b["log_var"].data_ptr(), b["eps"].data_ptr(), 5, 7, b["tc"].data_ptr(), b["g_mu"].data_ptr(),
                                   b["g_log_var"].data_ptr(), st()), "vae_total_correlation")


def _make_latent_stats():
    b = Bufs()
    rng = np.random.default_rng(13)
    n, L, draws = 6, 5, 2
    b.inp("mu", torch.from_numpy(rng.standard_normal((n, L))).float())
    b.inp("log_var", torch.from_numpy(0.3 * rng.standard_normal((n, L))).float())
    f64 = dict(dtype=torch.float64)
    b.outp("log_qz", draws * n, **f64); b.outp("log_qz_dims", draws * n * L, **f64); b.outp("per_dim", 3 * L, **f64); b.outp("scalars", 4, **f64)
    return b


def _latent_stats(b):
    ok(lib().vae_latent_stats(b["mu"].data_ptr(), b["log_var"].data_ptr(), 6, 5, 2, 0, 3, b["log_qz"].data_ptr(), b["log_qz_dims"].data_ptr(),
                              b["per_dim"].data_ptr(), b["scalars"].data_ptr(), st()), "vae_latent_stats")


RM_THRESHOLDS = (C.c_float * 2)(0.5, 0.3)


def _make_recon_metrics():
    b = Bufs()
    rng = np.random.default_rng(14)
    rolls, roll_len = 3, 5000                                     # a roll above 4096 cells: two chunks, the per-roll fold
    b.inp("xhat", torch.from_numpy(rng.uniform(0.0, 1.0, (rolls, roll_len))).float())
    b.inp("target", torch.from_numpy((rng.random((rolls, roll_len)) < 0.1).astype(np.float32)))
    b.outp("roll_sums", rolls, 3, dtype=torch.float64); b.outp("roll_counts", rolls, 5, dtype=torch.int64)
    b.outp("totals", 8, dtype=torch.float64); b.outp("total_counts", 5, dtype=torch.int64)
    return b


def _recon_metrics(b):
    for accumulate in (0, 1):
        ok(lib().vae_recon_metrics(b["xhat"].data_ptr(), b["target"].data_ptr(), 3, 5000, RM_THRESHOLDS, 2, 0.5, b["roll_sums"].data_ptr(),
                                   b["roll_counts"].data_ptr(), b["totals"].data_ptr(), b["total_counts"].data_ptr(), accumulate, st()),
           "vae_recon_metrics")


def _make_synth():
    b = Bufs()
    b.outp("x", 4, 1, 32, 32)
    return b


def _synth(b):
    ok(lib().vae_synth_pianoroll(b["x"].data_ptr(), 4, 32, 17, st()), "vae_synth_pianoroll")


def _make_expand(pinned):
    def make():
        b = Bufs()
        rng = np.random.default_rng(15)
        b.inp("planes", torch.from_numpy(rng.integers(0, 256, (4, 1, 32, 4), dtype=np.uint8)), poison=0xFF, pinned=pinned)   # filled late, by a copy on s
        b.outp("x", 4, 1, 32, 32)
        return b
    return make


def _expand(b):
    ok(lib().vae_expand_stimuli(b["planes"].data_ptr(), 1, b["x"].data_ptr(), 4 * 32 * 32, st()), "vae_expand_stimuli")


GATHER = dict(n_rolls=5, h=16, src_w=48, batch=3, w=32)


def _make_gather():
    b = Bufs()
    rng = np.random.default_rng(16)
    g = GATHER
    b.inp("rolls", torch.from_numpy(rng.integers(0, 256, (g["n_rolls"], g["h"], g["src_w"] // 8), dtype=np.uint8)), poison=0xFF)
    b.inp("index", torch.tensor([4, 1, 3], dtype=torch.int64), poison=0)
    b.outp("x", g["batch"], 1, g["h"], g["w"])
    b.outp("params", g["batch"], 2, dtype=torch.int32)
    return b


def _gather(b):
    g = GATHER
    ok(lib().vae_gather_rolls(b["rolls"].data_ptr(), 1, g["n_rolls"], g["h"], g["src_w"], b["index"].data_ptr(), 0, 0, 21, 6, 1, 2, 3, 0, 1.0,
                              b["x"].data_ptr(), g["batch"], g["w"], st()), "vae_gather_rolls")
    ok(lib().vae_augment_params(b["params"].data_ptr(), g["batch"], g["src_w"], g["w"], 21, 6, 1, 2, 3, 0, st()), "vae_augment_params")


def _make_notes():
    b = Bufs()
    rng = np.random.default_rng(17)
    x = rng.random((2, 8, 32)) * (rng.random((2, 8, 32)) < 0.4)
    b.inp("rolls", torch.from_numpy(x).float())
    b.outp("events", 64, 4, dtype=torch.int32); b.outp("peaks", 64); b.outp("offsets", 3, dtype=torch.int64)
    b.outp("cleaned", 2, 8, 4, dtype=torch.uint8)
    return b


def _notes(b):
    ok(lib().vae_extract_notes(b["rolls"].data_ptr(), 2, 8, 32, 0.5, 0.3, 1, 1, b["events"].data_ptr(), b["peaks"].data_ptr(), 64, b["offsets"].data_ptr(),
                               b["cleaned"].data_ptr(), st()), "vae_extract_notes")


def _make_nearest():
    b = Bufs()
    rng = np.random.default_rng(18)
    planes = lambda n: torch.from_numpy((rng.integers(0, 256, (n, 8, 4)) & rng.integers(0, 256, (n, 8, 4))).astype(np.uint8))
    b.inp("queries", planes(3), poison=0xFF); b.inp("rolls", planes(20), poison=0xFF)
    b.inp("exclude", torch.tensor([0, -1, 5], dtype=torch.int64), poison=-1)
    for s in (0, 3):
        i32 = dict(dtype=torch.int32)
        b.outp(f"index{s}", 3, 3, dtype=torch.int64); b.outp(f"distance{s}", 3, 3, **i32); b.outp(f"shift{s}", 3, 3, 2, **i32)
        b.outp(f"intersection{s}", 3, 3, **i32); b.outp(f"query_cells{s}", 3, **i32)
    return b


def _nearest(b):
    for s in (0, 3):
        ok(lib().vae_nearest_rolls(b["queries"].data_ptr(), 3, b["rolls"].data_ptr(), 20, 8, 32, 1, 2, b["exclude"].data_ptr(), 3, s,
                                   b[f"index{s}"].data_ptr(), b[f"distance{s}"].data_ptr(), b[f"shift{s}"].data_ptr(), b[f"intersection{s}"].data_ptr(),
                                   b[f"query_cells{s}"].data_ptr(), st()), "vae_nearest_rolls")


def _kernel_cases():
    return [
        net_case("log_likelihood/bf16", ("vae_log_likelihood",), ("bf16",) + R32, _loglik, _setup_loglik, max_batch=8),
        Case("adamw_step", ("vae_adamw_step",), lambda: _make_opt(False), _adamw),
        Case("grad_norm+adamw_step_clipped", ("vae_grad_norm", "vae_adamw_step_clipped"), lambda: _make_opt(True), _adamw_clipped),
        Case("elbo_generic", ("vae_elbo_generic",), _make_elbo, _elbo("generic")),
        Case("elbo_generic_ex", ("vae_elbo_generic_ex",), _make_elbo, _elbo("ex")),
        Case("elbo_generic_kl", ("vae_elbo_generic_kl",), _make_elbo, _elbo("kl")),
        Case("elbo_generic_w", ("vae_elbo_generic_w",), _make_elbo, _elbo("w")),
        Case("total_correlation", ("vae_total_correlation",), _make_tc, _tc),
        Case("latent_stats", ("vae_latent_stats",), _make_latent_stats, _latent_stats),
        Case("recon_metrics", ("vae_recon_metrics",), _make_recon_metrics, _recon_metrics),
        Case("synth_pianoroll", ("vae_synth_pianoroll",), _make_synth, _synth),
        Case("expand_stimuli/device", ("vae_expand_stimuli",), _make_expand(False), _expand),
        Case("expand_stimuli/pinned", ("vae_expand_stimuli",), _make_expand(True), _expand),
        Case("gather_rolls+augment_params", ("vae_gather_rolls", "vae_augment_params"), _make_gather, _gather),
        Case("extract_notes", ("vae_extract_notes",), _make_notes, _notes),
        Case("nearest_rolls", ("vae_nearest_rolls",), _make_nearest, _nearest),
    ]


# ---- two streams ---------------------------------------------------------------------------------------------------------------------
def _two_streams(n):
    """Forward and loss on the current stream, the backward on a second one that waits for it; the results are ordered on the second."""
    s1 = torch.cuda.current_stream()
    n.forward(1); n.loss()
    if s1 == torch.cuda.default_stream():
        n.backward()
        return None
    s2 = torch.cuda.Stream()
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        n.backward()
    return s2


def _overlapped_allreduce(n):
    n.forward(1); n.loss(); n.backward_part(1)
    comm = C.c_void_p()
    ok(lib().vae_comm_stream(n.h, st(), C.byref(comm)), "vae_comm_stream")
    ok(lib().vae_allreduce_grads(n.h, n.b["grads"].data_ptr(), 1, n.dec[0], n.dec[1], 1, comm.value), "vae_allreduce_grads")
    n.backward_part(2)


COMM_CFG = ("f32", 64, 16, 6, True)     # the shape of test_library_allreduce_single_rank_rccl


def _comm_cases():
    return [
        net_case("comm/part1_allreduce_on_comm_stream_part2", ("vae_forward", "vae_loss", "vae_backward_part", "vae_comm_stream", "vae_allreduce_grads"),
                 COMM_CFG, _overlapped_allreduce, comm=True),
        net_case("comm/train_step_fused_exchange1", ("vae_train_step_fused",), COMM_CFG, lambda n: n.train_step_fused(1), Net.moments, comm=True),
        net_case("comm/train_step_fused_exchange2", ("vae_train_step_fused",), COMM_CFG, lambda n: n.train_step_fused(2), Net.moments, comm=True),
    ]


STEP_CASES = _step_cases()
READBACK_CASES = _readback_cases()
KERNEL_CASES = _kernel_cases()
TWO_STREAM_CASES = [net_case(f"two_streams/{d}", ("vae_forward", "vae_loss", "vae_backward"), (d,) + R32, _two_streams) for d in ("f32", "bf16")]
COMM_CASES = _comm_cases()
CASES = STEP_CASES + READBACK_CASES + KERNEL_CASES + TWO_STREAM_CASES + COMM_CASES      # the C-ABI case table


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("VAE_STREAM_RECORD")
    if path:
        sh.write_record(path)


def test_control_sees_the_poison():
    """The harness can see a violation: an op on the default stream racing the staged copy on the delayed stream reads NaN."""
    s = sh.case_stream()                     # (fails when none of the streams tried lets the control see the poison)
    print("streams tried:", sh._case_stream["tried"])
    c = sh.control(s)                        # and once more on the stream the cases use
    print(c)
    assert c["pending"], "the chain was over before the racing op had run"
    assert c["saw_poison"] and c["all_poison"], "an op that is NOT ordered on the stream saw the true values: the harness is blind"
    assert c["settled"] and c["chain_ms"] >= sh.DELAY_MS


@pytest.mark.parametrize("case", STEP_CASES + READBACK_CASES + KERNEL_CASES + TWO_STREAM_CASES, ids=repr)
def test_stream_contract(case):
    sh.check_case(case, EXEMPT)


@pytest.fixture(scope="module")
def single_rank_group():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29577")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", COMM_CASES, ids=repr)
def test_stream_contract_with_a_communicator(case, single_rank_group):
    sh.check_case(case, EXEMPT)


def test_exchange_1_and_2_give_equal_bits(single_rank_group):
    """include/vae_step.h: "1 and 2 need vae_comm_init and produce bit-identical results" - on a delayed non-default stream."""
    res = [sh.stream_run(c)[0] for c in COMM_CASES[1:]]     # (each compared with its own default-stream run above)
    for name in res[0]:
        assert sh.same_bits(res[0][name], res[1][name]), name


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
def _py_model(dtype="bf16"):
    from tests.util import make_model
    from torch_vae_amd.optim import FusedAdamW
    H, L, B, gen = R32[0], R32[1], R32[2], R32[3]
    m = make_model(H, L, gen, dtype, _params(H, L, gen))
    opt = FusedAdamW([{"params": list(m.encoder.parameters())}, {"params": list(m.decoder.parameters())}], lr=LR, weight_decay=WD)
    opt._bind()
    b = Bufs()
    b.keep += [m, opt]
    inp = _inputs(H, L, B)
    b.inp("x", inp["x"]); b.inp("eps", inp["eps"])
    b.adopt("params", m._flat, inout=True); b.adopt("bn_running", m._bnflat, inout=True)
    b.adopt("num_batches_tracked", m._nbt, inout=True, poison=0); b.adopt("grads", m._gflat, inout=True)
    b.adopt("exp_avg", opt._m, inout=True); b.adopt("exp_avg_sq", opt._v, inout=True)
    return b


def _py_reset(b):
    m, opt = b.keep[0], b.keep[1]
    opt._step = 0
    opt._step_t.zero_()             # (a host tensor)
    m._fwd_count = 0
    m._ll_count = 0


def _py_fused_steps(b):
    from torch_vae_amd.train import fused_step
    m, opt = b.keep[0], b.keep[1]
    for i in range(3):
        out3, xhat = fused_step(m, opt, b["x"], eps=b["eps"])
        b.out[f"out3_{i}"] = out3.clone()
    b.out["xhat"] = xhat


def _py_autograd(b):
    m, opt = b.keep[0], b.keep[1]
    m.train()
    m.set_next_eps(b["eps"])
    out = m(b["x"])
    lo = m.loss(out)
    opt.zero_grad()
    lo["loss"].backward()           # the autograd engine's thread, on the forward's stream
    opt.step()
    b.out["loss"] = torch.stack([lo["loss"].detach(), lo["reconstruction_loss"].detach(), lo["kld_loss"].detach()])
    b.out["xhat"] = out["output"].detach()


def _make_accumulator():
    from torch_vae_amd.evaluation import ReconMetricsAccumulator
    b = _make_recon_metrics()
    acc = ReconMetricsAccumulator(thresholds=(0.5, 0.3))
    first = torch.from_numpy(np.random.default_rng(20).random((2, 5000))).float().cuda()
    acc.update(first, (first > 0.8).float())                   # a state that is not the empty one
    b.out.clear()
    b.adopt("state", acc._state, inout=True, poison=0)
    b.keep.append(acc)
    return b


def _accumulate(b):
    b.keep[0].update(b["xhat"], b["target"])


def _make_loader_notes():
    from torch_vae_amd.data import DevicePianorollLoader, PianorollDataset
    b = _py_model("bf16")
    rng = np.random.default_rng(19)
    ds = PianorollDataset(torch.from_numpy((rng.random((10, 32, 48)) < 0.1).astype(np.float32)), storage="bits")
    sq = PianorollDataset(torch.from_numpy((rng.random((12, 32, 32)) < 0.1).astype(np.float32)), storage="bits")
    b.adopt("rolls", ds.data, poison=0xFF); b.adopt("train_rolls", sq.data, poison=0xFF)
    b.keep += [DevicePianorollLoader(ds, 4, width=32, train=True, seed=3, max_pitch_shift=2, max_time_shift=3), sq]
    return b


def _loader_notes(b):
    from torch_vae_amd.evaluation import nearest_rolls
    m, loader, sq = b.keep[0], b.keep[2], b.keep[3]
    x, _ = next(iter(loader))
    b.out["batch"] = x
    notes = m.sample_notes(4, seed=5, max_notes=256, return_rolls=True, cleaned=True)
    # slots past the count are not written and hold whatever the allocator returned: compare the written ones (a device-side mask)
    written = torch.arange(256, device=x.device) < notes["total"]
    b.out["notes_events"] = torch.where(written[:, None], notes["events"], torch.zeros_like(notes["events"]))
    b.out["notes_peaks"] = torch.where(written, notes["peaks"], torch.zeros_like(notes["peaks"]))
    for k in ("offsets", "cleaned", "rolls"):
        b.out["notes_" + k] = notes[k]
    near = nearest_rolls(notes["rolls"], sq, k=2, max_pitch_shift=1, max_time_shift=1)
    for k in ("index", "distance", "shift", "intersection", "query_cells"):
        b.out["near_" + k] = near[k]


def _numbers(d):
    """The numbers of a result dict (sorted by key, lists flattened) as one float64 device tensor."""
    flat = []
    for k in sorted(d):
        v = d[k]
        flat += [float(e) for e in v] if isinstance(v, (list, tuple)) else [float(v)] if isinstance(v, (int, float)) else []
    assert flat, d
    return torch.tensor(flat, dtype=torch.float64).cuda()


class _Batches:
    """Four host batches as a loader.  When the loop comes back for a fifth, every step has been enqueued and the epoch's closing
    read of the loss sum has not happened yet: that is where the case asks whether the stream is still held up."""

    def __init__(self, batches, bufs):
        self.batches, self.bufs = batches, bufs

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        yield from self.batches
        if self.bufs.probe is not None:
            self.bufs.checkpoint = self.bufs.probe()


def _make_epoch():
    from types import SimpleNamespace
    from torch_vae_amd.train import pack_bits
    b = _py_model("bf16")
    m, opt = b.keep[0], b.keep[1]
    rng = np.random.default_rng(21)
    batches = []
    for i in range(4):                                          # four batches of bit planes in pinned host memory
        planes = pack_bits(torch.from_numpy((rng.random((4, 1, 32, 32)) < 0.1).astype(np.float32)))
        batches.append((b.inp(f"planes{i}", planes, poison=0xFF, pinned=True), torch.zeros(4, dtype=torch.long)))
    # (a rank other than 0 prints nothing: no step's scalars are read back, the epoch's one read is the loss sum at its end)
    config = SimpleNamespace(log_interval=100, print_interval=None, global_rank=1)
    b.keep += [_Batches(batches, b), torch.optim.lr_scheduler.LambdaLR(opt, lambda step: 1.0), config]
    return b


def _epoch(b):
    from torch_vae_amd.train import train_one_epoch
    m, opt, batches, sched, config = b.keep
    torch.manual_seed(3)                                        # the loop draws eps from torch's device generator
    results, steps, seen = train_one_epoch(config, m, opt, sched, m.loss, batches, device="cuda", epoch=1)
    assert (steps, seen) == (4, 16)
    b.out["results"] = _numbers(results)


def _make_evaluate():
    from torch_vae_amd.data import DevicePianorollLoader, PianorollDataset
    b = _py_model("bf16")
    rng = np.random.default_rng(22)
    sq = PianorollDataset(torch.from_numpy((rng.random((12, 32, 32)) < 0.1).astype(np.float32)), storage="bits")
    b.adopt("rolls", sq.data, poison=0xFF)
    b.keep += [DevicePianorollLoader(sq, 4, train=False), sq]
    return b


def _evaluate(b):
    from torch_vae_amd.evaluation import evaluate, sample_novelty
    m, loader, sq = b.keep[0], b.keep[2], b.keep[3]
    torch.manual_seed(4)                                        # the eval forward draws eps from torch's device generator
    res = evaluate(loader, m, "cuda", verbosity=0, nll_samples=2, latent_rolls=4, note_thresholds=(0.5, 0.3),
                   note_events=dict(onset_threshold=0.5, min_duration=1))
    b.out["evaluate"] = _numbers(res)
    summary, near, notes = sample_novelty(m, sq, 4, seed=5, k=2, max_pitch_shift=1, max_time_shift=1, max_notes=256)
    b.out["novelty_summary"] = _numbers(summary)
    for k in ("index", "distance", "shift", "intersection", "query_cells"):
        b.out["near_" + k] = near[k]
    m.train()


PY_CASES = [
    Case("python/fused_step_x3", ("vae_train_step_fused",), _py_model, _py_fused_steps, dtype="bf16", reset=_py_reset, sync_free=False, warmups=2),
    Case("python/autograd_step", ("vae_forward", "vae_loss", "vae_backward", "vae_adamw_step"), lambda: _py_model("f32"), _py_autograd, dtype="f32",
         reset=_py_reset, sync_free=False, warmups=2),
    Case("python/recon_metrics_accumulator", ("vae_recon_metrics",), _make_accumulator, _accumulate, sync_free=False, warmups=2),
    Case("python/loader_batch+sample_notes+nearest_rolls", ("vae_gather_rolls", "vae_decode", "vae_extract_notes", "vae_nearest_rolls"),
         _make_loader_notes, _loader_notes, dtype="bf16", reset=_py_reset, sync_free=False, warmups=2),
    Case("python/train_one_epoch_pinned_bit_planes", ("vae_expand_stimuli", "vae_train_step_fused"), _make_epoch, _epoch, dtype="bf16", reset=_py_reset,
         sync_free=False, warmups=2, reads_back="train_one_epoch ends with one read of the epoch's loss sum; pending is taken when all four steps are enqueued, in front of it"),
    Case("python/evaluate+novelty_summary", ("vae_forward", "vae_log_likelihood", "vae_latent_stats", "vae_recon_metrics", "vae_extract_notes",
                                             "vae_decode", "vae_nearest_rolls", "vae_gather_rolls"), _make_evaluate, _evaluate, dtype="bf16",
         reset=_py_reset, sync_free=False, warmups=2, reads_back="evaluate() and novelty_summary() return Python numbers: they read back by design"),
]


@pytest.mark.parametrize("case", PY_CASES, ids=repr)
def test_stream_contract_python_layer(case):
    sh.check_case(case, EXEMPT)
