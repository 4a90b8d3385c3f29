"""Host side (no GPU) of the weight-averaging tests: the numpy reference (tests/average_ref.py) against
torch.optim.swa_utils.AveragedModel; the weight rule at its edges; the training loop's schedule; the refusals of
include/vae_average.h through fake, never dereferenced pointers and those of the Python layer; the header / export / binding
bookkeeping; and the arithmetic update_bn's recovery of a batch statistic rests on."""
import ctypes as C
import inspect
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch
from torch import nn
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from tests import average_ref as R
from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_average.h")
OTHER_HEADERS = ("vae_step.h", "vae_mixture.h", "vae_music.h", "vae_fidelity.h", "vae_attributes.h", "vae_denoise.h")
A0, S0, A1, S1, ST, OPT = 1 << 12, 1 << 30, 1 << 32, 1 << 34, 1 << 36, (1 << 38) + 8      # fake device addresses, far apart
NAN, INF = float("nan"), float("inf")


# ---- the reference against torch's AveragedModel ---------------------------------------------------------------------------------
def small_net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(1, 4, 3, padding=1), nn.BatchNorm2d(4), nn.LeakyReLU(), nn.Flatten(), nn.Linear(4 * 6 * 6, 5))


def float_state(module):
    return {k: v.detach().numpy().astype(np.float64) for k, v in module.state_dict().items() if v.dtype.is_floating_point}


@pytest.mark.parametrize("case", ["ema_0.9", "ema_0.999", "swa"])
def test_reference_against_torch_averaged_model(case):
    net = small_net()
    if case == "swa":
        torch_avg, ref = AveragedModel(net, use_buffers=True), R.AverageRef("swa")
    else:
        decay = float(case.split("_")[1])
        torch_avg, ref = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True), R.AverageRef("ema", decay=decay)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    g = torch.Generator().manual_seed(5)
    keys = sorted(float_state(net))
    assert any("running_mean" in k for k in keys) and any("running_var" in k for k in keys)
    for step in range(12):
        x = torch.randn(8, 1, 6, 6, generator=g)
        net.train()
        opt.zero_grad()
        net(x).square().mean().backward()          # (the train-mode forward moves the BatchNorm buffers too)
        opt.step()
        torch_avg.update_parameters(net)
        state = float_state(net)
        assert ref.update([state[k] for k in keys]) and ref.n_averaged == step + 1
        want = float_state(torch_avg.module)
        for k, got in zip(keys, ref.avg):
            assert np.abs(got - want[k]).max() <= 1e-6 * max(np.abs(want[k]).max(), 1e-30), (case, step, k)
    assert int(torch_avg.n_averaged) == ref.n_averaged == 12
    # the average moved away from the model (the comparison had a subject)
    assert max(np.abs(a - float_state(net)[k]).max() for k, a in zip(keys, ref.avg)) > 1e-4


# ---- the weight rule ----------------------------------------------------------------------------------------------------------------
def test_weight_rule():
    for kind in (R.EMA, R.EQUAL):
        assert R.weight(kind, 0, 0.3, 7.0) == (True, 1.0)
    assert [R.weight(R.EQUAL, n)[1] for n in (1, 2, 3, 9)] == [1 / 2, 1 / 3, 1 / 4, 1 / 10]
    assert R.weight(R.EMA, 5, 0.999) == (False, 1.0 - 0.999)
    # decay 0: the average follows the source (w = 1); decay 1: it never moves after the first copy (w = 0)
    assert R.weight(R.EMA, 1, 0.0) == (False, 1.0) and R.weight(R.EMA, 1, 1.0) == (False, 0.0)
    assert R.weight(R.EMA, 4, 1.0, warmup=10.0) == (False, 1.0 - 5 / 14)
    # the warm-up (1 + n) / (warmup + n) takes w = 1 - d down through 0.5, where the lerp changes branch, and ends at 1 - decay
    ws = [R.weight(R.EMA, n, 0.999, warmup=10.0)[1] for n in range(1, 20000)]
    assert all(a >= b for a, b in zip(ws, ws[1:])) and ws[0] > 0.5 > ws[-1]
    cross = next(n for n in range(1, 100) if R.weight(R.EMA, n, 0.999, warmup=10.0)[1] < 0.5)
    assert cross == 9 and R.weight(R.EMA, 8, 0.999, warmup=10.0)[1] == 0.5       # (1 + 8) / (10 + 8) = 0.5 exactly: the other branch
    assert ws[-1] == 1.0 - 0.999 and R.weight_f32(R.EMA, 19999, 0.999, 10.0) == float(np.float32(1.0 - 0.999))
    # the lerp and the gate
    assert np.array_equal(R.lerp([1.0, 2.0], [3.0, 6.0], 0.25), [1.5, 3.0]) and np.array_equal(R.lerp([9.0], [3.0], 0.1, copy=True), [3.0])
    ref = R.AverageRef("swa")
    assert ref.update([np.array([2.0])], opt_step=0) and not ref.update([np.array([4.0])], opt_step=0)
    assert (ref.n_averaged, ref.seen_step, ref.avg[0].tolist()) == (1, 0, [2.0])
    assert ref.update([np.array([4.0])], opt_step=1) and ref.avg[0].tolist() == [3.0] and ref.last_weight == 0.5
    assert ref.update([np.array([6.0])]) and ref.seen_step == 1 and ref.n_averaged == 3 and abs(ref.avg[0][0] - 4.0) < 1e-15


def test_the_schedule_is_a_function_of_total_step():
    from torch_vae_amd.averaging import schedule_due
    assert [t for t in range(1, 9) if schedule_due(t, 2, 2)] == [2, 4, 6, 8]
    assert [t for t in range(1, 12) if schedule_due(t, 5, 3)] == [5, 8, 11]
    assert [t for t in range(1, 5) if schedule_due(t)] == [1, 2, 3, 4]
    assert [t for t in range(1, 8) if schedule_due(t, 0, 10)] == []
    src = inspect.getsource(__import__("torch_vae_amd.train", fromlist=["train_one_epoch"]).train_one_epoch)
    body = src[src.index("scheduler.step()"):]
    assert body.index("total_step += 1") < body.index("averager.due(total_step)") < body.index("averager.update(optimizer)")


# ---- the Python refusals ---------------------------------------------------------------------------------------------------------
def test_python_refusals():
    from torch_vae_amd.averaging import WeightAverage
    from torch_vae_amd.models import VanillaVAE
    m = VanillaVAE(1, 16, 32)
    with pytest.raises(TypeError, match="VanillaVAE"):
        WeightAverage(nn.Linear(2, 2))
    for kw, word in ((dict(kind="mean"), "kind"), (dict(kind=0), "kind"), (dict(decay=1.5), "decay"), (dict(decay=-0.1), "decay"),
                     (dict(decay=NAN), "decay"), (dict(decay="0.9"), "decay"), (dict(decay=True), "decay"), (dict(warmup=-1.0), "warmup"),
                     (dict(warmup=INF), "warmup"), (dict(warmup=NAN), "warmup"), (dict(use_buffers=1), "use_buffers")):
        with pytest.raises(ValueError, match=word):
            WeightAverage(m, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):          # (every argument fine: it is the device that is missing)
        WeightAverage(m, kind="swa", decay=1.0, warmup=0.0, use_buffers=False)
    assert WeightAverage.from_config(Namespace(), m) is None and WeightAverage.from_config(Namespace(weight_average=None, ema_decay=0.5), m) is None
    for cfg, word in ((Namespace(weight_average="ema", avg_every=0), "avg_every"), (Namespace(weight_average="ema", avg_start_step=-1), "avg_start_step"),
                      (Namespace(weight_average="ema", avg_every=2.0), "avg_every"), (Namespace(weight_average="median"), "kind"),
                      (Namespace(weight_average="ema", ema_decay=2.0), "decay"), (Namespace(weight_average="ema", ema_warmup=-3), "warmup")):
        with pytest.raises(ValueError, match=word):
            WeightAverage.from_config(cfg, m)
    with pytest.raises(RuntimeError, match="HIP device"):
        WeightAverage.from_config(Namespace(weight_average="swa", avg_start_step=3, avg_every=2), m)
    sig = inspect.signature(WeightAverage.__init__)
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("self", "model")} == dict(kind="ema", decay=0.999, warmup=0.0, use_buffers=True)
    import torch_vae_amd
    assert "WeightAverage" in torch_vae_amd.__all__ and torch_vae_amd.WeightAverage is WeightAverage


def test_checkpoint_modules_only_change_with_an_average():
    from torch_vae_amd import utils
    from torch_vae_amd.models import VanillaVAE
    m = VanillaVAE(1, 16, 32)
    assert list(utils.checkpoint_modules(m, "o", "s")) == ["encoder", "decoder", "optimizer", "scheduler"]
    m.weight_average = marker = object()
    mods = utils.checkpoint_modules(m, "o", "s")
    assert list(mods) == ["encoder", "decoder", "optimizer", "scheduler", "weight_average"] and mods["weight_average"] is marker
    assert "weight_average" not in m.state_dict() and not any("weight_average" in k for k in m.state_dict())


# ---- the C refusals -----------------------------------------------------------------------------------------------------------------
def update(L, avg0=A0, src0=S0, n0=1000, sc0=1.0, avg1=A1, src1=S1, n1=96, sc1=1.0, kind=0, decay=0.999, warmup=0.0, opt=OPT, state=ST):
    return L.vae_average_update(avg0, src0, n0, sc0, avg1, src1, n1, sc1, kind, decay, warmup, opt, state, None)


def swap(L, a0=A0, b0=S0, n0=1000, a1=A1, b1=S1, n1=96):
    return L.vae_average_swap(a0, b0, n0, a1, b1, n1, None)


def state_init(L, state=ST, opt=OPT, n=0):
    return L.vae_average_state_init(state, opt, n, None)


ALIGN_U, ALIGN_S, ALIGN_ST = "avg, src must be 16-byte aligned", "a, b must be 16-byte aligned", "state must be 16-byte, opt_step 8-byte aligned"
OVER_U, OVER_S = "avg must not overlap src or the other avg", "the buffers must not overlap"
REFUSALS = {
    "update/null_state": (lambda L: update(L, state=None), "null pointer (state)"),
    "update/null_avg": (lambda L: update(L, avg0=None), "null pointer (avg, src)"),
    "update/null_src": (lambda L: update(L, src0=None), "null pointer (avg, src)"),
    "update/null_second_avg": (lambda L: update(L, avg1=None), "null pointer (avg, src)"),
    "update/null_second_src": (lambda L: update(L, src1=None), "null pointer (avg, src)"),
    "update/negative_n": (lambda L: update(L, n0=-1), "n must be >= 0"),
    "update/negative_second_n": (lambda L: update(L, n1=-5), "n must be >= 0"),
    "update/n_above_2^40": (lambda L: update(L, n0=(1 << 40) + 1), "n must stay within 2^40"),
    "update/in_place": (lambda L: update(L, src0=A0), OVER_U),
    "update/src_inside_avg": (lambda L: update(L, src0=A0 + 4000 - 16), OVER_U),
    "update/avg_inside_second_src": (lambda L: update(L, avg0=S1 + 16, n0=8), OVER_U),
    "update/second_avg_inside_src": (lambda L: update(L, avg1=S0 + 3984), OVER_U),
    "update/avgs_overlap": (lambda L: update(L, avg1=A0 + 3984), OVER_U),
    "update/avg_over_state": (lambda L: update(L, avg0=ST - 3984), "avg must not overlap the state"),
    "update/decay_above_1": (lambda L: update(L, decay=1.0000001), "decay must lie in [0, 1]"),
    "update/decay_negative": (lambda L: update(L, decay=-1e-9), "decay must lie in [0, 1]"),
    "update/decay_nan": (lambda L: update(L, decay=NAN), "decay must lie in [0, 1]"),
    "update/warmup_negative": (lambda L: update(L, warmup=-1.0), "warmup must be finite and >= 0"),
    "update/warmup_nan": (lambda L: update(L, warmup=NAN), "warmup must be finite and >= 0"),
    "update/warmup_inf": (lambda L: update(L, warmup=INF), "warmup must be finite and >= 0"),
    "update/kind_2": (lambda L: update(L, kind=2), "kind must be VAE_AVG_EMA or VAE_AVG_EQUAL"),
    "update/kind_negative": (lambda L: update(L, kind=-1), "kind must be VAE_AVG_EMA or VAE_AVG_EQUAL"),
    "update/scale_inf": (lambda L: update(L, sc0=INF), "src_scale must be finite"),
    "update/second_scale_nan": (lambda L: update(L, sc1=NAN), "src_scale must be finite"),
    "update/avg_plus_4": (lambda L: update(L, avg0=A0 + 4), ALIGN_U),
    "update/src_plus_8": (lambda L: update(L, src0=S0 + 8), ALIGN_U),
    "update/second_src_plus_12": (lambda L: update(L, src1=S1 + 12), ALIGN_U),
    "update/state_plus_8": (lambda L: update(L, state=ST + 8), ALIGN_ST),
    "update/opt_step_plus_4": (lambda L: update(L, opt=OPT + 4), ALIGN_ST),
    "update/refused_with_n_0_too": (lambda L: update(L, n0=0, n1=0, decay=2.0), "decay must lie in [0, 1]"),
    "swap/null_a": (lambda L: swap(L, a0=None), "null pointer (a, b)"),
    "swap/null_second_b": (lambda L: swap(L, b1=None), "null pointer (a, b)"),
    "swap/negative_n": (lambda L: swap(L, n1=-1), "n must be >= 0"),
    "swap/same_buffer": (lambda L: swap(L, b0=A0), OVER_S),
    "swap/b_inside_a": (lambda L: swap(L, b0=A0 + 3984), OVER_S),
    "swap/pairs_share_a": (lambda L: swap(L, a1=A0), OVER_S),
    "swap/second_b_inside_first_b": (lambda L: swap(L, b1=S0 + 16), OVER_S),
    "swap/a_plus_4": (lambda L: swap(L, a0=A0 + 4), ALIGN_S),
    "swap/second_b_plus_8": (lambda L: swap(L, b1=S1 + 8), ALIGN_S),
    "state_init/null_state": (lambda L: state_init(L, state=None), "null pointer (state)"),
    "state_init/state_plus_8": (lambda L: state_init(L, state=ST + 8), ALIGN_ST),
    "state_init/opt_step_plus_2": (lambda L: state_init(L, opt=OPT + 2), ALIGN_ST),
    "state_init/negative_n": (lambda L: state_init(L, n=-1), "n_averaged must be >= 0"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = REFUSALS[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == "vae_average_" + case.split("/")[0] + ": " + want


def test_absent_segments_are_not_looked_at():
    """(nothing is launched: n = 0 in both segments returns before any device work)"""
    L = _lib.lib()
    assert update(L, n0=0, n1=0) == 0 and update(L, avg0=None, src0=None, n0=0, avg1=None, src1=None, n1=0, opt=None) == 0
    assert update(L, avg0=A0 + 4, src0=A0 + 4, n0=0, n1=0, decay=0.0, warmup=5.0, kind=1) == 0       # an absent segment's pointers: ignored
    assert swap(L, n0=0, n1=0) == 0 and swap(L, a0=None, b0=None, n0=0, a1=None, b1=None, n1=0) == 0


# ---- the header, the exports and the binding -----------------------------------------------------------------------------------------
def _header(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def test_header_declares_exactly_the_average_exports():
    declared = set(re.findall(r"\b(vae_[a-z0-9_]+)\s*\(", _header(HEADER)))
    assert declared == set(_lib.AVERAGE_EXPORTS) == {"vae_average_update", "vae_average_swap", "vae_average_state_init"}
    L = _lib.lib()
    assert not [n for n in _lib.AVERAGE_EXPORTS if not hasattr(L, n)]
    others = (set(_lib.EXPORTS) | set(_lib.MIXTURE_EXPORTS) | set(_lib.MUSIC_EXPORTS) | set(_lib.FIDELITY_EXPORTS) | set(_lib.ATTR_EXPORTS)
              | set(_lib.DENOISE_EXPORTS))
    assert not set(_lib.AVERAGE_EXPORTS) & others
    assert L.vae_abi_version() == 1
    text = open(HEADER).read()
    for name, value in (("EMA", _lib.AVG_EMA), ("EQUAL", _lib.AVG_EQUAL), ("STATE_BYTES", _lib.AVG_STATE_BYTES)):
        assert int(re.search(rf"#define VAE_AVG_{name} (\d+)", text).group(1)) == value, name
    assert (_lib.AVG_EMA, _lib.AVG_EQUAL) == (R.EMA, R.EQUAL) and _lib.AVG_STATE_BYTES == 32
    for name in OTHER_HEADERS:
        assert "vae_average_" not in _header(os.path.join(ROOT, "include", name)), name


CTYPE = {"float*": C.c_void_p, "const float*": C.c_void_p, "void*": C.c_void_p, "const int64_t*": C.c_void_p, "vae_stream_t": C.c_void_p,
         "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "double": C.c_double}


def test_binding_signatures_agree_with_the_header():
    L = _lib.lib()
    found = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(vae_\w+)\s*\(([^;{}]*?)\)\s*;", _header(HEADER))}
    assert sorted(found) == sorted(_lib.AVERAGE_EXPORTS)
    for name, params in found.items():
        types = [CTYPE[" ".join(a.split()[:-1])] for a in (p.strip() for p in params.split(","))]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == types, name
        assert params.split(",")[-1].split()[0] == "vae_stream_t", name            # the stream is the last argument
    # no argument of the update changes from call to call: no step number, no parity, no weight
    names = [a.split()[-1] for a in found["vae_average_update"].split(",")]
    assert names == ["avg0", "src0", "n0", "src_scale0", "avg1", "src1", "n1", "src_scale1", "kind", "decay", "warmup", "opt_step", "state", "stream"]


def test_the_build_has_the_translation_unit():
    mk = open(os.path.join(ROOT, "torch_vae_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert "vae_average.hip" in srcs and "weight_average.cuh" in hdrs and "../../include/vae_average.h" in hdrs


# ---- update_bn: what a forward from zeroed buffers leaves, and what comes back ---------------------------------------------------------
def test_update_bn_recovers_the_batch_statistic():
    from torch_vae_amd.averaging import BN_RECOVER
    assert BN_RECOVER == 10.0
    rng = np.random.default_rng(17)
    b = np.concatenate([rng.standard_normal(200000), rng.uniform(1e-6, 1e-3, 50000), rng.uniform(1e3, 1e6, 50000),
                        np.exp(rng.uniform(-60, 60, 100000)) * rng.choice([-1.0, 1.0], 100000)]).astype(np.float32)
    left = np.float32(0.1) * b                      # running' = (1 - 0.1f) * 0 + 0.1f * b, in float32
    back = R.recovered_bn_stat(left)
    b64 = b.astype(np.float64)
    rel = np.abs(back - b64) / np.abs(b64)
    print("update_bn recovery: largest relative error", rel.max(), "bound", 2.0 ** -22)
    assert rel.max() <= 2.0 ** -22
    # the cumulative mean of three such batches, folded with w = 1, 1/2, 1/3, against the float64 mean
    stats = [np.float32(0.1) * rng.standard_normal(1000).astype(np.float32) for _ in range(3)]
    ref = R.AverageRef("swa")
    for s in stats:
        ref.update([s], scales=[10.0])
    mean = np.mean([R.recovered_bn_stat(s) for s in stats], axis=0)
    assert np.abs(ref.avg[0] - mean).max() <= 1e-15 * np.abs(mean).max() + 1e-18
