"""Host side (no GPU) of the attribute-regularisation tests: the numpy reference (tests/attr_ref.py) against torch autograd on the CPU,
against tests/music_ref.py and against a textbook tau-b; the refusals of include/vae_attributes.h through fake, never dereferenced
pointers; the header / export bookkeeping; the stream-case table of tests/test_attr_gpu.py; and the argument checks of the Python
layer."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attr_ref as R
from tests import music_ref
from tests import test_attr_gpu as gpu_cases
from torch_vae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vae_attributes.h")
OTHER_HEADERS = ("vae_step.h", "vae_mixture.h", "vae_music.h", "vae_fidelity.h")
P = 4096          # a fake device address, 16-byte aligned


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def torch_regularizer(z, a, delta):
    """F.l1_loss(tanh(delta Dz), sign(Da)) in f64 and its gradient, by autograd"""
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    at = torch.from_numpy(a)
    loss = F.l1_loss(torch.tanh(delta * (zt[:, None] - zt[None, :])), torch.sign(at[:, None] - at[None, :]))
    loss.backward()
    return loss.item(), zt.grad.numpy()


@pytest.mark.parametrize("kind", ["random", "heavy_ties", "all_equal"])
@pytest.mark.parametrize("B", [1, 2, 5, 33])
def test_reference_loss_and_gradient_equal_torch_autograd(B, kind):
    z, c = R.latent_case(B, 3, seed=100 + B, duplicates=kind == "heavy_ties")
    if kind == "all_equal":
        c[:] = c[0]
    delta = np.float32(10.0)
    pairs = [("note_density", 0), ("mean_pitch", 2), ("polyphony", 1)]
    loss, g = R.regularizer(z, c, pairs, delta, 1.0)
    for k, (name, d) in enumerate(pairs):
        want, want_g = torch_regularizer(z[:, d], R.attribute_values(c, [name])[:, 0], float(delta))
        assert abs(loss[1 + k] - want) <= 1e-12 * max(1.0, abs(want)), (name, loss[1 + k], want)
        assert np.abs(g[:, d] - want_g).max() <= 1e-12 * max(1.0, np.abs(want_g).max()), name
    assert loss[0] == loss[1:].sum()
    if B == 1:
        assert loss.tolist() == [0.0] * 4 and not g[:, :3].any()
    if kind == "all_equal" and B > 1:       # every target sign is 0: the loss is mean |tanh|
        assert loss[1] > 0


def test_reference_counters_equal_the_music_reference():
    rng = np.random.default_rng(3)
    for h, w in ((1, 32), (3, 64), (13, 192), (5, 288)):
        cells = np.stack([R.random_runs(rng, h, w, d) for d in (0.02, 0.1, 0.4)] + [np.zeros((h, w), bool), np.ones((h, w), bool)])
        got = R.counters(cells)
        want = music_ref.features(music_ref.pack(cells.astype(np.uint8)))[:, 2:9]
        assert np.array_equal(R.to_music_columns(got), want), (h, w)
        assert got[3].tolist() == [0, 0, 0, -1, -1, 0, 0, 0]
        assert got[4].tolist() == [h * w, h, h, 0, h - 1, w, 1, w * h * (h - 1) // 2]


def test_reference_attribute_values():
    c = np.array([[0, 0, 0, -1, -1, 0, 0, 0], [6, 2, 2, 3, 7, 4, 2, 31]], np.int32)
    v = R.attribute_values(c, R.NAMES)
    assert v[0].tolist() == [0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    assert v[1].tolist() == [6.0, 2.0, 5.0, 31 / 6, 6 / 4, 2.0, 2.0]
    from torch_vae_amd.attributes import attribute_values
    assert torch.equal(attribute_values(torch.from_numpy(c), R.NAMES), torch.from_numpy(v))          # the package's own, bit for bit
    z, big = R.latent_case(67, 2, seed=5)
    assert torch.equal(attribute_values(torch.from_numpy(big), R.NAMES[::-1]), torch.from_numpy(R.attribute_values(big, R.NAMES[::-1])))


@pytest.mark.parametrize("n", [2, 3, 40])
def test_tau_b_from_the_sums_equals_a_direct_tau_b(n):
    from torch_vae_amd.attributes import tau_b
    z, c = R.latent_case(n, 3, seed=n, ld=3, duplicates=True)
    names = ["note_density", "mean_pitch", "pitch_range"]
    S, tz, ta = R.concordance(z, c, names)
    got = R.tau_b(S, tz, ta, n)
    a = R.attribute_values(c, names)
    for k in range(3):
        for d in range(3):
            want = R.tau_b_direct(z[:, d], a[:, k])
            assert (math.isnan(want) and math.isnan(got[k, d])) or abs(got[k, d] - want) <= 1e-12, (k, d, got[k, d], want)
    mine = tau_b(torch.from_numpy(S), torch.from_numpy(tz), torch.from_numpy(ta), n).numpy()
    assert np.array_equal(np.isnan(mine), np.isnan(got)) and np.allclose(np.nan_to_num(mine), np.nan_to_num(got), rtol=1e-15, atol=0)
    const = R.concordance(np.zeros((n, 1), np.float32), c, names)
    assert np.isnan(R.tau_b(*const, n)).all() and const[1][0] == n * (n - 1) // 2


def test_the_counter_cases_hold_what_the_issue_asks_for():
    cases = R.counter_cases()
    assert gpu_cases.COUNTER_KEYS == list(cases) and len(cases) == len(R.SHAPES) * len(R.COUNTS)
    for (h, w, n), (x, c) in cases.items():
        assert x.shape == (n, h, w) and x.dtype == np.float32 and c.shape == (n, 8) and c.dtype == np.int32
        assert x[0, h // 2, 0] == R.THRESHOLD and (w == 1 or h == 1 or np.isnan(x[0, 0, w - 1]))
        if h > 1:
            assert (x[0, h // 2] >= R.THRESHOLD).all()                     # the run from t = 0 to w - 1
        if n >= 3:
            assert c[1].tolist() == [0, 0, 0, -1, -1, 0, 0, 0] and c[2, 0] == h * w and c[2, 1] == h
        if w > 128 and h > 1:
            assert (x[0, 0, 62:66] >= 0.5).all() and (x[0, 0, 126:130] >= 0.5).all()
    assert max(c[:, 7].max() for _, c in cases.values()) == 64 * 1024 * 1023 // 2


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def counters(L, rolls=P, n=3, h=4, w=32, thr=0.5, out=P):
    return L.vae_attr_roll_counters(rolls, n, h, w, thr, out, None)


def reg(L, z=P, ldz=8, Ld=8, c=P, B=4, npairs=2, attr=(0, 3), dim=(1, 5), delta=10.0, weight=1.0, loss=P, g=P):
    return L.vae_attr_regularizer(z, ldz, Ld, c, B, npairs, None if attr is None else i32(*attr), None if dim is None else i32(*dim), delta, weight,
                                  loss, g, None)


def conc(L, z=P, ldz=8, Ld=8, c=P, N=5, nattr=2, attr=(0, 6), S=P, tz=P, ta=P):
    return L.vae_attr_concordance(z, ldz, Ld, c, N, nattr, None if attr is None else i32(*attr), S, tz, ta, None)


NULLS_R = "null pointer (z, counters, loss, attr, dim)"
NULLS_C = "null pointer (z, counters, attr, S, ties_z, ties_a)"
ALIGN_R = "z, counters and g_z must be 4-byte, loss 8-byte aligned"
ALIGN_C = "z and counters must be 4-byte, S, ties_z and ties_a 8-byte aligned"
REFUSALS = {
    "counters/null_rolls": (lambda L: counters(L, rolls=None), "null pointer (rolls, counters)"),
    "counters/null_counters": (lambda L: counters(L, out=None), "null pointer (rolls, counters)"),
    "counters/negative_n": (lambda L: counters(L, n=-1), "n must be >= 0"),
    "counters/h_0": (lambda L: counters(L, h=0), "h must be in 1..1024"),
    "counters/h_1025": (lambda L: counters(L, h=1025, w=1), "h must be in 1..1024"),
    "counters/w_0": (lambda L: counters(L, w=0), "w must be >= 1"),
    "counters/cells_above_2^20": (lambda L: counters(L, h=1024, w=1025), "a roll (h * w cells) must stay within 2^20"),
    "counters/n_h_w": (lambda L: counters(L, n=(1 << 26) + 1, h=1024, w=1024), "n * h * w must stay within 2^46"),
    "counters/rolls_plus_2": (lambda L: counters(L, rolls=P + 2), "rolls and counters must be 4-byte aligned"),
    "counters/counters_plus_1": (lambda L: counters(L, out=P + 1), "rolls and counters must be 4-byte aligned"),
    "counters/refused_with_n_0_too": (lambda L: counters(L, n=0, h=0), "h must be in 1..1024"),
    "regularizer/null_z": (lambda L: reg(L, z=None), NULLS_R),
    "regularizer/null_counters": (lambda L: reg(L, c=None), NULLS_R),
    "regularizer/null_loss": (lambda L: reg(L, loss=None), NULLS_R),
    "regularizer/null_attr": (lambda L: reg(L, attr=None), NULLS_R),
    "regularizer/null_dim": (lambda L: reg(L, dim=None), NULLS_R),
    "regularizer/B_0": (lambda L: reg(L, B=0), "B must be in 1..4096"),
    "regularizer/B_4097": (lambda L: reg(L, B=4097), "B must be in 1..4096"),
    "regularizer/L_0": (lambda L: reg(L, Ld=0, ldz=0), "L must be in 1..4096"),
    "regularizer/L_4097": (lambda L: reg(L, Ld=4097, ldz=4097), "L must be in 1..4096"),
    "regularizer/ldz_below_L": (lambda L: reg(L, ldz=7), "ldz must be >= L"),
    "regularizer/npairs_0": (lambda L: reg(L, npairs=0), "npairs must be in 1..8"),
    "regularizer/npairs_9": (lambda L: reg(L, npairs=9, attr=(0,) * 9, dim=tuple(range(9)), Ld=16, ldz=16), "npairs must be in 1..8"),
    "regularizer/attribute_7": (lambda L: reg(L, attr=(0, 7)), "unknown attribute (0..6)"),
    "regularizer/attribute_negative": (lambda L: reg(L, attr=(-1, 0)), "unknown attribute (0..6)"),
    "regularizer/dim_L": (lambda L: reg(L, dim=(1, 8)), "dim must be in 0..L-1"),
    "regularizer/dim_negative": (lambda L: reg(L, dim=(-1, 2)), "dim must be in 0..L-1"),
    "regularizer/dim_twice": (lambda L: reg(L, dim=(5, 5)), "a dim is named twice"),
    "regularizer/delta_nan": (lambda L: reg(L, delta=float("nan")), "delta and weight must be finite"),
    "regularizer/delta_inf": (lambda L: reg(L, delta=float("inf")), "delta and weight must be finite"),
    "regularizer/weight_inf": (lambda L: reg(L, weight=float("-inf")), "delta and weight must be finite"),
    "regularizer/delta_0": (lambda L: reg(L, delta=0.0), "delta must be > 0"),
    "regularizer/delta_negative": (lambda L: reg(L, delta=-1.0), "delta must be > 0"),
    "regularizer/z_plus_2": (lambda L: reg(L, z=P + 2), ALIGN_R),
    "regularizer/g_plus_1": (lambda L: reg(L, g=P + 1), ALIGN_R),
    "regularizer/loss_plus_4": (lambda L: reg(L, loss=P + 4), ALIGN_R),
    "concordance/null_z": (lambda L: conc(L, z=None), NULLS_C),
    "concordance/null_attr": (lambda L: conc(L, attr=None), NULLS_C),
    "concordance/null_S": (lambda L: conc(L, S=None), NULLS_C),
    "concordance/null_ties_z": (lambda L: conc(L, tz=None), NULLS_C),
    "concordance/null_ties_a": (lambda L: conc(L, ta=None), NULLS_C),
    "concordance/N_negative": (lambda L: conc(L, N=-1), "N must be in 0..65536"),
    "concordance/N_65537": (lambda L: conc(L, N=65537), "N must be in 0..65536"),
    "concordance/L_0": (lambda L: conc(L, Ld=0, ldz=0), "L must be in 1..4096"),
    "concordance/ldz_below_L": (lambda L: conc(L, ldz=7), "ldz must be >= L"),
    "concordance/nattr_0": (lambda L: conc(L, nattr=0), "nattr must be in 1..7"),
    "concordance/nattr_8": (lambda L: conc(L, nattr=8, attr=(0,) * 8), "nattr must be in 1..7"),
    "concordance/attribute_7": (lambda L: conc(L, attr=(7, 0)), "unknown attribute (0..6)"),
    "concordance/S_plus_4": (lambda L: conc(L, S=P + 4), ALIGN_C),
    "concordance/counters_plus_2": (lambda L: conc(L, c=P + 2), ALIGN_C),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = REFUSALS[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == "vae_attr_" + {"counters": "roll_counters"}.get(case.split("/")[0], case.split("/")[0]) + ": " + want


def test_limits_are_accepted_up_to_the_refusal():
    """(nothing is launched: n = 0 returns before any device work)"""
    L = _lib.lib()
    assert counters(L, n=0, h=1024, w=1024) == 0
    assert counters(L, n=0, h=1, w=1 << 20, thr=float("nan")) == 0
    assert counters(L, n=0, h=7, w=33) == 0


# ---- the header, the exports and the stream-case table ------------------------------------------------------------------------------
def _header(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def test_header_declares_exactly_the_attr_exports():
    declared = set(re.findall(r"\b(vae_[a-z0-9_]+)\s*\(", _header(HEADER)))
    assert declared == set(_lib.ATTR_EXPORTS) == {"vae_attr_roll_counters", "vae_attr_regularizer", "vae_attr_concordance"}
    assert all(n.startswith("vae_attr_") for n in _lib.ATTR_EXPORTS)
    L = _lib.lib()
    assert not [n for n in _lib.ATTR_EXPORTS if not hasattr(L, n)]
    others = set(_lib.EXPORTS) | set(_lib.MIXTURE_EXPORTS) | set(_lib.MUSIC_EXPORTS) | set(_lib.FIDELITY_EXPORTS)
    assert not set(_lib.ATTR_EXPORTS) & others
    assert L.vae_abi_version() == 1
    text = open(HEADER).read()
    for name, value in (("COUNTERS", len(_lib.ATTR_COUNTERS)), ("COUNT", len(_lib.ATTRIBUTES)), ("MAX_PAIRS", _lib.ATTR_MAX_PAIRS),
                        ("MAX_BATCH", _lib.ATTR_MAX_BATCH), ("MAX_DIM", _lib.ATTR_MAX_DIM), ("MAX_ROWS", _lib.ATTR_MAX_ROWS),
                        ("MAX_POINTS", _lib.ATTR_MAX_POINTS)):
        assert int(re.search(rf"#define VAE_ATTR_{name} (\d+)", text).group(1)) == value, name
    macro = {"note_density": "CELLS", "note_count": "NOTES", "pitch_range": "PITCH_RANGE", "mean_pitch": "MEAN_PITCH", "polyphony": "POLYPHONY",
             "onset_steps": "ONSET_STEPS", "used_pitches": "USED_PITCHES"}
    for name, number in _lib.ATTRIBUTES.items():
        assert int(re.search(rf"#define VAE_ATTR_{macro[name]} (\d+)", text).group(1)) == number, name
    assert tuple(_lib.ATTRIBUTES) == R.NAMES and tuple(_lib.ATTR_COUNTERS) == R.COUNTERS


def test_the_other_headers_declare_no_attr_function():
    for name in OTHER_HEADERS:
        assert "vae_attr_" not in _header(os.path.join(ROOT, "include", name)), name


def stream_entry_points():
    found = [m.group(1) for m in re.finditer(r"\b(vae_\w+)\s*\(([^;{}]*?)\)\s*;", _header(HEADER)) if re.search(r"\bvae_stream_t\b", m.group(2))]
    assert len(found) == len(set(found))
    return found


def test_every_stream_entry_point_of_the_header_has_a_stream_case():
    """The rule of tests/test_music_host.py on this header and its own case table."""
    names = stream_entry_points()
    assert sorted(names) == sorted(_lib.ATTR_EXPORTS)
    covered = set()
    for c in gpu_cases.STREAM_CASES:
        assert c.sync_free and c.reads_back is None, c.name
        covered |= set(c.covers)
    assert not [n for n in names if n not in covered]
    assert not [n for n in covered if n not in names]
    called = {a or b for a, b in re.findall(r"lib\(\)\.(vae_\w+)\(|L_\.(vae_\w+)\(", inspect.getsource(gpu_cases))}
    for c in gpu_cases.STREAM_CASES:
        assert not [n for n in c.covers if n not in called], c.name
    all_names = [c.name for c in gpu_cases.STREAM_CASES + gpu_cases.PY_STREAM_CASES]
    assert len(set(all_names)) == len(all_names)
    for c in gpu_cases.PY_STREAM_CASES:
        assert c.reads_back is None or (not c.sync_free and len(c.reads_back.split()) >= 5), c.name
    assert any(c.sync_free for c in gpu_cases.PY_STREAM_CASES)


# ---- Python argument checks (all raised before anything touches a device) ------------------------------------------------------------
def test_attr_reg_validation():
    from torch_vae_amd.attributes import checked_attr_reg
    assert checked_attr_reg(None, 16) is None
    assert checked_attr_reg({"note_density": 0, "mean_pitch": 3}, 16, 2, 5.0, 0.25, batch=4096) == ([0, 3], [0, 3], 2.0, 5.0, 0.25)
    bad = [({"loudness": 0}, {}, "unknown attribute"), ({"note_density": 16}, {}, "latent dimension in 0..15"),
           ({"note_density": -1}, {}, "latent dimension"), ({"note_density": 1.0}, {}, "latent dimension"),
           ({"note_density": True}, {}, "latent dimension"), ({"note_density": 2, "polyphony": 2}, {}, "twice"),
           ({}, {}, "must be None or a dict"), ([("note_density", 0)], {}, "must be None or a dict"),
           ({"note_density": 0}, dict(weight=float("nan")), "attr_weight"), ({"note_density": 0}, dict(weight="1"), "attr_weight"),
           ({"note_density": 0}, dict(delta=float("inf")), "attr_delta"), ({"note_density": 0}, dict(delta=0.0), "attr_delta"),
           ({"note_density": 0}, dict(threshold=float("nan")), "attr_threshold"), ({"note_density": 0}, dict(batch=4097), "at most 4096")]
    for reg_, kw, word in bad:
        with pytest.raises(ValueError, match=word):
            checked_attr_reg(reg_, 16, **kw)
    # more than 8 pairs needs more than 7 names: refused on the name before the count can matter, and the count is checked first
    with pytest.raises(ValueError, match="more than the 8"):
        checked_attr_reg({f"a{k}": k for k in range(9)}, 16)


def test_model_validates_attr_reg_when_it_is_read():
    from torch_vae_amd.models import VanillaVAE
    with pytest.raises(ValueError, match="unknown attribute"):
        VanillaVAE(1, 16, 32, attr_reg={"tempo": 0})
    with pytest.raises(ValueError, match="latent dimension"):
        VanillaVAE(1, 4, 32, attr_reg={"note_density": 4})
    m = VanillaVAE(1, 16, 32, attr_reg={"note_density": 0, "pitch_range": 1}, attr_weight=2.0, attr_delta=5.0, attr_threshold=0.25)
    assert m._attr_setting(8) == ([0, 2], [0, 1], 2.0, 5.0, 0.25)
    assert VanillaVAE(1, 16, 32)._attr_setting(8) is None
    m.attr_reg = {"note_density": 0, "polyphony": 0}
    with pytest.raises(ValueError, match="twice"):
        m._attr_setting(8)
    m.attr_reg = {"note_density": 0}
    m.attr_delta = float("nan")
    with pytest.raises(ValueError, match="attr_delta"):
        m._attr_setting(8)
    m.attr_delta = 10.0
    with pytest.raises(ValueError, match="at most 4096"):
        m._attr_setting(4097)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.attribute_loss()


def test_python_argument_checks():
    from torch_vae_amd.evaluation import attribute_correlation, attribute_values, roll_attributes
    from torch_vae_amd.attributes import attribute_regularizer
    x = torch.zeros(2, 4, 32)
    with pytest.raises(ValueError, match="must be on the GPU"):
        roll_attributes(x)
    for shape, dtype, err, word in (((2, 4), torch.float32, ValueError, r"\[n, h, w\]"), ((2, 2, 4, 8), torch.float32, ValueError, r"\[n, 1, h, w\]"),
                                    ((2, 4, 8), torch.uint8, TypeError, "float32"), ((1, 1025, 1), torch.float32, ValueError, "pitch rows"),
                                    ((1, 1024, 1025), torch.float32, ValueError, "2\\^20 cells"), ((1, 4, 0), torch.float32, ValueError, "time step")):
        with pytest.raises(err, match=word):
            roll_attributes(torch.zeros(*shape, dtype=dtype))
    with pytest.raises(TypeError, match="tensor"):
        roll_attributes(x.numpy())
    with pytest.raises(ValueError, match="threshold"):
        roll_attributes(x, threshold=float("nan"))
    c = torch.zeros(3, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="unknown attribute"):
        attribute_values(c, ["loudness"])
    with pytest.raises(ValueError, match=r"\[n, 8\]"):
        attribute_values(c[:, :7], ["polyphony"])
    z = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="same GPU"):
        attribute_correlation(z, c, ["polyphony"])
    with pytest.raises(ValueError, match="1..7 attribute names"):
        attribute_correlation(z, c, [])
    with pytest.raises(ValueError, match="int32"):
        attribute_correlation(z, c.long(), ["polyphony"])
    with pytest.raises(ValueError, match="float32 tensor"):
        attribute_correlation(z.double(), c, ["polyphony"])
    with pytest.raises(ValueError, match="same GPU"):
        attribute_regularizer(z, c, [0], [0], 10.0, 1.0)


def test_traverse_argument_checks():
    from torch_vae_amd.generation import traverse
    from torch_vae_amd.models import VanillaVAE
    m = VanillaVAE(1, 16, 32)
    with pytest.raises(RuntimeError, match="HIP device"):
        traverse(m, torch.zeros(2, 16), 0, [0.0, 1.0])


def test_fused_step_signature_and_config_fields():
    """train.fused_step keeps the one-call path off when attr_reg is set (decided on the host, before any device work)."""
    from torch_vae_amd import train
    src = inspect.getsource(train.fused_step)
    assert "attr_reg" in src and "one_call = False" in src
    src = inspect.getsource(train.train_one_epoch)
    for field in ("attr_reg", "attr_weight", "attr_delta"):
        assert f'config, "{field}"' in src, field
