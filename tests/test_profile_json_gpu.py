"""The three profile writers of the C ABI (vae_profile_report / vae_profile_sequence / vae_profile_timeline) around one one-call
training step: each writes JSON, the three agree with one another, and each refuses a buffer without room for the terminating
NUL.  Reference-exact model, 32x32, latent 3, batch 2, f32."""
import ctypes
import json

import pytest
import torch

from oracle import vae_oracle as vo
from tests.util import make_model, perturbed_params
from torch_vae_amd import _lib

pytestmark = pytest.mark.gpu

H, L, B = 32, 3, 2


def test_profile_writers_agree_and_check_the_capacity():
    from torch_vae_amd.optim import FusedAdamW
    m = make_model(H, L, False, "f32", perturbed_params(L, H, 41, False))
    opt = FusedAdamW([{"params": m.encoder.parameters()}, {"params": m.decoder.parameters()}], lr=1e-3, weight_decay=0.0)
    x = torch.from_numpy(vo.synth_pianoroll(B, H, 42)).float().cuda()
    lib, h = _lib.lib(), m._context(B).handle
    assert lib.vae_profile(h, 1) == 0
    m.fused_train_step(opt, x)
    torch.cuda.synchronize()
    assert m._ctx.handle == h
    big = ctypes.create_string_buffer(1 << 20)
    text = {}
    for name in ("report", "sequence", "timeline"):
        write = getattr(lib, "vae_profile_" + name)
        assert write(h, big, len(big)) == 0, lib.vae_last_error().decode()
        text[name] = big.value.decode()
        # the text and its NUL must fit: a capacity equal to the text length is refused, one more byte is enough
        n = len(text[name])
        small = ctypes.create_string_buffer(n + 1)
        assert write(h, small, n) == -1
        assert lib.vae_last_error().decode() == f"vae_profile_{name}: buffer too small"
        assert write(h, small, n + 1) == 0, lib.vae_last_error().decode()
        assert small.value.decode() == text[name]
    assert lib.vae_profile(h, 0) == 0
    report, sequence, timeline = (json.loads(text[k]) for k in ("report", "sequence", "timeline"))
    assert report and all(set(r) == {"name", "calls", "ms", "bytes", "flops", "side"} for r in report)
    assert len(timeline) == sum(r["calls"] for r in report)
    assert {r["name"] for r in report} == set(sequence)
