"""Latent sizes the library accepts, host side (no GPU): vae_param_layout takes every latent_dim in 1..4096 and refuses the rest,
and VanillaVAE refuses an unsupported size when it is constructed, not at its first step.  Every accepted size runs on the device:
the kernels whose LDS would grow with the latent size stage it in passes (test_parity_gpu.py's LATENT_SWEEP runs 4096)."""
import ctypes as C

import pytest

from torch_vae_amd import _lib

LATENT_MAX = 4096


def _layout(H, L, gen):
    offs, sizes, total = (C.c_int64 * _lib.NUM_PARAMS)(), (C.c_int64 * _lib.NUM_PARAMS)(), C.c_int64()
    return _lib.lib().vae_param_layout(H, L, gen, offs, sizes, C.byref(total)), sizes


@pytest.mark.parametrize("H,gen", [(32, 0), (128, 1)])
def test_param_layout_accepts_exactly_1_to_4096(H, gen):
    F = 256 * (H // 16 if gen else 2) ** 2
    for L in (1, LATENT_MAX):
        rc, sizes = _layout(H, L, gen)
        assert rc == 0, _lib.lib().vae_last_error().decode()
        assert sizes[16] == sizes[18] == sizes[20] == L * F        # fc_mu, fc_var, decoder_input weights
    for L in (0, -1, LATENT_MAX + 1):
        rc, _ = _layout(H, L, gen)
        assert rc == -1, L
        assert "latent_dim must be in 1..4096" in _lib.lib().vae_last_error().decode()


def test_model_refuses_an_unsupported_latent_size_at_construction():
    from torch_vae_amd.models import VanillaVAE
    m = VanillaVAE(1, LATENT_MAX, 32, compute_dtype="f32")
    assert tuple(m.fc_mu.weight.shape) == (LATENT_MAX, 1024) and tuple(m.decoder_input.weight.shape) == (1024, LATENT_MAX)
    with pytest.raises(ValueError, match="latent_dim must be in 1..4096"):
        VanillaVAE(1, LATENT_MAX + 1, 32, compute_dtype="f32")
