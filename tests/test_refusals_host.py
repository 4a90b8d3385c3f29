"""Refusals of the C ABI that need no GPU: every call below hands the library fake, never dereferenced addresses and must fail on
the host, before anything is enqueued, with exactly the message listed (the whole text of vae_last_error(), entry-point name
included).  The table pins the argument checks that several entry points share: group / range / scratch checks of the optimiser,
the null-context preambles, the argument checks of the context-free utilities."""
import ctypes as C

import pytest

from torch_vae_amd import _lib

P = 4096          # a fake device address, 16-byte aligned
OFFS, SIZES = (C.c_int64 * 2)(0, 1024), (C.c_int64 * 2)(1000, 1000)
LRS, B1S = (C.c_double * 2)(1e-3, 1e-3), (C.c_double * 2)(0.9, 0.9)
TH = (C.c_float * 9)(*[0.1 * (k + 1) for k in range(9)])
BUF = C.create_string_buffer(64)


def grad_norm(L, grads=P, n=2, offs=OFFS, sizes=SIZES, norm=256, scratch=P):
    return L.vae_grad_norm(grads, n, offs, sizes, 1.0, norm, scratch, None)


def adamw(L, n=2, step=1):
    return L.vae_adamw_step(P, P, P, P, n, OFFS, SIZES, LRS, B1S, 0.999, 1e-8, 0.0, 1.0, step, None)


def expand(L, src=P, kind=0, cells=64):
    return L.vae_expand_stimuli(src, kind, P, cells, None)


def recon_metrics(L, nth):
    return L.vae_recon_metrics(P, P, 4, 64, TH, nth, 0.5, P, P, P, P, 0, None)


def train_step_fused(L):
    return L.vae_train_step_fused(None, P, 4, P, P, P, P, P, P, None, 0, 1.0, 2, OFFS, SIZES, LRS, B1S, 0.999, 1e-8, 0.0, 1.0, 1, 0,
                                  P, P, P, P, P, None)


CASES = {
    # vae_grad_norm: the gradient buffer first, then the group / range checks, then its own pointer message, then the alignment
    "grad_norm/3_groups": (lambda L: grad_norm(L, n=3), "vae_grad_norm: 1 or 2 groups"),
    "grad_norm/null_offsets": (lambda L: grad_norm(L, offs=None), "vae_grad_norm: null offsets / sizes"),
    "grad_norm/negative_offset": (lambda L: grad_norm(L, offs=(C.c_int64 * 2)(0, -8)), "vae_grad_norm: empty or negative range"),
    "grad_norm/size_0": (lambda L: grad_norm(L, sizes=(C.c_int64 * 2)(1000, 0)), "vae_grad_norm: empty or negative range"),
    "grad_norm/null_norm_out": (lambda L: grad_norm(L, norm=0), "vae_grad_norm: null device pointer (norm_out, scratch)"),
    "grad_norm/null_scratch": (lambda L: grad_norm(L, scratch=0), "vae_grad_norm: null device pointer (norm_out, scratch)"),
    "grad_norm/scratch_plus_4": (lambda L: grad_norm(L, scratch=P + 4), "vae_grad_norm: scratch must be 16-byte aligned"),
    "grad_norm/null_grads": (lambda L: grad_norm(L, grads=0, n=3), "vae_grad_norm: null gradient buffer"),
    "adamw_step/0_groups": (lambda L: adamw(L, n=0), "vae_adamw_step: 1 or 2 groups"),
    "adamw_step/3_groups": (lambda L: adamw(L, n=3), "vae_adamw_step: 1 or 2 groups"),
    "adamw_step/step_0": (lambda L: adamw(L, step=0), "vae_adamw_step: step is 1-based"),
    "expand_stimuli/null_source": (lambda L: expand(L, src=0), "vae_expand_stimuli: null pointer"),
    "expand_stimuli/kind_2": (lambda L: expand(L, kind=2), "vae_expand_stimuli: kind must be 0 (bytes) or 1 (bit planes)"),
    "expand_stimuli/60_cells": (lambda L: expand(L, cells=60), "vae_expand_stimuli: the number of cells must be a multiple of 8"),
    "recon_metrics/0_thresholds": (lambda L: recon_metrics(L, 0), "vae_recon_metrics: n_thresholds must be in 1..8"),
    "recon_metrics/9_thresholds": (lambda L: recon_metrics(L, 9), "vae_recon_metrics: n_thresholds must be in 1..8"),
    # null context
    "null_ctx/vae_forward": (lambda L: L.vae_forward(None, P, 4, P, P, P, None, 0, 1, P, P, P, P, None), "vae_forward: null ctx"),
    "null_ctx/vae_encode": (lambda L: L.vae_encode(None, P, 4, P, P, P, None, 0, 1, P, P, P, None), "vae_encode: null ctx"),
    "null_ctx/vae_decode": (lambda L: L.vae_decode(None, P, 4, P, P, P, 1, P, None), "vae_decode: null ctx"),
    "null_ctx/vae_log_likelihood": (lambda L: L.vae_log_likelihood(None, P, 4, P, P, 8, 2, None, 0, None, P, P, None),
                                    "vae_log_likelihood: null ctx"),
    "null_ctx/vae_profile_report": (lambda L: L.vae_profile_report(None, BUF, 64), "vae_profile_report: null ctx"),
    "null_ctx/vae_profile_sequence": (lambda L: L.vae_profile_sequence(None, BUF, 64), "vae_profile_sequence: null ctx"),
    "null_ctx/vae_profile_timeline": (lambda L: L.vae_profile_timeline(None, BUF, 64), "vae_profile_timeline: null ctx"),
    "null_ctx/vae_train_step_fused": (train_step_fused, "vae_train_step_fused: null ctx"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal_message(case):
    L = _lib.lib()
    call, want = CASES[case]
    assert call(L) == -1
    assert L.vae_last_error().decode() == want
