"""Dict shapes returned by the model (mirror of the reference's types_helpers.py:15-37)."""
from typing import TypedDict

from torch import Tensor


class EncoderOutput(TypedDict):
    mu: Tensor
    log_var: Tensor
    pre_latents: Tensor


class ModelOutput(TypedDict):
    output: Tensor
    input: Tensor
    encoded: EncoderOutput
    latents: Tensor


class LossOutput(TypedDict):
    loss: Tensor
    reconstruction_loss: Tensor
    kld_loss: Tensor


class LikelihoodOutput(TypedDict):
    log_likelihood: Tensor    # [B] float64: importance-weighted estimate of log p(x) (nats)
    elbo: Tensor              # [B] float64: per-sample evidence lower bound (nats)
    log_weights: Tensor       # [K, B] float64: log p(x|z_k) + log p(z_k) - log q(z_k|x)
