"""The loss of the reference's training step as one HIP pass (csrc/optim.hip, vp_v_loss_bf16).

train/train_cogvideox_inpainting_i2v_video.py:1879-1891:

    model_pred = scheduler.get_velocity(model_output, noisy_video_latents, timesteps)
    weights = 1 / (1 - alphas_cumprod[timesteps])
    loss = mean_b mean(weights (model_pred - target)^2)
         + inpainting_loss_weight * mean_b mean(weights (model_pred masks - target masks)^2)

`inpainting_v_loss` computes it in fp32 from the bf16 tensors (the script evaluates it in bf16) together with
d loss / d model_output, reading `timesteps` on the device; its backward hands that bf16 gradient, times the incoming
scalar, to the transformer head's backward (videopainter_amd/autograd.py), so `loss.backward()` reaches the branch
parameters.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import kernels as K


class _VLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model_output, noisy_latents, target, timesteps, alphas_cumprod, masks, lam):
        loss, dout = K.v_loss(model_output, noisy_latents, target, timesteps, alphas_cumprod, masks, lam)
        ctx.save_for_backward(dout)
        return loss

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        (dout,) = ctx.saved_tensors
        return (K.scale(dout, g.reshape(1).to(torch.float32).contiguous()),) + (None,) * 6


def inpainting_v_loss(model_output: torch.Tensor, noisy_latents: torch.Tensor, target: torch.Tensor,
                      timesteps: torch.Tensor, alphas_cumprod: torch.Tensor, masks: Optional[torch.Tensor] = None,
                      inpainting_loss_weight: float = 1.0) -> torch.Tensor:
    """The training loss (fp32 0-dim device tensor), differentiable w.r.t. `model_output` only.

    model_output, noisy_latents, target: bf16 [B, F, C, H, W]; masks: [B, F, 1, H, W] bf16 / fp32 or None (then there
    is no inpainting term, whatever the weight); timesteps: integer [B] on the device (never read on the host;
    values are clamped to the table); alphas_cumprod: the scheduler's fp32 table (moved to the device if it is not
    there — keep a device copy, as the script does at :1731, to avoid the copy every step)."""
    dev = model_output.device
    if timesteps.dtype != torch.int64 or timesteps.device != dev:
        timesteps = timesteps.to(device=dev, dtype=torch.int64)
    if alphas_cumprod.dtype != torch.float32 or alphas_cumprod.device != dev:
        alphas_cumprod = alphas_cumprod.to(device=dev, dtype=torch.float32)
    if masks is not None and masks.device != dev:
        masks = masks.to(dev)
    c = lambda t: t if t is None or t.is_contiguous() else t.contiguous()  # noqa: E731
    return _VLossFn.apply(c(model_output), c(noisy_latents.detach()), c(target.detach()), c(timesteps),
                          c(alphas_cumprod), c(masks), float(inpainting_loss_weight))
