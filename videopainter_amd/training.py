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

The front of the iteration (:1774-1853, between the batch's pixels and the models) is `prepare_training_inputs` with
its noise source `TrainingNoise`, further down (csrc/train_inputs.hip).
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


# ----------------------------------------------------------------------------------------------------------------------
# The front of the iteration: train/train_cogvideox_inpainting_i2v_video.py:1774-1853 (csrc/train_inputs.hip)
# ----------------------------------------------------------------------------------------------------------------------

# tensor ids of the Philox streams of one step (fixed: a checkpoint's (seed, step) names the same noise for ever)
NOISE_IMAGE_PIXELS = 0      # :1779 randn_like(images)
NOISE_POSTERIOR_IMAGE = 1   # :1780 latent_dist.sample()
NOISE_POSTERIOR_VIDEO = 2   # :1784
NOISE_POSTERIOR_COND = 3    # :1789
NOISE_DIFFUSION = 4         # :1826 randn_like(model_input)
_NOISE_KEYS = {"image_pixels": NOISE_IMAGE_PIXELS, "image": NOISE_POSTERIOR_IMAGE, "video": NOISE_POSTERIOR_VIDEO,
               "conditioning": NOISE_POSTERIOR_COND, "diffusion": NOISE_DIFFUSION}
_MAX_RANK, _MAX_STEP = 1 << 16, 1 << 44


class TrainingNoise:
    """The reproducible noise of the training iteration.  Host state: (seed, step).  The device noise of tensor
    `tensor_id` in this step on this rank is the Philox stream `step * 2^20 + rank * 2^4 + tensor_id` of `seed`
    (vp_philox_normal), indexed by the element's position: independent of the launch and of the number of ranks, and
    continued after a resume by restoring `step`.  The two per-sample host draws (:1775-1778, :1830-1833) come from a
    torch.Generator seeded from (seed, step, rank) and go up in one asynchronous copy.  Nothing reads the device."""

    def __init__(self, seed: int, rank: int = 0):
        if not 0 <= int(rank) < _MAX_RANK:
            raise ValueError(f"rank must be in [0, {_MAX_RANK})")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.rank = int(rank)
        self.step = 0

    def stream(self, tensor_id: int) -> int:
        if not 0 <= int(tensor_id) < 16:
            raise ValueError("tensor_id must be in [0, 16)")
        return (self.step << 20) + (self.rank << 4) + int(tensor_id)

    def next_step(self) -> int:
        if self.step + 1 >= _MAX_STEP:
            raise OverflowError("TrainingNoise: step counter exhausted")
        self.step += 1
        return self.step

    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state: dict) -> None:
        self.seed = int(state["seed"]) & 0xFFFFFFFFFFFFFFFF
        self.step = int(state["step"])

    def _generator(self) -> torch.Generator:
        x = self.seed  # splitmix64 over (seed, step, rank): nearby triples give unrelated generator seeds
        for v in (self.step, self.rank):
            x = (x + 0x9E3779B97F4A7C15 + v) & 0xFFFFFFFFFFFFFFFF
            x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
            x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
            x ^= x >> 31
        return torch.Generator().manual_seed(x)

    def host_draws(self, batch: int, num_train_timesteps: int):
        """(timesteps int64 [B], image_noise_sigma bf16 [B] = exp(N(-3, 0.5)), u in [0, 1) for the image dropout), all
        on the host, a function of (seed, step, rank) alone."""
        g = self._generator()
        ts = torch.randint(0, int(num_train_timesteps), (batch,), generator=g, dtype=torch.int64)
        sigma = torch.exp(torch.normal(-3.0, 0.5, (batch,), generator=g).to(torch.bfloat16))
        u = float(torch.rand((), generator=g))
        return ts, sigma, u

    @staticmethod
    def upload(timesteps: torch.Tensor, sigma: torch.Tensor, device):
        """Host int64 [B] and bf16 [B] -> their device copies, by one asynchronous copy from pinned memory."""
        B = timesteps.numel()
        stage = torch.empty(10 * B, dtype=torch.uint8).pin_memory()
        stage[:8 * B].view(torch.int64).copy_(timesteps.to(torch.int64))
        stage[8 * B:].view(torch.bfloat16).copy_(sigma.to(torch.bfloat16))
        dev = stage.to(device, non_blocking=True)
        return dev[:8 * B].view(torch.int64), dev[8 * B:].view(torch.bfloat16)


class TrainingInputs:
    """What :1774-1853 leave for the models, named as the script names them."""
    __slots__ = ("model_input", "noisy_video_latents", "noisy_model_input", "conditioning_latents", "masks",
                 "timesteps", "image_noise_sigma", "image_dropout")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _check_inputs(pixel_values, conditioning_pixel_values, masks):
    for t, n in ((pixel_values, "pixel_values"), (conditioning_pixel_values, "conditioning_pixel_values"),
                 (masks, "masks")):
        if not isinstance(t, torch.Tensor) or t.dim() != 5:
            raise ValueError(f"{n} must be a 5-D tensor [B, F, C, H, W]")
    if conditioning_pixel_values.shape != pixel_values.shape:
        raise ValueError(f"conditioning_pixel_values {tuple(conditioning_pixel_values.shape)} must have the shape of "
                         f"pixel_values {tuple(pixel_values.shape)}")
    if masks.shape[0] != pixel_values.shape[0] or masks.shape[2] != 1:
        raise ValueError(f"masks must be [B, F, 1, H, W] with the batch of pixel_values, got {tuple(masks.shape)}")
    if masks.shape[1] != pixel_values.shape[1]:
        raise ValueError(f"masks has {masks.shape[1]} frames, pixel_values {pixel_values.shape[1]}")
    for t, n in ((pixel_values, "pixel_values"), (conditioning_pixel_values, "conditioning_pixel_values"),
                 (masks, "masks")):
        if not t.is_cuda:
            raise ValueError(f"{n} is a host tensor: the training inputs are assembled on the device")
    if masks.device != pixel_values.device or conditioning_pixel_values.device != pixel_values.device:
        raise ValueError("pixel_values, conditioning_pixel_values and masks must be on one device")


def prepare_training_inputs(vae, scheduler, pixel_values: torch.Tensor, conditioning_pixel_values: torch.Tensor,
                            masks: torch.Tensor, *, noise: TrainingNoise, noised_image_dropout: float = 0.0,
                            timesteps: Optional[torch.Tensor] = None, noises: Optional[dict] = None,
                            image_noise_sigma: Optional[torch.Tensor] = None,
                            image_dropout: Optional[bool] = None) -> TrainingInputs:
    """:1774-1853: from the batch's pixels to the models' inputs, on the device, without a host read.

    pixel_values / conditioning_pixel_values: [B, F, C, H, W] fp32 or bf16 in [-1, 1]; masks: [B, F, 1, H, W] fp32,
    bf16 or uint8 (1 = inpaint).  Runs vp_noise_frame on the first frame, the three `vae.encode` calls as the VAE is
    configured (tiling, slicing), and one vp_train_inputs_bf16 launch that reads the encoder's channels-last
    posterior parameters.  All noise comes from `noise` (this step's streams); `timesteps` (int64 [B]),
    `image_noise_sigma` (bf16 [B]), `image_dropout` and `noises` — a dict with any of the keys "image_pixels"
    ([B, C, H, W] in pixel_values' dtype), "image" ([B, L, 1, h, w]), "video", "conditioning" ([B, L, T, h, w]) and
    "diffusion" ([B, T, L, h, w]), bf16 — replace the draws so that a given draw can be reproduced."""
    if not isinstance(noise, TrainingNoise):
        raise ValueError("noise must be a TrainingNoise")
    noises = dict(noises or {})
    unknown = set(noises) - set(_NOISE_KEYS)
    if unknown:
        raise ValueError(f"noises: unknown keys {sorted(unknown)} (known: {sorted(_NOISE_KEYS)})")
    _check_inputs(pixel_values, conditioning_pixel_values, masks)
    dev = pixel_values.device
    B = pixel_values.shape[0]
    n_train = int(scheduler.config.num_train_timesteps)
    ts_h, sigma_h, u = noise.host_draws(B, n_train)
    if image_dropout is None:
        image_dropout = u < float(noised_image_dropout)
    for t, n, dt in ((timesteps, "timesteps", torch.int64), (image_noise_sigma, "image_noise_sigma", torch.bfloat16)):
        if t is not None and (t.shape != (B,) or t.dtype != dt):
            raise ValueError(f"{n} must be a {dt} [B] tensor")
    # a given host tensor takes the draw's place in the one upload; a given device tensor is used as it is
    ts_dev = timesteps if timesteps is not None and timesteps.is_cuda else None
    sigma_dev = image_noise_sigma if image_noise_sigma is not None and image_noise_sigma.is_cuda else None
    if ts_dev is None or sigma_dev is None:
        up_ts, up_sigma = TrainingNoise.upload(ts_h if timesteps is None or ts_dev is not None else timesteps,
                                               sigma_h if image_noise_sigma is None or sigma_dev is not None
                                               else image_noise_sigma, dev)
        ts_dev = up_ts if ts_dev is None else ts_dev
        sigma_dev = up_sigma if sigma_dev is None else sigma_dev
    timesteps, image_noise_sigma = ts_dev, sigma_dev

    with torch.no_grad():
        first = pixel_values[:, 0]  # [B, C, H, W]: the memory order of images [B, C, 1, H, W] (:1774)
        noisy_images = K.noise_frame(first, image_noise_sigma.contiguous(), noises.get("image_pixels"),
                                     seed=noise.seed, stream=noise.stream(NOISE_IMAGE_PIXELS)).unsqueeze(2)
        p_image = vae.encode(noisy_images).latent_dist._p
        p_video = vae.encode(pixel_values.permute(0, 2, 1, 3, 4)).latent_dist._p
        p_cond = vae.encode(conditioning_pixel_values.permute(0, 2, 1, 3, 4)).latent_dist._p
        T = p_video.shape[1]
        t_mask = (masks.shape[1] - 1) // int(vae.config.temporal_compression_ratio) + 1
        if t_mask != T:
            raise ValueError(f"masks' {masks.shape[1]} frames give {t_mask} latent frames, the video's encode {T}")
        ids = (NOISE_POSTERIOR_VIDEO, NOISE_POSTERIOR_COND, NOISE_POSTERIOR_IMAGE, NOISE_DIFFUSION)
        target, noisy, nmi, mlat, cond = K.train_inputs(
            p_video.contiguous(), p_cond.contiguous(), p_image.contiguous(), masks.contiguous(), timesteps.contiguous(),
            scheduler.add_noise_table(torch.bfloat16, dev), float(vae.config.scaling_factor),
            latent_channels=int(vae.config.latent_channels), image_dropout=bool(image_dropout),
            noises=(noises.get("video"), noises.get("conditioning"), noises.get("image"), noises.get("diffusion")),
            seed=noise.seed, streams=tuple(noise.stream(i) for i in ids))
    return TrainingInputs(model_input=target, noisy_video_latents=noisy, noisy_model_input=nmi,
                          conditioning_latents=cond, masks=mlat, timesteps=timesteps,
                          image_noise_sigma=image_noise_sigma, image_dropout=bool(image_dropout))
