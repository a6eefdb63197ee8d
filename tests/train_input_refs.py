"""Restatements for the front of the training iteration (csrc/train_inputs.hip; include/vp_hip.h, ABI 31), written
from the formulas of the header: Philox4x32-10 in numpy integer arithmetic, Box-Muller in float64 on the exact 24-bit
uniforms, torch's nearest index map, and train/train_cogvideox_inpainting_i2v_video.py:1774-1853 as plain torch CPU
ops on bf16 tensors (the script's own expressions, so every rounding is torch's).

`front_of_step` takes switches that each break one thing (a fused sample rounding, no scaling factor, sa / sb
swapped, image frames >= 1 kept, an integer-division mask map): tests/test_train_inputs_cpu.py checks that the
comparison used on the GPU tells every one of them from the true restatement.
"""
import numpy as np
import torch

BF16 = torch.bfloat16
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: (k0, k1) -> uint32 [..., 4].  Every product in uint64."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_words(seed: int, stream: int, offset: int, n: int):
    """The uint32 word pairs (xa, xb) and the lane parity of elements offset .. offset + n - 1."""
    e = np.arange(n, dtype=np.uint64) + np.uint64(offset)
    blk = e >> np.uint64(2)
    lane = (e & np.uint64(3)).astype(np.int64)
    ub, inv = np.unique(blk, return_inverse=True)
    ctr = np.stack([ub & MASK32, ub >> np.uint64(32), np.full_like(ub, stream & 0xFFFFFFFF),
                    np.full_like(ub, (stream >> 32) & 0xFFFFFFFF)], axis=-1).astype(np.uint32)
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[inv]
    pair = lane >> 1
    xa = np.where(pair == 0, x[:, 0], x[:, 2])
    xb = np.where(pair == 0, x[:, 1], x[:, 3])
    return xa, xb, lane & 1


def philox_normal_f64(seed: int, stream: int, offset: int, n: int) -> np.ndarray:
    """Normal numbers offset .. offset + n - 1 of (seed, stream): Box-Muller in float64 on the exact uniforms."""
    xa, xb, odd = philox_words(seed, stream, offset, n)
    u1 = ((xa >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (xb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.where(odd == 0, r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2))


def philox_normal_f32(seed: int, stream: int, offset: int, n: int) -> np.ndarray:
    """The same in float32 arithmetic (numpy's): what a float32 implementation may differ by."""
    xa, xb, odd = philox_words(seed, stream, offset, n)
    u1 = ((xa >> np.uint32(8)).astype(np.float32) + np.float32(1)) * np.float32(2.0 ** -24)
    u2 = (xb >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    r = np.sqrt(np.float32(-2.0) * np.log(u1))
    a = np.float32(2.0 * np.pi) * u2
    return np.where(odd == 0, r * np.cos(a), r * np.sin(a)).astype(np.float32)


def normal_bound(ref: np.ndarray) -> np.ndarray:
    """|out - ref| allowed per element, for the fp32 and for the bf16 output: 2^-7 |ref| + 4e-6."""
    return 2.0 ** -7 * np.abs(ref) + 4e-6


def to_bf16(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).to(BF16)


def nearest_map(n_in: int, n_out: int, integer_division: bool = False):
    """F.interpolate(mode="nearest") source index of each output index: min(floor(dst * (in / out)), in - 1) in
    float32.  integer_division: the stride taken as in // out (dst * (in // out): 0 3 6 ... for 49 -> 13, where
    torch gives 0 3 7 11 ...)."""
    if integer_division:
        return [min(i * (n_in // n_out), n_in - 1) for i in range(n_out)]
    scale = np.float32(n_in) / np.float32(n_out)
    return [min(int(np.floor(np.float32(i) * scale)), n_in - 1) for i in range(n_out)]


def resize_mask(masks: torch.Tensor, size, integer_division: bool = False) -> torch.Tensor:
    """:1802-1810: [B, Fp, 1, Hp, Wp] -> bf16 [B, T, 1, h, w] by the nearest map per axis (any mask dtype)."""
    T, h, w = size
    ft = torch.tensor(nearest_map(masks.shape[1], T, integer_division))
    fy = torch.tensor(nearest_map(masks.shape[3], h, integer_division))
    fx = torch.tensor(nearest_map(masks.shape[4], w, integer_division))
    return masks[:, ft][:, :, :, fy][:, :, :, :, fx].to(BF16)


def nudge_bf16(x: torch.Tensor, ulps: int) -> torch.Tensor:
    """A positive bf16 tensor moved by `ulps` representable values."""
    return (x.view(torch.int16) + ulps).view(BF16)


def posterior_std(params: torch.Tensor, L: int) -> torch.Tensor:
    """std = exp(0.5 clamp(logvar)) of the reference's DiagonalGaussianDistribution, bf16 [B, L, T, h, w]."""
    logvar = torch.clamp(params[..., L:2 * L].permute(0, 4, 1, 2, 3), -30.0, 20.0)
    return torch.exp(0.5 * logvar)


def sample_scaled(params: torch.Tensor, noise: torch.Tensor, L: int, scaling_factor: float, *, fused=False,
                  no_scaling=False, std_ulps: int = 0, std=None) -> torch.Tensor:
    """latent_dist.sample() with the given noise, permuted and scaled (:1780-1782): params [B, T, h, w, ld] bf16
    channels-last, noise [B, L, T, h, w] bf16 -> [B, T, L, h, w] bf16.  std: a bf16 [B, L, T, h, w] tensor to use in
    place of exp(0.5 logvar) (another exp's rounding); std_ulps moves the computed std by that many bf16 values."""
    mean = params[..., :L].permute(0, 4, 1, 2, 3)
    std = posterior_std(params, L) if std is None else std
    if std_ulps:
        std = nudge_bf16(std.contiguous(), std_ulps)
    if fused:  # one rounding for mean + std * n
        x = (mean.float() + std.float() * noise.float()).to(BF16)
    else:
        x = mean + std * noise
    z = x.permute(0, 2, 1, 3, 4)
    if not no_scaling:
        z = z * scaling_factor
    return z.to(memory_format=torch.contiguous_format, dtype=BF16)


def add_noise(alphas_cumprod: torch.Tensor, x: torch.Tensor, eps: torch.Tensor, timesteps: torch.Tensor, *,
              swap=False) -> torch.Tensor:
    """scheduler.add_noise (DF/schedulers/scheduling_dpm_cogvideox.py:442-466) on bf16 samples; the timesteps are
    clamped to the table first (the kernel's rule)."""
    ac = alphas_cumprod.to(dtype=x.dtype)
    t = timesteps.clamp(0, ac.numel() - 1)
    sa = (ac[t] ** 0.5).flatten()
    sb = ((1 - ac[t]) ** 0.5).flatten()
    if swap:
        sa, sb = sb, sa
    while sa.dim() < x.dim():
        sa = sa.unsqueeze(-1)
        sb = sb.unsqueeze(-1)
    return sa * x + sb * eps


def front_of_step(p_video, p_cond, p_image, noises, timesteps, alphas_cumprod, scaling_factor, masks, *,
                  image_dropout=False, L=16, fused_sample=False, no_scaling=False, swap_sa_sb=False,
                  keep_image_frames=False, integer_division=False, std_ulps=(0, 0, 0), stds=(None, None, None)):
    """:1780-1853 on host tensors.  noises = (video, conditioning, image posterior noises, diffusion noise);
    stds / std_ulps: the replacement / bf16 nudge of the (video, conditioning, image) std.  Returns a dict named as
    the kernel's outputs."""
    n_video, n_cond, n_image, eps = noises
    kw = dict(fused=fused_sample, no_scaling=no_scaling)
    image_latents = sample_scaled(p_image, n_image, L, scaling_factor, std_ulps=std_ulps[2], std=stds[2], **kw)
    model_input = sample_scaled(p_video, n_video, L, scaling_factor, std_ulps=std_ulps[0], std=stds[0], **kw)
    cond = sample_scaled(p_cond, n_cond, L, scaling_factor, std_ulps=std_ulps[1], std=stds[1], **kw)
    B, T = cond.shape[:2]
    if keep_image_frames:
        image_latents = image_latents.expand(B, T, *image_latents.shape[2:]).contiguous()
    else:
        padding = image_latents.new_zeros((B, T - 1, *cond.shape[2:]))
        image_latents = torch.cat([image_latents, padding], dim=1)
    if image_dropout:
        image_latents = torch.zeros_like(image_latents)
    m = resize_mask(masks, (T, cond.shape[3], cond.shape[4]), integer_division)
    cond = torch.concat([cond, m], -3).to(BF16)
    noisy = add_noise(alphas_cumprod, model_input, eps, timesteps, swap=swap_sa_sb)
    return dict(target=model_input, noisy=noisy, noisy_model_input=torch.cat([noisy, image_latents], dim=2),
                masks_latent=m, conditioning_latents=cond)


def noise_frame(x: torch.Tensor, noise: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    """:1779-1780: (images + randn * sigma[:, None]).to(bf16) in torch's promoted arithmetic; x, noise [B, n]."""
    return (x + noise * sigma[:, None]).to(BF16)


def synthetic_case(B, T, h, w, ld, mask_shape, mask_dtype, seed=0, L=16):
    """Posterior parameters with logvar beyond both clamps, the four noises, and a box mask of the given dtype."""
    g = torch.Generator().manual_seed(seed)
    def params(t):
        p = torch.randn(B, t, h, w, ld, generator=g)
        p[..., L:2 * L] = p[..., L:2 * L] * 6.0 - 4.0          # mostly [-22, 14]
        p[..., L:2 * L][..., 0, :2] = torch.tensor([-41.0, 27.0])  # below -30 and above 20
        return p.to(BF16)
    p_video, p_cond, p_image = params(T), params(T), params(1)
    noises = (torch.randn(B, L, T, h, w, generator=g).to(BF16), torch.randn(B, L, T, h, w, generator=g).to(BF16),
              torch.randn(B, L, 1, h, w, generator=g).to(BF16), torch.randn(B, T, L, h, w, generator=g).to(BF16))
    Fp, Hp, Wp = mask_shape
    m = torch.zeros(B, Fp, 1, Hp, Wp)
    m[:, Fp // 3:, :, Hp // 4: Hp // 4 + Hp // 2, Wp // 5: Wp // 5 + Wp // 2] = 1.0
    if mask_dtype != torch.uint8:
        m = m * 0.6171875 + 0.001953125 * torch.rand(m.shape, generator=g)  # not only {0, 1}; fp32 needs a rounding
    return p_video, p_cond, p_image, noises, m.to(mask_dtype)


def alphas_cumprod_table():
    """The scheduler's table (videopainter_amd.scheduler: host code only)."""
    from videopainter_amd.scheduler import CogVideoXDPMScheduler
    return CogVideoXDPMScheduler().alphas_cumprod
