"""The front of the training iteration on the GPU (csrc/train_inputs.hip; include/vp_hip.h ABI 31): the Philox normal
generator, vp_noise_frame, vp_train_inputs_bf16 on synthetic posterior parameters, and prepare_training_inputs end to
end on the tiny VAE.  References: tests/train_input_refs.py (numpy Philox + float64 Box-Muller; the script's torch CPU
ops).  Every kernel output sits in a NaN-filled buffer with guard elements before and after, compared too.

The device's exp may round to the neighbouring bf16 of torch's CPU exp on a few elements.  The kernel itself tells
where: run on the same logvar with zero mean, unit noise and scaling factor 1 its `target` IS its std.  The
restatement is evaluated with that std; the elements where it differs from torch's are counted (cap 1e-3 of the
total) and must be one bf16 value apart.
"""
import numpy as np
import pytest
import torch

from tests import train_input_refs as R

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
SEEDS_STREAMS = (((0x9E3779B9 << 32) | 12345, (7 << 32) | 3), (42, (0xFFFFFFFF << 32) | 0xFFFFFFF0))


@pytest.fixture(scope="module")
def K():
    from videopainter_amd import kernels
    return kernels


def guarded(shape, dtype, guard=8):
    """(buffer, view): a NaN-filled 1-D buffer and the contiguous view of `shape` inside it, `guard` elements in."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), NAN, device=dev, dtype=dtype)
    return buf, buf[guard:guard + n].view(shape)


def guards_intact(buf, n, guard=8):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


# ------------------------------------------------------------------------------------------------------------------
# Philox fill
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["vector", "scalar"])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_philox_fill_matches_float64_box_muller(K, dtype, layout):
    """Head and tail lanes, the carry into counter word 1, high seed / stream words.  layout: where the first whole
    block of four lands on a vector-store boundary, or one element off it (all scalar stores)."""
    runs = []
    for seed, stream in SEEDS_STREAMS:
        for offset in (0, 1, 2, 3, 2 ** 32 - 2, 2 ** 34 + 1):
            for n in (1, 3, 4, 5, 255, 1027):
                guard = 8 + (offset & 3) + (layout == "scalar")
                buf, view = guarded((n,), dtype, guard)
                K.philox_normal_(view, seed, stream, offset)
                runs.append((seed, stream, offset, n, guard, buf))
    total = diff = 0
    for seed, stream, offset, n, guard, buf in runs:
        got = buf.cpu()
        assert guards_intact(got, n, guard), (offset, n)
        ref = R.philox_normal_f64(seed, stream, offset, n)
        out = got[guard:guard + n]
        err = np.abs(out.double().numpy() - ref)
        assert np.all(err <= R.normal_bound(ref)), (seed, stream, offset, n, float(err.max()))
        if dtype == BF16:
            total += n
            diff += int((bits(out) != bits(R.to_bf16(ref))).sum())
    if dtype == BF16:
        print(f"bf16 elements not bit-identical to the rounded float64 reference: {diff} of {total}")
        assert diff <= 1e-3 * total


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_philox_fill_is_a_function_of_the_element_index(K, dtype):
    seed, stream = SEEDS_STREAMS[0]
    whole = K.philox_normal_(torch.empty(5 + 1000, device=dev, dtype=dtype), seed, stream, 0)
    for offset, n in ((5, 1000), (1, 3), (2, 2), (3, 1002)):
        buf, view = guarded((n,), dtype)
        K.philox_normal_(view, seed, stream, offset)
        assert guards_intact(buf, n)
        assert same_bits(view, whole[offset:offset + n]), (offset, n)
    big = 2 ** 33 + 3  # the slice rule across a 64-bit offset
    a = K.philox_normal_(torch.empty(64, device=dev, dtype=dtype), seed, stream, big)
    b = K.philox_normal_(torch.empty(32, device=dev, dtype=dtype), seed, stream, big + 17)
    assert same_bits(a[17:49], b)


def _lag_correlations(a, b, lags=range(-4, 5)):
    a = (a - a.mean()) / a.std()
    b = (b - b.mean()) / b.std()
    n = a.numel()
    out = {}
    for k in lags:
        x, y = (a[k:], b[:n - k]) if k >= 0 else (a[:n + k], b[-k:])
        out[k] = float((x * y).mean())
    return out


def test_philox_streams_and_seeds_share_no_shifted_run(K):
    n = 1 << 18
    f = lambda seed, stream: K.philox_normal_(torch.empty(n, device=dev), seed, stream, 0).double()  # noqa: E731
    s = 1000
    for a, b in ((f(77, s), f(77, s + 1)), (f(s, 5), f(s + 2, 5)), (f(s, 5), f(s + 1, 5))):
        c = _lag_correlations(a, b)
        assert max(abs(v) for v in c.values()) < 0.02, c
    c = _lag_correlations(f(77, s), f(77, s), lags=range(1, 5))  # and no correlation within a stream
    assert max(abs(v) for v in c.values()) < 0.02, c


def test_philox_moments(K):
    z = K.philox_normal_(torch.empty(1 << 20, device=dev), 2024, 6, 0).double()
    m, v, k = float(z.mean()), float(z.var()), float((z ** 4).mean())
    print(f"mean {m:.5f} variance {v:.5f} fourth moment {k:.4f}")
    assert abs(m) < 4e-3 and abs(v - 1) < 1e-2 and abs(k - 3) < 0.1
    zb = K.philox_normal_(torch.empty(1 << 20, device=dev, dtype=BF16), 2024, 6, 0)
    assert same_bits(zb, z.float().to(BF16))  # the bf16 output is the one rounding of the fp32 value


# ------------------------------------------------------------------------------------------------------------------
# vp_noise_frame
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_per", [1, 7, 1031, 1032])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_noise_frame_given_noise(K, dtype, n_per):
    """Bit-equal to torch's promoted arithmetic on the CPU.  1032: the 16-byte path (n_per a multiple of 8)."""
    g = torch.Generator().manual_seed(n_per)
    x = (torch.rand(2, n_per, generator=g) * 2 - 1).to(dtype)
    n = torch.randn(2, n_per, generator=g).to(dtype)
    sigma = torch.tensor([0.0371, 0.21], dtype=BF16)
    buf, out = guarded((2, n_per), BF16)
    K.noise_frame(x.to(dev), sigma.to(dev), n.to(dev), out=out)
    assert guards_intact(buf, 2 * n_per)
    assert same_bits(out, (x + n * sigma[:, None]).to(BF16))
    assert same_bits(out, R.noise_frame(x, n, sigma))


@pytest.mark.parametrize("n_per", [1, 7, 1031, 1032])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_noise_frame_draws_the_philox_stream(K, dtype, n_per):
    seed, stream = SEEDS_STREAMS[1]
    g = torch.Generator().manual_seed(n_per)
    x = (torch.rand(2, n_per, generator=g) * 2 - 1).to(dtype).to(dev)
    sigma = torch.tensor([0.0371, 0.21], dtype=BF16, device=dev)
    n = K.philox_normal_(torch.empty(2, n_per, device=dev, dtype=dtype), seed, stream, 0)
    want = K.noise_frame(x, sigma, n)
    buf, out = guarded((2, n_per), BF16)
    K.noise_frame(x, sigma, None, seed=seed, stream=stream, out=out)
    assert guards_intact(buf, 2 * n_per)
    assert same_bits(out, want)
    assert not same_bits(out, K.noise_frame(x, sigma, None, seed=seed + 1, stream=stream))


# ------------------------------------------------------------------------------------------------------------------
# vp_train_inputs_bf16
# ------------------------------------------------------------------------------------------------------------------

SHAPES = (((3, 5, 6), (9, 44, 50)), ((1, 5, 6), (1, 40, 48)), ((2, 8, 16), (5, 64, 128)))
OUT_CHANNELS = (16, 16, 32, 1, 17)
NAMES = ("target", "noisy", "noisy_model_input", "masks_latent", "conditioning_latents")
SF = 1.15258426
_TABLES = {}


def tables():
    if not _TABLES:
        from videopainter_amd.scheduler import CogVideoXDPMScheduler
        s = CogVideoXDPMScheduler()
        _TABLES["ac"] = s.alphas_cumprod
        _TABLES["sa_sb"] = s.add_noise_table(BF16, dev)
    return _TABLES["ac"], _TABLES["sa_sb"]


def launch(K, B, T, h, w, p, mask, ts, noises, dropout=False, seed=0, streams=(0, 0, 0, 0), sf=SF):
    """One guarded vp_train_inputs_bf16 call; returns the five outputs on the host after checking the guards."""
    outs = [guarded((B, T, c, h, w), BF16) for c in OUT_CHANNELS]
    K.train_inputs(p[0], p[1], p[2], mask, ts, tables()[1], sf, image_dropout=dropout, noises=noises, seed=seed,
                   streams=streams, out=[v for _, v in outs])
    got = {}
    for name, c, (buf, view) in zip(NAMES, OUT_CHANNELS, outs):
        host = buf.cpu()
        assert guards_intact(host, B * T * c * h * w), name
        got[name] = host[8:8 + view.numel()].view(view.shape)
        assert not bool(torch.isnan(got[name].float()).any()), name
    return got


def device_std(K, p_dev, L=16):
    """The kernel's own std = rbf(expf(rbf(0.5 clamp(logvar)))) of a posterior, bf16 [B, L, T, h, w] on the host:
    with zero mean, unit noise and scaling factor 1 the sample is rbf(0 + rbf(std * 1)) * 1 = std."""
    B, T, h, w, ld = p_dev.shape
    q = p_dev.clone()
    q[..., :L] = 0
    ones = torch.ones(B, L, T, h, w, device=dev, dtype=BF16)
    img = q[:, :1].contiguous()
    mask, ts = torch.zeros(B, 1, 1, 1, 1, device=dev), torch.zeros(B, device=dev, dtype=torch.int64)
    out = K.train_inputs(q, q, img, mask, ts, tables()[1], 1.0,
                         noises=(ones, ones, ones[:, :, :1].contiguous(), ones.permute(0, 2, 1, 3, 4).contiguous()))
    return out[0].permute(0, 2, 1, 3, 4).contiguous().cpu()


def checked_stds(K, ps_host, ps_dev, counts):
    """The device's std per posterior, after checking it against torch's: one bf16 value apart where it differs."""
    stds = []
    for ph, pd in zip(ps_host, ps_dev):
        sd, st = device_std(K, pd), R.posterior_std(ph, 16).contiguous()
        differ = bits(sd) != bits(st)
        counts[0] += int(differ.sum())
        counts[1] += sd.numel()
        assert bool(((bits(sd).int() - bits(st).int()).abs() <= 1).all())
        stds.append(sd)
    return stds


@pytest.mark.parametrize("ldp", [32, 40])
@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=["3x5x6", "1x5x6", "2x8x16"])
def test_train_inputs_given_noises(K, shape, ldp):
    """Every output element against the script's torch CPU ops, for each mask dtype, timestep pair and dropout."""
    (T, h, w), mask_shape = SHAPES[shape]
    B, L = 2, 16
    ac, _ = tables()
    counts = [0, 0]
    for mask_dtype in (torch.float32, BF16, torch.uint8):
        p_video, p_cond, p_image, noises, mask = R.synthetic_case(B, T, h, w, ldp, mask_shape, mask_dtype,
                                                                  seed=10 * shape + ldp)
        assert float(p_video[..., L:2 * L].float().min()) < -30 and float(p_video[..., L:2 * L].float().max()) > 20
        ps_dev = [t.to(dev) for t in (p_video, p_cond, p_image)]
        stds = checked_stds(K, (p_video, p_cond, p_image), ps_dev, counts)
        nz_dev = tuple(t.to(dev) for t in noises)
        for ts in ((0, 999), (500, 500), (-3, 1500)):
            for dropout in (False, True):
                t_host = torch.tensor(ts, dtype=torch.int64)
                got = launch(K, B, T, h, w, ps_dev, mask.to(dev), t_host.to(dev), nz_dev, dropout)
                want = R.front_of_step(p_video, p_cond, p_image, noises, t_host, ac, SF, mask, image_dropout=dropout,
                                       stds=stds)
                plain = R.front_of_step(p_video, p_cond, p_image, noises, t_host, ac, SF, mask, image_dropout=dropout)
                for name in NAMES:
                    assert same_bits(got[name], want[name]), (name, mask_dtype, ts, dropout)
                # the mask outputs do not depend on std: the plain restatement, everywhere
                assert same_bits(got["masks_latent"], plain["masks_latent"])
                assert same_bits(got["conditioning_latents"][:, :, L], plain["conditioning_latents"][:, :, L])
                assert same_bits(got["noisy_model_input"][:, :, :L], got["noisy"])
                assert same_bits(got["conditioning_latents"][:, :, L], got["masks_latent"][:, :, 0])
                assert torch.count_nonzero(got["noisy_model_input"][:, 1:, L:]) == 0
                if dropout:
                    assert torch.count_nonzero(got["noisy_model_input"][:, :, L:]) == 0
                if ts == (-3, 1500):  # clamped: the same bytes as (0, 999)
                    again = launch(K, B, T, h, w, ps_dev, mask.to(dev), torch.tensor((0, 999)).to(dev), nz_dev, dropout)
                    assert all(same_bits(got[k], again[k]) for k in NAMES)
    print(f"std elements where the device's exp and torch's round apart: {counts[0]} of {counts[1]}")
    assert counts[0] <= 1e-3 * counts[1]


def test_train_inputs_unaligned_buffers_take_the_elementwise_path(K):
    """Noise and output pointers off a 16-byte boundary (h w a multiple of 8): the same values as the vector path."""
    (T, h, w), mask_shape = SHAPES[2]
    B = 2
    p_video, p_cond, p_image, noises, mask = R.synthetic_case(B, T, h, w, 32, mask_shape, torch.float32, seed=5)
    ps_dev = [t.to(dev) for t in (p_video, p_cond, p_image)]
    nz = tuple(t.to(dev) for t in noises)
    ts = torch.tensor((17, 803)).to(dev)
    want = launch(K, B, T, h, w, ps_dev, mask.to(dev), ts, nz)
    outs = [guarded((B, T, c, h, w), BF16, guard=3) for c in OUT_CHANNELS]
    odd = []
    for t in nz:
        buf = torch.empty(t.numel() + 1, device=dev, dtype=BF16)
        buf[1:].copy_(t.flatten())
        odd.append(buf[1:].view(t.shape))
    K.train_inputs(*ps_dev, mask.to(dev), ts, tables()[1], SF, noises=odd, out=[v for _, v in outs])
    for name, c, (buf, view) in zip(NAMES, OUT_CHANNELS, outs):
        assert guards_intact(buf, view.numel(), guard=3), name
        assert same_bits(view, want[name]), name


@pytest.mark.parametrize("shape", [0, 2], ids=["3x5x6", "2x8x16"])
def test_train_inputs_draws_the_philox_streams(K, shape):
    (T, h, w), mask_shape = SHAPES[shape]
    B, L = 2, 16
    p_video, p_cond, p_image, _, mask = R.synthetic_case(B, T, h, w, 32, mask_shape, BF16, seed=3)
    ps_dev = [t.to(dev) for t in (p_video, p_cond, p_image)]
    ts = torch.tensor((250, 740)).to(dev)
    seed = (0xABCDEF << 32) | 99
    streams = ((5 << 20) + 2, (5 << 20) + 3, (5 << 20) + 1, (1 << 40) + 4)
    shapes = ((B, L, T, h, w), (B, L, T, h, w), (B, L, 1, h, w), (B, T, L, h, w))
    fills = tuple(K.philox_normal_(torch.empty(s, device=dev, dtype=BF16), seed, st, 0)
                  for s, st in zip(shapes, streams))
    want = launch(K, B, T, h, w, ps_dev, mask.to(dev), ts, fills)
    none = (None, None, None, None)
    got = launch(K, B, T, h, w, ps_dev, mask.to(dev), ts, none, seed=seed, streams=streams)
    again = launch(K, B, T, h, w, ps_dev, mask.to(dev), ts, none, seed=seed, streams=streams)
    other = launch(K, B, T, h, w, ps_dev, mask.to(dev), ts, none, seed=seed + 1, streams=streams)
    for name in NAMES:
        assert same_bits(got[name], want[name]), name
        assert same_bits(got[name], again[name]), name
    for name in ("target", "noisy", "noisy_model_input", "conditioning_latents"):
        assert not same_bits(got[name], other[name]), name
    assert not same_bits(got["noisy_model_input"][:, 0, L:], other["noisy_model_input"][:, 0, L:])
    assert same_bits(got["masks_latent"], other["masks_latent"])
    # one given tensor among generated ones
    mixed = launch(K, B, T, h, w, ps_dev, mask.to(dev), ts, (None, fills[1], None, fills[3]), seed=seed,
                   streams=streams)
    assert all(same_bits(mixed[k], want[k]) for k in NAMES)


# ------------------------------------------------------------------------------------------------------------------
# prepare_training_inputs end to end
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_step():
    """The tiny VAE (synthetic weights), 9 frames of 128 x 192 pixels (latent 3 x 16 x 24, the tiny models' grid)."""
    from tests.golden.cases import VAE_TINY_CFG, make_mask
    from videopainter_amd.scheduler import CogVideoXDPMScheduler
    from videopainter_amd.vae import AutoencoderKLCogVideoX
    vae = AutoencoderKLCogVideoX.from_config(dict(VAE_TINY_CFG, sample_height=128, sample_width=192), device=dev)
    vae.init_synthetic_weights_(7)
    g = torch.Generator().manual_seed(21)
    px = (torch.rand(2, 9, 3, 128, 192, generator=g) * 2 - 1).to(dev)
    mk = torch.from_numpy(make_mask(2, 9, 128, 192, "train_inputs.mask")).to(dev)
    cpx = px * (mk < 0.5)
    return vae, CogVideoXDPMScheduler(), px, cpx, mk


def _fields(r):
    return (r.model_input, r.noisy_video_latents, r.noisy_model_input, r.conditioning_latents, r.masks)


def test_prepare_training_inputs_end_to_end(K, tiny_step):
    from videopainter_amd import TrainingNoise, prepare_training_inputs
    from videopainter_amd import training as TR
    vae, sched, px, cpx, mk = tiny_step
    B, L, T, h, w = 2, 16, 3, 16, 24
    noise = TrainingNoise(77, rank=1)
    noise.next_step()
    first = prepare_training_inputs(vae, sched, px, cpx, mk, noise=noise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = prepare_training_inputs(vae, sched, px, cpx, mk, noise=noise)  # no host read of the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert res.model_input.shape == (B, T, L, h, w) and res.noisy_model_input.shape == (B, T, 2 * L, h, w)
    assert res.conditioning_latents.shape == (B, T, L + 1, h, w) and res.masks.shape == (B, T, 1, h, w)
    assert res.timesteps.dtype == torch.int64 and res.timesteps.shape == (B,) and res.timesteps.is_cuda
    assert all(same_bits(a, b) for a, b in zip(_fields(first), _fields(res)))  # same (seed, step, rank), same bytes
    assert torch.equal(first.timesteps, res.timesteps)

    # the draws, made explicitly
    ts_h, sigma_h, _ = noise.host_draws(B, 1000)
    assert torch.equal(res.timesteps.cpu(), ts_h) and same_bits(res.image_noise_sigma, sigma_h)
    fill = lambda shape, tid, dtype=BF16: K.philox_normal_(torch.empty(shape, device=dev, dtype=dtype),  # noqa: E731
                                                            noise.seed, noise.stream(tid), 0)
    nz = {"image_pixels": fill((B, 3, 128, 192), TR.NOISE_IMAGE_PIXELS, torch.float32),
          "image": fill((B, L, 1, h, w), TR.NOISE_POSTERIOR_IMAGE),
          "video": fill((B, L, T, h, w), TR.NOISE_POSTERIOR_VIDEO),
          "conditioning": fill((B, L, T, h, w), TR.NOISE_POSTERIOR_COND),
          "diffusion": fill((B, T, L, h, w), TR.NOISE_DIFFUSION)}
    given = prepare_training_inputs(vae, sched, px, cpx, mk, noise=TrainingNoise(1), timesteps=ts_h, noises=nz,
                                    image_noise_sigma=sigma_h, image_dropout=False)
    assert all(same_bits(a, b) for a, b in zip(_fields(given), _fields(res)))

    # the restatement on this VAE's own posterior parameters
    first_frame = px[:, 0].cpu()
    noisy_images = (first_frame + nz["image_pixels"].cpu() * sigma_h[:, None, None, None]).to(BF16)
    with torch.no_grad():
        p_image = vae.encode(noisy_images.to(dev).unsqueeze(2)).latent_dist._p
        p_video = vae.encode(px.permute(0, 2, 1, 3, 4)).latent_dist._p
        p_cond = vae.encode(cpx.permute(0, 2, 1, 3, 4)).latent_dist._p
    assert p_video.shape[:4] == (B, T, h, w) and p_image.shape[1] == 1
    ps_dev = [p.contiguous() for p in (p_video, p_cond, p_image)]
    ps = [p.cpu() for p in ps_dev]
    counts = [0, 0]
    stds = checked_stds(K, ps, ps_dev, counts)
    assert counts[0] <= 1e-3 * counts[1]
    nz_host = tuple(nz[k].cpu() for k in ("video", "conditioning", "image", "diffusion"))
    want = R.front_of_step(ps[0], ps[1], ps[2], nz_host, ts_h, sched.alphas_cumprod,
                           float(vae.config.scaling_factor), mk.cpu(), stds=stds)
    names = ("target", "noisy", "noisy_model_input", "conditioning_latents", "masks_latent")
    for got, name in zip(_fields(res), names):
        assert same_bits(got, want[name]), name
    assert torch.count_nonzero(res.noisy_model_input[:, 0, L:]) > 0

    # another step, another rank, the dropout
    noise.next_step()
    nxt = prepare_training_inputs(vae, sched, px, cpx, mk, noise=noise)
    other = TrainingNoise(77, rank=2)
    other.load_state_dict({"seed": 77, "step": 1})
    rk = prepare_training_inputs(vae, sched, px, cpx, mk, noise=other)
    for r in (nxt, rk):
        for a, b in zip(_fields(r)[:4], _fields(res)[:4]):
            assert not same_bits(a, b)
        assert same_bits(r.masks, res.masks)
    drop = prepare_training_inputs(vae, sched, px, cpx, mk, noise=noise, noised_image_dropout=1.0)
    assert drop.image_dropout and torch.count_nonzero(drop.noisy_model_input[:, :, L:]) == 0
    assert same_bits(drop.noisy_video_latents, nxt.noisy_video_latents)


def test_prepare_training_inputs_rejects_a_frame_mismatch(tiny_step):
    from videopainter_amd import TrainingNoise, prepare_training_inputs
    vae, sched, px, cpx, mk = tiny_step
    with pytest.raises(ValueError, match="frames"):
        prepare_training_inputs(vae, sched, px, cpx, mk[:, :5], noise=TrainingNoise(1))
    with pytest.raises(ValueError):
        prepare_training_inputs(vae, sched, px, cpx, mk, noise=TrainingNoise(1),
                                timesteps=torch.zeros(3, dtype=torch.int64))


def test_prepared_inputs_feed_the_training_step(tiny_step):
    """The result drives the tiny branch + frozen transformer + inpainting_v_loss step of tests/test_training_gpu.py:
    loss.backward() leaves finite gradients on the branch."""
    from tests.golden.cases import TINY_CFG, TINY_BRANCH_CFG, tiny_inputs, tiny_weights
    from videopainter_amd import (CogVideoXTransformer3DModel, CogvideoXBranchModel, TrainingNoise, device_scope,
                                  inpainting_v_loss, prepare_training_inputs)
    vae, sched, px, cpx, mk = tiny_step
    tsd, bsd = tiny_weights()
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**TINY_CFG)
        br = CogvideoXBranchModel(**TINY_BRANCH_CFG)
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    br.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()})
    tr.requires_grad_(False)
    br.requires_grad_(True)
    i = tiny_inputs()
    enc = i["enc"].to(dev).bfloat16()
    r = prepare_training_inputs(vae, sched, px, cpx, mk, noise=TrainingNoise(5))
    samples = br(hidden_states=r.noisy_video_latents, encoder_hidden_states=enc, branch_cond=r.conditioning_latents,
                 timestep=r.timesteps, image_rotary_emb=i["rope"], return_dict=False)[0]
    out = tr(hidden_states=r.noisy_model_input, encoder_hidden_states=enc, timestep=r.timesteps,
             image_rotary_emb=i["rope"], branch_block_samples=samples, branch_block_masks=r.masks,
             return_dict=False)[0]
    loss = inpainting_v_loss(out, r.noisy_video_latents, r.model_input, r.timesteps, sched.alphas_cumprod.to(dev),
                             r.masks, 1.0)
    loss.backward()
    assert bool(torch.isfinite(loss))
    grads = [p.grad for p in br.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g.float()).all()) for g in grads)
    assert any(float(g.float().abs().max()) > 0 for g in grads)
