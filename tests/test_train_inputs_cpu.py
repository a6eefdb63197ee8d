"""The front of the training iteration (csrc/train_inputs.hip, videopainter_amd/training.py) — what needs no GPU:
the restatements of tests/train_input_refs.py against known answers and torch, their power to tell the mutants
apart, the host pieces (add_noise_table, TrainingNoise), and the argument errors, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_input_refs as R
from videopainter_amd import _native as N

BF16 = torch.bfloat16
PAIRS = ((49, 13), (9, 3), (5, 2), (17, 5), (44, 5), (40, 5), (480, 60), (720, 90))


# ---- the restatements ----

@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(np.array(counter, dtype=np.uint32), key)
    assert " ".join("%08x" % v for v in got) == want


def test_philox_stream_is_indexed_by_element():
    """Block e >> 2, lane e & 3, the carry into counter word 1, and the stream / seed words."""
    a = R.philox_normal_f64(3, 9, 0, 64)
    assert np.array_equal(R.philox_normal_f64(3, 9, 5, 20), a[5:25])
    big = R.philox_normal_f64(3, 9, 2 ** 34 - 3, 8)  # crosses block 2^32
    assert np.array_equal(big[3:], R.philox_normal_f64(3, 9, 2 ** 34, 5))
    xa, xb, odd = R.philox_words((7 << 32) | 5, (9 << 32) | 4, 2 ** 34 + 4, 4)
    w = R.philox4x32_10(np.array([1, 1, 4, 9], dtype=np.uint32), (5, 7))
    assert (xa[0], xb[0], xa[2], xb[2]) == (w[0], w[1], w[2], w[3]) and odd.tolist() == [0, 1, 0, 1]
    assert xa[0] == xa[1] and xb[2] == xb[3]
    z = R.philox_normal_f64(11, 2, 0, 1 << 18)
    assert abs(z.mean()) < 8e-3 and abs(z.var() - 1) < 2e-2
    z32 = R.philox_normal_f32(11, 2, 0, 1 << 18)  # float32 arithmetic stays inside the GPU test's bound
    assert np.all(np.abs(z32 - z) <= R.normal_bound(z))


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_nearest_map_is_torchs(n_in, n_out):
    t = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1, 1)
    assert F.interpolate(t, size=(n_out, 1, 1)).flatten().long().tolist() == R.nearest_map(n_in, n_out)


def test_nearest_map_example():
    assert R.nearest_map(49, 13) == [0, 3, 7, 11, 15, 18, 22, 26, 30, 33, 37, 41, 45]
    m = torch.rand(2, 9, 1, 44, 50)
    want = F.interpolate(m.permute(0, 2, 1, 3, 4), size=(3, 5, 6)).permute(0, 2, 1, 3, 4).to(BF16)
    assert torch.equal(R.resize_mask(m, (3, 5, 6)), want)


def _case(image_dropout=False, **mut):
    p_video, p_cond, p_image, noises, m = R.synthetic_case(2, 3, 5, 6, 32, (9, 44, 50), torch.float32, seed=1)
    return R.front_of_step(p_video, p_cond, p_image, noises, torch.tensor([0, 999]), R.alphas_cumprod_table(),
                           1.15258426, m, image_dropout=image_dropout, **mut)


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)) for k in a)


@pytest.mark.parametrize("mutant", ["fused_sample", "no_scaling", "swap_sa_sb", "keep_image_frames",
                                    "integer_division"])
def test_bit_comparison_rejects_mutant(mutant):
    """The comparison of the GPU test (bit equality per output) tells each broken restatement from the true one."""
    true = _case()
    assert _same(true, _case())
    assert not _same(true, _case(**{mutant: True}))


def test_restatement_shapes_and_edges():
    o = _case()
    assert o["target"].shape == (2, 3, 16, 5, 6) and o["noisy_model_input"].shape == (2, 3, 32, 5, 6)
    assert o["conditioning_latents"].shape == (2, 3, 17, 5, 6) and o["masks_latent"].shape == (2, 3, 1, 5, 6)
    assert torch.count_nonzero(o["noisy_model_input"][:, 1:, 16:]) == 0
    assert torch.count_nonzero(o["noisy_model_input"][:, 0, 16:]) > 0
    assert torch.count_nonzero(_case(image_dropout=True)["noisy_model_input"][:, :, 16:]) == 0
    assert torch.equal(o["conditioning_latents"][:, :, 16], o["masks_latent"][:, :, 0])
    # a std one bf16 value away changes some outputs but not most (the GPU test's substitution)
    p_video, p_cond, p_image, noises, m = R.synthetic_case(2, 3, 5, 6, 32, (9, 44, 50), torch.float32, seed=1)
    up = R.front_of_step(p_video, p_cond, p_image, noises, torch.tensor([0, 999]), R.alphas_cumprod_table(),
                         1.15258426, m, std_ulps=(1, 0, 0))
    frac = (up["target"] != o["target"]).float().mean().item()
    assert 0 < frac < 0.5 and torch.equal(up["conditioning_latents"], o["conditioning_latents"])


def test_noise_frame_promotion():
    x, n = torch.randn(2, 7), torch.randn(2, 7)
    s = torch.tensor([0.0371, 0.0454], dtype=BF16)
    want = (x + (n * s.float()[:, None])).to(BF16)  # fp32 x: sigma widened, product and sum in fp32
    assert torch.equal(R.noise_frame(x, n, s), want)
    xb, nb = x.to(BF16), n.to(BF16)
    assert R.noise_frame(xb, nb, s).dtype == BF16
    assert torch.equal(R.noise_frame(xb, nb, s), xb + (nb * s[:, None]))


# ---- host pieces ----

def test_add_noise_table_matches_scalars():
    from videopainter_amd.scheduler import CogVideoXDPMScheduler
    s = CogVideoXDPMScheduler()
    tab = s.add_noise_table()
    assert tab.dtype == torch.float32 and tab.shape == (1000, 2) and tab.is_contiguous()
    for t in (0, 1, 500, 999):
        assert tuple(tab[t].tolist()) == s.add_noise_scalars(t)
    assert s.add_noise_table() is tab  # kept
    assert torch.equal(tab.to(BF16).float(), tab)  # the values are the sample dtype's
    x, eps = torch.randn(2, 3, 4).to(BF16), torch.randn(2, 3, 4).to(BF16)
    ts = torch.tensor([3, 800])
    want = s.add_noise(x, eps, ts)
    sa, sb = tab[ts, 0].to(BF16)[:, None, None], tab[ts, 1].to(BF16)[:, None, None]
    assert torch.equal(sa * x + sb * eps, want)


def test_training_noise_streams_and_state():
    from videopainter_amd import TrainingNoise
    from videopainter_amd import training as TR
    ids = (TR.NOISE_IMAGE_PIXELS, TR.NOISE_POSTERIOR_IMAGE, TR.NOISE_POSTERIOR_VIDEO, TR.NOISE_POSTERIOR_COND,
           TR.NOISE_DIFFUSION)
    assert len(set(ids)) == 5 and all(0 <= i < 16 for i in ids)
    n = TrainingNoise(1234, rank=3)
    assert n.stream(TR.NOISE_DIFFUSION) == 3 * 16 + TR.NOISE_DIFFUSION
    n.next_step()
    n.next_step()
    assert n.step == 2 and n.stream(TR.NOISE_POSTERIOR_COND) == 2 * 2 ** 20 + 3 * 2 ** 4 + TR.NOISE_POSTERIOR_COND
    seen = set()
    for rank in (0, 1, 7, 4095):
        m = TrainingNoise(1234, rank=rank)
        for step in range(3):
            for i in ids:
                seen.add(m.stream(i))
            m.next_step()
    assert len(seen) == 4 * 3 * 5  # distinct per rank, step and tensor
    sd = n.state_dict()
    assert sd == {"seed": 1234, "step": 2}
    r = TrainingNoise(0, rank=3)
    r.load_state_dict(sd)
    assert (r.seed, r.step) == (1234, 2) and r.stream(4) == n.stream(4)
    a, b = n.host_draws(4, 1000), r.host_draws(4, 1000)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[0].dtype == torch.int64 and a[1].dtype == BF16 and a[0].shape == a[1].shape == (4,)
    assert int(a[0].min()) >= 0 and int(a[0].max()) < 1000 and 0.0 <= a[2] < 1.0
    assert bool((a[1].float() > 0.005).all()) and bool((a[1].float() < 0.5).all())  # exp(N(-3, 0.5))
    r.next_step()
    c = r.host_draws(4, 1000)
    d = TrainingNoise(1234, rank=4)
    d.load_state_dict(sd)
    e = d.host_draws(4, 1000)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[0], e[0])
    with pytest.raises(ValueError):
        TrainingNoise(1, rank=-1)
    with pytest.raises(ValueError):
        n.stream(16)


def test_public_names():
    import videopainter_amd as V
    from videopainter_amd import training
    assert V.TrainingNoise is training.TrainingNoise
    assert V.prepare_training_inputs is training.prepare_training_inputs


# ---- argument errors: nothing is launched ----

def _desc():
    d = N.TrainInputsDesc()
    d.struct_bytes = C.sizeof(N.TrainInputsDesc)
    d.B, d.T, d.h, d.w, d.L, d.ldp, d.image_T = 2, 3, 5, 6, 16, 32, 1
    d.Fp, d.Hp, d.Wp, d.mask_dtype, d.n_alphas = 9, 44, 50, 0, 1000
    d.scaling_factor = 1.0
    for f in ("p_video", "p_cond", "p_image", "timesteps", "sa_sb", "mask", "target", "noisy", "noisy_model_input",
              "masks_latent", "conditioning_latents"):
        setattr(d, f, 64)  # never dereferenced: each call below fails its host check
    return d


def test_argument_errors_launch_nothing():
    L = N.lib()
    assert L.vp_abi_version() >= 31 and N.ABI_VERSION >= 31
    assert L.vp_philox_normal(None, 0, 8, 1, 2, 0, None) == N.ERR_ARG
    assert L.vp_philox_normal(64, 0, 0, 1, 2, 0, None) == N.ERR_ARG
    assert L.vp_philox_normal(64, 1, -1, 1, 2, 0, None) == N.ERR_ARG
    assert L.vp_philox_normal(64, 1, 8, 1, 2, 2 ** 64 - 4, None) == N.ERR_ARG  # the offset would wrap
    for x, sigma, out, B, n in ((None, 64, 64, 2, 7), (64, None, 64, 2, 7), (64, 64, None, 2, 7), (64, 64, 64, 0, 7),
                                (64, 64, 64, 2, 0)):
        assert L.vp_noise_frame(x, 1, sigma, None, out, B, n, 1, 2, None) == N.ERR_ARG
    assert L.vp_train_inputs_bf16(None, None) == N.ERR_ARG
    assert L.vp_train_inputs_bf16(C.byref(N.TrainInputsDesc()), None) == N.ERR_ARG
    bad = [("struct_bytes", 8), ("L", 8), ("L", 32), ("ldp", 31), ("ldp", 30), ("image_T", 2), ("image_T", 0),
           ("T", 0), ("h", 0), ("w", -1), ("B", 0), ("Fp", 0), ("Hp", 0), ("Wp", 0), ("n_alphas", 0),
           ("mask_dtype", 3)]
    bad += [(f, None) for f in ("p_video", "p_cond", "p_image", "timesteps", "sa_sb", "mask", "target", "noisy",
                                "noisy_model_input", "masks_latent", "conditioning_latents")]
    for field, value in bad:
        d = _desc()
        setattr(d, field, value)
        assert L.vp_train_inputs_bf16(C.byref(d), None) == N.ERR_ARG, field


def test_prepare_training_inputs_rejects_without_a_device():
    from videopainter_amd import TrainingNoise, prepare_training_inputs
    from videopainter_amd.scheduler import CogVideoXDPMScheduler
    s, nz = CogVideoXDPMScheduler(), TrainingNoise(1)
    px = torch.zeros(1, 9, 3, 16, 16)
    mk = torch.zeros(1, 9, 1, 16, 16)
    with pytest.raises(ValueError, match="host tensor"):
        prepare_training_inputs(None, s, px, px, mk, noise=nz)
    with pytest.raises(ValueError, match="5-D"):
        prepare_training_inputs(None, s, px[0], px, mk, noise=nz)
    with pytest.raises(ValueError, match="shape of"):
        prepare_training_inputs(None, s, px, px[:, :5], mk, noise=nz)
    with pytest.raises(ValueError, match="frames"):
        prepare_training_inputs(None, s, px, px, mk[:, :5], noise=nz)
    with pytest.raises(ValueError, match=r"\[B, F, 1, H, W\]"):
        prepare_training_inputs(None, s, px, px, px, noise=nz)
    with pytest.raises(ValueError, match="TrainingNoise"):
        prepare_training_inputs(None, s, px, px, mk, noise=None)
    with pytest.raises(ValueError, match="unknown keys"):
        prepare_training_inputs(None, s, px, px, mk, noise=nz, noises={"latents": None})


def test_wrappers_refuse_host_tensors():
    from videopainter_amd import kernels as K
    with pytest.raises(TypeError):
        K.philox_normal_(torch.zeros(8), 1, 2)
    with pytest.raises(TypeError):
        K.noise_frame(torch.zeros(2, 8), torch.zeros(2, dtype=BF16))
    p = torch.zeros(1, 1, 2, 2, 32, dtype=BF16)
    with pytest.raises(ValueError):
        K.train_inputs(p, p, p, torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, dtype=torch.int64), torch.zeros(10, 2), 1.0)
