"""The classifier-free-guidance halves' shared first-block work (forward(cfg_shared_video=True)), GPU only.

A tiny transformer (4 layers) and branch (2 layers) of the existing model tests' kind — 2 heads x 64, latent
3 x 20 x 30 (450 video tokens), 34 text tokens — on duplicated halves that differ in their text only.  Errors are
measured against the CPU oracle in fp32 and gated in the project's form (tests/test_model_gpu.py gate()): the hinted
path may drift at most 1.25 x the plain path's drift + 1e-3.
"""
import numpy as np
import pytest
import torch

from tests.golden.cases import TINY_CFG

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16
T, F, HL, WL = 34, 3, 20, 30
CFG = dict(TINY_CFG, max_text_seq_length=T, sample_height=HL, sample_width=WL)
BCFG = dict(CFG, num_layers=2)
GATE_MUL, GATE_ADD = 1.25, 1e-3


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle.cogvideox_oracle import prepare_rotary_positional_embeddings
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd.config import full_config, state_dict_shapes
    from videopainter_amd.weights import synth_state_dict
    tcfg, bcfg = full_config(CFG), full_config(BCFG, True)
    tsd = synth_state_dict(state_dict_shapes(tcfg), 11)
    bsd = synth_state_dict({("B." + k): v for k, v in state_dict_shapes(bcfg, True).items()}, 11)
    tsd = {k: torch.from_numpy(v) for k, v in tsd.items()}
    bsd = {k[2:]: torch.from_numpy(v) for k, v in bsd.items()}
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**CFG)
        br = CogvideoXBranchModel(**BCFG)
    tr.load_diffusers_state_dict(tsd)
    br.load_diffusers_state_dict(bsd)
    g = torch.Generator().manual_seed(21)
    video = torch.randn(1, F, 16, HL, WL, generator=g)
    image = torch.zeros(1, F, 16, HL, WL)
    image[:, 0] = torch.randn(1, 16, HL, WL, generator=g) * 0.7
    mask = torch.zeros(1, F, 1, HL, WL)
    mask[:, 1:, :, HL // 4:HL // 4 + HL // 2, WL // 4:WL // 4 + WL // 2] = 1.0
    masked = torch.randn(1, F, 16, HL, WL, generator=g) * (1.0 - mask)
    r = lambda x: x.to(BF16).float()  # noqa: E731  (the oracle sees the bf16-rounded inputs the HIP path gets)
    inp = dict(video=r(torch.cat([video] * 2)), hidden=r(torch.cat([torch.cat([video, image], dim=2)] * 2)),
               mask=torch.cat([mask] * 2), branch_cond=r(torch.cat([torch.cat([masked, mask], dim=2)] * 2)),
               enc=r(torch.randn(2, T, 32, generator=g)), timestep=torch.tensor([500, 500], dtype=torch.int64),
               rope=prepare_rotary_positional_embeddings(HL * 8, WL * 8, F, 64),
               latents=r(video), image_latents=r(image), masked_video=r(masked),
               video_latents=r(torch.randn(1, F, 16, HL, WL, generator=g)),
               noise=r(torch.randn(1, F, 16, HL, WL, generator=g)),
               step_noise=[r(torch.randn(1, F, 16, HL, WL, generator=g)) for _ in range(2)])
    return dict(tr=tr, br=br, tsd=tsd, bsd=bsd, tcfg=tcfg, bcfg=bcfg, inp=inp)


def _d(x):
    return x.to(dev, BF16)


@pytest.fixture
def probe(monkeypatch):
    """Records what block 0's shared path computes, from outside the model: the QKV GEMM's operand (the modulated
    rows) and the q / k / v handed to cfg_shared_attention; with probe["poison"] batch 1's video rows of the QKV
    buffer are filled with NaN before the attention runs."""
    from videopainter_amd import _native as NAT
    from videopainter_amd import kernels as K
    from videopainter_amd import transformer as TR
    p = {}
    gemm, shared = K.gemm, TR.cfg_shared_attention

    def gemm_rec(a, *args, **kw):
        if kw.get("epilogue") == NAT.EPI_BIAS_QKNORM_ROPE:
            p["_a"] = a
        return gemm(a, *args, **kw)

    def shared_rec(q, k, v, out, heads, text_len, **kw):
        qkv = q._base  # q / k / v are column slices of one [2, N, 3 D] buffer
        if p.get("poison"):
            qkv[1, text_len:] = float("nan")
        p.update(xn_rows=p.pop("_a"), qkv=qkv)
        return shared(q, k, v, out, heads, text_len, **kw)

    monkeypatch.setattr(K, "gemm", gemm_rec)
    monkeypatch.setattr(TR, "cfg_shared_attention", shared_rec)
    return p


@torch.no_grad()
@pytest.mark.parametrize("which", ["transformer", "branch"])
def test_block0_operands_bit_equal_on_the_rows_computed(env, probe, which):
    """The first N + T rows (batch 0 whole, batch 1's text rows) of block 0's modulated input and QKV output equal
    the plain path's bit for bit."""
    from videopainter_amd import kernels as K
    from videopainter_amd.attention_processor import _qkv, _rope_dev
    i = env["inp"]
    model = env["tr"] if which == "transformer" else env["br"]
    if which == "transformer":
        x = model.patch_embed.embed(_d(i["enc"]), _d(i["hidden"]))
    else:
        x = model.patch_embed.embed(_d(i["enc"]), _d(i["video"]), _d(i["branch_cond"]))
    assert torch.equal(x[0, T:], x[1, T:]) and not torch.equal(x[0, :T], x[1, :T])
    emb = model._time_embed(i["timestep"].to(dev), 2, torch.device(dev))
    rope = _rope_dev(i["rope"], torch.device(dev), grid=(F, HL // 2, WL // 2))
    blk = model.transformer_blocks[0]
    blk.forward_joint(x, T, emb, rope, cfg_shared_video=True)
    assert "qkv" in probe, "the shared path did not run"
    n1 = blk.norm1.norm
    xn = K.adaln_modulate(x, n1.weight, n1.bias, blk.norm1.modulation(emb), T, n1.eps)
    qkv = _qkv(blk.attn1, xn, (T, rope))
    rows = x.shape[1] + T
    D = x.shape[2]
    xn_rows, qkv_shared = probe["xn_rows"], probe["qkv"]  # (recorded when the shared path ran)
    assert tuple(xn_rows.shape) == (rows, D)  # the GEMM saw exactly N + T rows
    assert torch.equal(xn_rows, xn.view(-1, D)[:rows])
    assert torch.equal(qkv_shared.view(-1, 3 * D)[:rows], qkv.view(-1, 3 * D)[:rows])


@torch.no_grad()
def test_models_with_hint_match_oracle_and_never_read_batch1_video_rows(env, probe):
    """Branch and transformer outputs with the hint (batch 1's video rows of block 0's QKV output poisoned
    with NaN before the attention) and without it, each against the fp32 CPU oracle."""
    from oracle import cogvideox_oracle as O
    i = env["inp"]
    ob = O.branch_forward(env["bsd"], env["bcfg"], i["video"], i["enc"], i["branch_cond"], i["timestep"], i["rope"])
    ot = O.transformer_forward(env["tsd"], env["tcfg"], i["hidden"], i["enc"], i["timestep"], i["rope"],
                               branch_block_samples=ob, branch_block_masks=i["mask"])[0]

    def run(**hint):
        bs = env["br"](hidden_states=_d(i["video"]), encoder_hidden_states=_d(i["enc"]),
                       branch_cond=_d(i["branch_cond"]), timestep=i["timestep"].to(dev), image_rotary_emb=i["rope"],
                       return_dict=False, **hint)[0]
        out = env["tr"](hidden_states=_d(i["hidden"]), encoder_hidden_states=_d(i["enc"]),
                        timestep=i["timestep"].to(dev), image_rotary_emb=i["rope"],
                        branch_block_samples=[_d(b) for b in ob], branch_block_masks=_d(i["mask"]),
                        return_dict=False, **hint)[0]
        return bs, out

    bs_p, out_p = run()
    assert "qkv" not in probe  # no hint: the plain path
    probe["poison"] = True
    bs_h, out_h = run(cfg_shared_video=True)
    assert "qkv" in probe, "the shared path did not run"
    assert torch.isnan(probe["qkv"][1, T:]).all()  # (the poison was in place)
    for t in list(bs_h) + [out_h]:
        assert torch.isfinite(t.float()).all()
    for name, h, p, want in [("branch.0", bs_h[0], bs_p[0], ob[0]), ("branch.1", bs_h[1], bs_p[1], ob[1]),
                             ("transformer", out_h, out_p, ot)]:
        rh, rp = rel(h, want), rel(p, want)
        print(f"{name}: hinted rel-L2 {rh:.3e}  plain rel-L2 {rp:.3e}")
        assert rh <= GATE_MUL * rp + GATE_ADD, (name, rh, rp)


def _harness(tr, br):
    from videopainter_amd.pipeline import CogVideoXI2VDualInpaintAnyLHarness
    from videopainter_amd.scheduler import CogVideoXDPMScheduler
    sch = CogVideoXDPMScheduler(snr_shift_scale=1.0, prediction_type="v_prediction", rescale_betas_zero_snr=True,
                                clip_sample=False, set_alpha_to_one=True, timestep_spacing="trailing",
                                beta_start=0.00085, beta_end=0.012)
    sch.set_timesteps(2)
    return CogVideoXI2VDualInpaintAnyLHarness(tr, br, sch), sch.timesteps.cpu()


def _window(h, i, masked2=None, mask2=None):
    mask = i["mask"].permute(0, 2, 1, 3, 4)  # [2, 1, F, h, w], prepare_mask_latents' layout
    return h.make_window(i["latents"], i["image_latents"],
                         torch.cat([i["masked_video"]] * 2) if masked2 is None else masked2,
                         mask if mask2 is None else mask2, i["video_latents"], i["noise"])


@torch.no_grad()
def test_make_window_sets_the_flag_only_for_equal_halves(env):
    i = env["inp"]
    h, _ = _harness(env["tr"], env["br"])
    assert _window(h, i).cfg_shared is True
    masked2 = torch.cat([i["masked_video"], i["masked_video"] * 0.5])
    assert _window(h, i, masked2=masked2).cfg_shared is False
    mask2 = i["mask"].permute(0, 2, 1, 3, 4).clone()
    mask2[1, :, 1, 0, 0] = 1.0
    assert _window(h, i, mask2=mask2).cfg_shared is False


class _OracleModel:
    """The CPU oracle behind the harness's model calls (fp32 on the bf16 inputs the HIP models get)."""

    def __init__(self, model, sd, cfg, rope, branch):
        self.proj_out, self.config = model.proj_out, model.config
        self.sd, self.cfg, self.rope, self.branch = sd, cfg, rope, branch

    def __call__(self, hidden_states, encoder_hidden_states, timestep, **kw):
        from oracle import cogvideox_oracle as O
        f = lambda x: x.float().cpu()  # noqa: E731
        if self.branch:
            out = O.branch_forward(self.sd, self.cfg, f(hidden_states), f(encoder_hidden_states),
                                   f(kw["branch_cond"]), timestep.cpu(), self.rope, kw["conditioning_scale"])
            return ([o.to(dev) for o in out],)  # (fp32: the oracle transformer below takes them unrounded)
        out = O.transformer_forward(self.sd, self.cfg, f(hidden_states), f(encoder_hidden_states), timestep.cpu(),
                                    self.rope, branch_block_samples=[f(b) for b in kw["branch_block_samples"]],
                                    branch_block_masks=f(kw["branch_block_masks"]))[0]
        return out.to(dev, BF16).contiguous(), [], None


@torch.no_grad()
def test_harness_step_with_and_without_the_knob(env, probe, knobs):
    """One denoising step (CFG combine + DPM solver + replace-gt on the same noise draws): the latents with the
    halves' shared work and with VP_CFG_SHARED=0, each against the step run on the CPU oracle's model outputs."""
    i = env["inp"]
    pe = _d(i["enc"])

    def step(tr, br):
        h, ts = _harness(tr, br)
        st = _window(h, i)
        assert st.cfg_shared
        it = iter(i["step_noise"])
        h.step(st, 0, ts, pe, i["rope"], guidance_scale=6.0, use_dynamic_cfg=True, replace_gt=True, mask_add=True,
               step_noise=lambda: next(it))
        torch.cuda.synchronize()
        return st.latents

    hinted = step(env["tr"], env["br"])
    assert "qkv" in probe, "the harness did not pass the hint"
    probe.clear()
    knobs.setenv("VP_CFG_SHARED", "0")
    plain = step(env["tr"], env["br"])
    assert "qkv" not in probe
    want = step(_OracleModel(env["tr"], env["tsd"], env["tcfg"], i["rope"], False),
                _OracleModel(env["br"], env["bsd"], env["bcfg"], i["rope"], True))
    rh, rp = rel(hinted, want), rel(plain, want)
    print(f"step latents: hinted rel-L2 {rh:.3e}  plain rel-L2 {rp:.3e}  hinted vs plain {rel(hinted, plain):.3e}")
    assert np.isfinite(rh) and rh <= GATE_MUL * rp + GATE_ADD, (rh, rp)
