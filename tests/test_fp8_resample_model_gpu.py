"""The ID-resample processor on the fp8 two-segment attention (enable_fp8_attention(resample=True)), GPU only, on the
tiny model of tests/test_model_gpu.py's `env`: window 0 and the later window against the reference's fp32 goldens, the
launches every block makes, and the fall-backs to bf16 (a rope without a grid at the processor boundary, the switch
cleared).

Gate: r8 <= 1.5 * r16, the band of test_fp8_attention_model_modes (which measured a ratio of 1.00 on the standard
processor); the resample ratios are printed."""
import pytest
import torch

from tests.golden.cases import TINY_T
from tests.test_model_gpu import _d, env, rel  # noqa: F401  (env: the module fixture, reused here)

pytestmark = pytest.mark.gpu
dev = "cuda"


def _windows(env_):
    """Window 0 and the later window, run as test_resample_processor_matches_reference runs them."""
    i, g = env_["inp"], env_["g"]
    bs = [_d(g["branch.0"]), _d(g["branch.1"])]
    kw = dict(encoder_hidden_states=_d(i["enc"]), timestep=i["timestep"].to(dev), image_rotary_emb=i["rope"],
              branch_block_samples=bs, branch_block_masks=_d(i["mask"]), id_pool_resample_learnable=True,
              return_hidden_states=True, return_resample_mask=True, return_dict=False)
    out, hs, rm = env_["trr"](hidden_states=_d(i["hidden"]), **kw)
    out1 = env_["trr"](hidden_states=_d(i["hidden2"]),
                       attention_kwargs={"prev_hidden_states": {k: h for k, h in enumerate(hs)},
                                         "prev_clip_weight": 0.5, "prev_resample_mask": rm}, **kw)[0]
    return out, out1


@torch.no_grad()
def test_resample_windows_on_fp8(env, knobs):  # noqa: F811
    from videopainter_amd import kernels as K
    g, trr = env["g"], env["trr"]
    out16 = _windows(env)
    calls = {"fp8": [], "bf16": 0}
    real8, real16 = K.attention_fp8, K.attention

    def count8(*a, **kw):
        calls["fp8"].append(kw)
        return real8(*a, **kw)

    def count16(*a, **kw):
        calls["bf16"] += 1
        return real16(*a, **kw)
    trr.enable_fp8_attention(resample=True)
    try:
        knobs.setattr(K, "attention_fp8", count8)
        knobs.setattr(K, "attention", count16)
        out8 = _windows(env)
    finally:
        trr.enable_fp8_attention(False)
        knobs.setattr(K, "attention_fp8", real8)
        knobs.setattr(K, "attention", real16)
    torch.cuda.synchronize()
    nblk = len(trr.transformer_blocks)
    assert calls["bf16"] == 0 and len(calls["fp8"]) == 2 * nblk, (calls["bf16"], len(calls["fp8"]))
    for kw in calls["fp8"]:  # every block: one call with both segments, the count and the null-key mass
        assert all(kw.get(n) is not None for n in ("k2", "vp2", "k2_len", "l_extra")), sorted(kw)
    for o8, o16, gold in ((out8[0], out16[0], "resample0.out"), (out8[1], out16[1], "resample1.out")):
        r8, r16 = rel(o8, g[gold]), rel(o16, g[gold])
        print(f"fp8 resample attention {gold}: vs fp32 {r8:.3e} (bf16 HIP {r16:.3e}, ratio {r8 / r16:.2f}); "
              f"vs bf16 {rel(o8, o16):.3e}")
        assert torch.isfinite(o8.float()).all()
        assert r8 <= 1.5 * r16, (gold, r8, r16)
    # the switch cleared: bf16 again, bit for bit
    again = _windows(env)
    assert torch.equal(again[0], out16[0]) and torch.equal(again[1], out16[1])


@torch.no_grad()
@pytest.mark.parametrize("mode", ["resample0", "resample1"])
def test_rope_without_grid_falls_back_to_bf16(env, mode):  # noqa: F811
    """At the processor boundary (`Attention.forward` -> `processor.__call__`) the rope is a plain tuple: no grid,
    no closed-form plan — the opted-in block runs the bf16 code, bit for bit."""
    i = env["inp"]
    blk = env["trr"].transformer_blocks[0]
    attn = blk.attn1
    B, T, D = 2, TINY_T, 128
    Nv = i["rope"][0].shape[0]
    gen = torch.Generator().manual_seed(17)
    h = torch.randn(B, Nv, D, generator=gen)
    e = torch.randn(B, T, D, generator=gen)
    prev = torch.randn(B, T + Nv, D, generator=gen)
    rmask = torch.zeros(B, T + Nv, dtype=torch.bool)
    rmask[:, T:] = torch.rand(B, Nv, generator=gen) > 0.5
    kw = dict(resample_mask=rmask.to(dev))
    if mode == "resample1":
        kw.update(prev_hidden_states=_d(prev), prev_clip_weight=0.5, prev_resample_mask=rmask.to(dev))
    run = lambda: attn(hidden_states=_d(h), encoder_hidden_states=_d(e), image_rotary_emb=i["rope"], **kw)  # noqa: E731
    h16, e16 = run()
    blk.enable_fp8_attention(resample=True)
    try:
        h8, e8 = run()
    finally:
        blk.enable_fp8_attention(False)
    assert torch.equal(h8, h16) and torch.equal(e8, e16)
