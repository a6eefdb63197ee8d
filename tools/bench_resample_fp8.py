"""A/B of the ID-resample processor's attention in bf16 (p2a, two bf16 segments) against the fp8 two-segment kernel
(enable_fp8_attention(resample=True)) at BASELINE config 4's shape, versions interleaved in one process, device
events, every shape warmed up first.  Three measurements:

  stage     everything `attend_heads` does after the QKV GEMM — B 2, H 48, N 226 + 13*30*45 = 17 776, grid
            (13, 30, 45), the mask of the config-4 bench state — for window 0 and for a later window (prev-clip 0.5),
            bf16 (q / k normed by the GEMM's fused epilogue, as the bf16 path runs) against fp8 with all its
            quantise and pack launches; the attention launch alone beside it.
  chain     the config-4 chain (bench.py's own models, windows and harness): 2 windows x 1 step,
            enable_fp8(resample_attention=False) against True.
  accuracy  the full-width resample block of tests/golden/block_resample.safetensors (r0, r1) on the fp8 resample
            path against the reference's fp32 slice, beside fp8_block_gate(ref_bf16_rel) of tests/test_model_gpu.py.

  lora      (only when named) the same chain with enable_fp8(resample_attention=True) and a rank-256 adapter on
            to_q / to_k / to_v / to_out.0 of every block (bench.py --lora-rank's synthetic factors): loaded as the
            reference loads it — unfused, the adapters as low-rank bf16 launches beside the MX-FP8 projections —
            against fuse_lora() (folded, the folded weights re-quantised), interleaved.

    python tools/bench_resample_fp8.py [--rounds 5] [--iters 3] [--only stage,chain,accuracy]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videopainter_amd import kernels as K  # noqa: E402
from tools.bench_kernels import timeit  # noqa: E402

BF16 = torch.bfloat16
GRID = (13, 30, 45)
T = 226
dev = "cuda"


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "rounds_ms": [round(x, 4) for x in ms]}


def grid_rope(seed=0):
    """A separable 3D RoPE table for GRID (dims 0-15 by frame, 16-39 by row, 40-63 by column), with the grid attached
    as the transformer's forward attaches it."""
    from videopainter_amd.attention_processor import RopeTables
    g = torch.Generator().manual_seed(seed)
    F_, Hh, Ww = GRID
    at, ay, ax = (torch.rand(n, w // 2, generator=g).repeat_interleave(2, dim=1) * 6.28
                  for n, w in ((F_, 16), (Hh, 24), (Ww, 24)))
    ang = torch.cat([at[:, None, None, :].expand(F_, Hh, Ww, 16), ay[None, :, None, :].expand(F_, Hh, Ww, 24),
                     ax[None, None, :, :].expand(F_, Hh, Ww, 24)], dim=-1).reshape(-1, 64)
    rope = RopeTables((ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev)))
    rope.grid = GRID
    return rope


def bench_state_mask(B):
    """The resample mask of the config-4 bench state (bench._window_inputs: frames 1.., the centred half x half
    rectangle), patchified as the transformer does: uint8 [B, T + Nv], text rows clear."""
    import bench
    bench.set_config(2)
    F_, HL, WL = bench.F, bench.HL, bench.WL
    mask = torch.zeros(B, F_, 1, HL, WL)
    mask[:, 1:, :, HL // 4:HL // 4 + HL // 2, WL // 4:WL // 4 + WL // 2] = 1.0
    tok = K.patch_mask(mask.to(dev, BF16), 2)
    m = torch.zeros(B, T + tok.shape[1], device=dev, dtype=torch.uint8)
    m[:, T:] = tok
    return m


def stage(rounds, iters):
    from videopainter_amd import device_scope
    from videopainter_amd.transformer import CogVideoXBlock
    from videopainter_amd.attention_processor import bounded_scores
    B, H, D = 2, 48, 3072
    N = T + GRID[0] * GRID[1] * GRID[2]
    with device_scope(dev):
        blk = CogVideoXBlock(dim=D, num_attention_heads=H, attention_head_dim=64, time_embed_dim=512,
                             attention_bias=True, id_pool_resample_learnable=True)
    attn, proc = blk.attn1, blk.attn1.processor
    torch.manual_seed(0)
    with torch.no_grad():
        for ln in (attn.norm_q, attn.norm_k):
            ln.weight.copy_(1 + 0.1 * torch.randn(64, device=dev))
            ln.bias.copy_(0.1 * torch.randn(64, device=dev))
    blk.enable_fp8_attention(True, resample=True)
    rope, m = grid_rope(), bench_state_mask(B)
    plan = proc.plan(attn, m, T, rope)
    exps = proc.fp8_exponents(attn, plan)
    assert plan[3] is not None and exps is not None, "the closed-form null-key plan is needed"
    n_masked = [int(c) for c in plan[1].cpu()]
    qkv = torch.randn(B, N, 3 * D, device=dev).to(BF16)
    pkv = torch.randn(B, N, 2 * D, device=dev).to(BF16)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    pk, pv = pkv[..., :D], pkv[..., D:]
    o = torch.empty(B, N, D, device=dev, dtype=BF16)
    # (q / k are normed in place by some arms: LayerNorm outputs stay LayerNorm-sized inputs, the work is the same)
    arms = {
        "w0.bf16": lambda: proc.attend_heads(attn, q, k, v, T, rope, m, plan, True, o=o),
        "w0.fp8": lambda: proc.attend_heads(attn, q, k, v, T, rope, m, plan, False, o=o, fp8=exps),
        "later.bf16": lambda: proc.attend_heads(attn, q, k, v, T, rope, m, plan, True, pk, pv, 0.5, o),
        "later.fp8": lambda: proc.attend_heads(attn, q, k, v, T, rope, m, plan, False, pk, pv, 0.5, o, fp8=exps),
    }
    # the attention launches alone, on operands built once by the same producers (window 0's)
    dst, cnt, segments, axes = plan
    nq, nk = attn.norm_q, attn.norm_k
    q_exp, k_exp = exps
    q8 = K.head_norm_rope_fp8(q, H, T, nq.weight, nq.bias, nq.eps, rope, attn.scale * K.LOG2E * 2.0 ** q_exp)
    k8 = K.head_norm_rope_fp8(k, H, T, nk.weight, nk.bias, nk.eps, rope, 2.0 ** k_exp)
    vp = K.v_pack_fp8(v, H)
    k2_8 = torch.zeros(B, N, D, device=dev, dtype=torch.uint8)
    K.head_norm_rope_fp8(k, H, T, nk.weight, nk.bias, nk.eps, rope, 2.0 ** k_exp, out=k2_8, tok_mask=m, dst_rows=dst)
    v2 = torch.zeros(B, N, D, device=dev, dtype=BF16)
    K.mask_scale_rows(v, v2, m, 1.0, dst_rows=dst)
    vp2 = K.v_pack_fp8(v2, H, lens=cnt)
    k2 = torch.zeros(B, N, D, device=dev, dtype=BF16)
    K.head_norm_rope(k, k2, H, T, nk.weight, nk.bias, nk.eps, rope, tok_mask=m, pre_scale=1.0, dst_rows=dst)
    qn, kn = torch.empty_like(k2), torch.empty_like(k2)
    K.head_norm_rope(q, qn, H, T, nq.weight, nq.bias, nq.eps, rope)
    K.head_norm_rope(k, kn, H, T, nk.weight, nk.bias, nk.eps, rope)
    lx = K.null_key_mass(qn, H, T, GRID, nk.bias, axes, m, segments, attn.scale)
    bs = bounded_scores(attn)
    arms["launch.bf16"] = lambda: K.attention(qn, kn, v, o, H, k2=k2, v2=v2, scale=attn.scale, bounded_scores=bs,
                                              k2_len=cnt, l_extra=lx)
    arms["launch.fp8"] = lambda: K.attention_fp8(q8, k8, vp, o, H, q_exp, k_exp, k2=k2_8, vp2=vp2, k2_len=cnt,
                                                 l_extra=lx)
    res = {a: [] for a in arms}
    with torch.no_grad():
        for fn in arms.values():  # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for a, fn in arms.items():
                res[a].append(timeit(fn, iters) * 1e3)
    fl = sum(4.0 * H * N * (N + c) * 64 for c in n_masked)  # MFMA FLOP of the attention launch (both segments)
    out = {"shape": {"B": B, "H": H, "N": N, "grid": GRID, "masked_rows": n_masked}, "arms": {}}
    for a, ms in res.items():
        out["arms"][a] = summary(ms)
        if a.startswith("launch"):
            out["arms"][a]["median_pflops"] = round(fl / (statistics.median(ms) / 1e3) / 1e15, 4)
    for w in ("w0", "later", "launch"):
        b16, f8 = out["arms"][w + ".bf16"], out["arms"][w + ".fp8"]
        out[w + ".fp8_over_bf16_median"] = round(f8["median_ms"] / b16["median_ms"], 4)
    print("stage " + json.dumps(out), flush=True)


def _chain_models():
    """(transformer, branch, run): bench.py's config-4 models on the fp8 path and a call that runs the chain's 2
    windows x 1 step."""
    import bench
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd.config import COGVIDEOX_5B_I2V
    from videopainter_amd.pipeline import CogVideoXI2VDualInpaintAnyLHarness
    from videopainter_amd.scheduler import CogVideoXDPMScheduler
    bench.set_config(2)
    device = torch.device("cuda", 0)
    cfg = dict(COGVIDEOX_5B_I2V, sample_height=bench.HL, sample_width=bench.WL)
    with device_scope(device):
        tr = CogVideoXTransformer3DModel(**dict(cfg, id_pool_resample_learnable=True))
        br = CogvideoXBranchModel(**dict(cfg, num_layers=bench.LB))
    tr.init_synthetic_weights_(1234)
    br.init_synthetic_weights_(1235)
    tr.enable_fp8()
    br.enable_fp8()
    sched = CogVideoXDPMScheduler(snr_shift_scale=1.0, prediction_type="v_prediction", rescale_betas_zero_snr=True,
                                  clip_sample=False, set_alpha_to_one=True, timestep_spacing="trailing")
    harness = CogVideoXI2VDualInpaintAnyLHarness(tr, br, sched)
    g = torch.Generator().manual_seed(42)
    wins = [bench._window_inputs(g, device, w == 0) for w in range(2)]
    pe = torch.randn(1, bench.T, 4096, generator=g).to(device, BF16)
    npe = torch.randn(1, bench.T, 4096, generator=g).to(device, BF16)
    kw = dict(num_frames=49, stride=49, guidance_scale=6.0, use_dynamic_cfg=True, replace_gt=True, mask_add=True,
              prev_clip_weight=0.5, id_pool_resample_learnable=True)

    def run():
        return harness(wins, pe, npe, num_inference_steps=1, generator=torch.Generator().manual_seed(0), **kw)
    return tr, br, run


def chain(rounds):
    tr, br, run = _chain_models()
    res = {"resample_attention=False": [], "resample_attention=True": []}
    outs = {}
    with torch.no_grad():
        for arm in res:  # warm-up of both forms
            tr.enable_fp8_attention(True, resample=arm.endswith("True"))
            outs[arm] = run().float()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for arm in res:
                tr.enable_fp8_attention(True, resample=arm.endswith("True"))
                res[arm].append(timeit(run, 1) * 1e3 / 2)  # per step: 2 windows x 1 step
    a, b = outs.values()
    out = {"what": "config-4 chain, 2 windows x 1 step, ms per denoising step (QKV / out / FFN in fp8 in both arms)",
           "arms": {k: summary(v) for k, v in res.items()},
           "latents_rel_true_vs_false": float((b - a).norm() / (a.norm() + 1e-30))}
    f, t = (out["arms"][k]["median_ms"] for k in res)
    out["true_over_false_median"] = round(t / f, 4)
    print("chain " + json.dumps(out), flush=True)


def lora(rounds, rank=256):
    from videopainter_amd.lora import attach_lora_
    tr, br, run = _chain_models()
    tr.enable_fp8_attention(True, resample=True)
    gl = torch.Generator(device=dev).manual_seed(91)
    lsd = {}
    for i, blk in enumerate(tr.transformer_blocks):  # (bench.py --lora-rank's adapter)
        for t, lin in (("to_q", blk.attn1.to_q), ("to_k", blk.attn1.to_k), ("to_v", blk.attn1.to_v),
                       ("to_out.0", blk.attn1.to_out[0])):
            o_f, i_f = lin.weight.shape
            lsd[f"transformer_blocks.{i}.attn1.{t}.lora_A.weight"] = (
                torch.randn(rank, i_f, device=dev, generator=gl) * i_f ** -0.5).to(BF16)
            lsd[f"transformer_blocks.{i}.attn1.{t}.lora_B.weight"] = (
                torch.randn(o_f, rank, device=dev, generator=gl) * 0.01).to(BF16)
    with torch.no_grad():
        none = run().float()
    attach_lora_(tr, lsd, 1.0, "vpid")
    del lsd

    def arm(fused):
        tr.fuse_lora() if fused else tr.unfuse_lora()
    res, outs = {"unfused": [], "fused": []}, {}
    with torch.no_grad():
        for a in res:  # warm-up of both forms
            arm(a == "fused")
            outs[a] = run().float()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for a in res:
                arm(a == "fused")
                torch.cuda.synchronize()
                res[a].append(timeit(run, 1) * 1e3 / 2)  # per step: 2 windows x 1 step
    u, f = outs["unfused"], outs["fused"]
    out = {"what": f"config-4 chain on the fp8 path (QKV, resample attention, out, FFN), rank-{rank} adapter on every "
                   "block's q / k / v / out, 2 windows x 1 step, ms per denoising step",
           "arms": {k: summary(v) for k, v in res.items()},
           "latents_rel_unfused_vs_fused": float((u - f).norm() / (f.norm() + 1e-30)),
           "latents_rel_adapter_effect": float((f - none).norm() / (none.norm() + 1e-30))}
    um, fm = (out["arms"][k]["median_ms"] for k in res)
    out["unfused_over_fused_median"] = round(um / fm, 4)
    print("lora " + json.dumps(out), flush=True)


def accuracy():
    from safetensors.torch import load_file
    from tests.golden.cases import resample_block_case
    from tests.test_model_gpu import fp8_block_gate, gate, rel
    from videopainter_amd import device_scope
    from videopainter_amd.attention_processor import RopeTables
    from videopainter_amd.transformer import CogVideoXBlock
    c = resample_block_case()
    gold = load_file(os.path.join(ROOT, "tests", "golden", "block_resample.safetensors"))
    with device_scope(dev):
        blk = CogVideoXBlock(dim=3072, num_attention_heads=48, attention_head_dim=64, time_embed_dim=512,
                             attention_bias=True, id_pool_resample_learnable=True)
    with torch.no_grad():
        for k, p in blk.state_dict().items():
            p.copy_(torch.from_numpy(c["weights"][k]))
    rope = RopeTables(c["rope"])
    rope.grid = GRID
    d = lambda x: x.to(dev, BF16)  # noqa: E731
    out = {}
    with torch.no_grad():
        for form in ("bf16", "fp8 resample attention", "fp8 QKV + resample attention + out + FFN"):
            if form != "bf16":
                blk.enable_fp8_attention(True, resample=True)
            if form.startswith("fp8 QKV"):
                blk.enable_fp8_ffn()
                blk.enable_fp8_qkv()
                blk.enable_fp8_out()
            for mode in ("r0", "r1"):
                kw = None
                if mode == "r1":
                    kw = {"prev_hidden_states": d(c["prev"]), "prev_clip_weight": 0.5,
                          "prev_resample_mask": c["prev_resample_mask"].to(dev)}
                h, e = blk(hidden_states=d(c["h"]), encoder_hidden_states=d(c["e"]), temb=d(c["temb"]),
                           image_rotary_emb=rope, resample_mask=c["resample_mask"].to(dev), attention_kwargs=kw)
                flat = torch.cat([e, h], dim=1).reshape(-1).float().cpu()
                rb = float(gold[f"{mode}.ref_bf16_rel"][0])
                out[f"{mode}.{form}"] = {"rel_vs_reference_fp32": rel(flat[::997], gold[f"{mode}.slice"]),
                                         "reference_bf16_rel": rb, "bf16_gate": gate(rb),
                                         "fp8_block_gate": fp8_block_gate(rb)}
    print("accuracy " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", default="stage,chain,accuracy")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("an A/B here takes at least 5 interleaved rounds")
    only = a.only.split(",")
    if "stage" in only:
        stage(a.rounds, a.iters)
    if "accuracy" in only:
        accuracy()
    if "chain" in only:
        chain(a.rounds)
    if "lora" in only:
        lora(a.rounds)


if __name__ == "__main__":
    main()
