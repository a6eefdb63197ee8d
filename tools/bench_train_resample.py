"""A/B of the VideoPainterID LoRA training step with the ID-resample processor's backward in its explicit 2N-key form
(the default) against the closed-form one (`enable_closed_form_resample_backward`), arms interleaved in one process.

    python tools/bench_train_resample.py [--rounds 5] [--rank 256] [--height 60 --width 90] [--fp8-gemm [ffn,qkv,out]]

One step = the reference's ID training iteration (train/VideoPainterID.sh ->
train/train_cogvideox_inpainting_i2v_video_resample.py:1520-1526, 1940-1961) at B = 1, 49 frames 480x720 (latent
13x60x90, N = 226 + 13*30*45 = 17 776): the frozen 2-layer branch's forward, the frozen 42-layer 5b-I2V transformer
with the resample processor (window 0) and trainable LoRA (rank 256) on to_q / to_k / to_v / to_out.0, the branch
samples injected under the mask, and the backward of a synthetic output gradient into every LoRA factor.  The mask is
the box of BASELINE config 4's bench state (frames 1.., the centred half x half rectangle: 4 416 masked token rows, as
tools/bench_resample_fp8.py builds it).  Random-init weights, synthetic latents.

Per arm: wall-clock ms per step over `--rounds` interleaved rounds (median, min, max) and, from one more step under
HIP events (kernels.timed_launches), the summed time of the attention-class launches (attention forward, flash
backward, null-key mass backward).  Also the flash backward alone at this shape, per call: N keys (the plain training
step's call, which the new template instance must leave as it was), 2N keys (the explicit arm's) and 2N with
k_len = N + masked rows (the closed-form arm's).  Prints one JSON line.

--fp8-gemm [SUBSET] (default when given: ffn,qkv,out): each backward form also runs with the frozen transformer's
projections on the MX-FP8 GEMMs (enable_fp8(attention=False); the LoRA adapters beside them as low-rank bf16 launches,
forward and backward), the four arms interleaved in this one process — the bf16 arms are the code path without the
switch, so each fp8 arm is compared with the bf16 arm of the same rounds.  Per arm then also the peak memory of one
step and the step's time by launch class under HIP events (the bf16 GEMMs, the MX GEMMs, the attention classes and
the rest), which says where a gain went if the arms tie.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, LB = 226, 13, 2
CLASSES = ("attention", "attention_bwd", "null_key_mass_bwd")
GEMM_CLASSES = ("gemm", "gemm_mx")
BF16 = torch.bfloat16


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2),
            "rounds_ms": [round(x, 2) for x in ms]}


def backward_calls(K, dev, ntok, masked, iters=3, rounds=5):
    """ms per flash-backward call at H = 48: (N keys), (2N keys), (2N keys, k_len = N + masked)."""
    H, D = 48, 3072
    g = torch.Generator().manual_seed(3)
    q, do = (torch.randn(1, ntok, D, generator=g).to(dev, BF16) for _ in range(2))
    k, v = (torch.randn(1, 2 * ntok, D, generator=g).to(dev, BF16) for _ in range(2))
    kl = torch.tensor([ntok + masked], dtype=torch.int32, device=dev)
    arms = {}
    for name, nk, kw in (("N", ntok, {}), ("2N", 2 * ntok, {}), ("2N_k_len", 2 * ntok, {"k_len": kl})):
        o = torch.empty(1, ntok, D, device=dev, dtype=BF16)
        lse = torch.empty(1, H, ntok, device=dev, dtype=torch.float32)
        n_real = ntok + masked if kw else nk
        K.attention(q, k[:, :n_real], v[:, :n_real], o, H, lse=lse)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k[:, :nk]), torch.empty_like(v[:, :nk])
        arms[name] = (lambda nk=nk, o=o, lse=lse, dq=dq, dk=dk, dv=dv, kw=kw:
                      K.attention_bwd(q, k[:, :nk], v[:, :nk], o, do, lse, H, dq=dq, dk=dk, dv=dv, **kw))
    res = {a: [] for a in arms}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for a, fn in arms.items():
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            for _ in range(iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            res[a].append(ev[0].elapsed_time(ev[1]) / iters)
    return {a: summary(ms) for a, ms in res.items()}


def fp8_gemm_ab(args, K, step, which, grads_of) -> dict:
    """The four arms (explicit / closed form x bf16 / fp8) interleaved: step ms over --rounds rounds, each fp8 arm
    against the bf16 arm of its form (a gain is claimed only where their ranges do not overlap), the fp8 arms'
    gradients against the bf16 arms', and per arm one step under HIP events by launch class and its peak memory."""
    arms = [(f"{form}_{prec}", closed, fp8) for form, closed in (("explicit", False), ("closed_form", True))
            for prec, fp8 in (("bf16", False), ("fp8", True))]
    grad_rel = {}
    for form, closed in (("explicit", False), ("closed_form", True)):  # (also the fp8 arms' warm-up)
        g16, g8 = grads_of(closed, False), grads_of(closed, True)
        num = sum(float((a.float() - b.float()).square().sum()) for a, b in zip(g8, g16))
        grad_rel[form] = (num / sum(float(b.float().square().sum()) for b in g16)) ** 0.5
        del g16, g8
    torch.cuda.synchronize()
    res = {a: [] for a, _, _ in arms}
    for r in range(args.rounds):
        for a, closed, fp8 in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(closed, fp8=fp8)
            torch.cuda.synchronize()
            res[a].append((time.perf_counter() - t0) * 1e3)
        print(f"fp8-gemm round {r}: " + "  ".join(f"{a} {res[a][-1]:.1f} ms" for a, _, _ in arms), file=sys.stderr,
              flush=True)
    out = dict(fp8_gemm=which, rounds=args.rounds, step_ms={a: summary(ms) for a, ms in res.items()},
               fp8_vs_bf16_grad_rel=grad_rel, class_ms_per_step={}, launches_per_step={}, peak_mem_gib={})
    names = GEMM_CLASSES + CLASSES
    for a, closed, fp8 in arms:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        with K.timed_launches(*names) as tl:
            ev[0].record()
            step(closed, fp8=fp8)
            ev[1].record()
        torch.cuda.synchronize()
        cl = {n: round(tl.mean_ms(n) * tl.count(n), 2) for n in names}
        cl["rest"] = round(ev[0].elapsed_time(ev[1]) - sum(cl.values()), 2)
        out["class_ms_per_step"][a] = cl
        out["launches_per_step"][a] = {n: tl.count(n) for n in names}
        out["peak_mem_gib"][a] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    for form in ("explicit", "closed_form"):
        b, f = out["step_ms"][f"{form}_bf16"], out["step_ms"][f"{form}_fp8"]
        out[f"{form}_ranges_overlap"] = not (f["max_ms"] < b["min_ms"] or b["max_ms"] < f["min_ms"])
        out[f"{form}_fp8_over_bf16"] = round(f["median_ms"] / b["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rank", type=int, default=256)
    ap.add_argument("--height", type=int, default=60)
    ap.add_argument("--width", type=int, default=90)
    ap.add_argument("--fp8-gemm", nargs="?", const="ffn,qkv,out", default=None, metavar="SUBSET",
                    help="also run each backward form on the MX-FP8 GEMMs (subset of ffn,qkv,out), interleaved")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("at least 5 rounds")
    which = set(filter(None, args.fp8_gemm.split(","))) if args.fp8_gemm is not None else set()
    if args.fp8_gemm is not None and (not which or which - {"ffn", "qkv", "out"}):
        raise SystemExit(f"--fp8-gemm takes a subset of ffn,qkv,out, got {args.fp8_gemm!r}")
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd import kernels as K
    from videopainter_amd.config import COGVIDEOX_5B_I2V
    from videopainter_amd.embeddings import prepare_rotary_positional_embeddings

    dev = "cuda"
    HL, WL = args.height, args.width
    cfg = dict(COGVIDEOX_5B_I2V, sample_height=HL, sample_width=WL)
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**dict(cfg, id_pool_resample_learnable=True))
        br = CogvideoXBranchModel(**dict(cfg, num_layers=LB))
    tr.init_synthetic_weights_(1234)
    br.init_synthetic_weights_(1235)
    br.requires_grad_(False)
    tr.add_adapter({"r": args.rank, "lora_alpha": args.rank, "init_lora_weights": True,
                    "target_modules": ["to_q", "to_k", "to_v", "to_out.0"]})
    params = [p for p in tr.parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():  # (PEFT starts B at 0: a trained-looking pair, so that no gradient is identically zero)
        for p in params:
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    lat = torch.randn(1, F, 16, HL, WL, generator=g).to(dev, BF16)
    img = torch.zeros(1, F, 16, HL, WL)
    img[:, 0] = torch.randn(1, 16, HL, WL, generator=g)
    img = img.to(dev, BF16)
    mask = torch.zeros(1, F, 1, HL, WL)
    mask[:, 1:, :, HL // 4:HL // 4 + HL // 2, WL // 4:WL // 4 + WL // 2] = 1.0
    mask = mask.to(dev, BF16)
    masked = int(K.patch_mask(mask, 2).sum())
    cond = torch.cat([lat * (1 - mask), mask], 2)
    hidden = torch.cat([lat, img], 2)
    enc = torch.randn(1, T, 4096, generator=g).to(dev, BF16)
    ts = torch.tensor([500], device=dev)
    rope = tuple(t.to(dev) for t in prepare_rotary_positional_embeddings(HL * 8, WL * 8, F, 64))
    dout = torch.randn(1, F, 16, HL, WL, generator=g).to(dev, BF16)
    ntok = T + F * (HL // 2) * (WL // 2)

    mx = None
    if which:  # quantised once; an arm switches the blocks' MX weights on or off (as tools/bench_train.py --fp8-gemm)
        tr.enable_fp8(ffn="ffn" in which, attention=False, qkv="qkv" in which, out="out" in which)
        mx = [(b.ff_mx, b.qkv_mx, b.out_mx) for b in tr.transformer_blocks]

    def step(closed: bool, keep_grads: bool = False, fp8: bool = False):
        tr.enable_closed_form_resample_backward(closed)
        if mx is not None:
            for b, m in zip(tr.transformer_blocks, mx):
                b.ff_mx, b.qkv_mx, b.out_mx = m if fp8 else (None, None, None)
        with torch.no_grad():
            samples = br(hidden_states=lat, encoder_hidden_states=enc, branch_cond=cond, timestep=ts,
                         image_rotary_emb=rope, return_dict=False)[0]
        out = tr(hidden_states=hidden, encoder_hidden_states=enc, timestep=ts, image_rotary_emb=rope,
                 branch_block_samples=samples, branch_block_masks=mask, id_pool_resample_learnable=True,
                 return_dict=False)[0]
        out.backward(dout)
        grads = [p.grad for p in params] if keep_grads else None
        for p in params:
            p.grad = None
        return grads

    arms = (("explicit", False), ("closed_form", True))
    # warm-up of both arms; their gradients against each other (the same function differentiated two ways)
    g_exp, g_cf = step(False, True), step(True, True)
    num = sum(float((a.float() - b.float()).square().sum()) for a, b in zip(g_cf, g_exp))
    den = sum(float(b.float().square().sum()) for b in g_exp)
    grad_rel = (num / den) ** 0.5
    del g_exp, g_cf
    torch.cuda.synchronize()
    res = {a: [] for a, _ in arms}
    for r in range(args.rounds):
        for a, closed in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(closed)
            torch.cuda.synchronize()
            res[a].append((time.perf_counter() - t0) * 1e3)
        print(f"round {r}: " + "  ".join(f"{a} {res[a][-1]:.1f} ms" for a, _ in arms), file=sys.stderr, flush=True)
    classes, counts = {}, {}
    for a, closed in arms:
        with K.timed_launches(*CLASSES) as tl:
            step(closed)
        torch.cuda.synchronize()
        classes[a] = {n: round(tl.mean_ms(n) * tl.count(n), 2) for n in CLASSES}
        classes[a]["sum"] = round(sum(classes[a].values()), 2)
        counts[a] = {n: tl.count(n) for n in CLASSES}
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    out = dict(metric="VideoPainterID LoRA training step, ms (5b-I2V frozen + LoRA, resample processor, 49f 480x720, "
                      "B=1)", ntok=ntok, masked_rows=masked, lora_rank=args.rank, rounds=args.rounds,
               step_ms={a: summary(ms) for a, ms in res.items()}, attention_class_ms_per_step=classes,
               launches_per_step=counts, closed_form_vs_explicit_grad_rel=grad_rel, peak_mem_gib=round(peak, 2))
    e, c = out["step_ms"]["explicit"], out["step_ms"]["closed_form"]
    out["ranges_overlap"] = not (c["max_ms"] < e["min_ms"] or e["max_ms"] < c["min_ms"])
    out["closed_form_over_explicit"] = round(c["median_ms"] / e["median_ms"], 4)
    if which:
        out["fp8_gemm"] = fp8_gemm_ab(args, K, step, sorted(which), grads_of=lambda c, f: step(c, True, f))
    del tr, br
    torch.cuda.empty_cache()
    out["attention_bwd_call_ms"] = backward_calls(K, dev, ntok, masked)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
