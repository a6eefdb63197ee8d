"""Training-step throughput of the VideoPainter training path on one MI355X.

    python tools/bench_train.py [--steps K] [--warmup W] [--height 60 --width 90]
                                [--optimizer none|torch|fused|adam|prodigy|sharded|sharded-adam|sharded-prodigy]
                                [--loss] [--accumulate K] [--inputs]
                                [--fp8-gemm [ffn,qkv,out]] [--rounds R]
    python tools/bench_train.py --inputs-ab [--steps K] [--warmup W] [--rounds R]

One step = the reference's training iteration (train/train_cogvideox_inpainting_i2v_video.py:1856-1892 with the
launch script train/VideoPainter.sh: 49 frames 480x720 -> latent 13x60x90, batch 1, bf16, branch_layer_num 2,
--mask_add, --gradient_checkpointing): 2-layer branch forward (trainable) -> 42-layer 5b-I2V transformer forward
(frozen) with the samples injected under the mask -> backward of a synthetic loss gradient into every branch
parameter.  --optimizer torch adds torch's AdamW (foreach) stepped directly on the bf16 branch parameters (PyTorch's
kernels, and no master weights: most of an lr = 1e-5 update is lost below the bf16 ulp); --optimizer fused adds
videopainter_amd.FusedAdamW(max_grad_norm=1.0): gradient norm + clip + AdamW with fp32 master weights on the HIP
kernels (csrc/optim.hip); --optimizer adam and --optimizer prodigy add videopainter_amd.FusedAdam and
videopainter_amd.FusedProdigy (lr 1.0, csrc/prodigy.hip) with the same clip, the script's other two --optimizer
choices; --optimizer sharded runs videopainter_amd.ShardedFusedAdamW(max_grad_norm=1.0), the
data-parallel step (csrc/zero.hip): alone it forms a one-rank group, under `torchrun --nproc_per_node N` one rank per
GPU (the group is initialised as bench.py does, the branch replicated from rank 0 with broadcast_module, every rank
draws its own latents, and verify_replicas runs after the last step: "replicas_identical" in the JSON line, which
rank 0 prints); --optimizer sharded-adam and --optimizer sharded-prodigy run videopainter_amd.ShardedFusedAdam and
videopainter_amd.ShardedFusedProdigy (lr 1.0) on the same two paths, with the same clip.  --loss replaces the synthetic loss gradient with inpainting_v_loss(...).backward()
(:1879-1892).  Default: neither.  Random-init weights, synthetic latents.  Prints one JSON line; optimizer_ms = HIP
events around optimizer.step().  --accumulate K runs K micro-batches per optimizer step (opt.accumulate() after the
first K - 1, opt.step() after the last: fp32 gradient accumulation, the script's --gradient_accumulation_steps); --steps and
--warmup then count optimizer steps, and the line adds ms_per_micro_batch and accumulate_ms (HIP events around
accumulate()) beside ms_per_step, optimizer_ms and the peak memory.

--fp8-gemm [SUBSET] (default when given: ffn,qkv,out) is the A/B of training through the frozen transformer on the
MX-FP8 GEMMs (forward and dgrad; the attention stays bf16): the bf16 arm and the fp8 arm run INTERLEAVED in this one
process, --rounds rounds (at least 5) of --steps steps per arm after --warmup steps of each, and the JSON line holds
per arm the step time (median, min, max over all timed steps), the per-class HIP-event split of one more step (gemm,
gemm_mx, attention, attention_bwd) and the peak memory of the arm's timed steps, plus whether the two arms' ranges
overlap.  Both arms' cached transposed dgrad weights (bf16 and MX) stay resident throughout, so the peaks compare
the arms' activations, not their weight caches.

--inputs (with --loss) starts the step from pixels, the script's lines 1774-1853 included: a synthetic 49-frame
480x720 fp32 video, its masked copy and a box mask go through videopainter_amd.prepare_training_inputs (the
first-frame noise, the three VAE encodes with enable_tiling + enable_slicing as train/VideoPainter.sh runs them, on a
5b VAE with synthetic weights, and the one fused launch), and the models and the loss run on what it returns.  The
JSON line adds, by HIP events per step, vae_encode_ms (the three encodes together), prepare_ms (vp_noise_frame +
vp_train_inputs_bf16) and step_ms_events (the whole step), and vae_encode_share.

--inputs-ab times that front without the encodes against its restatement from torch ops (torch_front below), both
on the same three encodes, alternating in one process, --rounds rounds (at least 5) of --steps calls per arm.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, D, L, LB = 226, 13, 3072, 42, 2
# --optimizer choice -> (class in videopainter_amd, its options besides betas, weight_decay and max_grad_norm)
SHARDED = {"sharded": ("ShardedFusedAdamW", dict(lr=1e-5)), "sharded-adam": ("ShardedFusedAdam", dict(lr=1e-5)),
           "sharded-prodigy": ("ShardedFusedProdigy", dict(lr=1.0))}


def flops(ntok: int, nv: int) -> dict:
    """Algorithmic FLOP of one training step at B=1: forward of both models, input-gradient (dgrad) backward of
    every block and of the injection path, weight-gradient backward of the branch.  Recompute (checkpointing) and
    the attention backward's score recompute are overhead, not counted."""
    gemm_f = 24 * ntok * D * D
    attn_f = 4 * ntok * ntok * D
    fwd = (L + LB) * (gemm_f + attn_f) + LB * 2 * ntok * D * D
    dgrad = (L + LB) * (gemm_f + 2 * attn_f) + LB * 2 * ntok * D * D
    wgrad = LB * (gemm_f + 2 * ntok * D * D)
    return dict(forward=float(fwd), backward=float(dgrad + wgrad), total=float(fwd + dgrad + wgrad))


def fp8_gemm_ab(args, tr, step, K) -> dict:
    """The interleaved A/B of --fp8-gemm: the arms differ in the blocks' MX weights alone (quantised once, then
    attached and detached per arm)."""
    import statistics
    which = set(filter(None, args.fp8_gemm.split(",")))
    if not which or which - {"ffn", "qkv", "out"}:
        raise SystemExit(f"--fp8-gemm takes a subset of ffn,qkv,out, got {args.fp8_gemm!r}")
    if args.optimizer in SHARDED:
        raise SystemExit("--fp8-gemm is a single-process A/B")
    rounds = max(5, args.rounds)
    tr.requires_grad_(False)
    tr.enable_fp8(ffn="ffn" in which, attention=False, qkv="qkv" in which, out="out" in which)
    blocks = list(tr.transformer_blocks)
    mx = [(b.ff_mx, b.qkv_mx, b.out_mx) for b in blocks]

    def arm(fp8: bool):
        for b, m in zip(blocks, mx):
            b.ff_mx, b.qkv_mx, b.out_mx = m if fp8 else (None, None, None)

    arms = (("bf16", False), ("fp8", True))
    for name, fp8 in arms:  # warm-up: also builds each arm's transposed dgrad weights
        arm(fp8)
        for _ in range(max(1, args.warmup)):
            step()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in arms}
    peak = {n: 0.0 for n, _ in arms}
    for r in range(rounds):
        for name, fp8 in arms:
            arm(fp8)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(args.steps):
                t0 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated() / 2 ** 30)
            print(f"round {r} {name}: {ms[name][-args.steps:]}", file=sys.stderr, flush=True)
    res = dict(metric="training step, bf16 against the frozen transformer on the MX-FP8 GEMMs (49f 480x720, B=1)",
               fp8_gemm=sorted(which), rounds=rounds, steps_per_round=args.steps, unit="ms/step", arms={})
    classes = ("gemm", "gemm_mx", "attention", "attention_bwd")
    for name, fp8 in arms:
        arm(fp8)
        a = dict(median=statistics.median(ms[name]), min=min(ms[name]), max=max(ms[name]), peak_mem_gib=peak[name])
        with K.timed_launches(*classes) as tl:
            step()
        torch.cuda.synchronize()
        a["classes_ms"] = {n: tl.mean_ms(n) * tl.count(n) for n in classes}
        a["counts"] = {n: tl.count(n) for n in classes}
        res["arms"][name] = a
    b, f = res["arms"]["bf16"], res["arms"]["fp8"]
    res["ranges_overlap"] = not (f["max"] < b["min"] or b["max"] < f["min"])
    res["fp8_minus_bf16_median_ms"] = f["median"] - b["median"]
    return res


PIX_F, PIX_H, PIX_W = 49, 480, 720  # the launch script's clip


def synthetic_pixels(dev, rank: int = 0):
    """A 49-frame 480x720 fp32 video in [-1, 1], its masked copy (the conditioning video) and the box mask
    [1, 49, 1, 480, 720] (frame 0 clear), made on the device."""
    g = torch.Generator(device=dev).manual_seed(11 + rank)
    px = torch.rand(1, PIX_F, 3, PIX_H, PIX_W, generator=g, device=dev) * 2 - 1
    mk = torch.zeros(1, PIX_F, 1, PIX_H, PIX_W, device=dev)
    mk[:, 1:, :, PIX_H // 4:PIX_H // 4 + PIX_H // 2, PIX_W // 4:PIX_W // 4 + PIX_W // 2] = 1.0
    return px, px * (1 - mk), mk


def training_vae(dev):
    """The 5b VAE with synthetic weights, tiled and sliced as train/VideoPainter.sh runs it."""
    from videopainter_amd.vae import AutoencoderKLCogVideoX
    vae = AutoencoderKLCogVideoX.from_config({}, device=dev)
    vae.init_synthetic_weights_(1236)
    vae.enable_tiling()
    vae.enable_slicing()
    return vae


def timed_encodes(vae, events):
    """Wrap vae.encode so that every call leaves a pair of HIP events in `events`."""
    encode = vae.encode

    def timed(x, *a, **kw):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        out = encode(x, *a, **kw)
        ev[1].record()
        events.append(ev)
        return out

    vae.encode = timed


def torch_front(sched, p_image_of, px, p_video, p_cond, mk, scaling_factor, L=16):
    """train/train_cogvideox_inpainting_i2v_video.py:1774-1853 from torch ops on the device, on the encoder's
    posterior parameters (channels-last [B, T, h, w, 2L]; the permuted views cost nothing).  p_image_of(noisy_images)
    returns the image posterior (the A/B hands both arms the same three encodes)."""
    import torch.nn.functional as Fn
    bf = torch.bfloat16

    def sample(p):
        mean = p[..., :L].permute(0, 4, 1, 2, 3)
        std = torch.exp(0.5 * torch.clamp(p[..., L:2 * L].permute(0, 4, 1, 2, 3), -30.0, 20.0))
        x = mean + std * torch.randn(mean.shape, device=p.device, dtype=bf)
        return (x.permute(0, 2, 1, 3, 4) * scaling_factor).to(memory_format=torch.contiguous_format, dtype=bf)

    images = px[:, :1].permute(0, 2, 1, 3, 4)
    sigma = torch.exp(torch.normal(mean=-3.0, std=0.5, size=(images.size(0),), device=px.device, dtype=bf))
    noisy_images = images + torch.randn_like(images) * sigma[:, None, None, None, None]
    image_latents = sample(p_image_of(noisy_images.to(bf)))
    model_input = sample(p_video)
    cond = sample(p_cond)
    padding = image_latents.new_zeros((cond.shape[0], cond.shape[1] - 1, *cond.shape[2:]))
    image_latents = torch.cat([image_latents, padding], dim=1)
    m = mk.permute(0, 2, 1, 3, 4)
    m = Fn.interpolate(m, size=(cond.shape[1], cond.shape[3], cond.shape[4])).permute(0, 2, 1, 3, 4).to(bf)
    cond = torch.concat([cond, m], -3).to(bf)
    noise = torch.randn_like(model_input).to(bf)
    ts = torch.randint(0, sched.config.num_train_timesteps, (model_input.shape[0],), device=px.device).long()
    noisy = sched.add_noise(model_input, noise, ts)
    return model_input, noisy, torch.cat([noisy, image_latents], dim=2), cond, m, ts


def inputs_ab(args) -> dict:
    """--inputs-ab: the torch-op front against vp_noise_frame + vp_train_inputs_bf16, on the same three encodes
    (made once), the arms alternating in this process: --rounds rounds (at least 5) of --steps calls per arm.  Per
    call: HIP events around the arm, and the host clock around the arm plus a synchronise."""
    import statistics
    from videopainter_amd import CogVideoXDPMScheduler, TrainingNoise
    from videopainter_amd import kernels as K
    from videopainter_amd import training as TR
    dev = "cuda"
    vae, sched = training_vae(dev), CogVideoXDPMScheduler()
    px, cpx, mk = synthetic_pixels(dev)
    noise = TrainingNoise(1)
    sf = float(vae.config.scaling_factor)
    with torch.no_grad():
        p_image = vae.encode(px[:, :1].permute(0, 2, 1, 3, 4).to(torch.bfloat16)).latent_dist._p.contiguous()
        p_video = vae.encode(px.permute(0, 2, 1, 3, 4)).latent_dist._p.contiguous()
        p_cond = vae.encode(cpx.permute(0, 2, 1, 3, 4)).latent_dist._p.contiguous()
    table = sched.add_noise_table(torch.bfloat16, dev)
    ids = (TR.NOISE_POSTERIOR_VIDEO, TR.NOISE_POSTERIOR_COND, TR.NOISE_POSTERIOR_IMAGE, TR.NOISE_DIFFUSION)

    def native():
        ts_h, sigma_h, _ = noise.host_draws(1, 1000)
        ts, sigma = TrainingNoise.upload(ts_h, sigma_h, dev)
        K.noise_frame(px[:, 0], sigma, None, seed=noise.seed, stream=noise.stream(TR.NOISE_IMAGE_PIXELS))
        out = K.train_inputs(p_video, p_cond, p_image, mk, ts, table, sf, seed=noise.seed,
                             streams=tuple(noise.stream(i) for i in ids))
        noise.next_step()
        return out

    def torch_ops():
        with torch.no_grad():
            return torch_front(sched, lambda noisy_images: p_image, px, p_video, p_cond, mk, sf)

    arms = (("torch", torch_ops), ("native", native))
    rounds = max(5, args.rounds)
    for _, fn in arms:
        for _ in range(max(2, args.warmup)):
            fn()
    torch.cuda.synchronize()
    dev_ms = {n: [] for n, _ in arms}
    wall_ms = {n: [] for n, _ in arms}
    for r in range(rounds):
        for name, fn in arms:
            for _ in range(args.steps):
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                wall_ms[name].append((time.perf_counter() - t0) * 1e3)
                dev_ms[name].append(ev[0].elapsed_time(ev[1]))
            print(f"round {r} {name}: events {[round(v, 3) for v in dev_ms[name][-args.steps:]]} ms, host "
                  f"{[round(v, 3) for v in wall_ms[name][-args.steps:]]} ms", file=sys.stderr, flush=True)
    res = dict(metric="front of the training step without the encodes (:1774-1853; 49f 480x720, B=1): torch ops "
                      "against vp_noise_frame + vp_train_inputs_bf16", rounds=rounds, steps_per_round=args.steps,
               unit="ms/call", arms={})
    for name, _ in arms:
        res["arms"][name] = {k: dict(median=statistics.median(v), min=min(v), max=max(v))
                             for k, v in (("events_ms", dev_ms[name]), ("host_ms", wall_ms[name]))}
    t, n = res["arms"]["torch"], res["arms"]["native"]
    for k in ("events_ms", "host_ms"):
        res[f"native_minus_torch_median_{k}"] = n[k]["median"] - t[k]["median"]
        res[f"ranges_overlap_{k}"] = not (n[k]["max"] < t[k]["min"] or t[k]["max"] < n[k]["min"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", action="store_true",
                    help="start the step from synthetic pixels: prepare_training_inputs (frame noise, three tiled and "
                         "sliced VAE encodes, the fused front) feeds the models and the loss")
    ap.add_argument("--inputs-ab", action="store_true",
                    help="interleaved A/B of the front without the encodes: torch ops against the HIP front")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=60)
    ap.add_argument("--width", type=int, default=90)
    ap.add_argument("--optimizer", choices=("none", "torch", "fused", "adam", "prodigy", *SHARDED), default="none")
    ap.add_argument("--loss", action="store_true",
                    help="inpainting_v_loss(...).backward() instead of out.backward(dout)")
    ap.add_argument("--classes", action="store_true", help="per-class HIP-event timing pass afterwards")
    ap.add_argument("--fp8-gemm", nargs="?", const="ffn,qkv,out", default=None, metavar="SUBSET",
                    help="interleaved A/B: bf16 against the frozen transformer on the MX-FP8 GEMMs (subset of "
                         "ffn,qkv,out; default all three)")
    ap.add_argument("--rounds", type=int, default=5, help="--fp8-gemm: interleaved rounds (at least 5)")
    ap.add_argument("--accumulate", type=int, default=1, metavar="K",
                    help="K micro-batches per optimizer step: opt.accumulate() after the first K - 1, opt.step() "
                         "after the last (--steps and --warmup count optimizer steps)")
    args = ap.parse_args()
    if args.inputs_ab:
        print(json.dumps(inputs_ab(args)))
        return
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd import kernels as K
    from videopainter_amd.config import COGVIDEOX_5B_I2V
    from videopainter_amd.embeddings import prepare_rotary_positional_embeddings

    dev = "cuda"
    rank, world = 0, 1
    if args.optimizer in SHARDED:
        import torch.distributed as dist
        from videopainter_amd import distributed as VD
        rank, world, local = VD.env_rank_world()
        if "MASTER_ADDR" not in os.environ:  # stand-alone: a one-rank group on this GPU
            import socket
            sock = socket.socket()
            sock.bind(("127.0.0.1", 0))
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(sock.getsockname()[1]), RANK="0",
                              WORLD_SIZE="1")
            sock.close()
        # VP_BENCH_DIST_BACKEND=gloo: a functional rehearsal with several ranks on the GPUs there are (as bench.py:
        # ranks share a device and the collectives go through host copies; the timing says nothing about scaling)
        backend = os.environ.get("VP_BENCH_DIST_BACKEND", "nccl")
        if backend != "nccl":
            local = local % max(1, torch.cuda.device_count())
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        VD.init(backend, dev)
    HL, WL = args.height, args.width
    cfg = dict(COGVIDEOX_5B_I2V, sample_height=HL, sample_width=WL)
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**cfg)
        br = CogvideoXBranchModel(**dict(cfg, num_layers=LB))
    tr.init_synthetic_weights_(1234)
    br.init_synthetic_weights_(1235)
    br.requires_grad_(True)
    params = [p for p in br.parameters() if p.requires_grad]
    opt = None
    if args.optimizer == "torch":
        opt = torch.optim.AdamW(params, lr=1e-5, betas=(0.9, 0.95), foreach=True)
    elif args.optimizer == "fused":
        from videopainter_amd import FusedAdamW
        opt = FusedAdamW(params, lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-4, max_grad_norm=1.0)
    elif args.optimizer == "adam":
        from videopainter_amd import FusedAdam
        opt = FusedAdam(params, lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-4, max_grad_norm=1.0)
    elif args.optimizer == "prodigy":
        from videopainter_amd import FusedProdigy
        opt = FusedProdigy(params, lr=1.0, betas=(0.9, 0.95), weight_decay=1e-4, max_grad_norm=1.0)
    elif args.optimizer in SHARDED:
        import videopainter_amd
        name, kw = SHARDED[args.optimizer]
        VD.broadcast_module(br, src=0, always=True)  # the replicas start from rank 0's bytes
        opt = getattr(videopainter_amd, name)(params, betas=(0.9, 0.95), weight_decay=1e-4, max_grad_norm=1.0, **kw)

    g = torch.Generator().manual_seed(7 + rank)  # (every rank its own data)
    lat = torch.randn(1, F, 16, HL, WL, generator=g).to(dev, torch.bfloat16)
    img = torch.zeros(1, F, 16, HL, WL)
    img[:, 0] = torch.randn(1, 16, HL, WL, generator=g)
    img = img.to(dev, torch.bfloat16)
    mask = torch.zeros(1, F, 1, HL, WL)
    mask[:, 1:, :, HL // 4:HL // 4 + HL // 2, WL // 4:WL // 4 + WL // 2] = 1.0
    mask = mask.to(dev, torch.bfloat16)
    cond = torch.cat([lat * (1 - mask), mask], 2)
    hidden = torch.cat([lat, img], 2)
    enc = torch.randn(1, T, 4096, generator=g).to(dev, torch.bfloat16)
    ts = torch.tensor([500], device=dev)
    rope = tuple(t.to(dev) for t in prepare_rotary_positional_embeddings(HL * 8, WL * 8, F, 64))
    dout = torch.randn(1, F, 16, HL, WL, generator=g).to(dev, torch.bfloat16)
    nv = F * (HL // 2) * (WL // 2)
    ntok = T + nv
    if args.loss:
        from videopainter_amd import CogVideoXDPMScheduler, inpainting_v_loss
        alphas_cumprod = CogVideoXDPMScheduler().alphas_cumprod.to(dev, torch.float32)
        target = torch.randn(1, F, 16, HL, WL, generator=g).to(dev, torch.bfloat16)
    enc_events, prep = [], None
    if args.inputs:
        if (HL, WL) != (PIX_H // 8, PIX_W // 8) or not args.loss or args.accumulate > 1 or args.fp8_gemm is not None:
            raise SystemExit("--inputs runs the default 480x720 clip with --loss (no --accumulate, no --fp8-gemm)")
        from videopainter_amd import TrainingNoise, prepare_training_inputs
        vae, sched = training_vae(dev), CogVideoXDPMScheduler()
        px, cpx, pmask = synthetic_pixels(dev, rank)
        tnoise = TrainingNoise(2024, rank=rank)
        timed_encodes(vae, enc_events)
        prep = K.timed_launches("noise_frame", "train_inputs")
    K_acc = args.accumulate
    if K_acc < 1 or (K_acc > 1 and args.optimizer in ("none", "torch")):
        raise SystemExit("--accumulate K needs K >= 1 and one of the fused / sharded optimizers")
    opt_events, acc_events = [], []

    def timed_call(fn, events):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        fn()
        ev[1].record()
        events.append(ev)

    def micro_batch(last: bool):
        samples = br(hidden_states=lat, encoder_hidden_states=enc, branch_cond=cond, timestep=ts,
                     image_rotary_emb=rope, return_dict=False)[0]
        out = tr(hidden_states=hidden, encoder_hidden_states=enc, timestep=ts, image_rotary_emb=rope,
                 branch_block_samples=samples, branch_block_masks=mask, return_dict=False)[0]
        if args.loss:  # (unscaled: step() takes the mean over the micro-batches)
            inpainting_v_loss(out, lat, target, ts, alphas_cumprod, mask, 1.0).backward()
        else:
            out.backward(dout)
        if last:
            timed_call(opt.step, opt_events)
        else:
            timed_call(opt.accumulate, acc_events)
        for p in params:
            p.grad = None

    def accumulated_step():
        for j in range(K_acc):
            micro_batch(j == K_acc - 1)

    def step():
        if args.inputs:  # pixels in: the step's front, then the models on what it made
            r = prepare_training_inputs(vae, sched, px, cpx, pmask, noise=tnoise)
            tnoise.next_step()
            samples = br(hidden_states=r.noisy_video_latents, encoder_hidden_states=enc,
                         branch_cond=r.conditioning_latents, timestep=r.timesteps, image_rotary_emb=rope,
                         return_dict=False)[0]
            out = tr(hidden_states=r.noisy_model_input, encoder_hidden_states=enc, timestep=r.timesteps,
                     image_rotary_emb=rope, branch_block_samples=samples, branch_block_masks=r.masks,
                     return_dict=False)[0]
            inpainting_v_loss(out, r.noisy_video_latents, r.model_input, r.timesteps, alphas_cumprod, r.masks,
                              1.0).backward()
            finish_step()
            return
        samples = br(hidden_states=lat, encoder_hidden_states=enc, branch_cond=cond, timestep=ts,
                     image_rotary_emb=rope, return_dict=False)[0]
        out = tr(hidden_states=hidden, encoder_hidden_states=enc, timestep=ts, image_rotary_emb=rope,
                 branch_block_samples=samples, branch_block_masks=mask, return_dict=False)[0]
        if args.loss:
            inpainting_v_loss(out, lat, target, ts, alphas_cumprod, mask, 1.0).backward()
        else:
            out.backward(dout)
        finish_step()

    def finish_step():
        if opt is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            opt.step()
            ev[1].record()
            opt_events.append(ev)
        for p in params:
            p.grad = None

    if args.fp8_gemm is not None:
        res = fp8_gemm_ab(args, tr, step, K)
        res.update(ntok=ntok, flop_per_step=flops(ntok, nv))
        print(json.dumps(res))
        return
    if K_acc > 1:
        step = accumulated_step
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    opt_events.clear()
    acc_events.clear()
    enc_events.clear()
    step_events = []
    if prep is not None:
        prep.__enter__()
    t0 = time.perf_counter()
    for i in range(args.steps):
        timed_call(step, step_events)
        torch.cuda.synchronize()
        print(f"step {i}: {time.perf_counter() - t0:.2f}s", file=sys.stderr, flush=True)
    el = (time.perf_counter() - t0) / args.steps
    if prep is not None:
        prep.__exit__(None, None, None)
    replicas = None
    if args.optimizer in SHARDED:
        el = VD.max_over_ranks(el, dev)
        ok, n_buckets = VD.verify_replicas(br, always=True)
        replicas = dict(identical=ok, buckets=n_buckets, world=world)
    fl = flops(ntok, nv)
    res = dict(metric="training steps/sec (VideoPainter branch, 5b-I2V frozen, 49f 480x720, B=1)",
               value=1.0 / el, unit="steps/s", ms_per_step=el * 1e3, steps=args.steps, warmup=args.warmup,
               optimizer={"none": None, "torch": "torch AdamW foreach",
                          "fused": "FusedAdamW(max_grad_norm=1.0)", "adam": "FusedAdam(max_grad_norm=1.0)",
                          "prodigy": "FusedProdigy(lr=1.0, max_grad_norm=1.0)",
                          "sharded": "ShardedFusedAdamW(max_grad_norm=1.0)",
                          "sharded-adam": "ShardedFusedAdam(max_grad_norm=1.0)",
                          "sharded-prodigy": "ShardedFusedProdigy(lr=1.0, max_grad_norm=1.0)"}[args.optimizer],
               optimizer_ms=(sum(a.elapsed_time(b) for a, b in opt_events) / len(opt_events)) if opt_events else None,
               loss="inpainting_v_loss" if args.loss else None,
               tflops_per_s=fl["total"] / el / 1e12, flop_per_step=fl, ntok=ntok,
               peak_mem_gib=torch.cuda.max_memory_allocated() / 2 ** 30)
    if args.inputs:  # HIP events: the three encodes of a step together, the frame noise + the fused launch, the step
        ev_ms = lambda evs: sum(a.elapsed_time(b) for a, b in evs) / args.steps  # noqa: E731
        res.update(inputs="prepare_training_inputs (49f 480x720 fp32 pixels, tiled + sliced VAE)",
                   vae_encode_ms=ev_ms(enc_events),
                   prepare_ms=ev_ms(prep.events["noise_frame"]) + ev_ms(prep.events["train_inputs"]),
                   step_ms_events=ev_ms(step_events))
        res["vae_encode_share"] = res["vae_encode_ms"] / res["step_ms_events"]
    if K_acc > 1:
        res.update(accumulate=K_acc, ms_per_micro_batch=el * 1e3 / K_acc,
                   accumulate_ms=sum(a.elapsed_time(b) for a, b in acc_events) / len(acc_events))
        print(f"--accumulate {K_acc}: {el * 1e3 / K_acc:.1f} ms per micro-batch, {el * 1e3:.1f} ms per optimizer step; "
              f"accumulate() {res['accumulate_ms']:.3f} ms, step() {res['optimizer_ms']:.3f} ms; peak "
              f"{res['peak_mem_gib']:.2f} GiB", file=sys.stderr)
    if replicas is not None:
        res["world"] = world
        res["replicas_identical"] = replicas["identical"]
        res["replica_buckets"] = replicas["buckets"]
    if args.classes:
        with K.timed_launches("gemm", "attention", "attention_bwd") as tl:
            step()
        torch.cuda.synchronize()
        res["classes_ms"] = {n: tl.mean_ms(n) * tl.count(n) for n in ("gemm", "attention", "attention_bwd")}
        res["counts"] = {n: tl.count(n) for n in ("gemm", "attention", "attention_bwd")}
    if rank == 0:
        print(json.dumps(res))
    if args.optimizer in SHARDED:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
