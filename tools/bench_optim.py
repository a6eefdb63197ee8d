"""Optimizer-step time at the real branch parameter set on one MI355X: FusedAdamW against the torch equivalents.

    python tools/bench_optim.py [--rounds R] [--iters N] [--sharded] [--prodigy] [--sharded-prodigy]

Parameters: the trainable VideoPainter branch (5b-I2V config, num_layers=2, init_synthetic_weights_), bf16, with
random bf16 gradients N(0, 1e-3^2); the training script's hyper-parameters (lr 1e-5, betas (0.9, 0.95), weight decay
1e-4, max_grad_norm 1.0).  Three variants, interleaved round by round in one process:

    fused      videopainter_amd.FusedAdamW(max_grad_norm=1.0).step(): norm + clip + AdamW on fp32 masters + bf16
               write-back, on the HIP kernels (csrc/optim.hip)
    torch_fp32 the honest torch equivalent: fp32 copies of the parameters; per step the bf16 gradients cast to the
               fp32 copies' .grad, torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True) on them, and the
               bf16 copy-back
    torch_bf16 torch.optim.AdamW(foreach=True) directly on the bf16 parameters (no master weights: the
               wrong-but-cheap baseline)

--sharded adds a fourth variant, interleaved with the others: videopainter_amd.ShardedFusedAdamW(max_grad_norm=1.0) at
world size 1 over RCCL (the process initialises a one-rank "nccl" group itself: the reduce-scatter and both all-gathers
run in RCCL on the device buffers, as copies), and afterwards times its kernels one by one, each with its achieved
bytes/s from its own byte count — pack 2 B read + 4 B written per parameter, shard AdamW 16 + 14 B, unpack 2 + 2 B —
next to vp_mt_adamw_bf16's in the same run (the yardstick), and the three collectives.  No figure for world > 1 can be
produced on one GPU.

--prodigy adds videopainter_amd.FusedProdigy(lr=1.0, max_grad_norm=1.0) as a variant interleaved with the others, and
afterwards times its two passes one by one, round by round beside vp_mt_adamw_bf16's update pass (the yardstick of
the same round): pass 1 (vp_mt_prodigy_moments_bf16) 22 B read + 12 B written per parameter, pass 2
(vp_mt_prodigy_update_bf16) 12 + 6 B; with the norm pass's 2 B the step moves 54 B per parameter against AdamW's 30.

--sharded-prodigy adds videopainter_amd.ShardedFusedProdigy(lr=1.0, max_grad_norm=1.0) at world size 1 over RCCL as a
variant (give --prodigy too to have FusedProdigy beside it in the same rounds), and afterwards times the pieces of its
step one by one: pass 1 (vp_zero_shard_prodigy_moments) 24 B read + 12 B written per parameter, pass 2
(vp_zero_shard_prodigy_update) 12 + 6 B, the gated unpack 2 + 2 B, the record kernel, the d update over the records and
the 16-byte all-gather.

--accumulate times the gradient-accumulation kernels at the same tensors, round by round beside vp_mt_adamw_bf16's
update pass (the yardstick of the same round): the first fold (vp_mt_accumulate_bf16, 2 B read + 4 B written per
parameter), a later fold (6 + 4 B; 6 + 6 B with zero_grads), the fp32-gradient norm (vp_mt_grad_sqnorm_f32, 4 B) and
the fp32-gradient AdamW update (vp_mt_adamw_f32, 16 + 14 B).

Prints ms per step per round (HIP events around N back-to-back steps), and for `fused` the effective bandwidth
30 B x n_params / t (norm pass: 2 B read; update pass: 14 B read + 14 B written per parameter) as a fraction of
6.3 TB/s, with the per-kernel split (norm pass / update pass).  One JSON line at the end.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
HYP = dict(lr=1e-5, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sharded", action="store_true", help="add ShardedFusedAdamW at world 1 over RCCL")
    ap.add_argument("--prodigy", action="store_true", help="add FusedProdigy and time its two passes")
    ap.add_argument("--sharded-prodigy", action="store_true",
                    help="add ShardedFusedProdigy at world 1 over RCCL and time the pieces of its step")
    ap.add_argument("--accumulate", action="store_true",
                    help="time the gradient-accumulation kernels beside vp_mt_adamw_bf16's update pass")
    args = ap.parse_args()
    from videopainter_amd import CogvideoXBranchModel, FusedAdamW, device_scope
    from videopainter_amd import kernels as K
    from videopainter_amd.config import COGVIDEOX_5B_I2V

    dev = "cuda"
    with device_scope(dev):
        br = CogvideoXBranchModel(**dict(COGVIDEOX_5B_I2V, num_layers=2))
    br.init_synthetic_weights_(1235)
    br.requires_grad_(True)
    base = [p for p in br.parameters() if p.requires_grad]
    n_params = sum(p.numel() for p in base)
    for i, p in enumerate(base):
        p.grad = torch.empty_like(p)
        K.fill_normal_(p.grad, 77 + i, 0.0, 1e-3)
    clone = lambda: [torch.nn.Parameter(p.detach().clone()) for p in base]  # noqa: E731

    def with_grads(ps):
        for p, b in zip(ps, base):
            p.grad = b.grad  # shared, read-only for every variant
        return ps

    pf = with_grads(clone())
    fused = FusedAdamW(pf, **HYP, max_grad_norm=1.0)

    pb = clone()  # the bf16 model of the fp32 variant
    p32 = [torch.nn.Parameter(p.detach().float()) for p in pb]
    opt32 = torch.optim.AdamW(p32, **HYP, foreach=True)

    def torch_fp32():
        for m, b in zip(p32, base):
            m.grad = b.grad.float()
        torch.nn.utils.clip_grad_norm_(p32, 1.0, foreach=True)
        opt32.step()
        with torch.no_grad():
            torch._foreach_copy_(pb, p32)

    p16 = with_grads(clone())
    opt16 = torch.optim.AdamW(p16, **HYP, foreach=True)

    variants = dict(fused=fused.step, torch_fp32=torch_fp32, torch_bf16=opt16.step)
    sharded = prodigy = sprodigy = None
    if args.prodigy:
        from videopainter_amd import FusedProdigy
        prodigy = FusedProdigy(with_grads(clone()), **dict(HYP, lr=1.0), max_grad_norm=1.0)
        variants["prodigy"] = prodigy.step
    if args.sharded or args.sharded_prodigy:
        import socket
        from videopainter_amd import distributed as VD
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", str(port)), ("RANK", "0"), ("WORLD_SIZE", "1")):
            os.environ.setdefault(k, v)
        torch.cuda.set_device(0)
        VD.init("nccl", torch.device("cuda", 0))
    if args.sharded:
        from videopainter_amd import ShardedFusedAdamW
        sharded = ShardedFusedAdamW(with_grads(clone()), **HYP, max_grad_norm=1.0)
        variants["sharded"] = sharded.step
    if args.sharded_prodigy:
        from videopainter_amd import ShardedFusedProdigy
        sprodigy = ShardedFusedProdigy(with_grads(clone()), **dict(HYP, lr=1.0), max_grad_norm=1.0)
        variants["sharded_prodigy"] = sprodigy.step
    for fn in variants.values():  # warm-up (allocations, table upload)
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for r in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, args.iters))
        print("round %d: " % r + "  ".join(f"{k} {ms[k][-1]:.3f} ms" for k in variants), flush=True)

    # the fused step's kernels one by one
    t = fused._tables
    norm_ms = timed(lambda: K.mt_grad_sqnorm(t.tensors, t.chunks, t.n_chunks, t.partials, t.flags), args.iters)
    upd_ms = timed(lambda: K.mt_adamw(t.tensors, t.chunks, 0, t.n_chunks, fused._master, fused._exp_avg,
                                      fused._exp_avg_sq, fused._scalars, lr=HYP["lr"], betas=HYP["betas"],
                                      eps=HYP["eps"], weight_decay=HYP["weight_decay"], use_clip=True,
                                      zero_grads=False), args.iters)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    bw = 30.0 * n_params / (med["fused"] * 1e-3)
    res = dict(metric="optimizer step, VideoPainter branch (5b-I2V, 2 layers), bf16 params + fp32 masters",
               n_params=n_params, n_tensors=len(base), n_chunks=t.n_chunks, rounds=args.rounds, iters=args.iters,
               ms=ms, median_ms=med, min_ms={k: min(v) for k, v in ms.items()},
               max_ms={k: max(v) for k, v in ms.items()},
               fused_gb_per_s=bw / 1e9, fused_fraction_of_6p3_tb_s=bw / HBM,
               norm_pass_ms=norm_ms, norm_pass_gb_per_s=2.0 * n_params / (norm_ms * 1e-3) / 1e9,
               update_pass_ms=upd_ms, update_pass_gb_per_s=28.0 * n_params / (upd_ms * 1e-3) / 1e9,
               speedup_vs_torch_fp32=med["torch_fp32"] / med["fused"])
    if prodigy is not None:
        z, zt = prodigy, prodigy._tables
        b3 = HYP["betas"][1] ** 0.5
        d_steps = float(prodigy.d)  # (the passes below run out of their step's order: d means nothing afterwards)
        passes = dict(
            adamw_update=(28.0, lambda: K.mt_adamw(t.tensors, t.chunks, 0, t.n_chunks, fused._master, fused._exp_avg,
                                                   fused._exp_avg_sq, fused._scalars, lr=HYP["lr"],
                                                   betas=HYP["betas"], eps=HYP["eps"],
                                                   weight_decay=HYP["weight_decay"], use_clip=True,
                                                   zero_grads=False)),
            moments=(34.0, lambda: K.mt_prodigy_moments(zt.tensors, zt.chunks, 0, zt.n_chunks, z._master, z._p0,
                                                        z._exp_avg, z._exp_avg_sq, z._s, z._pairs, z._scalars,
                                                        z._d_block, betas=HYP["betas"], beta3=b3, weight_decay=0.0,
                                                        d0=z.d0, safeguard_warmup=False, use_clip=True)),
            update=(18.0, lambda: K.mt_prodigy_update(zt.tensors, zt.chunks, 0, zt.n_chunks, z._master, z._exp_avg,
                                                      z._exp_avg_sq, z._scalars, z._d_block, eps=HYP["eps"],
                                                      weight_decay=HYP["weight_decay"], zero_grads=False)),
            finalize=(0.0, lambda: K.prodigy_finalize(1, z._pairs, zt.n_chunks, z._scalars, z._d_block, lr=1.0,
                                                      betas=HYP["betas"], beta3=b3, d0=z.d0, d_coef=z.d_coef,
                                                      growth_rate=z.growth_rate, use_bias_correction=False)))
        pms = {k: [] for k in passes}
        for r in range(args.rounds):
            for k, (_, fn) in passes.items():
                pms[k].append(timed(fn, args.iters))
            print("pass round %d: " % r + "  ".join(f"{k} {pms[k][-1]:.3f} ms" for k in passes), flush=True)
        pmed = {k: sorted(v)[len(v) // 2] for k, v in pms.items()}
        yard = 28.0 * n_params / (pmed["adamw_update"] * 1e-3) / 1e9
        res["prodigy_passes"] = dict(ms=pms, median_ms=pmed, yardstick_mt_adamw_gb_per_s=yard)
        for name in ("moments", "update"):
            gbs = passes[name][0] * n_params / (pmed[name] * 1e-3) / 1e9
            res["prodigy_passes"][name] = dict(bytes_per_param=passes[name][0], gb_per_s=gbs,
                                               fraction_of_6p3_tb_s=gbs * 1e9 / HBM, vs_mt_adamw=gbs / yard)
            print(f"prodigy {name}: {pmed[name]:.3f} ms = {gbs:.0f} GB/s = {gbs * 1e9 / HBM:.2f} of 6.3 TB/s "
                  f"({gbs / yard:.2f} of vp_mt_adamw_bf16's {yard:.0f} GB/s in the same rounds)")
        print(f"prodigy step: {med['prodigy']:.3f} ms against fused {med['fused']:.3f} ms (54 B against 30 B of "
              f"traffic per parameter; d = {d_steps:.3e} after the steps); finaliser {pmed['finalize'] * 1e3:.1f} us")
    if args.accumulate:
        # the folds and the fp32-gradient passes at the same tensors, interleaved round by round with the yardstick;
        # gradients of its own (the zero_grads fold writes them)
        pa = clone()
        for p, q in zip(pa, base):
            p.grad = q.grad.clone()
        z = FusedAdamW(pa, **HYP, max_grad_norm=1.0)
        z.accumulate()
        z.step()  # (tables, accumulator, a valid scalars block)
        zt, acc = z._tables, z.grad_accumulator
        hyper = dict(lr=HYP["lr"], betas=HYP["betas"], eps=HYP["eps"], weight_decay=HYP["weight_decay"],
                     use_clip=True)
        fold = lambda **kw: K.mt_accumulate(zt.tensors, zt.chunks, zt.n_chunks, acc, **kw)  # noqa: E731
        pieces = dict(
            adamw_update=(28.0, lambda: K.mt_adamw(t.tensors, t.chunks, 0, t.n_chunks, fused._master, fused._exp_avg,
                                                   fused._exp_avg_sq, fused._scalars, **hyper, zero_grads=False)),
            first_fold=(6.0, lambda: fold(first=True)),
            later_fold=(10.0, lambda: fold(first=False)),
            later_fold_zero_grads=(12.0, lambda: fold(first=False, zero_grads=True)),
            norm_f32=(4.0, lambda: K.mt_grad_sqnorm_f32(zt.tensors, zt.chunks, zt.n_chunks, acc, zt.partials,
                                                        zt.flags)),
            adamw_f32=(30.0, lambda: K.mt_adamw_f32(zt.tensors, zt.chunks, 0, zt.n_chunks, acc, z._master, z._exp_avg,
                                                    z._exp_avg_sq, z._scalars, **hyper)))
        ams = {k: [] for k in pieces}
        for r in range(args.rounds):
            for k, (_, fn) in pieces.items():
                ams[k].append(timed(fn, args.iters))
            print("accumulate round %d: " % r + "  ".join(f"{k} {ams[k][-1]:.3f} ms" for k in pieces), flush=True)
        amed = {k: sorted(v)[len(v) // 2] for k, v in ams.items()}
        yard = 28.0 * n_params / (amed["adamw_update"] * 1e-3) / 1e9
        res["accumulate"] = dict(ms=ams, median_ms=amed, yardstick_mt_adamw_gb_per_s=yard)
        for name, (nbytes, _) in list(pieces.items())[1:]:
            gbs = nbytes * n_params / (amed[name] * 1e-3) / 1e9
            res["accumulate"][name] = dict(bytes_per_param=nbytes, gb_per_s=gbs, fraction_of_6p3_tb_s=gbs * 1e9 / HBM,
                                           vs_mt_adamw=gbs / yard)
            print(f"accumulate {name}: {amed[name]:.3f} ms = {gbs:.0f} GB/s = {gbs * 1e9 / HBM:.2f} of 6.3 TB/s "
                  f"({gbs / yard:.2f} of vp_mt_adamw_bf16's {yard:.0f} GB/s in the same rounds)")
    if sharded is not None:
        z, zt, c = sharded, sharded._tables, sharded._comm
        mine = z._flat16[z._lo:z._hi]
        ksteps = dict(
            pack=(6.0, lambda: K.zero_pack(zt.tensors, zt.chunks, zt.n_chunks, z._flat32, inv_world=1.0,
                                           zero_grads=False)),
            shard_norm=(4.0, lambda: K.zero_shard_sqnorm(zt.ranges, zt.n_ranges, z._grad_shard, zt.partials, zt.flags,
                                                         z._record)),
            shard_adamw=(30.0, lambda: K.zero_shard_adamw(zt.ranges, 0, zt.n_ranges, z._grad_shard, z._master,
                                                          z._exp_avg, z._exp_avg_sq, mine, z._scalars, lr=HYP["lr"],
                                                          betas=HYP["betas"], eps=HYP["eps"],
                                                          weight_decay=HYP["weight_decay"], use_clip=True)),
            unpack=(4.0, lambda: K.zero_unpack(zt.tensors, zt.chunks, zt.n_chunks, z._flat16, z._scalars)),
            reduce_scatter_f32=(8.0, lambda: c.reduce_scatter_sum(0, z._grad_shard, z._flat32)),
            all_gather_bf16=(4.0, lambda: c.all_gather(0, z._flat16, mine)))
        res["sharded_kernels"] = {}
        yard = res["update_pass_gb_per_s"]
        for name, (nbytes, fn) in ksteps.items():
            t_ms = timed(fn, args.iters)
            gbs = nbytes * n_params / (t_ms * 1e-3) / 1e9
            res["sharded_kernels"][name] = dict(ms=t_ms, bytes_per_param=nbytes, gb_per_s=gbs,
                                                fraction_of_6p3_tb_s=gbs * 1e9 / HBM, vs_mt_adamw=gbs / yard)
            print(f"sharded {name}: {t_ms:.3f} ms = {gbs:.0f} GB/s = {gbs * 1e9 / HBM:.2f} of 6.3 TB/s "
                  f"({gbs / yard:.2f} of vp_mt_adamw_bf16's {yard:.0f} GB/s in this run)")
        res["sharded_n_ranges"] = zt.n_ranges
        res["sharded_note"] = "world 1 over RCCL on one GPU: the collectives are device copies; world > 1 unmeasured"
        print(f"sharded step: {med['sharded']:.3f} ms against fused {med['fused']:.3f} ms "
              f"(about 50 B against 30 B of traffic per parameter)")
    if sprodigy is not None:
        z, zt, c = sprodigy, sprodigy._tables, sprodigy._comm
        b3 = HYP["betas"][1] ** 0.5
        fin = dict(lr=1.0, betas=HYP["betas"], beta3=b3, d0=z.d0, d_coef=z.d_coef, growth_rate=z.growth_rate,
                   use_bias_correction=False)
        d_steps = float(z.d)  # (the pieces below run out of their step's order: d means nothing afterwards)
        pieces = dict(
            pack=(6.0, lambda: K.zero_pack(zt.tensors, zt.chunks, zt.n_chunks, z._flat32, inv_world=1.0,
                                           zero_grads=False)),
            reduce_scatter_f32=(8.0, lambda: c.reduce_scatter_sum(0, z._grad_shard, z._flat32)),
            shard_norm=(4.0, lambda: K.zero_shard_sqnorm(zt.ranges, zt.n_ranges, z._grad_shard, zt.partials, zt.flags,
                                                         z._record)),
            all_gather_norm_record=(0.0, lambda: c.all_gather(0, z._records, z._record)),
            moments=(36.0, lambda: K.zero_shard_prodigy_moments(zt.ranges, 0, zt.n_ranges, z._grad_shard, z._master,
                                                                z._p0, z._exp_avg, z._exp_avg_sq, z._s, z._pairs,
                                                                z._scalars, z._d_block, betas=HYP["betas"], beta3=b3,
                                                                weight_decay=0.0, d0=z.d0, safeguard_warmup=False,
                                                                use_clip=True)),
            record=(0.0, lambda: K.zero_prodigy_record(z._pairs, zt.n_ranges, z._scalars, z._d_record)),
            all_gather_d_record=(0.0, lambda: c.all_gather(0, z._d_records, z._d_record)),
            d_update=(0.0, lambda: K.zero_prodigy_finalize(1, z._d_records, 1, z._scalars, z._d_block, **fin)),
            update=(18.0, lambda: K.zero_shard_prodigy_update(zt.ranges, 0, zt.n_ranges, z._master, z._exp_avg,
                                                              z._exp_avg_sq, z._mine16, z._scalars, z._d_block,
                                                              eps=HYP["eps"], weight_decay=HYP["weight_decay"])),
            all_gather_bf16=(4.0, lambda: c.all_gather(0, z._flat16, z._mine16)),
            unpack_gated=(4.0, lambda: K.zero_unpack_gated(zt.tensors, zt.chunks, zt.n_chunks, z._flat16, z._scalars,
                                                           z._d_block)))
        res["sharded_prodigy_pieces"] = {}
        yard, total = res["update_pass_gb_per_s"], 0.0
        for name, (nbytes, fn) in pieces.items():
            t_ms = sorted(timed(fn, args.iters) for _ in range(args.rounds))[args.rounds // 2]
            total += t_ms
            gbs = nbytes * n_params / (t_ms * 1e-3) / 1e9
            res["sharded_prodigy_pieces"][name] = dict(ms=t_ms, bytes_per_param=nbytes, gb_per_s=gbs,
                                                       vs_mt_adamw=gbs / yard)
            rate = f" = {gbs:.0f} GB/s ({gbs / yard:.2f} of vp_mt_adamw_bf16's {yard:.0f} GB/s)" if nbytes else ""
            print(f"sharded prodigy {name}: {t_ms * 1e3:.1f} us{rate}")
        other = f" against prodigy {med['prodigy']:.3f} ms" if prodigy is not None else ""
        print(f"sharded prodigy step: {med['sharded_prodigy']:.3f} ms{other} (the pieces above add up to {total:.3f} "
              f"ms; d = {d_steps:.3e} after the steps)")
    if sharded is not None or sprodigy is not None:
        import torch.distributed as dist
        dist.destroy_process_group()
    print(f"fused: {med['fused']:.3f} ms = {bw / 1e9:.0f} GB/s = {bw / HBM:.2f} of 6.3 TB/s "
          f"(norm pass {norm_ms:.3f} ms, update pass {upd_ms:.3f} ms); torch fp32 equivalent "
          f"{med['torch_fp32']:.3f} ms, torch on bf16 {med['torch_bf16']:.3f} ms")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
