"""A/B of the two kernels of the head-parallel split's fp8 exchange against the launches they replace, on one GPU at
BASELINE config 5's shard shapes (N = 47 026 joint rows, B = 2, D = 3072, H = 48; P = 2 and P = 8, n = ceil(N / P)),
arms interleaved in one process, device events, every shape warmed up first.

  pack     kernels.qkv_heads_pack_fp8 (one launch: the shard's pre-norm qkv read once, q / k written as e4m3, v as
           bf16, in the exchange layout: 6 B read + 4 B written per element) against what the existing launches need
           for the same operands: today's bf16 send re-layout (permute + contiguous), the receive re-layout, and the
           two head_norm_rope_fp8 launches on the head group.
  gather   kernels.mx_quantize_heads (the second exchange's receive buffer -> the fp8 output projection's operand:
           2 B read + 1 B written per element) against the receive re-layout + mx_quantize.
  stream   mx_quantize on the contiguous [B n, D] tensor: the HBM bar (2 B + 1 B per element).

No time is fixed in advance: the yardstick is the composition, measured in the same run; by bytes the new kernels
should win in every round (`new_wins_every_round`).

    python tools/bench_ulysses_fp8.py [--rounds 5] [--iters 5] [--P 2,8]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videopainter_amd import kernels as K  # noqa: E402
from tools.bench_kernels import timeit  # noqa: E402

BF16 = torch.bfloat16
N, T, B, D, H = 47026, 226, 2, 3072, 48
dev = "cuda"


def shapes(P, rounds, iters):
    n = -(-N // P)
    Dp, hp = D // P, H // P
    g = torch.Generator().manual_seed(P)
    ln = [types.SimpleNamespace(weight=(1 + 0.1 * torch.randn(64, generator=g)).to(dev, BF16),
                                bias=(0.1 * torch.randn(64, generator=g)).to(dev, BF16), eps=1e-6) for _ in range(2)]
    nq, nk = ln
    q_mul, k_mul = 0.125 * K.LOG2E * 2.0 ** 3, 2.0 ** 3
    ang = 6.283 * torch.rand(N - T, 64, generator=g)
    rope_full = (ang.cos().to(dev).contiguous(), ang.sin().to(dev).contiguous())
    # rank 0's shard: the text rows and the first n - T video rows
    rope = tuple(t[:n - T].contiguous() for t in rope_full)
    qkv = torch.randn(B, n, 3 * D, device=dev).to(BF16)
    send8 = torch.empty(P, n, B, 4 * Dp, device=dev, dtype=torch.uint8)
    # the bf16 exchange's buffers ([P, B, n, 3, Dp] on both sides; the wire itself is not timed: it is a copy here)
    wire = qkv.reshape(B, n, 3, P, Dp).permute(3, 0, 1, 2, 4).contiguous()
    full = wire.permute(1, 0, 2, 3, 4).reshape(B, P * n, 3 * Dp)
    q8 = torch.empty(B, P * n, Dp, device=dev, dtype=torch.uint8)
    k8 = torch.empty(B, N, Dp, device=dev, dtype=torch.uint8)

    def pack_old():
        w = qkv.reshape(B, n, 3, P, Dp).permute(3, 0, 1, 2, 4).contiguous()
        f = w.permute(1, 0, 2, 3, 4).reshape(B, P * n, 3 * Dp)
        K.head_norm_rope_fp8(f[:, :N, :Dp], hp, T, nq.weight, nq.bias, nq.eps, rope_full, q_mul, out=q8[:, :N])
        K.head_norm_rope_fp8(f[:, :N, Dp:2 * Dp], hp, T, nk.weight, nk.bias, nk.eps, rope_full, k_mul, out=k8)

    def pack_old_norms():  # (the two norm launches alone, beside the composition)
        K.head_norm_rope_fp8(full[:, :N, :Dp], hp, T, nq.weight, nq.bias, nq.eps, rope_full, q_mul, out=q8[:, :N])
        K.head_norm_rope_fp8(full[:, :N, Dp:2 * Dp], hp, T, nk.weight, nk.bias, nk.eps, rope_full, k_mul, out=k8)

    o_recv_old = torch.randn(P, B, n, Dp, device=dev).to(BF16)     # today's second receive buffer
    o_recv_new = o_recv_old.permute(0, 2, 1, 3).contiguous()        # the fp8 path's: [P, n, B, Dp]
    mx = K.MXTensor(B * n, D, dev, zero=False)
    flat = o_recv_old.permute(1, 2, 0, 3).reshape(B * n, D)

    def gather_old():
        K.mx_quantize(o_recv_old.permute(1, 2, 0, 3).reshape(B * n, D), out=mx)

    arms = {
        "pack.new": lambda: K.qkv_heads_pack_fp8(qkv, H, P, T, nq, nk, rope, q_mul, k_mul, out=send8),
        "pack.old": pack_old,
        "pack.old_norms_only": pack_old_norms,
        "gather.new": lambda: K.mx_quantize_heads(o_recv_new, out=mx),
        "gather.old": gather_old,
        "stream.mx_quantize": lambda: K.mx_quantize(flat, out=mx),
    }
    elems = B * n * D
    bytes_moved = {"pack.new": 10 * elems, "gather.new": 3 * elems, "stream.mx_quantize": 3 * elems}
    res = {a: [] for a in arms}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for a, fn in arms.items():
            res[a].append(timeit(fn, iters) * 1e6)
    out = {"P": P, "n": n, "Dp": Dp, "elements": elems, "arms": {}}
    for a, us in res.items():
        out["arms"][a] = {"median_us": round(statistics.median(us), 1), "rounds_us": [round(x, 1) for x in us]}
        if a in bytes_moved:
            out["arms"][a]["median_GBps"] = round(bytes_moved[a] / statistics.median(us) / 1e3, 1)
    for w in ("pack", "gather"):
        new, old = res[w + ".new"], res[w + ".old"]
        out[w + ".new_over_old_median"] = round(statistics.median(new) / statistics.median(old), 4)
        out[w + ".new_wins_every_round"] = all(x < y for x, y in zip(new, old))
    print("shapes " + json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--P", default="2,8")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("an A/B here takes at least 5 interleaved rounds")
    ok = True
    with torch.no_grad():
        for P in (int(p) for p in a.P.split(",")):
            r = shapes(P, a.rounds, a.iters)
            ok = ok and r["pack.new_wins_every_round"] and r["gather.new_wins_every_round"]
    print("verdict " + json.dumps({"new_wins_every_round": ok}), flush=True)


if __name__ == "__main__":
    main()
