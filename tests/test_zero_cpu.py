"""Sharded optimizer (videopainter_amd/zero.py, csrc/zero.hip, distributed.py) — the parts that need no GPU: the shard
layout and the range table, host-side argument validation of the C entry points, and the collective helpers on gloo
(spawned processes, worlds 2 and 3, host tensors).

Parameter sets: those of tests/test_optim_gpu.py — shapes [1], [7], [3072], [CHUNK+1], [64, 3072], [3, 5, 7] plus one
5-element parameter that never has a gradient (at index 2), and a small set of [1], [7] alone, with which two of four
ranks own nothing but padding."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from videopainter_amd import _native as N
from videopainter_amd.optim import CHUNK
from videopainter_amd.zero import RANGE_DTYPE, build_range_table, flat_offsets, shard_size

VP_ERR_ARG = 1000
WORLDS = (1, 2, 3, 4, 7)


def numels_of(kind, idle):
    shapes = [(1,), (7,)] if kind == "small" else [(1,), (7,), (3072,), (CHUNK + 1,), (64, 3072), (3, 5, 7)]
    n = [int(np.prod(s)) for s in shapes]
    active = [True] * len(n)
    if idle:
        n, active = n[:2] + [5] + n[2:], active[:2] + [False] + active[2:]
    return n, active


@pytest.mark.parametrize("two_groups", [False, True], ids=["one_group", "two_groups"])
@pytest.mark.parametrize("idle", [False, True], ids=["all_active", "idle_param"])
@pytest.mark.parametrize("kind", ["main", "small"])
@pytest.mark.parametrize("world", WORLDS)
def test_layout_and_range_table(world, kind, idle, two_groups):
    numels, active = numels_of(kind, idle)
    offs, total = flat_offsets(numels)
    assert all(o % 8 == 0 for o in offs) and total % 8 == 0
    assert all(offs[i] + numels[i] <= offs[i + 1] for i in range(len(offs) - 1))  # FusedAdamW's offsets
    per = shard_size(total, world)
    assert per % 8 == 0 and per * world >= total and (per - 8) * world < total
    split = 1 if kind == "small" else 4  # the first `split` tensors are group 0, the rest group 1
    group_of = [0 if (not two_groups or i < split) else 1 for i in range(len(numels))]
    seen = np.zeros(world * per, dtype=np.int64)
    kindmap = np.full(world * per, -1, dtype=np.int64)  # tensor index of every flat element, -1 = padding
    for t, (o, n) in enumerate(zip(offs, numels)):
        kindmap[o:o + n] = t
    n_ranges = 0
    for rank in range(world):
        tab, owner = build_range_table(offs, numels, active, rank, per)
        assert tab.dtype == RANGE_DTYPE and tab.itemsize == C.sizeof(N.ZeroRange) and len(owner) == len(tab)
        n_ranges += len(tab)
        assert (np.diff(owner) >= 0).all()  # tensor order: a parameter group's ranges are one contiguous run
        gs = np.asarray(group_of)[owner] if len(owner) else owner
        assert (np.diff(gs) >= 0).all()
        for row, t in zip(tab, owner):
            s, n = int(row["start"]), int(row["n"])
            assert row["pad"] == 0 and 1 <= n <= CHUNK and s % 8 == 0
            assert 0 <= s and s + n <= per, "a range leaves the shard"
            lo = rank * per + s
            assert (kindmap[lo:lo + n] == t).all(), "a range touches padding or another tensor"
            assert active[t], "a range of an idle tensor"
            assert (lo - offs[t]) // CHUNK == (lo + n - 1 - offs[t]) // CHUNK, "a range crosses a chunk of its tensor"
            seen[lo:lo + n] += 1
        e = N.ZeroRange.from_buffer_copy(tab[:1].tobytes()) if len(tab) else None
        if e is not None:
            assert (e.start, e.n, e.pad) == (int(tab[0]["start"]), int(tab[0]["n"]), 0)
    want = np.zeros_like(seen)
    for t, (o, n) in enumerate(zip(offs, numels)):
        if active[t]:
            want[o:o + n] = 1
    assert (seen == want).all()  # every element of every with-gradient tensor exactly once; nothing else
    if kind == "small" and world == 4:  # [1] at 0, [7] at 8 (idle [5] at 16): two or more ranks own only padding
        empty = [len(build_range_table(offs, numels, active, r, per)[0]) == 0 for r in range(world)]
        assert sum(empty) >= 2 and n_ranges >= 2


def test_shard_boundaries_cut_tensors_chunks_and_groups():
    """At world 3 and 7 of the main set some shard boundary lies strictly inside a tensor and inside one of its
    16384-element chunks (so the cases above do exercise the cut), and shard_size rejects a bad world."""
    numels, active = numels_of("main", True)
    offs, total = flat_offsets(numels)
    for world in (3, 7):
        per = shard_size(total, world)
        cuts = [r * per for r in range(1, world)]
        inside = [(c, t) for c in cuts for t, (o, n) in enumerate(zip(offs, numels)) if o < c < o + n]
        assert inside and any((c - offs[t]) % CHUNK for c, t in inside)
    assert shard_size(1, 4) == 8
    with pytest.raises(ValueError):
        shard_size(100, 0)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    L = N.lib()
    p = 4096  # a non-null "pointer": every call below must return before any launch
    assert L.vp_abi_version() >= 22
    assert L.vp_zero_pack_bf16(None, None, 1, p, 64, 0.5, 0, None) == VP_ERR_ARG
    assert L.vp_zero_pack_bf16(p, p, 1, None, 64, 0.5, 0, None) == VP_ERR_ARG
    assert L.vp_zero_pack_bf16(p, p, -1, p, 64, 0.5, 0, None) == VP_ERR_ARG
    assert L.vp_zero_pack_bf16(p, p, 1, p, -8, 0.5, 0, None) == VP_ERR_ARG
    assert L.vp_zero_pack_bf16(p, p, 1, p, 64, 0.0, 0, None) == VP_ERR_ARG  # inv_world outside (0, 1]
    assert L.vp_zero_pack_bf16(p, p, 1, p, 64, 2.0, 0, None) == VP_ERR_ARG
    assert L.vp_zero_pack_bf16(p, p, 1, p, 64, float("nan"), 0, None) == VP_ERR_ARG
    assert L.vp_zero_unpack_bf16(None, None, 1, p, 64, p, None) == VP_ERR_ARG
    assert L.vp_zero_unpack_bf16(p, p, 1, None, 64, p, None) == VP_ERR_ARG
    assert L.vp_zero_unpack_bf16(p, p, 1, p, 64, None, None) == VP_ERR_ARG
    assert L.vp_zero_unpack_bf16(p, p, -3, p, 64, p, None) == VP_ERR_ARG
    assert L.vp_zero_shard_sqnorm(p, 1, p, 64, p, p, None, None) == VP_ERR_ARG  # no record
    assert L.vp_zero_shard_sqnorm(None, 1, p, 64, p, p, p, None) == VP_ERR_ARG
    assert L.vp_zero_shard_sqnorm(p, 1, None, 64, p, p, p, None) == VP_ERR_ARG
    assert L.vp_zero_shard_sqnorm(p, 1, p, 64, None, p, p, None) == VP_ERR_ARG
    assert L.vp_zero_shard_sqnorm(p, -1, p, 64, p, p, p, None) == VP_ERR_ARG
    assert L.vp_zero_shard_sqnorm(p, 1, p, -64, p, p, p, None) == VP_ERR_ARG
    assert L.vp_zero_finalize(None, 2, 1.0, 0.9, 0.95, 0, p, None) == VP_ERR_ARG
    assert L.vp_zero_finalize(p, 2, 1.0, 0.9, 0.95, 0, None, None) == VP_ERR_ARG
    assert L.vp_zero_finalize(p, 0, 1.0, 0.9, 0.95, 0, p, None) == VP_ERR_ARG
    assert L.vp_zero_finalize(p, 2, float("nan"), 0.9, 0.95, 0, p, None) == VP_ERR_ARG
    assert L.vp_zero_finalize(p, 2, 1.0, 1.0, 0.95, 0, p, None) == VP_ERR_ARG  # beta1 = 1
    adam = lambda *a, lr=1e-5, b1=0.9, b2=0.95, eps=1e-8, wd=1e-4: L.vp_zero_shard_adamw(  # noqa: E731
        *a, lr, b1, b2, eps, wd, 1, None)
    assert adam(None, 0, 1, p, p, p, p, p, 64, p) == VP_ERR_ARG
    assert adam(p, 0, 1, None, p, p, p, p, 64, p) == VP_ERR_ARG
    assert adam(p, 0, 1, p, None, p, p, p, 64, p) == VP_ERR_ARG
    assert adam(p, 0, 1, p, p, p, p, None, 64, p) == VP_ERR_ARG
    assert adam(p, 0, 1, p, p, p, p, p, 64, None) == VP_ERR_ARG
    assert adam(p, -1, 1, p, p, p, p, p, 64, p) == VP_ERR_ARG
    assert adam(p, 0, -1, p, p, p, p, p, 64, p) == VP_ERR_ARG
    assert adam(p, 0, 1, p, p, p, p, p, -1, p) == VP_ERR_ARG
    assert adam(p, 0, 1, p, p, p, p, p, 64, p, lr=-1.0) == VP_ERR_ARG
    assert adam(p, 0, 1, p, p, p, p, p, 64, p, b2=1.5) == VP_ERR_ARG
    assert adam(p, 0, 1, p, p, p, p, p, 64, p, eps=float("nan")) == VP_ERR_ARG
    # empty work is accepted without a launch
    assert L.vp_zero_pack_bf16(None, None, 0, None, 0, 1.0, 0, None) == 0
    assert L.vp_zero_unpack_bf16(None, None, 0, None, 0, p, None) == 0
    assert adam(None, 0, 0, p, p, p, p, p, 64, p) == 0


def test_constructor_validation_and_export():
    import videopainter_amd as V
    from videopainter_amd import zero
    from videopainter_amd.distributed import LocalComm
    assert V.ShardedFusedAdamW is zero.ShardedFusedAdamW
    assert issubclass(V.ShardedFusedAdamW, torch.optim.Optimizer)
    bf = lambda *s: torch.nn.Parameter(torch.zeros(*s, dtype=torch.bfloat16))  # noqa: E731
    comm = LocalComm(2)
    S = V.ShardedFusedAdamW
    with pytest.raises(TypeError):
        S([torch.nn.Parameter(torch.zeros(4))], comm=comm, rank=0)  # fp32
    with pytest.raises(ValueError):
        S([torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.bfloat16).t())], comm=comm, rank=0)  # not contiguous
    with pytest.raises(ValueError):
        S([], comm=comm, rank=0)
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-1.0),
               dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            S([bf(4)], comm=comm, rank=0, **kw)
    with pytest.raises(ValueError):
        S([bf(4)], comm=comm, rank=0)  # valid dtype and layout, but not on a device: nothing is allocated for it
    with pytest.raises(ValueError):
        S([bf(4)], comm=comm)  # comm= without rank=
    with pytest.raises(ValueError):
        S([bf(4)])  # neither a communicator nor an initialised process group


# ------------------------------------------------------------------------------------------------------------------
# the collective helpers on gloo
# ------------------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _layout(world):
    """The main set (idle parameter included) in the optimizer's flat space at `world`: (offs, numels, active, per)."""
    numels, active = numels_of("main", True)
    offs, total = flat_offsets(numels)
    return offs, numels, active, shard_size(total, world)


def _rank_data(rank, world):
    """What rank `rank`'s pack leaves in its fp32 staging buffer [world * per]: bf16 gradients N(0, 1e-3^2) times
    fp32(1 / world) at every active tensor's offset, zeros in the idle tensor and in all padding — the 8-element
    alignment gaps and the tail behind T that `per`'s rounding adds."""
    offs, numels, active, per = _layout(world)
    g = torch.Generator().manual_seed(900 + rank)
    flat = torch.zeros(world * per)
    inv = torch.tensor(1.0 / world, dtype=torch.float32)
    for o, n, a in zip(offs, numels, active):
        if a:
            flat[o:o + n] = (torch.randn(n, generator=g) * 1e-3).to(torch.bfloat16).float() * inv
    return flat


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from videopainter_amd.distributed import GroupComm, init
    init("gloo")
    comm = GroupComm()
    assert (comm.world, comm.rank) == (world, rank)
    per = _layout(world)[3]
    flat = _rank_data(rank, world)
    out = torch.empty(per)
    comm.reduce_scatter_sum(rank, out, flat)
    rec = torch.tensor([rank + 1, 10 * rank], dtype=torch.int32)
    recs = torch.zeros(2 * world, dtype=torch.int32)
    comm.all_gather(rank, recs, rec)
    flat16 = torch.zeros(world * per, dtype=torch.bfloat16)
    mine = flat16[rank * per:(rank + 1) * per]
    mine.copy_(flat[rank * per:(rank + 1) * per].to(torch.bfloat16) + rank)
    comm.all_gather(rank, flat16, mine)  # in place: the input is this rank's slice of the output
    q.put((rank, out.numpy().copy(), recs.numpy().copy(), flat16.float().numpy().copy()))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_collective_helpers_gloo(world):
    """On gloo, reduce_scatter_sum equals the slice of the rank-ordered fp32 sum within 1 ulp of that sum (the helper
    adds the host-staged slices in rank order itself, so the error is in fact 0: printed), exactly at world 2; both
    all-gathers are exact.  The buffers have the optimizer's own layout of the main set: at world 3 per = 72072, the
    shard boundaries cut tensor [64, 3072] twice, and the last shard ends in 8 elements of padding."""
    offs, numels, active, per = _layout(world)
    total = offs[-1] + (numels[-1] + 7) // 8 * 8
    if world == 3:
        assert per == 72072 and world * per - total == 8  # (a padded tail that exists only because per is rounded up)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=240) for _ in ps), key=lambda x: x[0])
    for p in ps:
        p.join(60)
    flats = [_rank_data(r, world) for r in range(world)]
    want = flats[0].clone()
    for f in flats[1:]:
        want += f  # rank order, fp32
    want16 = torch.cat([flats[r][r * per:(r + 1) * per].to(torch.bfloat16) + r for r in range(world)]).float()
    pad = torch.ones(world * per, dtype=torch.bool)
    for o, n, a in zip(offs, numels, active):
        if a:
            pad[o:o + n] = False
    assert int(pad.sum()) > world * per - total and bool(pad[total:].all())
    for rank, out, recs, flat16 in res:
        w = want[rank * per:(rank + 1) * per]
        got = torch.from_numpy(out)
        ulp = torch.ldexp(torch.ones_like(w), torch.frexp(w)[1].clamp(min=-125) - 24)  # the spacing of fp32 at w
        worst = float(((got - w).abs() / ulp).max())
        print(f"world {world} rank {rank}: reduce-scatter worst error {worst:.2f} ulp of the rank-ordered sum")
        assert worst <= 1.0
        if world == 2:
            assert torch.equal(got, w)
        assert not got[pad[rank * per:(rank + 1) * per]].any()  # padding and the idle tensor stay zero
        assert recs.tolist() == [v for r in range(world) for v in (r + 1, 10 * r)]
        assert torch.equal(torch.from_numpy(flat16), want16)
