"""Data-parallel training: gradients averaged by a reduce-scatter, AdamW on a 1 / world shard of the fp32 state, the
updated bf16 parameters all-gathered back (csrc/zero.hip; the reference trains under DeepSpeed ZeRO stage 2 + bf16,
train/VideoPainter.sh with accelerate_config_machine_single_ds.yaml).

Layout.  The flat element space is `FusedAdamW`'s (optim.flat_offsets, laid out by the base class both optimizers
derive from): every trainable parameter at its state offset, aligned to 8 elements, T elements in all.  per =
ceil(T / world) rounded up to a multiple of 8, the flat length is world * per and rank r owns [r * per, (r + 1) * per):
a shard boundary may cut a tensor, a 16384-element chunk or a parameter group anywhere that is a multiple of 8, and a
rank may own nothing but padding.  Each rank holds

    master, exp_avg, exp_avg_sq   fp32 [per]           12 B per parameter / world
    gradient staging              fp32 [world * per]   4 B per parameter (full size: the reduce-scatter is one
                                                       message, not bucketed and not overlapped with the backward)
    parameter staging             bf16 [world * per]   2 B per parameter

against FusedAdamW's 12 B per parameter.  Padding is zero and stays zero.

One step, three collectives, no host synchronisation:

    pack            bf16 grads -> fp32 staging, scaled by 1 / world        2 B read, 4 B written per parameter
    reduce-scatter  fp32, sum                                              -> the averaged gradient of this shard
    shard norm      sum of squares + non-finite flag of the shard          4 B read per parameter / world
    all-gather      one 8-byte record per rank
    finalise        FusedAdamW's finaliser over the records in rank order  -> the same scalars block on every rank
    shard AdamW     per parameter group, over this rank's ranges           16 B read, 14 B written per parameter / world
    all-gather      bf16                                                   the updated shard of every rank
    unpack          bf16 staging -> the bf16 parameters                    2 B read, 2 B written per parameter
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .optim import (BF16, CHUNK, _STATE_ALIGN, _STATE_KEYS, DeviceTables, _align, _FlatAdamW, build_chunk_table,
                    build_tensor_table)
from .optim import flat_offsets  # noqa: F401  (part of this module's interface too)

RANGE_DTYPE = np.dtype([("start", "<i8"), ("n", "<i4"), ("pad", "<i4")])  # N.ZeroRange
assert RANGE_DTYPE.itemsize == C.sizeof(N.ZeroRange)


def shard_size(total: int, world: int) -> int:
    """per: ceil(total / world) rounded up to a multiple of 8 (at least 8, so no buffer is empty)."""
    if world < 1:
        raise ValueError("world size must be positive")
    return max(_align((int(total) + world - 1) // world), _STATE_ALIGN)


def build_range_table(offs: Sequence[int], numels: Sequence[int], active: Sequence[bool], rank: int, per: int,
                      chunk: int = CHUNK) -> Tuple[np.ndarray, np.ndarray]:
    """The ranges of rank `rank`: (N.ZeroRange rows, the tensor index of every row).  A range is the part of one
    `chunk`-element chunk of one active tensor (one that has a gradient this step) that lies inside the rank's shard
    [rank * per, (rank + 1) * per); its start is relative to the shard.  So no range crosses a tensor (hence a
    parameter group), a chunk or the shard, none touches padding or an idle tensor, every element of an active tensor
    is in exactly one range of exactly one rank, and the rows follow the tensor order (a parameter group's ranges are
    one contiguous run)."""
    lo_s, hi_s = rank * per, (rank + 1) * per
    starts, ns, owner = [], [], []
    for t, (o, n, a) in enumerate(zip(offs, numels, active)):
        o, n = int(o), int(n)
        lo, hi = max(o, lo_s), min(o + n, hi_s)
        if not a or lo >= hi:
            continue
        c0, c1 = (lo - o) // chunk, (hi - o - 1) // chunk
        edges = o + np.arange(c0, c1 + 2, dtype=np.int64) * chunk  # chunk boundaries in flat coordinates
        a0 = np.maximum(edges[:-1], lo)
        a1 = np.minimum(edges[1:], hi)
        starts.append(a0 - lo_s)
        ns.append(a1 - a0)
        owner.append(np.full(a0.shape[0], t, dtype=np.int64))
    tab = np.zeros(sum(x.shape[0] for x in starts), dtype=RANGE_DTYPE)
    if starts:
        tab["start"] = np.concatenate(starts)
        tab["n"] = np.concatenate(ns)
    return tab, (np.concatenate(owner) if owner else np.zeros(0, dtype=np.int64))


class _ShardTables(DeviceTables):
    """The device tables of one step — the tensor and chunk tables of ALL trainable tensors (pack / unpack; a NULL
    gradient pointer marks an idle tensor) and this rank's range table, one reduction slot per range — rebuilt only
    when a pointer or the set of tensors with a gradient changed."""

    def __init__(self, device, offs, numels, group_of, n_groups, rank, per):
        super().__init__(device)
        self.offs, self.numels = list(offs), list(numels)
        self.group_of, self.n_groups, self.rank, self.per = list(group_of), n_groups, rank, per
        self.n_chunks = 0
        self.n_ranges = 0
        self.group_ranges: List[Tuple[int, int]] = [(0, 0)] * n_groups  # (first range, count) per parameter group

    def update(self, grad_ptrs: Sequence[int], param_ptrs: Sequence[int]) -> None:
        key = (tuple(grad_ptrs), tuple(param_ptrs))
        if key == self.key:
            return
        tt = build_tensor_table(list(grad_ptrs), list(param_ptrs), self.offs, self.numels)
        ct = build_chunk_table(self.numels)
        rt, owner = build_range_table(self.offs, self.numels, [g != 0 for g in grad_ptrs], self.rank, self.per)
        if ct.shape[0] >= 2 ** 31 or rt.shape[0] >= 2 ** 31:
            raise ValueError("too many chunks / ranges")
        self.upload(key, (tt, ct, rt), int(rt.shape[0]))
        self.n_chunks, self.n_ranges = int(ct.shape[0]), int(rt.shape[0])
        groups = np.asarray(self.group_of, dtype=np.int64)[owner] if owner.size else owner
        first = 0
        for g in range(self.n_groups):
            cnt = int((groups == g).sum())
            self.group_ranges[g] = (first, cnt)
            first += cnt

    @property
    def tensors(self) -> torch.Tensor:
        return self.buf

    @property
    def chunks(self) -> torch.Tensor:
        return self.table(1)

    @property
    def ranges(self) -> torch.Tensor:
        return self.table(2)


class ShardedFusedAdamW(_FlatAdamW):
    """The data-parallel counterpart of `FusedAdamW`: the same per-element AdamW arithmetic (one shared device
    function), gradients averaged over the ranks by a reduce-scatter, fp32 master weights and moments kept for this
    rank's 1 / world slice of the flat parameter space only (ZeRO stage 1 / 2 style), the updated bf16 parameters
    all-gathered back.  `step()` is pack, reduce-scatter, shard norm, record all-gather, finalise, shard AdamW per
    parameter group, bf16 all-gather, unpack: three collectives, no device-to-host copy, no synchronisation.

      process_group   a torch.distributed group (None: the default group); RCCL takes the device buffers as they
                      are, gloo goes through host copies (the one-GPU rehearsal).
      comm, rank      instead of a process group: an in-process communicator (distributed.LocalComm: the ranks are
                      threads of one process) and this instance's rank in it.  Both run the same step code.
      max_grad_norm   clip by the norm of the AVERAGED gradient (accelerator.clip_grad_norm_'s job under DeepSpeed);
                      folded into the update, the bf16 gradients are never scaled.
      skip_nonfinite  when the averaged gradient holds an inf / NaN in ANY rank's shard, every rank skips: no master,
                      moment, parameter or step counter changes and `last_step_skipped` is 1 everywhere.
      zero_grads      zero the bf16 gradients in the pack pass — also in a step that is skipped later.

    Contracts the constructor and step() do not check (checking would cost a collective and a host read):
      * at construction the bf16 parameters are identical on all ranks: call `distributed.broadcast_module(model)`
        first.  Masters start as the fp32 value of the bf16 parameters.
      * the set of parameters whose `.grad` is None is the same on every rank in every step.  Such a parameter is
        left untouched (no decay, no moment update), as in FusedAdamW; its flat gradient region is written as zeros.
    `step()` consumes whatever is in `.grad` (gradient accumulation is the caller's business).  `grad_norm` (of the
    averaged gradient, before the clip), `clip_coef`, `nonfinite`, `step_count` and `last_step_skipped` are device
    tensors, bit-identical on every rank.  Other differences from torch.optim.AdamW are FusedAdamW's: one step
    counter, the same betas in every group, bf16 contiguous parameters on one device.

    The state is flat, so `state[p]` stays empty; `master_shard`, `exp_avg_shard`, `exp_avg_sq_shard` are this rank's
    fp32 [per] slices.  `state_dict()` is the local shard; `full_state_dict()` (collective) is FusedAdamW's format, and
    `load_state_dict()` takes either — checkpoints move between FusedAdamW and any world size."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 *, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, zero_grads: bool = False,
                 process_group=None, comm=None, rank: Optional[int] = None):
        if comm is not None and process_group is not None:
            raise ValueError("ShardedFusedAdamW: give process_group= or comm=, not both")
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, zero_grads)
        if comm is None:
            from .distributed import GroupComm
            comm = GroupComm(process_group)
            if rank is not None and rank != comm.rank:
                raise ValueError(f"rank={rank} is not this process's rank in the group ({comm.rank})")
            rank = comm.rank
        elif rank is None:
            raise ValueError("ShardedFusedAdamW: comm= needs rank=")
        self._comm, self.world, self.rank = comm, int(comm.world), int(rank)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {self.rank} outside world size {self.world}")
        dev = self._device
        self.per = per = shard_size(self.total, self.world)
        self._lo, self._hi = self.rank * per, (self.rank + 1) * per
        self._alloc_scalars()
        self._master = torch.zeros(per, device=dev, dtype=torch.float32)
        self._exp_avg = torch.zeros_like(self._master)
        self._exp_avg_sq = torch.zeros_like(self._master)
        self._grad_shard = torch.zeros_like(self._master)
        self._flat32 = torch.zeros(self.world * per, device=dev, dtype=torch.float32)  # gradient staging
        self._flat16 = torch.zeros(self.world * per, device=dev, dtype=BF16)            # parameter staging
        self._record = torch.zeros(2, device=dev, dtype=torch.int32)                # N.ZeroRecord
        self._records = torch.zeros(2 * self.world, device=dev, dtype=torch.int32)  # every rank's, in rank order
        self._tables = _ShardTables(dev, self._offs.values(), [p.numel() for p in self._params], self._group_of,
                                    len(self.param_groups), self.rank, per)
        with torch.no_grad():  # masters = the fp32 value of the bf16 parameters, this rank's slice
            for p, o in self._offs.items():
                self._copy_slice(self._master, p.detach().reshape(-1), o)

    def _copy_slice(self, shard: torch.Tensor, full: torch.Tensor, off: int) -> None:
        """shard[...] = the part of a tensor (flat, at flat offset `off`) that lies inside this rank's shard."""
        lo, hi = max(off, self._lo), min(off + full.numel(), self._hi)
        if lo < hi:
            shard[lo - self._lo:hi - self._lo].copy_(full[lo - off:hi - off])

    # this rank's slice of the flat state
    @property
    def master_shard(self) -> torch.Tensor:
        return self._master

    @property
    def exp_avg_shard(self) -> torch.Tensor:
        return self._exp_avg

    @property
    def exp_avg_sq_shard(self) -> torch.Tensor:
        return self._exp_avg_sq

    # (the layout, for checkpoint tools and tests: total (T), per, world and rank are plain attributes; flat_offset(p)
    # is the base class's)
    @property
    def comm(self):
        """The communicator the step runs on (distributed.GroupComm or the comm= given)."""
        return self._comm

    @property
    def n_ranges(self) -> int:
        """The number of ranges this rank's shard was cut into in the last step (0: only padding or idle tensors)."""
        return self._tables.n_ranges

    @property
    def grad_staging(self) -> torch.Tensor:
        """fp32 [world * per]: what the last pack wrote (every rank's contribution to the reduce-scatter)."""
        return self._flat32

    @property
    def param_staging(self) -> torch.Tensor:
        """bf16 [world * per]: the all-gathered bf16(master) of the tensors updated in the last step."""
        return self._flat16

    @torch.no_grad()
    def step(self, closure=None):
        from . import kernels as K
        loss, betas = self._begin_step(closure)
        gp = [0 if p.grad is None else p.grad.data_ptr() for p in self._params]
        t, c, r = self._tables, self._comm, self.rank
        with torch.cuda.device(self._master.device):
            t.update(gp, [p.data_ptr() for p in self._params])
            K.zero_pack(t.tensors, t.chunks, t.n_chunks, self._flat32, inv_world=1.0 / self.world,
                        zero_grads=self.zero_grads)
            c.reduce_scatter_sum(r, self._grad_shard, self._flat32)
            K.zero_shard_sqnorm(t.ranges, t.n_ranges, self._grad_shard, t.partials, t.flags, self._record)
            c.all_gather(r, self._records, self._record)
            K.zero_finalize(self._records, self.world, self._scalars, max_norm=self.max_grad_norm or 0.0,
                            betas=betas, skip_nonfinite=self.skip_nonfinite)
            mine = self._flat16[self._lo:self._hi]
            for group, (r0, nr) in zip(self.param_groups, t.group_ranges):
                K.zero_shard_adamw(t.ranges, r0, nr, self._grad_shard, self._master, self._exp_avg, self._exp_avg_sq,
                                   mine, self._scalars, lr=float(group["lr"]), betas=betas, eps=float(group["eps"]),
                                   weight_decay=float(group["weight_decay"]),
                                   use_clip=self.max_grad_norm is not None)
            c.all_gather(r, self._flat16, mine)
            K.zero_unpack(t.tensors, t.chunks, t.n_chunks, self._flat16, self._scalars)
        return loss

    # ---- checkpoints ----
    def state_dict(self):
        """This rank's shard: {"world", "rank", "per", "step", "master", "exp_avg", "exp_avg_sq" (fp32 [per] clones),
        "param_groups"}.  Reloads into the same world size and rank only; `full_state_dict()` is the portable form.
        Reading the step counter is a device-to-host copy (not on the step path)."""
        return {"world": self.world, "rank": self.rank, "per": self.per, "step": int(self._scalars[3].item()),
                "master": self._master.detach().clone(), "exp_avg": self._exp_avg.detach().clone(),
                "exp_avg_sq": self._exp_avg_sq.detach().clone(), "param_groups": self._groups_dict()}

    @torch.no_grad()
    def full_state_dict(self):
        """COLLECTIVE (every rank calls it): the state of all ranks in exactly FusedAdamW.state_dict()'s format —
        {"state": {index: {master, exp_avg, exp_avg_sq}}, "param_groups", "step"}, per-parameter fp32 clones.  Three
        fp32 all-gathers through the gradient staging buffer (no extra flat buffer)."""
        state = {i: {} for i, p in self._indexed() if p in self._offs}
        with torch.cuda.device(self._master.device):
            for k, shard in (("master", self._master), ("exp_avg", self._exp_avg), ("exp_avg_sq", self._exp_avg_sq)):
                self._comm.all_gather(self.rank, self._flat32, shard)
                for i, p in self._indexed():
                    if p in self._offs:
                        o = self._offs[p]
                        state[i][k] = self._flat32[o:o + p.numel()].view(p.shape).clone()
            # (the next pack overwrites every tensor's region; padding is zero in every shard, so it stays zero)
        return {"state": state, "param_groups": self._groups_dict(), "step": int(self._scalars[3].item())}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Either format.  From the local format: the same world, rank and per.  From the full format (FusedAdamW's,
        or full_state_dict() of any world size): this rank's slice of every tensor.  Restores masters, moments, the
        parameter groups' options and the step counter; the bf16 parameters are left as they are (a checkpoint's
        model weights are bf16(master) already)."""
        self._check_groups(state_dict)
        keys = _STATE_KEYS
        mine = dict(zip(keys, (self._master, self._exp_avg, self._exp_avg_sq)))
        if "state" not in state_dict:
            if (state_dict["world"], state_dict["rank"], state_dict["per"]) != (self.world, self.rank, self.per):
                raise ValueError(f"loaded shard is rank {state_dict['rank']} of {state_dict['world']} (per "
                                 f"{state_dict['per']}); this optimizer is rank {self.rank} of {self.world} (per "
                                 f"{self.per}): use full_state_dict() to move between world sizes")
            for k in keys:
                if tuple(state_dict[k].shape) != (self.per,):
                    raise ValueError(f"loaded {k} shard has shape {tuple(state_dict[k].shape)}")
            for k in keys:
                mine[k].copy_(state_dict[k])
        else:
            for p, s in self._full_state(state_dict):
                for k in keys:
                    self._copy_slice(mine[k], s[k].reshape(-1), self._offs[p])
        self._restore_options(state_dict)
