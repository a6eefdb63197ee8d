"""Data-parallel training: gradients averaged by a reduce-scatter, the optimizer on a 1 / world shard of the fp32 state,
the updated bf16 parameters all-gathered back (csrc/zero.hip; the reference trains under DeepSpeed ZeRO stage 2 + bf16,
train/VideoPainter.sh with accelerate_config_machine_single_ds.yaml) — for the three optimizers of the reference's
get_optimizer: `ShardedFusedAdamW`, `ShardedFusedAdam` and `ShardedFusedProdigy`.

Layout.  The flat element space is `FusedAdamW`'s (optim.flat_offsets, laid out by the base class all optimizers
derive from): every trainable parameter at its state offset, aligned to 8 elements, T elements in all.  per =
ceil(T / world) rounded up to a multiple of 8, the flat length is world * per and rank r owns [r * per, (r + 1) * per):
a shard boundary may cut a tensor, a 16384-element chunk or a parameter group anywhere that is a multiple of 8, and a
rank may own nothing but padding.  Each rank holds

    master, exp_avg, exp_avg_sq   fp32 [per]           12 B per parameter / world
    (Prodigy: and s, p0           fp32 [per]           20 B per parameter / world in all)
    gradient staging              fp32 [world * per]   4 B per parameter (full size: the reduce-scatter is one
                                                       message, not bucketed and not overlapped with the backward)
    parameter staging             bf16 [world * per]   2 B per parameter

against FusedAdamW's 12 B (FusedProdigy's 20 B) per parameter.  Padding is zero and stays zero.

One step of AdamW / Adam, three collectives, no host synchronisation:

    pack            bf16 grads -> fp32 staging, scaled by 1 / world        2 B read, 4 B written per parameter
    reduce-scatter  fp32, sum                                              -> the averaged gradient of this shard
    shard norm      sum of squares + non-finite flag of the shard          4 B read per parameter / world
    all-gather      one 8-byte record per rank
    finalise        FusedAdamW's finaliser over the records in rank order  -> the same scalars block on every rank
    shard AdamW     per parameter group, over this rank's ranges           16 B read, 14 B written per parameter / world
    all-gather      bf16                                                   the updated shard of every rank
    unpack          bf16 staging -> the bf16 parameters                    2 B read, 2 B written per parameter

Prodigy has the same prologue (pack .. finalise) and epilogue (all-gather, unpack).  Between them, where AdamW has its
one pass, it has two passes around the only part of Prodigy that is not element-wise, the two sums of the d update:
a fourth collective, of 16 bytes per rank.

    d-phase 0       dlr of the step from the old d (every rank on its own copy of the d block)
    pass 1          per group: moments, s, one (dot, sum |s|) pair per range   24 B read, 12 B written per parameter / world
    record          this rank's pairs summed in double                         -> two doubles
    all-gather      one 16-byte record per rank
    d-phase 1       FusedProdigy's d update over the records in rank order     -> the same d block on every rank
    pass 2          per group: the update with the new d, bf16(p)              12 B read, 6 B written per parameter / world

Gradient accumulation (`accumulate()`, optim._FlatAdamW): a micro-batch that does not step is one launch,
vp_mt_accumulate_bf16 into the gradient staging buffer, and NO collective (DDP's no_sync); the stepping call folds the
last micro-batch with the scale 1 / (micro-batches x world) in the pack's place, and everything from the
reduce-scatter on is the step above.  No memory is added.

A skipped step (a non-finite averaged gradient under skip_nonfinite) and Prodigy's no-progress step (sum |s| == 0 over
all ranks) leave every bf16 parameter byte as it was on every rank: the unpack is gated on both, on the device.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .optim import (BF16, CHUNK, _PRODIGY_KEYS, _STATE_ALIGN, _STATE_KEYS, DeviceTables, _align, _FlatAdamW,
                    _ProdigyCore, build_chunk_table, build_tensor_table)
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


class _Sharded(_FlatAdamW):
    """What the three sharded optimizers share on top of `_FlatAdamW`: the communicator and this rank's place in it,
    the fp32 [per] state shards named by `_KEYS` (attributes `_master`, `_exp_avg`, ...; masters start as the fp32
    value of the bf16 parameters), the staging buffers, the norm records and the tables; the prologue of a step (tables,
    pack — or, with folds pending, the last fold — reduce-scatter, shard norm, record all-gather, finalise) and its
    epilogue (bf16 all-gather, unpack); and the two checkpoint formats over `_KEYS`.  A subclass owns what runs
    between prologue and epilogue."""

    _KEYS = _STATE_KEYS

    @staticmethod
    def _check_comm_args(name: str, process_group, comm, rank: Optional[int]) -> None:
        """What can be said about process_group= / comm= / rank= before anything else is looked at."""
        if comm is not None and process_group is not None:
            raise ValueError(f"{name}: give process_group= or comm=, not both")
        if comm is not None and rank is None:
            raise ValueError(f"{name}: comm= needs rank=")
        if comm is not None and not 0 <= int(rank) < int(comm.world):
            raise ValueError(f"rank {rank} outside world size {comm.world}")

    def _init_shards(self, process_group, comm, rank: Optional[int]) -> None:
        """After `_FlatAdamW.__init__` and the subclass's own checks: the first device allocations."""
        if comm is None:
            from .distributed import GroupComm
            comm = GroupComm(process_group)
            if rank is not None and rank != comm.rank:
                raise ValueError(f"rank={rank} is not this process's rank in the group ({comm.rank})")
            rank = comm.rank
        self._comm, self.world, self.rank = comm, int(comm.world), int(rank)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {self.rank} outside world size {self.world}")
        dev = self._device
        self.per = per = shard_size(self.total, self.world)
        self._lo, self._hi = self.rank * per, (self.rank + 1) * per
        self._alloc_scalars()
        for k in self._KEYS:
            setattr(self, "_" + k, torch.zeros(per, device=dev, dtype=torch.float32))
        self._grad_shard = torch.zeros_like(self._master)
        self._flat32 = torch.zeros(self.world * per, device=dev, dtype=torch.float32)  # gradient staging
        self._flat16 = torch.zeros(self.world * per, device=dev, dtype=BF16)            # parameter staging
        self._mine16 = self._flat16[self._lo:self._hi]  # this rank's slice of the parameter staging
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
    def grad_accumulator(self) -> torch.Tensor:
        """The fp32 accumulator of `accumulate()`: the gradient staging buffer itself (no memory of its own)."""
        return self._flat32

    def _fold_target(self):
        """(the tables of ALL trainable tensors, the accumulator): a fold runs where the pack runs."""
        gp = [0 if p.grad is None else p.grad.data_ptr() for p in self._params]
        self._tables.update(gp, [p.data_ptr() for p in self._params])
        return self._tables, self._flat32

    @property
    def param_staging(self) -> torch.Tensor:
        """bf16 [world * per]: the all-gathered bf16(master) of the tensors updated in the last step."""
        return self._flat16

    def _prologue(self, K, betas) -> _ShardTables:
        """Tables, pack, reduce-scatter, shard norm, record all-gather, finalise: after it `_grad_shard` holds the
        averaged gradient of this shard and the scalars block is the step's, the same on every rank."""
        c, r = self._comm, self.rank
        if self._pending:  # the last fold takes the pack's place: the mean over micro-batches and ranks in one scale
            t = self._last_fold(K, self.world)
        else:
            t, _ = self._fold_target()
            K.zero_pack(t.tensors, t.chunks, t.n_chunks, self._flat32, inv_world=1.0 / self.world,
                        zero_grads=self.zero_grads)
        c.reduce_scatter_sum(r, self._grad_shard, self._flat32)
        K.zero_shard_sqnorm(t.ranges, t.n_ranges, self._grad_shard, t.partials, t.flags, self._record)
        c.all_gather(r, self._records, self._record)
        K.zero_finalize(self._records, self.world, self._scalars, max_norm=self.max_grad_norm or 0.0,
                        betas=betas, skip_nonfinite=self.skip_nonfinite)
        return t

    def _epilogue(self, K, t: _ShardTables, dstate: Optional[torch.Tensor] = None) -> None:
        """The bf16 all-gather of every rank's updated shard and the unpack into the parameters (with `dstate`, a
        Prodigy d block: not in a no-progress step either)."""
        self._comm.all_gather(self.rank, self._flat16, self._mine16)
        if dstate is None:
            K.zero_unpack(t.tensors, t.chunks, t.n_chunks, self._flat16, self._scalars)
        else:
            K.zero_unpack_gated(t.tensors, t.chunks, t.n_chunks, self._flat16, self._scalars, dstate)

    # ---- checkpoints ----
    def _shards(self):
        return {k: getattr(self, "_" + k) for k in self._KEYS}

    def state_dict(self):
        """This rank's shard: {"world", "rank", "per", "step", the state shards (fp32 [per] clones: "master",
        "exp_avg", "exp_avg_sq", ...), "param_groups"}.  Reloads into the same world size and rank only;
        `full_state_dict()` is the portable form.  Reading the step counter is a device-to-host copy (not on the step
        path)."""
        self._no_pending("state_dict")
        sd = {"world": self.world, "rank": self.rank, "per": self.per, "step": int(self._scalars[3].item())}
        sd.update({k: v.detach().clone() for k, v in self._shards().items()})
        sd["param_groups"] = self._groups_dict()
        return sd

    @torch.no_grad()
    def full_state_dict(self):
        """COLLECTIVE (every rank calls it): the state of all ranks in exactly the single-GPU optimizer's
        state_dict() format — {"state": {index: {master, exp_avg, exp_avg_sq, ...}}, "param_groups", "step"},
        per-parameter fp32 clones.  One fp32 all-gather per state buffer through the gradient staging buffer (no extra
        flat buffer)."""
        self._no_pending("full_state_dict")
        state = {i: {} for i, p in self._indexed() if p in self._offs}
        with torch.cuda.device(self._master.device):
            for k, shard in self._shards().items():
                self._comm.all_gather(self.rank, self._flat32, shard)
                for i, p in self._indexed():
                    if p in self._offs:
                        o = self._offs[p]
                        state[i][k] = self._flat32[o:o + p.numel()].view(p.shape).clone()
            # (the next pack overwrites every tensor's region; padding is zero in every shard, so it stays zero)
        return {"state": state, "param_groups": self._groups_dict(), "step": int(self._scalars[3].item())}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Either format.  From the local format: the same world, rank and per.  From the full format (the single-GPU
        optimizer's, or full_state_dict() of any world size): this rank's slice of every tensor.  Restores the state
        shards, the parameter groups' options and the step counter; the bf16 parameters are left as they are (a
        checkpoint's model weights are bf16(master) already)."""
        self._no_pending("load_state_dict")
        self._check_groups(state_dict)
        keys, mine = self._KEYS, self._shards()
        if "state" not in state_dict:
            if (state_dict["world"], state_dict["rank"], state_dict["per"]) != (self.world, self.rank, self.per):
                raise ValueError(f"loaded shard is rank {state_dict['rank']} of {state_dict['world']} (per "
                                 f"{state_dict['per']}); this optimizer is rank {self.rank} of {self.world} (per "
                                 f"{self.per}): use full_state_dict() to move between world sizes")
            for k in keys:
                if k not in state_dict:
                    raise ValueError(f"loaded shard has no {k}")
                if tuple(state_dict[k].shape) != (self.per,):
                    raise ValueError(f"loaded {k} shard has shape {tuple(state_dict[k].shape)}")
            for k in keys:
                mine[k].copy_(state_dict[k])
        else:
            for p, s in self._full_state(state_dict, keys):
                for k in keys:
                    self._copy_slice(mine[k], s[k].reshape(-1), self._offs[p])
        self._restore_options(state_dict)


class ShardedFusedAdamW(_Sharded):
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
    `step()` consumes whatever is in `.grad`, plus the micro-batches `accumulate()` has folded since the last step:
    `for i in range(k): backward(); opt.accumulate() if i < k - 1 else opt.step()` with UNSCALED micro-batch losses
    averages over micro-batches and ranks in fp32; `accumulate()` issues no collective, and the set of parameters
    with a gradient must be the same in every micro-batch.  The checkpoint methods are refused while folds are pending
    (`full_state_dict()` gathers through the staging buffer that holds them).  `grad_norm` (of the
    averaged gradient, before the clip), `clip_coef`, `nonfinite`, `step_count` and `last_step_skipped` are device
    tensors, bit-identical on every rank.  Other differences from torch.optim.AdamW are FusedAdamW's: one step
    counter, the same betas in every group, bf16 contiguous parameters on one device.

    The state is flat, so `state[p]` stays empty; `master_shard`, `exp_avg_shard`, `exp_avg_sq_shard` are this rank's
    fp32 [per] slices.  `state_dict()` is the local shard; `full_state_dict()` (collective) is FusedAdamW's format, and
    `load_state_dict()` takes either — checkpoints move between FusedAdamW and any world size."""

    _UPDATE = "zero_shard_adamw"  # the kernels.py wrapper of the shard update (ShardedFusedAdam: "zero_shard_adam")

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 *, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, zero_grads: bool = False,
                 process_group=None, comm=None, rank: Optional[int] = None):
        self._check_comm_args(type(self).__name__, process_group, comm, rank)
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, zero_grads)
        self._init_shards(process_group, comm, rank)

    @torch.no_grad()
    def step(self, closure=None):
        from . import kernels as K
        loss, betas = self._begin_step(closure)
        update = getattr(K, self._UPDATE)
        with torch.cuda.device(self._master.device):
            t = self._prologue(K, betas)
            for group, (r0, nr) in zip(self.param_groups, t.group_ranges):
                update(t.ranges, r0, nr, self._grad_shard, self._master, self._exp_avg, self._exp_avg_sq,
                       self._mine16, self._scalars, lr=float(group["lr"]), betas=betas, eps=float(group["eps"]),
                       weight_decay=float(group["weight_decay"]), use_clip=self.max_grad_norm is not None)
            self._epilogue(K, t)
        return loss


class ShardedFusedAdam(ShardedFusedAdamW):
    """The data-parallel counterpart of `FusedAdam` (torch.optim.Adam; the reference's `--optimizer adam`): everything
    is `ShardedFusedAdamW`'s — shards, collectives, launches, options, contracts and checkpoint formats — except where
    the weight decay enters: as an L2 term on the averaged gradient, g = grad (* clip) + weight_decay * master, before
    the moments (vp_zero_shard_adam), not as a factor on the master.  Checkpoints move between `FusedAdam` and any
    world size."""

    _UPDATE = "zero_shard_adam"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 *, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, zero_grads: bool = False,
                 process_group=None, comm=None, rank: Optional[int] = None):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm=max_grad_norm,
                         skip_nonfinite=skip_nonfinite, zero_grads=zero_grads, process_group=process_group, comm=comm,
                         rank=rank)


class ShardedFusedProdigy(_ProdigyCore, _Sharded):
    """The data-parallel counterpart of `FusedProdigy` (prodigyopt.Prodigy; the reference's `--optimizer prodigy`): the
    same per-element arithmetic in both passes and the same d update (shared device functions), gradients averaged by
    a reduce-scatter, the five fp32 state buffers (master, exp_avg, exp_avg_sq, s, p0) kept for this rank's 1 / world
    slice only — 20 B per parameter / world — and the bf16 parameters all-gathered back.  The options are
    `FusedProdigy`'s; `process_group` / `comm` / `rank`, the meaning of `max_grad_norm`, `skip_nonfinite` and
    `zero_grads` and the two unchecked contracts are `ShardedFusedAdamW`'s.

    `step()` is pack, reduce-scatter, shard norm, all-gather of the norm records, finalise, d-phase 0, pass 1 per
    group, this rank's Prodigy record, all-gather (16 B per rank), d-phase 1, pass 2 per group, bf16 all-gather,
    unpack: four collectives, no device-to-host copy, no synchronisation.  The two sums of the d update are the only
    part of Prodigy that is not element-wise: every rank sums its ranges' (dot, sum |s|) pairs in double into a record,
    and every rank runs the same d update over all records in rank order on its own copy of the d block, so `d`,
    `d_max`, `d_hat`, `d_numerator`, `d_denom`, `dlr`, `no_progress` (`d_block`) and the scalars block are
    bit-identical on every rank.  At world size 1 a step is bit-identical to `FusedProdigy`'s; at another world size
    the shard cuts re-associate the two double sums, so d agrees to rounding, not bit for bit.  A skipped step changes
    nothing; a no-progress step (sum |s| == 0 over all ranks) changes no parameter byte on any rank, not the counter
    and nothing of the d block but d_denom and `no_progress`.  lr and beta3 are checked every step, as there.

    The state is flat, so `state[p]` stays empty; `master_shard`, `exp_avg_shard`, `exp_avg_sq_shard`, `s_shard` and
    `p0_shard` are this rank's fp32 [per] slices.  `state_dict()` is the local shard (the five buffers, the d block
    and the options); `full_state_dict()` (collective) is exactly FusedProdigy.state_dict()'s format, and
    `load_state_dict()` takes either — checkpoints move between FusedProdigy and any world size."""

    _KEYS = _PRODIGY_KEYS

    def __init__(self, params, lr: float = 1.0, betas=(0.9, 0.999), beta3: Optional[float] = None, eps: float = 1e-8,
                 weight_decay: float = 0.0, decouple: bool = True, use_bias_correction: bool = False,
                 safeguard_warmup: bool = False, d0: float = 1e-6, d_coef: float = 1.0,
                 growth_rate: float = float("inf"), *, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, zero_grads: bool = False, process_group=None, comm=None,
                 rank: Optional[int] = None):
        self._check_comm_args("ShardedFusedProdigy", process_group, comm, rank)
        params = self._check_prodigy_args("ShardedFusedProdigy", params, lr, beta3, d0, d_coef, growth_rate)
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, zero_grads)
        self._set_prodigy_options(beta3, decouple, use_bias_correction, safeguard_warmup, d0, d_coef, growth_rate)
        self._init_shards(process_group, comm, rank)
        self._alloc_d_block()
        self._p0.copy_(self._master)
        self._pairs = None  # fp32 [2 * ranges]: pass 1's (dot, sum |s|) of every range of this rank
        self._d_record = torch.zeros(2, device=self._device, dtype=torch.float64)  # this rank's (sum dot, sum |s|)
        self._d_records = torch.zeros(2 * self.world, device=self._device, dtype=torch.float64)  # all, in rank order

    @property
    def s_shard(self) -> torch.Tensor:
        return self._s

    @property
    def p0_shard(self) -> torch.Tensor:
        return self._p0

    @property
    def d_records(self) -> torch.Tensor:
        """float64 [2 * world]: every rank's (sum dot, sum |s|) record of the last step, in rank order."""
        return self._d_records

    @torch.no_grad()
    def step(self, closure=None):
        from . import kernels as K
        loss, betas = self._begin_step(closure)
        lr, beta3 = self._check_shared()
        use_clip = self.max_grad_norm is not None
        fin = self._finalize_args(lr, betas, beta3)
        sc, ds = self._scalars, self._d_block
        with torch.cuda.device(self._master.device):
            t = self._prologue(K, betas)
            if self._pairs is None or self._pairs.numel() < 2 * t.n_ranges:
                self._pairs = torch.empty(max(2 * t.n_ranges, 2048), device=self._device, dtype=torch.float32)
            K.zero_prodigy_finalize(0, None, self.world, sc, ds, **fin)
            runs = list(zip(self.param_groups, t.group_ranges))
            for group, (r0, nr) in runs:
                K.zero_shard_prodigy_moments(t.ranges, r0, nr, self._grad_shard, self._master, self._p0,
                                             self._exp_avg, self._exp_avg_sq, self._s, self._pairs, sc, ds,
                                             betas=betas, beta3=beta3,
                                             weight_decay=0.0 if self.decouple else float(group["weight_decay"]),
                                             d0=self.d0, safeguard_warmup=self.safeguard_warmup, use_clip=use_clip)
            K.zero_prodigy_record(self._pairs, t.n_ranges, sc, self._d_record)
            self._comm.all_gather(self.rank, self._d_records, self._d_record)
            K.zero_prodigy_finalize(1, self._d_records, self.world, sc, ds, **fin)
            for group, (r0, nr) in runs:
                K.zero_shard_prodigy_update(t.ranges, r0, nr, self._master, self._exp_avg, self._exp_avg_sq,
                                            self._mine16, sc, ds, eps=float(group["eps"]),
                                            weight_decay=float(group["weight_decay"]) if self.decouple else 0.0)
            self._epilogue(K, t, ds)
        return loss

    # ---- checkpoints: the base class's two formats plus the "prodigy" entry (the d block and the options) ----
    def state_dict(self):
        """This rank's shard, as `ShardedFusedAdamW.state_dict()` with the five buffers, plus "prodigy": the d block's
        values and the optimizer-wide options (FusedProdigy.state_dict()'s entry of that name)."""
        sd = super().state_dict()
        sd["prodigy"] = self._prodigy_dict()
        return sd

    def full_state_dict(self):
        """COLLECTIVE: exactly FusedProdigy.state_dict()'s format (five fp32 all-gathers through the gradient staging
        buffer)."""
        sd = super().full_state_dict()
        sd["prodigy"] = self._prodigy_dict()
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Either format (a dict without the d block is refused before anything is copied)."""
        self._no_pending("load_state_dict")
        pr = self._prodigy_entry(state_dict)
        super().load_state_dict(state_dict)
        self._load_prodigy_dict(pr)
