"""The optimizer tail of the training step on the HIP kernels (csrc/optim.hip, csrc/prodigy.hip): gradient norm, clip,
and the three optimizers the reference's get_optimizer offers (--optimizer adam | adamw | prodigy,
train/train_cogvideox_inpainting_i2v_video.py:1283-1361), each with fp32 master weights behind the bf16 parameters.

The reference trains under accelerate + DeepSpeed bf16 (train/VideoPainter.sh: --mixed_precision bf16 --optimizer
AdamW --learning_rate 1e-5 --max_grad_norm 1.0), which keeps fp32 master weights and fp32 moments behind the bf16
model.  This package's branch parameters are bf16 device tensors with bf16 gradients; stepping a plain optimizer on
them loses most of an lr = 1e-5 update below half a bf16 ulp, and Prodigy's distance estimate, built from p0 - p,
would be mostly rounding noise.  The optimizers here own the fp32 masters and state and write the bf16 parameters
back every step.

    FusedAdamW(params, ..., max_grad_norm=1.0)   norm + clip + update in three launches (people who own their loop)
    FusedAdam(params, ...)                       the same with torch.optim.Adam's decay (an L2 term on the gradient)
    FusedProdigy(params, lr=1.0, ...)            prodigyopt.Prodigy: two passes around the update of d, on the device
    clip_grad_norm_(parameters, max_norm)        norm + in-place scale (accelerator.clip_grad_norm_'s job, :1897)
    get_gradient_norm(parameters)                norm only (the script's helper, :80-90, without its host loop)

Gradient accumulation (the script's --gradient_accumulation_steps, :348 / :1743 / :1894): every optimizer here and in
zero.py has `accumulate()`, which folds the current bf16 gradients into an fp32 flat accumulator, and a `step()` that,
with folds pending, folds the last micro-batch scaled to the mean and runs norm, clip and update on the accumulator
(vp_mt_accumulate_bf16 and the fp32-gradient forms of the norm and update kernels).  The mean is what accelerate's
loss / k gives, so micro-batch losses are passed unscaled.  Adding micro-batches into the bf16 `.grad` instead would
lose exactly what the fp32 masters keep.

Nothing here copies device memory to the host or synchronises: the norm, the clip coefficient, the non-finite flag,
the step counter and the bias corrections live in a small device block the kernels read, and so does Prodigy's d.

The data-parallel optimizers (zero.ShardedFusedAdamW, ShardedFusedAdam, ShardedFusedProdigy) are built on the same
parts: `_FlatAdamW` (validation, the flat layout of `flat_offsets`, the scalars block, the state-dict checks, the step
prologue, the gradient accumulation), `_ProdigyCore` (Prodigy's options, its d block and state-dict entry) and
`DeviceTables` (the table uploader over `pack_tables`).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N

BF16 = torch.bfloat16
CHUNK = N.MT_CHUNK
_STATE_ALIGN = 8  # elements: every tensor's fp32 state starts on a 16-byte boundary of the flat buffers


def build_chunk_table(numels: Sequence[int], chunk: int = CHUNK) -> np.ndarray:
    """int32 [n_chunks, 2] rows (tensor index, chunk index inside the tensor) — N.MtChunk.  Chunk c of tensor t covers
    elements [c * chunk, min(numel_t, (c + 1) * chunk)): every element exactly once, no chunk crosses a tensor, an
    empty tensor has no chunk."""
    rows = []
    for t, n in enumerate(numels):
        n = int(n)
        if n < 0:
            raise ValueError("negative tensor size")
        k = (n + chunk - 1) // chunk
        if k:
            rows.append(np.stack((np.full(k, t, dtype=np.int32), np.arange(k, dtype=np.int32)), 1))
    return np.concatenate(rows, 0) if rows else np.zeros((0, 2), dtype=np.int32)


def build_tensor_table(grad_ptrs: Sequence[int], param_ptrs: Sequence[int], state_offs: Sequence[int],
                       numels: Sequence[int]) -> np.ndarray:
    """int64 [n, 4] rows (grad pointer, param pointer, state offset, numel) — N.MtTensor."""
    return np.array([grad_ptrs, param_ptrs, state_offs, numels], dtype=np.int64).T.reshape(len(numels), 4).copy()


def _check_grad(g: torch.Tensor, what: str) -> None:
    if g.is_sparse:
        raise ValueError(f"{what}: sparse gradients are not supported")
    if g.dtype != BF16:
        raise TypeError(f"{what} must be torch.bfloat16, got {g.dtype}")
    if not g.is_cuda:
        raise ValueError(f"{what} must be a device tensor")
    if not g.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _align(n: int) -> int:
    return (n + _STATE_ALIGN - 1) // _STATE_ALIGN * _STATE_ALIGN


def flat_offsets(numels: Sequence[int]) -> Tuple[List[int], int]:
    """(state offset of every tensor, T): the flat element space of the optimizer state, every tensor aligned to 8
    elements."""
    offs, total = [], 0
    for n in numels:
        offs.append(total)
        total += _align(int(n))
    return offs, total


def pack_tables(arrays: Sequence[np.ndarray]) -> Tuple[np.ndarray, List[int]]:
    """(uint8 image, byte offset of every table): the tables laid end to end, each on a 16-byte boundary.  A tensor
    row is 32 bytes, so a chunk table after a tensor table begins at n_tensors * 32."""
    parts, offs, at = [], [], 0
    for a in arrays:
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        offs.append(at)
        parts += [b, np.zeros((-b.size) % 16, dtype=np.uint8)]
        at += b.size + (-b.size) % 16
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), offs


class DeviceTables:
    """Host-built tables in one device buffer, and the reduction workspace (one `partials` / `flags` slot per piece).

    A user builds its tables on the host and hands them to `upload` (one asynchronous copy from pinned memory, on the
    current stream) only when its key — the pointers, sizes and set of tensors — changed since the last call: so
    persistent `.grad` tensors cost nothing per step, and gradients reallocated every step (`p.grad = None`,
    `zero_grad(set_to_none=True)`) cost one small copy."""

    def __init__(self, device: torch.device):
        self.device = device
        self.key = None
        self.buf = None  # uint8 device buffer: the tables in upload order
        self.offsets: List[int] = []
        self.partials = None
        self.flags = None

    def upload(self, key, arrays: Sequence[np.ndarray], slots: int) -> None:
        host, self.offsets = pack_tables(arrays)
        if host.size:
            if self.buf is None or self.buf.numel() < host.size:
                self.buf = torch.empty(max(host.size, 4096), device=self.device, dtype=torch.uint8)
            pinned = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
            pinned.copy_(torch.from_numpy(host))
            self.buf[:host.size].copy_(pinned, non_blocking=True)
        if self.partials is None or self.partials.numel() < slots:
            self.partials = torch.empty(max(slots, 1024), device=self.device, dtype=torch.float32)
            self.flags = torch.empty(max(slots, 1024), device=self.device, dtype=torch.int32)
        self.key = key

    def table(self, i: int) -> Optional[torch.Tensor]:
        return None if self.buf is None else self.buf[self.offsets[i]:]


class MultiTensorTables(DeviceTables):
    """The tensor table and the chunk table of a list of gradients; one reduction slot per chunk."""

    def __init__(self, device: torch.device):
        super().__init__(device)
        self.n_tensors = 0
        self.n_chunks = 0
        self.numels: List[int] = []

    def update(self, grads: Sequence[torch.Tensor], params: Optional[Sequence[torch.Tensor]] = None,
               state_offs: Optional[Sequence[int]] = None) -> None:
        gp = [g.data_ptr() for g in grads]
        pp = [p.data_ptr() for p in params] if params is not None else [0] * len(gp)
        so = list(state_offs) if state_offs is not None else [0] * len(gp)
        ne = [g.numel() for g in grads]
        key = (tuple(gp), tuple(pp), tuple(so), tuple(ne))
        if key == self.key:
            return
        tt = build_tensor_table(gp, pp, so, ne)
        ct = build_chunk_table(ne)
        if len(ne) >= 2 ** 31 or ct.shape[0] >= 2 ** 31:
            raise ValueError("too many tensors / chunks")
        self.upload(key, (tt, ct), int(ct.shape[0]))
        self.n_tensors, self.n_chunks, self.numels = len(ne), int(ct.shape[0]), ne

    @property
    def tensors(self) -> Optional[torch.Tensor]:
        return self.buf

    @property
    def chunks(self) -> Optional[torch.Tensor]:
        return self.table(1)

    def chunks_of(self, first_tensor: int, n: int):
        """(first chunk, chunk count) of tensors [first_tensor, first_tensor + n) of the list."""
        per = [(x + CHUNK - 1) // CHUNK for x in self.numels]
        return sum(per[:first_tensor]), sum(per[first_tensor:first_tensor + n])


_TABLES: dict = {}  # device -> MultiTensorTables of the functional API


def _grads_of(parameters) -> List[torch.Tensor]:
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        _check_grad(g, "gradient")
    if len({g.device for g in grads}) > 1:
        raise ValueError("gradients on more than one device")
    return grads


def _norm_into(tables: MultiTensorTables, scalars: torch.Tensor, max_norm: float) -> None:
    from . import kernels as K
    K.mt_grad_sqnorm(tables.tensors, tables.chunks, tables.n_chunks, tables.partials, tables.flags)
    K.optim_finalize(tables.partials, tables.flags, tables.n_chunks, scalars, max_norm=max_norm)


def _functional(parameters, max_norm: float, scale: bool) -> torch.Tensor:
    grads = _grads_of(parameters)
    if not grads:
        return torch.zeros(())
    dev = grads[0].device
    tables = _TABLES.get(dev)
    if tables is None:
        tables = _TABLES[dev] = MultiTensorTables(dev)
    with torch.cuda.device(dev):
        tables.update(grads)
        scalars = torch.zeros(8, device=dev, dtype=torch.int32)
        _norm_into(tables, scalars, max_norm)
        if scale:
            from . import kernels as K
            K.mt_scale(tables.tensors, tables.chunks, tables.n_chunks, scalars)
    return scalars.view(torch.float32)[0]


def get_gradient_norm(parameters) -> torch.Tensor:
    """Total L2 norm of the bf16 gradients of `parameters` as a 0-dim fp32 DEVICE tensor (no host read; the
    reference's helper, train_cogvideox_inpainting_i2v_video.py:80-90, reads one .item() per parameter)."""
    return _functional(parameters, 0.0, False)


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ on the HIP kernels: grads *= min(1, max_norm / (norm + 1e-6)) in place (bf16
    rounding of each product), the total norm returned as a 0-dim fp32 device tensor.  Gradients are not touched at
    all when the coefficient is 1."""
    if float(norm_type) != 2.0:
        raise ValueError("clip_grad_norm_: only the L2 norm is implemented")
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("clip_grad_norm_: max_norm must be positive")
    return _functional(parameters, max_norm, True)


_STATE_KEYS = ("master", "exp_avg", "exp_avg_sq")


class _FlatAdamW(torch.optim.Optimizer):
    """What `FusedAdamW` and `zero.ShardedFusedAdamW` share: the validation of hyper-parameters and parameters, the
    trainable parameters laid out in one flat element space (`flat_offsets`), the int32[8] device scalars block
    (N.OptimScalars) with its read-only views, the checks of a loaded state dict, the prologue of `step()` and the
    gradient accumulation (`accumulate()`, `pending`, `reset_accumulation()`; a subclass names the tables and the
    accumulator in `_fold_target` and calls `_last_fold` from a step with folds pending).  A subclass owns the state
    buffers, the step itself and its checkpoint formats."""

    def __init__(self, params, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, zero_grads):
        """Validates everything and lays out the flat space; allocates nothing (`_alloc_scalars` is the subclass's
        first device allocation, after its own checks)."""
        name = type(self).__name__
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.zero_grads = bool(zero_grads)
        self._params, self._group_of = [], []  # the trainable parameters in list order, and their group index
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.requires_grad:
                    self._params.append(p)
                    self._group_of.append(gi)
        if not self._params:
            raise ValueError(f"{name}: no parameter requires a gradient")
        for p in self._params:
            if p.dtype != BF16:
                raise TypeError(f"{name} parameters must be torch.bfloat16, got {p.dtype}")
            if p.layout != torch.strided or not p.is_contiguous():
                raise ValueError(f"{name} parameters must be dense and contiguous")
            if p.grad is not None and p.grad.is_sparse:
                raise ValueError(f"{name} does not support sparse gradients")
        if not all(p.is_cuda for p in self._params):
            raise ValueError(f"{name} parameters must be device tensors")
        if len({p.device for p in self._params}) > 1:
            raise ValueError(f"{name} parameters must be on one device")
        self._device = self._params[0].device
        offs, self.total = flat_offsets([p.numel() for p in self._params])
        self._offs = dict(zip(self._params, offs))
        self._pending = 0         # micro-batches folded into the accumulator since the last step
        self._acc_active = None   # which trainable parameters had a gradient in the first fold of this step
        self._acc = None          # fp32 [total]: the single-GPU accumulator, allocated by the first accumulate()

    def _alloc_scalars(self) -> None:
        self._scalars = torch.zeros(8, device=self._device, dtype=torch.int32)  # N.OptimScalars
        self._scalars_f = self._scalars.view(torch.float32)

    # the device scalars of the last step
    @property
    def grad_norm(self) -> torch.Tensor:
        return self._scalars_f[0]

    @property
    def clip_coef(self) -> torch.Tensor:
        return self._scalars_f[1]

    @property
    def nonfinite(self) -> torch.Tensor:
        return self._scalars[2]

    @property
    def step_count(self) -> torch.Tensor:
        return self._scalars[3]

    @property
    def last_step_skipped(self) -> torch.Tensor:
        return self._scalars[6]

    @property
    def scalars(self) -> torch.Tensor:
        """The whole int32[8] block (N.OptimScalars)."""
        return self._scalars

    def flat_offset(self, p: torch.Tensor) -> int:
        """The flat element offset of trainable parameter `p`: its state is elements [offset, offset + p.numel()) of
        the flat space (`total` elements in all)."""
        if p not in self._offs:
            raise KeyError("not a trainable parameter of this optimizer")
        return self._offs[p]

    # ---- gradient accumulation ----
    @property
    def pending(self) -> int:
        """The number of micro-batches `accumulate()` has folded since the last step (a host int)."""
        return self._pending

    @property
    def grad_accumulator(self) -> Optional[torch.Tensor]:
        """The fp32 flat accumulator (the element space of `flat_offset`; read-only for callers).  None until the
        first `accumulate()`: an optimizer that never accumulates allocates nothing."""
        return self._acc

    def reset_accumulation(self) -> None:
        """Drops the pending folds: the next `accumulate()` or `step()` starts from the gradients alone."""
        self._pending, self._acc_active = 0, None

    @torch.no_grad()
    def accumulate(self) -> None:
        """Folds the current bf16 `.grad` of every parameter that has one into the fp32 accumulator as one more
        micro-batch — the first fold after a step overwrites, later ones add — and zeroes the gradients in the same
        pass under `zero_grads` (gradients set to None between micro-batches work as well).  One launch: no host
        read, no synchronisation, no collective.  The loop of k micro-batches is

            for i in range(k): backward(); opt.accumulate() if i < k - 1 else opt.step()

        and `step()` applies the 1 / k: it runs on the fp32 MEAN of the micro-batch gradients, which is what
        accelerate's loss / k gives, so the micro-batch losses are passed UNSCALED.  The set of parameters with a
        gradient must be the same in every micro-batch of one step (ValueError otherwise)."""
        from . import kernels as K
        self._begin_step(None)
        with torch.cuda.device(self._device):
            self._fold(K, 1.0)

    def _fold(self, K, scale: float):
        """One fold of the current gradients with `scale` (1, or the step's 1 / count in the last one); returns the
        tables it ran over."""
        active = tuple(p.grad is not None for p in self._params)
        if self._pending and active != self._acc_active:
            raise ValueError(f"{type(self).__name__}: the set of parameters with a gradient changed between the "
                             f"micro-batches of one step")
        t, acc = self._fold_target()
        K.mt_accumulate(t.tensors, t.chunks, t.n_chunks, acc, first=self._pending == 0, scale=scale,
                        zero_grads=self.zero_grads)
        self._acc_active = active
        self._pending += 1
        return t

    def _fold_target(self):
        """(the tables of the current gradients, the accumulator) — the single-GPU form: the active tensors' tables
        and an fp32 [total] buffer of this optimizer's own."""
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        self._tables.update([p.grad for p in params], params, [self._offs[p] for p in params])
        if self._acc is None:
            self._acc = torch.zeros(max(self.total, 1), device=self._device, dtype=torch.float32)
        return self._tables, self._acc

    def _last_fold(self, K, ranks: int = 1):
        """step() with pending folds: the current gradients as the last micro-batch, scaled to the mean (over the
        micro-batches and, for a sharded step, the `ranks` whose folds the reduce-scatter then sums)."""
        t = self._fold(K, 1.0 / ((self._pending + 1) * ranks))
        self.reset_accumulation()
        return t

    def _no_pending(self, what: str) -> None:
        if self._pending:
            raise RuntimeError(f"{type(self).__name__}.{what}() with {self._pending} accumulated micro-batch(es) "
                               f"pending: step() or reset_accumulation() first")

    def _begin_step(self, closure):
        """The prologue of step(): (the closure's loss, the betas every group shares), after checking every gradient
        there is."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        betas = self.param_groups[0]["betas"]
        for group in self.param_groups:
            if tuple(group["betas"]) != tuple(betas):
                raise ValueError(f"{name}: betas must be the same in every parameter group")
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p not in self._offs:
                    raise ValueError(f"{name}: a parameter that did not require a gradient at construction has one")
                _check_grad(p.grad, "gradient")
        return loss, betas

    def _indexed(self):
        i = 0
        for g in self.param_groups:
            for p in g["params"]:
                yield i, p
                i += 1

    def _groups_dict(self):
        groups, i = [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(i, i + len(g["params"])))
            i += len(g["params"])
            groups.append(d)
        return groups

    def _check_groups(self, state_dict) -> None:
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"])
                                                        for a, b in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict has different parameter groups")

    def _full_state(self, state_dict, keys=_STATE_KEYS):
        """[(trainable parameter, its {master, exp_avg, exp_avg_sq, ...: `keys`})] of a full-format state dict, every
        shape checked before anything is copied."""
        state, out = state_dict["state"], []
        for i, p in self._indexed():
            if p not in self._offs:
                continue
            s = state.get(i, state.get(str(i)))
            if s is None:
                raise ValueError(f"loaded state dict has no state for parameter {i}")
            for k in keys:
                if k not in s:
                    raise ValueError(f"loaded state dict has no {k} for parameter {i}")
                if tuple(s[k].shape) != tuple(p.shape):
                    raise ValueError(f"loaded {k} of parameter {i} has shape {tuple(s[k].shape)}")
            out.append((p, s))
        return out

    def _restore_options(self, state_dict) -> None:
        """The groups' options and the step counter of a loaded state dict (after the state itself)."""
        for mine, theirs in zip(self.param_groups, state_dict["param_groups"]):
            mine.update({k: v for k, v in theirs.items() if k != "params"})
        self._scalars[3:4].fill_(int(state_dict.get("step", 0)))
        self._scalars[6:7].zero_()


class FusedAdamW(_FlatAdamW):
    """torch.optim.AdamW (amsgrad=False, maximize=False) for bf16 device parameters with fp32 master weights.

    State lives in three flat fp32 device buffers (master, exp_avg, exp_avg_sq); `state[p]` exposes per-parameter
    views of them plus the shared device step counter.  Masters start as the fp32 value of the bf16 parameters.
    `step()` is three kinds of launches — gradient norm, its finaliser, one update per parameter group — with no
    device-to-host copy and no synchronisation; `grad_norm` (before the clip), `clip_coef` and `last_step_skipped`
    are device tensors.

      max_grad_norm   fold clip_grad_norm_(max_grad_norm) into the update.  The gradients themselves are left
                      UNSCALED (the update multiplies by the coefficient in fp32, without the bf16 rounding a separate
                      clip pass would add).
      skip_nonfinite  when any gradient element is inf / NaN the step changes no parameter, no state and not the
                      step counter, and `last_step_skipped` is 1.
      zero_grads      zero the gradients (in place, same storage) in the update pass — also in a skipped step.

    `accumulate()` / `pending` / `reset_accumulation()` / `grad_accumulator` (`_FlatAdamW`): fp32 gradient
    accumulation over micro-batches — `for i in range(k): backward(); opt.accumulate() if i < k - 1 else opt.step()`
    with UNSCALED micro-batch losses; the step runs on the fp32 mean.  State dicts are refused while folds are pending.

    Differences from torch's: one step counter for the whole optimizer (a parameter whose grad was None in some
    step shares the others' bias correction); betas must be the same in every parameter group (lr, weight_decay and
    eps may differ); parameters must be bf16, contiguous, on one device; amsgrad / maximize / foreach / capturable do
    not exist.  `load_state_dict` restores masters, moments and the step counter and leaves the bf16 parameters as
    they are (a checkpoint's model weights are bf16(master) already)."""

    _UPDATE = "mt_adamw"  # the kernels.py wrapper of the update pass (FusedAdam: "mt_adam")

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 *, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, zero_grads: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, zero_grads)
        self._alloc_scalars()
        self._master = torch.zeros(max(self.total, 1), device=self._device, dtype=torch.float32)
        self._exp_avg = torch.zeros_like(self._master)
        self._exp_avg_sq = torch.zeros_like(self._master)
        self._tables = MultiTensorTables(self._device)
        with torch.no_grad():
            for p in self._params:
                o, n = self._offs[p], p.numel()
                self._master[o:o + n].copy_(p.detach().reshape(-1))
                self.state[p] = dict(step=self._scalars[3], master=self._master[o:o + n].view(p.shape),
                                     exp_avg=self._exp_avg[o:o + n].view(p.shape),
                                     exp_avg_sq=self._exp_avg_sq[o:o + n].view(p.shape))

    @torch.no_grad()
    def step(self, closure=None):
        from . import kernels as K
        loss, betas = self._begin_step(closure)
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        t = self._tables
        with torch.cuda.device(self._device):
            accumulated = self._pending > 0
            if accumulated:  # the gradient of the step is the accumulator: the fp32 mean of the micro-batches
                self._last_fold(K)
                K.mt_grad_sqnorm_f32(t.tensors, t.chunks, t.n_chunks, self._acc, t.partials, t.flags)
            else:
                t.update([p.grad for p in params], params, [self._offs[p] for p in params])
                K.mt_grad_sqnorm(t.tensors, t.chunks, t.n_chunks, t.partials, t.flags)
            K.optim_finalize(t.partials, t.flags, t.n_chunks, self._scalars, max_norm=self.max_grad_norm or 0.0,
                             betas=betas, skip_nonfinite=self.skip_nonfinite, advance_step=True)
            first, update = 0, getattr(K, self._UPDATE + "_f32" if accumulated else self._UPDATE)
            for group in self.param_groups:  # the active tensors of a group are one run of the list
                n = sum(p.grad is not None for p in group["params"])
                c0, nc = t.chunks_of(first, n)
                first += n
                hyper = dict(lr=float(group["lr"]), betas=betas, eps=float(group["eps"]),
                             weight_decay=float(group["weight_decay"]), use_clip=self.max_grad_norm is not None)
                if accumulated:  # (the last fold zeroed the gradients)
                    update(t.tensors, t.chunks, c0, nc, self._acc, self._master, self._exp_avg, self._exp_avg_sq,
                           self._scalars, **hyper)
                else:
                    update(t.tensors, t.chunks, c0, nc, self._master, self._exp_avg, self._exp_avg_sq, self._scalars,
                           **hyper, zero_grads=self.zero_grads)
        return loss

    def state_dict(self):
        """{"state": {index: {master, exp_avg, exp_avg_sq}}, "param_groups": [...], "step": int} — clones; reading
        the step counter is the one device-to-host copy of this class (not on the step path)."""
        self._no_pending("state_dict")
        state = {i: {k: self.state[p][k].detach().clone() for k in _STATE_KEYS}
                 for i, p in self._indexed() if p in self._offs}
        return {"state": state, "param_groups": self._groups_dict(), "step": int(self._scalars[3].item())}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        self._no_pending("load_state_dict")
        self._check_groups(state_dict)
        for p, s in self._full_state(state_dict):
            for k in _STATE_KEYS:
                self.state[p][k].copy_(s[k])
        self._restore_options(state_dict)


class FusedAdam(FusedAdamW):
    """torch.optim.Adam (amsgrad=False, maximize=False) for bf16 device parameters with fp32 master weights: the
    reference's `--optimizer adam`.  Everything is `FusedAdamW`'s — state, launches, keyword-only options, state dict
    and the differences from torch's — except where the weight decay enters: as an L2 term on the gradient,
    g = grad (* clip) + weight_decay * master, before the moments (vp_mt_adam_bf16), not as a factor on the master."""

    _UPDATE = "mt_adam"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 *, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, zero_grads: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm=max_grad_norm,
                         skip_nonfinite=skip_nonfinite, zero_grads=zero_grads)


_PRODIGY_KEYS = ("master", "exp_avg", "exp_avg_sq", "s", "p0")
_D_FIELDS = ("d", "d_max", "d_hat", "d_numerator", "d_denom", "dlr")  # N.ProdigyScalars, its doubles in order


class _ProdigyCore:
    """What `FusedProdigy` and `zero.ShardedFusedProdigy` share beside `_FlatAdamW`: the validation of Prodigy's own
    options, the check of what every group must share, the float64[7] d block (N.ProdigyScalars) with its read-only
    views, and the "prodigy" entry of a state dict.  A subclass allocates `_d_block` with `_alloc_d_block`."""

    @staticmethod
    def _check_prodigy_args(name, params, lr, beta3, d0, d_coef, growth_rate):
        """Validates the options `_FlatAdamW` does not know; returns the parameters as a list."""
        if not 0.0 < d0 < float("inf"):
            raise ValueError(f"Invalid d0 value: {d0}")
        if not 0.0 < d_coef < float("inf"):
            raise ValueError(f"Invalid d_coef value: {d_coef}")
        if not growth_rate >= 1.0:
            raise ValueError(f"Invalid growth_rate value: {growth_rate}")
        if beta3 is not None and not 0.0 <= beta3 < 1.0:
            raise ValueError(f"Invalid beta3 value: {beta3}")
        params = list(params)
        groups = [g for g in params if isinstance(g, dict)]
        if len({float(g.get("lr", lr)) for g in groups}) > 1 or len({g.get("beta3", beta3) for g in groups}) > 1:
            raise ValueError(f"{name}: lr and beta3 must be the same in every parameter group")
        return params

    def _set_prodigy_options(self, beta3, decouple, use_bias_correction, safeguard_warmup, d0, d_coef, growth_rate):
        """After `_FlatAdamW.__init__`: beta3 into the groups, the optimizer-wide options, the first shared check."""
        self.defaults["beta3"] = beta3
        for g in self.param_groups:
            g.setdefault("beta3", beta3)
        self.decouple, self.use_bias_correction = bool(decouple), bool(use_bias_correction)
        self.safeguard_warmup = bool(safeguard_warmup)
        self.d0, self.d_coef, self.growth_rate = float(d0), float(d_coef), float(growth_rate)
        self._check_shared()

    def _alloc_d_block(self) -> None:
        self._d_block = torch.tensor([self.d0] * 3 + [0.0] * 4, dtype=torch.float64).to(self._device)

    def _check_shared(self) -> Tuple[float, float]:
        """(lr, beta3) of the step: what every group must share besides the betas."""
        g0 = self.param_groups[0]
        for g in self.param_groups:
            if float(g["lr"]) != float(g0["lr"]) or g["beta3"] != g0["beta3"]:
                raise ValueError(f"{type(self).__name__}: lr and beta3 must be the same in every parameter group")
        lr = float(g0["lr"])
        beta3 = float(g0["betas"][1]) ** 0.5 if g0["beta3"] is None else float(g0["beta3"])
        if not 0.0 <= lr < float("inf"):
            raise ValueError(f"Invalid learning rate: {lr}")
        return lr, beta3

    def _finalize_args(self, lr: float, betas, beta3: float) -> dict:
        """The keyword arguments both phases of the d finaliser take."""
        return dict(lr=lr, betas=betas, beta3=beta3, d0=self.d0, d_coef=self.d_coef, growth_rate=self.growth_rate,
                    use_bias_correction=self.use_bias_correction)

    # the d block of the last step (0-dim float64 device tensors)
    @property
    def d(self) -> torch.Tensor:
        return self._d_block[0]

    @property
    def d_max(self) -> torch.Tensor:
        return self._d_block[1]

    @property
    def d_hat(self) -> torch.Tensor:
        return self._d_block[2]

    @property
    def d_numerator(self) -> torch.Tensor:
        return self._d_block[3]

    @property
    def d_denom(self) -> torch.Tensor:
        return self._d_block[4]

    @property
    def dlr(self) -> torch.Tensor:
        return self._d_block[5]

    @property
    def no_progress(self) -> torch.Tensor:
        return self._d_block.view(torch.int32)[12]

    @property
    def d_block(self) -> torch.Tensor:
        """The whole float64[7] block (N.ProdigyScalars; the last slot holds the int32 `no_progress`)."""
        return self._d_block

    def _prodigy_dict(self) -> dict:
        """The "prodigy" entry of a state dict: the d block's values and the optimizer-wide options (a device-to-host
        copy; not on the step path)."""
        block = self._d_block.cpu()
        return dict(zip(_D_FIELDS, block[:6].tolist()), no_progress=int(block.view(torch.int32)[12]),
                    decouple=self.decouple, use_bias_correction=self.use_bias_correction,
                    safeguard_warmup=self.safeguard_warmup, d0=self.d0, d_coef=self.d_coef,
                    growth_rate=self.growth_rate)

    @staticmethod
    def _prodigy_entry(state_dict) -> dict:
        if "prodigy" not in state_dict:
            raise ValueError("loaded state dict has no d block (not a FusedProdigy state dict)")
        return state_dict["prodigy"]

    def _load_prodigy_dict(self, pr: dict) -> None:
        self.decouple, self.use_bias_correction = bool(pr["decouple"]), bool(pr["use_bias_correction"])
        self.safeguard_warmup = bool(pr["safeguard_warmup"])
        self.d0, self.d_coef, self.growth_rate = float(pr["d0"]), float(pr["d_coef"]), float(pr["growth_rate"])
        block = torch.tensor([float(pr[k]) for k in _D_FIELDS] + [0.0], dtype=torch.float64)
        block.view(torch.int32)[12] = int(pr["no_progress"])
        self._d_block.copy_(block.to(self._device))


class FusedProdigy(_ProdigyCore, _FlatAdamW):
    """prodigyopt.Prodigy (1.0, slice_p = 1, no FSDP) for bf16 device parameters with fp32 master weights: the
    reference's `--optimizer prodigy`.  Its distance estimate is built from p0 - p, which on bf16 parameters is mostly
    rounding noise; here p is the fp32 master.

    State lives in five flat fp32 device buffers (master, exp_avg, exp_avg_sq, s, p0 — the initial master);
    `state[p]` exposes per-parameter views of them plus the shared device step counter.  d, d_max, d_hat,
    d_numerator, d_denom and the dlr of the last step are doubles in a device block (`d_block`, N.ProdigyScalars; the
    reference keeps them in Python floats), read through the properties of the same names; `no_progress` is 1 after
    a step that found d_denom == 0.  `step()` is gradient norm, its finaliser, dlr from the old d, pass 1 per group
    (moments, s, one (dot, sum |s|) pair per chunk), the d update, pass 2 per group (the update with the new d in
    d * eps) — no device-to-host copy, no synchronisation, bit-identical run to run.

    `max_grad_norm`, `skip_nonfinite` and `zero_grads` mean what they mean on `FusedAdamW`; a skipped step leaves all
    five buffers, the d block and the counter as they were.

    Differences from prodigyopt's: lr, betas and beta3 must be the same in every parameter group, checked every step
    (prodigyopt also lets a group sit at lr = 0; that is not built), weight_decay and eps may differ; one step
    counter; decouple, use_bias_correction, safeguard_warmup, d0, d_coef and growth_rate belong to the optimizer, not
    to a group; a step with d_denom == 0 changes no parameter, not the counter and nothing of the d block but d_denom
    and `no_progress` (the moments and s were updated, as there); parameters must be bf16, contiguous, on one
    device; slice_p and fsdp_in_use do not exist."""

    def __init__(self, params, lr: float = 1.0, betas=(0.9, 0.999), beta3: Optional[float] = None, eps: float = 1e-8,
                 weight_decay: float = 0.0, decouple: bool = True, use_bias_correction: bool = False,
                 safeguard_warmup: bool = False, d0: float = 1e-6, d_coef: float = 1.0,
                 growth_rate: float = float("inf"), *, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, zero_grads: bool = False):
        params = self._check_prodigy_args("FusedProdigy", params, lr, beta3, d0, d_coef, growth_rate)
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, skip_nonfinite, zero_grads)
        self._set_prodigy_options(beta3, decouple, use_bias_correction, safeguard_warmup, d0, d_coef, growth_rate)
        self._alloc_scalars()
        self._alloc_d_block()
        self._master = torch.zeros(max(self.total, 1), device=self._device, dtype=torch.float32)
        self._exp_avg = torch.zeros_like(self._master)
        self._exp_avg_sq = torch.zeros_like(self._master)
        self._s = torch.zeros_like(self._master)
        self._tables = MultiTensorTables(self._device)
        self._pairs = None  # fp32 [2 * chunks]: pass 1's (dot, sum |s|) of every chunk
        with torch.no_grad():
            for p in self._params:
                o, n = self._offs[p], p.numel()
                self._master[o:o + n].copy_(p.detach().reshape(-1))
            self._p0 = self._master.clone()
            for p in self._params:
                o, n = self._offs[p], p.numel()
                self.state[p] = dict(step=self._scalars[3], **{k: getattr(self, "_" + k)[o:o + n].view(p.shape)
                                                               for k in _PRODIGY_KEYS})

    @torch.no_grad()
    def step(self, closure=None):
        from . import kernels as K
        loss, betas = self._begin_step(closure)
        lr, beta3 = self._check_shared()
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        t = self._tables
        use_clip = self.max_grad_norm is not None
        fin = self._finalize_args(lr, betas, beta3)
        with torch.cuda.device(self._device):
            accumulated = self._pending > 0
            if accumulated:  # the gradient of the step is the accumulator: the fp32 mean of the micro-batches
                self._last_fold(K)
            else:
                t.update([p.grad for p in params], params, [self._offs[p] for p in params])
            if self._pairs is None or self._pairs.numel() < 2 * t.n_chunks:
                self._pairs = torch.empty(max(2 * t.n_chunks, 2048), device=self._device, dtype=torch.float32)
            if accumulated:
                K.mt_grad_sqnorm_f32(t.tensors, t.chunks, t.n_chunks, self._acc, t.partials, t.flags)
            else:
                K.mt_grad_sqnorm(t.tensors, t.chunks, t.n_chunks, t.partials, t.flags)
            K.optim_finalize(t.partials, t.flags, t.n_chunks, self._scalars, max_norm=self.max_grad_norm or 0.0,
                             betas=betas, skip_nonfinite=self.skip_nonfinite, advance_step=True)
            K.prodigy_finalize(0, None, 0, self._scalars, self._d_block, **fin)
            runs, first = [], 0
            for group in self.param_groups:  # the active tensors of a group are one run of the list
                n = sum(p.grad is not None for p in group["params"])
                runs.append((group, *t.chunks_of(first, n)))
                first += n
            for group, c0, nc in runs:
                moments = dict(betas=betas, beta3=beta3,
                               weight_decay=0.0 if self.decouple else float(group["weight_decay"]), d0=self.d0,
                               safeguard_warmup=self.safeguard_warmup, use_clip=use_clip)
                state = (self._master, self._p0, self._exp_avg, self._exp_avg_sq, self._s, self._pairs,
                         self._scalars, self._d_block)
                if accumulated:
                    K.mt_prodigy_moments_f32(t.tensors, t.chunks, c0, nc, self._acc, *state, **moments)
                else:
                    K.mt_prodigy_moments(t.tensors, t.chunks, c0, nc, *state, **moments)
            K.prodigy_finalize(1, self._pairs, t.n_chunks, self._scalars, self._d_block, **fin)
            for group, c0, nc in runs:
                K.mt_prodigy_update(t.tensors, t.chunks, c0, nc, self._master, self._exp_avg, self._exp_avg_sq,
                                    self._scalars, self._d_block, eps=float(group["eps"]),
                                    weight_decay=float(group["weight_decay"]) if self.decouple else 0.0,
                                    zero_grads=self.zero_grads and not accumulated)  # (the last fold zeroed them)
        return loss

    def state_dict(self):
        """{"state": {index: {master, exp_avg, exp_avg_sq, s, p0}}, "param_groups": [...], "step": int, "prodigy":
        {the d block's values and the optimizer-wide options}} — clones; reading the step counter and the d block are
        the device-to-host copies of this class (not on the step path)."""
        self._no_pending("state_dict")
        state = {i: {k: self.state[p][k].detach().clone() for k in _PRODIGY_KEYS}
                 for i, p in self._indexed() if p in self._offs}
        return {"state": state, "param_groups": self._groups_dict(), "step": int(self._scalars[3].item()),
                "prodigy": self._prodigy_dict()}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        self._no_pending("load_state_dict")
        self._check_groups(state_dict)
        pr = self._prodigy_entry(state_dict)
        for p, s in self._full_state(state_dict, _PRODIGY_KEYS):
            for k in _PRODIGY_KEYS:
                self.state[p][k].copy_(s[k])
        self._restore_options(state_dict)
        self._load_prodigy_dict(pr)
