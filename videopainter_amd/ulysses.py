"""Ulysses head-parallel split of ONE clip's denoising forward over P ranks (the optional
"within one forward" row; not in the reference, whose multi-GPU story is data parallel only).

Every rank holds a contiguous shard of n = ceil(N / P) rows of the joint [B, N, D] buffer (text first, like the
single-GPU layout; the last shard zero-padded to n rows) for the whole forward: AdaLN, the fused QKV projection with
qk-norm + RoPE, to_out, the FeedForward, the gated residuals and the branch injection are row-local, so they run
unchanged on the shard (a shard's text rows are always a prefix of it: `text_len` becomes the shard's own count, the
RoPE table / injection / mask are sliced at the shard's first video row).  Only attention mixes rows:

    qkv [B, n, 3D] --all-to-all--> [B, N_pad, 3 * D/P]   (rank r receives every row of head group r)
    flash attention over the N real keys for H/P heads
    o [B, N_pad, D/P] --all-to-all--> [B, n, D]

two RCCL all-to-alls per block of 3 / 1 x n*D*2 B * (P-1)/P per rank.  The head gathers the proj_out rows
(all-gather of [B, n, 64]) and every rank unpatchifies the whole noise prediction, so the CFG / DPM step that follows
runs replicated exactly as on one GPU.  The branch runs sharded the same way and its samples stay local (the
injection of a shard's rows reads only the branch's same rows).

Communicators: `DistComm` (torch.distributed; backend "nccl" = RCCL over xGMI) and `ThreadComm`, which runs the P
ranks as P threads of one process on one GPU (same launches in the same order per rank; the exchanges are local
copies) — the single-GPU rehearsal the GPU tests use to check the split against the unsplit forward.

This module holds the communicators, the shard geometry, the two layout exchanges, the split context (`_Ctx`: the
blocks' `attend` hook and the head's row gather) and the harness views.  It holds no model forward: `branch_forward` /
`transformer_forward` call the models' own inference forwards (`_forward_infer(split=_Ctx(...))`, transformer.py /
branch.py), which shard x, slice the row-local operands and name there what the split leaves out (batched
modulations, ping-pong buffers, self-guidance, cfg_shared_video); the hook's attention is the processor's
`attend_heads` on the rank's head group.

Scope: both processors of the any-length pipeline — the standard one (config 2, the headline; with the
previous-clip blend) and the ID-resample one (config 4: window 0's masked second K / V segment, later windows' masked
previous-window K / V): the projections stay row-local, the masks and the RoPE table of the head-group attention are
the full ones — in bf16 and with any combination of the fp8 switches (`enable_fp8`, config 5), each behaving as it
does unsplit: the MX-FP8 AdaLN, projections and FeedForward are row-local and run on the shard as they are, and the
fp8 attention runs one workgroup per (batch, head, query block) over all keys, so a head group's launch computes the
bits of the whole launch.

The fp8 attention of the standard processor has an exchange of its own (`_Ctx._attend_fp8`):

    qkv [B, n, 3D] pre-norm --vp_qkv_heads_pack_fp8--> uint8 [P, n, B, 4 Dp]   (q e4m3 | k e4m3 | v bf16 per row)
    --all-to-all--> [P, n, B, 4 Dp] = q8 [B, P n, Dp], k8 / v [B, N, Dp] as strided views (`heads_fp8_views`)
    v pack + fp8 attention for H/P heads, written into the send buffer [P, n, B, Dp] through a [B, P n, Dp] view
    --all-to-all--> [P, n, B, Dp] --vp_mx_quantize_heads_bf16--> the fp8 output projection's operand [B n, D]
    (without the fp8 output projection: one re-layout to [B, n, D])

q and k are quantised on the shard with the norm kernel's own arithmetic, so the first exchange carries 4 B per
element instead of 6 (the second 2: 6 B against 8 per block), and the [n, B] order inside a chunk makes both receive
buffers the next kernel's operand as they stand — no `permute().contiguous()` on either side of either exchange.  The
previous window's K | V (prev-clip blend) and the ID-resample processor keep the bf16 pre-norm exchange: the first is
quantised on the head group, the second quantises there with the whole token masks and row permutation, which a shard
does not have (its two-segment fp8 kernel runs per head group with `enable_fp8(resample_attention=True)`).
"""
from __future__ import annotations

import threading
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.distributed as dist

from . import kernels as K
from .attention_processor import CogVideoXAttnProcessor2_0, CogVideoXAttnProcessor2_0_resample, _kv, _qkv
from .transformer import BF16, Transformer2DModelOutput

# ------------------------------------------------------------------------------------------------------------------
# communicators
# ------------------------------------------------------------------------------------------------------------------


class DistComm:
    """RCCL over a torch.distributed group (one process per GPU)."""

    def __init__(self, group=None):
        self.group = group
        self.P = dist.get_world_size(group)
        self.rank = dist.get_rank(group)

    def all_to_all(self, rank: int, send: torch.Tensor) -> torch.Tensor:
        """send [P, ...] contiguous, chunk j for rank j -> [P, ...], chunk j from rank j."""
        out = torch.empty_like(send)
        dist.all_to_all_single(out, send, group=self.group)
        return out

    def all_gather(self, rank: int, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous()
        out = torch.empty((self.P * x.shape[0],) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
        dist.all_gather_into_tensor(out, x, group=self.group)  # (concatenated along dim 0, as gloo requires)
        return out.view((self.P,) + tuple(x.shape))


class ThreadComm:
    """P ranks emulated by P threads of one process sharing one GPU stream (tests / single-GPU rehearsal).  An
    exchange publishes each thread's buffer, waits for all P, copies its chunks, and waits again before the slots
    are reused; every copy is launched after the producers' launches, so stream order makes it correct."""

    def __init__(self, P: int):
        self.P = P
        self._slots: List[Optional[torch.Tensor]] = [None] * P
        self._bar = threading.Barrier(P)

    def all_to_all(self, rank: int, send: torch.Tensor) -> torch.Tensor:
        self._slots[rank] = send
        self._bar.wait()
        out = torch.stack([self._slots[j][rank] for j in range(self.P)])
        self._bar.wait()
        return out

    def all_gather(self, rank: int, x: torch.Tensor) -> torch.Tensor:
        self._slots[rank] = x.contiguous()
        self._bar.wait()
        out = torch.stack(list(self._slots))
        self._bar.wait()
        return out

    def run(self, fn, *args, **kw):
        """fn(rank, *args, **kw) on P threads; returns the P results (the first exception re-raised)."""
        res: List = [None] * self.P
        err: List = []

        def body(r):
            try:
                with torch.no_grad():  # (grad mode is thread-local)
                    res[r] = fn(r, *args, **kw)
            except BaseException as e:  # noqa: BLE001 - re-raised below after every thread ended
                err.append(e)
                self._bar.abort()

        ts = [threading.Thread(target=body, args=(r,)) for r in range(self.P)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if err:
            self._bar.reset()
            raise err[0]
        return res


# ------------------------------------------------------------------------------------------------------------------
# shard geometry
# ------------------------------------------------------------------------------------------------------------------

@dataclass
class Shard:
    N: int       # real joint rows
    T: int       # text rows
    P: int
    rank: int

    def __post_init__(self):
        self.n = -(-self.N // self.P)
        self.r0 = self.rank * self.n
        self.Npad = self.n * self.P
        self.valid = max(0, min(self.n, self.N - self.r0))    # real rows in this shard
        self.tl = max(0, min(self.n, self.T - self.r0))       # local text rows (a prefix of the shard)
        self.v0 = max(0, self.r0 - self.T)                    # video index of the first local video row
        self.nv = self.n - self.tl                            # local video rows (padding included)
        if self.nv == 0:
            # the whole shard is text (T >= ceil(N / P) with a small clip or a large P): the row-local kernels would
            # get zero video rows and proj_out an empty launch
            raise ValueError(f"Ulysses split: shard {self.rank} of {self.P} holds only text rows (N = {self.N}, "
                             f"T = {self.T}, {self.n} rows per shard); use fewer ranks for this clip size")

    def rows(self, x: torch.Tensor) -> torch.Tensor:
        """This shard's rows of a full [B, N, ...] tensor (zero-padded)."""
        out = torch.zeros((x.shape[0], self.n) + tuple(x.shape[2:]), device=x.device, dtype=x.dtype)
        if self.valid > 0:
            out[:, :self.valid] = x[:, self.r0:self.r0 + self.valid]
        return out

    def video_rows(self, v: torch.Tensor) -> torch.Tensor:
        """This shard's video rows of a [B, Nv, ...] tensor (zero-padded)."""
        out = torch.zeros((v.shape[0], self.nv) + tuple(v.shape[2:]), device=v.device, dtype=v.dtype)
        k = max(0, min(self.nv, v.shape[1] - self.v0))
        if k > 0:
            out[:, :k] = v[:, self.v0:self.v0 + k]
        return out

    def rope(self, rope):
        if rope is None:
            return None
        cos, sin = rope
        return tuple(self.video_rows(t.unsqueeze(0))[0].contiguous() for t in (cos, sin))


class _Ctx:
    """One rank's split context of a model forward (`_forward_infer(split=...)`): the shard geometry `sh` (fixed by
    `shard` from the embedded joint buffer), the head-parallel `attend` hook of the blocks, and the head's
    `gather_rows`.  rope_full: the whole RoPE table (with its grid) for the head-group rows, set by the forward."""

    def __init__(self, comm, rank: int):
        self.comm, self.rank = comm, rank
        self.sh = self.rope_full = None

    def shard(self, x: torch.Tensor, T: int) -> torch.Tensor:
        """This rank's rows of the whole joint buffer x [B, N, D] with T text rows (zero-padded)."""
        self.sh = Shard(x.shape[1], T, self.comm.P, self.rank)
        return self.sh.rows(x)

    def attend(self, attn, xn: torch.Tensor, text_len: int, rope, pn: Optional[torch.Tensor] = None,
               prev_clip_weight=None, resample_mask=None, prev_resample_mask=None, qkv: Optional[torch.Tensor] = None,
               mx_out: bool = False):
        """Head-parallel attention of the shard's rows with the semantics of the block's processor (its
        `attend_heads` on this rank's head group): the row-local projections run on the shard — text_len / rope are
        the shard's —, q | k | v (and the previous window's k | v, projected from pn, its normed shard rows) are
        exchanged to every row of the head group, and the attention there takes the whole RoPE table and the whole
        token masks resample_mask / prev_resample_mask [B, N].  qkv: the block's fp8 QKV projection of the shard
        (bf16, pre-norm; xn then only gives the shape); mx_out: the block's output projection is the fp8 one — the
        fp8 exchange then returns its MX-FP8 operand (an MXTensor) instead of bf16 [B, n, D]."""
        B, n, D = xn.shape
        P = self.comm.P
        if attn.heads % P:
            raise ValueError(f"{attn.heads} heads do not split {P} ways")
        Dp = D // P
        N, T = self.sh.N, self.sh.T
        prev = pn is not None and prev_clip_weight is not None and prev_clip_weight > 0.0
        w = float(prev_clip_weight) if prev else 0.0
        resample = isinstance(attn.processor, CogVideoXAttnProcessor2_0_resample)
        if not resample and getattr(attn, "fp8_qk_exp", None) is not None:
            return self._attend_fp8(attn, xn if qkv is None else qkv, qkv is None, text_len, rope, pn if prev else None,
                                    w, mx_out)
        m, plan, fused = attn.processor.head_plan(attn, T, self.rope_full, prev, resample_mask, prev_resample_mask)
        # the resample processor's fp8 form (fp8_exponents: opted in, closed-form plan) quantises on the head group,
        # from the whole masks and the row permutation: it takes pre-norm q / k, like an fp8 projection's output
        kw = dict(fp8=attn.processor.fp8_exponents(attn, plan)) if resample else {}
        fused = fused and qkv is None and kw.get("fp8") is None
        if qkv is None:
            qkv = _qkv(attn, xn, (text_len, rope) if fused else None)
        full = qkv_to_heads(self.comm, self.rank, qkv)
        del qkv
        pk, pv = self._prev_heads(attn, pn if prev else None)
        o_full = torch.zeros(B, P * n, Dp, device=xn.device, dtype=BF16)
        # (q and o with the last shard's padding rows: the standard processor attends them too, the resample one
        # leaves them alone; the keys are the N real rows)
        attn.processor.attend_heads(attn, full[..., :Dp], full[:, :N, Dp:2 * Dp], full[:, :N, 2 * Dp:], T,
                                    self.rope_full, m, plan, fused, pk, pv, w, o_full, **kw)
        del full
        return heads_to_rows(self.comm, self.rank, o_full)

    def _prev_heads(self, attn, pn: Optional[torch.Tensor]):
        """(pk, pv): the previous window's K / V of this shard's rows pn (projected here, pre-norm, bf16) -> the N
        real rows of the head group; (None, None) without pn."""
        if pn is None:
            return None, None
        Dp, N = pn.shape[-1] // self.comm.P, self.sh.N
        pkv = qkv_to_heads(self.comm, self.rank, _kv(attn, pn), parts=2)
        return pkv[:, :N, :Dp], pkv[:, :N, Dp:]

    def _attend_fp8(self, attn, x: torch.Tensor, project: bool, text_len: int, rope, pn, w: float, mx_out: bool):
        """The standard processor's fp8 attention under the split.  q and k cross the first exchange as the e4m3
        operands the kernel wants (quantised on the shard, vp_qkv_heads_pack_fp8: 4 B per element on the wire instead
        of 6) in the layout [P, n, B, 4 Dp], so the received buffer is q8 / k8 / v of every row as it stands
        (`heads_fp8_views`), the attention writes straight into the second exchange's send buffer [P, n, B, Dp], and
        with the fp8 output projection the received heads are gathered by the quantiser (vp_mx_quantize_heads_bf16):
        no re-layout copy on either side of either exchange.  x: the shard's xn (project) or its pre-norm qkv.  The
        previous window's K | V keep the bf16 exchange and are quantised on the head group."""
        comm, rank, sh = self.comm, self.rank, self.sh
        P, N, T = comm.P, sh.N, sh.T
        qkv = _qkv(attn, x, None) if project else x
        B, n, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
        Dp = D // P
        q_exp, k_exp = attn.fp8_qk_exp
        send = K.qkv_heads_pack_fp8(qkv, attn.heads, P, text_len, attn.norm_q, attn.norm_k, rope,
                                    attn.scale * K.LOG2E * 2.0 ** q_exp, 2.0 ** k_exp)
        del qkv, x
        q8, k8, v = heads_fp8_views(comm.all_to_all(rank, send), N)
        del send
        o_send = torch.zeros(P, n, B, Dp, device=q8.device, dtype=BF16)
        attn.processor.attend_heads_fp8(attn, q8, k8, v, T, self.rope_full, lambda: self._prev_heads(attn, pn) + (w,),
                                        o_send.view(P * n, B, Dp).transpose(0, 1))
        del q8, k8, v
        recv = comm.all_to_all(rank, o_send)                                          # [P(head group), n, B, Dp]
        if mx_out:
            return K.mx_quantize_heads(recv, out=K.MXTensor(B * n, D, recv.device, zero=False))
        return recv.permute(2, 1, 0, 3).reshape(B, n, D)

    def gather_rows(self, proj: torch.Tensor, B: int) -> torch.Tensor:
        """The head's exchange: this rank's proj_out rows [B * nv, pc] -> every video row [B * Nv, pc], on every
        rank."""
        sh, P = self.sh, self.comm.P
        pc = proj.shape[-1]
        pad = torch.zeros(B, sh.n, pc, device=proj.device, dtype=BF16)
        pad[:, :sh.nv] = proj.view(B, sh.nv, pc)
        allp = self.comm.all_gather(self.rank, pad)                                   # [P, B, n, pc]
        rows = [allp[j, :, :Shard(sh.N, sh.T, P, j).nv] for j in range(P)]
        return torch.cat(rows, 1)[:, :sh.N - sh.T].reshape(-1, pc).contiguous()


def qkv_to_heads(comm, rank: int, qkv: torch.Tensor, parts: int = 3) -> torch.Tensor:
    """This shard's rows of q|k|v [B, n, 3D] (parts = 3; k|v: 2) -> every row of head group `rank`:
    [B, P n, parts * Dp]."""
    B, n, Dn = qkv.shape
    P = comm.P
    Dp = Dn // parts // P
    send = qkv.reshape(B, n, parts, P, Dp).permute(3, 0, 1, 2, 4).contiguous()  # [P(head group), B, n, parts, Dp]
    recv = comm.all_to_all(rank, send)                                            # [P(row shard), B, n, parts, Dp]
    return recv.permute(1, 0, 2, 3, 4).reshape(B, P * n, parts * Dp)


def heads_to_rows(comm, rank: int, o_full: torch.Tensor) -> torch.Tensor:
    """Head group `rank` of every row [B, P n, Dp] -> this shard's rows of all heads [B, n, P Dp]."""
    B, Npad, Dp = o_full.shape
    P = comm.P
    n = Npad // P
    send = o_full.view(B, P, n, Dp).permute(1, 0, 2, 3).contiguous()          # [P(row shard), B, n, Dp]
    recv = comm.all_to_all(rank, send)                                          # [P(head group), B, n, Dp]
    return recv.permute(1, 2, 0, 3).reshape(B, n, P * Dp)


def heads_fp8_views(recv: torch.Tensor, N: int):
    """The fp8 exchange's receive buffer uint8 [P, n, B, 4 Dp] (row shard, row, batch; per row q e4m3 | k e4m3 |
    v bf16 of this rank's head group, kernels.qkv_heads_pack_fp8) as the attention's operands, without a copy:
    q8 uint8 [B, P n, Dp] (every row, the last shard's padding included), k8 uint8 [B, N, Dp] and v bf16 [B, N, Dp]
    (the N real rows) — views with a row stride of B * 4 Dp bytes and a batch stride of 4 Dp bytes."""
    P, n, B, W = recv.shape
    if recv.dtype != torch.uint8 or not recv.is_contiguous() or W % 256:
        raise ValueError(f"recv must be contiguous uint8 [P, n, B, 4 Dp] with whole heads, got {tuple(recv.shape)}")
    Dp = W // 4
    rows = recv.view(P * n, B, W).transpose(0, 1)
    return rows[..., :Dp], rows[:, :N, Dp:2 * Dp], rows[:, :N, 2 * Dp:].view(BF16)


def _check(model):
    for blk in model.transformer_blocks:
        if type(blk.attn1.processor) not in (CogVideoXAttnProcessor2_0, CogVideoXAttnProcessor2_0_resample):
            raise NotImplementedError("the head-parallel split runs the standard and ID-resample processors")


# ------------------------------------------------------------------------------------------------------------------
# sharded forwards: the models' own inference forwards (`_forward_infer`) with this rank's split context
# ------------------------------------------------------------------------------------------------------------------

def branch_forward(branch, comm, rank: int, hidden_states, encoder_hidden_states, branch_cond, timestep,
                   image_rotary_emb=None, conditioning_scale: float = 1.0) -> List[torch.Tensor]:
    """CogvideoXBranchModel.forward on one shard: returns the samples as this shard's video rows [B, nv, D]."""
    _check(branch)
    inputs = branch._inputs(hidden_states, encoder_hidden_states, branch_cond, timestep, image_rotary_emb)
    return branch._forward_infer(*inputs, float(conditioning_scale), split=_Ctx(comm, rank))


def transformer_forward(model, comm, rank: int, hidden_states, encoder_hidden_states, timestep,
                        image_rotary_emb=None, branch_block_samples=None, branch_block_masks=None,
                        add_first: bool = False, return_hidden_states: bool = False,
                        id_pool_resample_learnable: bool = False, prev_hidden_states=None,
                        prev_clip_weight: Optional[float] = None, prev_resample_mask=None,
                        return_resample_mask: bool = False):
    """CogVideoXTransformer3DModel.forward on one shard.  `branch_block_samples` are the branch's shard samples
    (`branch_forward` on the same rank).  Returns the full noise prediction on every rank (and this shard's hidden
    states when asked: [B, n, D] each; with return_resample_mask too, the full bool [B, N] mask).  The any-length
    pipeline's window hand-off (anyl.py:962-988): prev_hidden_states = the previous window's shard hidden states
    ({layer: [B, n, D]}, what this function returned for it), prev_clip_weight, and prev_resample_mask = the full
    [B, N] mask the previous window returned.  No self-guidance and no cfg_shared_video under the split."""
    _check(model)
    out, hs_list, mask = model._forward_infer(
        hidden_states, encoder_hidden_states, timestep, image_rotary_emb,
        (prev_hidden_states, prev_clip_weight, prev_resample_mask), branch_block_samples, branch_block_masks, add_first,
        return_hidden_states=return_hidden_states, return_resample_mask=return_resample_mask,
        id_pool_resample_learnable=id_pool_resample_learnable, split=_Ctx(comm, rank))
    if not return_hidden_states:
        return (out,)
    return (out, hs_list, mask) if return_resample_mask else (out, hs_list)


class UlyssesModels:
    """The pair (transformer, branch) behind the harness's call forms, split head-parallel over `comm` (this process
    = rank `rank`).  Pass `.transformer` / `.branch` to `CogVideoXI2VDualInpaintAnyLHarness` in place of the models."""

    def __init__(self, transformer, branch, comm, rank: Optional[int] = None):
        self.comm = comm
        self.rank = comm.rank if rank is None else rank
        self.transformer = _TransformerView(transformer, self)
        self.branch = _BranchView(branch, self)


class _BranchView:
    def __init__(self, model, owner):
        self.model, self.o = model, owner
        self.config = model.config

    def __call__(self, hidden_states, encoder_hidden_states, branch_cond, timestep, image_rotary_emb=None,
                 conditioning_scale=1.0, attention_kwargs=None, return_dict=True, **_):
        outs = branch_forward(self.model, self.o.comm, self.o.rank, hidden_states, encoder_hidden_states,
                              branch_cond, timestep, image_rotary_emb, conditioning_scale)
        return (outs,)


class _TransformerView:
    def __init__(self, model, owner):
        self.model, self.o = model, owner
        self.config = model.config
        self.proj_out = model.proj_out

    def __call__(self, hidden_states, encoder_hidden_states, timestep, image_rotary_emb=None, attention_kwargs=None,
                 branch_block_samples=None, branch_block_masks=None, add_first=False,
                 id_pool_resample_learnable=False, return_hidden_states=False, return_resample_mask=False,
                 return_dict=True, **_):
        # the per-call LoRA scale (attention_kwargs["scale"], default 1.0): unfused adapters take it in their
        # augmented operands (rebuilt from the live factors, so an optimizer step's updates reach them too), exactly as
        # the single-GPU forward does (transformer.py, lora.AugmentedProjection)
        self.model._call_lora_scale(attention_kwargs)
        akw = attention_kwargs or {}
        res = transformer_forward(self.model, self.o.comm, self.o.rank, hidden_states, encoder_hidden_states,
                                  timestep, image_rotary_emb, branch_block_samples, branch_block_masks, add_first,
                                  return_hidden_states, id_pool_resample_learnable, akw.get("prev_hidden_states"),
                                  akw.get("prev_clip_weight"), akw.get("prev_resample_mask"),
                                  return_resample_mask=return_resample_mask)
        if not return_hidden_states and return_dict:
            return Transformer2DModelOutput(sample=res[0])
        return res
