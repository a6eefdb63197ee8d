"""The attention module and the two CogVideoX attention processors, on the HIP kernels.

Secondary drop-in boundary: `Attention.set_processor` / `set_attn_processor` and the processor
call signature `(attn, hidden_states, encoder_hidden_states, attention_mask=None, resample_mask=None,
image_rotary_emb=None, prev_hidden_states=None, prev_clip_weight=None, prev_resample_mask=None)
-> (hidden_states, encoder_hidden_states)` of DF/models/attention_processor.py:2107-2118 / :2223-2234.
The processors work on any `attn` object exposing to_q/to_k/to_v/to_out[0]/norm_q/norm_k/heads (ours, or a
reference `Attention` holding bf16 device weights).

`attend()` is the fused core (QKV projection -> qk-LN + RoPE -> flash attention, everything before to_out); the
block calls it directly so that to_out runs as one GEMM with the gated residual fused in its epilogue; `_qkv` is its
projection step alone (all a backward that kept its attention output recomputes of it).
"""
from __future__ import annotations

import inspect
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _native as NAT
from . import kernels as K
from .lora import AugmentedProjection, augmented_rows
from .modules import Dropout, LayerNorm, Linear

BF16 = torch.bfloat16


# Python-side A/B switches, read from the environment once at import (as the library's knob table is at load) and
# changed only through set_switch (tests/conftest.py `knobs`): VP_NO_QKV_FUSION=1 (separate qk-norm launches),
# VP_ATTN_BOUNDED=0 (no score-bound flag), VP_RESAMPLE_PARTITION / _NULLMASS / _K2_STRIDED=0 (resample-processor forms)
SWITCHES = {k: os.environ.get(k) for k in ("VP_NO_QKV_FUSION", "VP_ATTN_BOUNDED", "VP_RESAMPLE_PARTITION",
                                           "VP_RESAMPLE_NULLMASS", "VP_RESAMPLE_K2_STRIDED")}


def set_switch(name: str, value: Optional[str]) -> Optional[str]:
    """Set (value None: unset) one of SWITCHES; returns the previous value."""
    if name not in SWITCHES:
        raise KeyError(f"unknown switch {name}")
    prev = SWITCHES[name]
    SWITCHES[name] = value
    return prev


def _sw(name: str, default: str) -> str:
    v = SWITCHES[name]
    return default if v is None else v


class RopeTables(tuple):
    """(cos, sin) fp32 [F*Hh*Ww, 64] on the device, plus the video grid (F, Hh, Ww) they were built for when the
    transformer's forward knows it (None otherwise): the resample processor needs the grid to sum its null keys in
    closed form (kernels.null_key_mass)."""
    grid = None


def _rope_dev(rope, device, grid=None):
    if rope is None:
        return None
    cos, sin = rope
    if cos.device != device or cos.dtype != torch.float32 or not cos.is_contiguous():
        cos = cos.to(device=device, dtype=torch.float32).contiguous()
    if sin.device != device or sin.dtype != torch.float32 or not sin.is_contiguous():
        sin = sin.to(device=device, dtype=torch.float32).contiguous()
    out = RopeTables((cos, sin))
    out.grid = tuple(grid) if grid is not None else getattr(rope, "grid", None)
    return out


def _u8(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A token mask as contiguous uint8 (the kernels test a byte for non-zero).  An already contiguous uint8 mask is
    returned as is — the same tensor — so the per-forward mask plan (_mask_plan, keyed on the tensor) is built once
    and found by every layer."""
    if mask is None:
        return None
    if mask.dtype == torch.uint8 and mask.is_contiguous():
        return mask
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    return (mask != 0).to(torch.uint8).contiguous()


class Attention(nn.Module):
    """Parameter layout of the reference `Attention` as CogVideoXBlock builds it (attention_processor.py:96-264:
    qk_norm="layer_norm" eps 1e-6, bias=True, out_bias=True, scale = dim_head**-0.5)."""

    def __init__(self, query_dim: int, dim_head: int = 64, heads: int = 8, bias: bool = True, out_bias: bool = True,
                 eps: float = 1e-6, processor=None):
        super().__init__()
        self.inner_dim = dim_head * heads
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        self.is_cross_attention = False
        self.norm_q = LayerNorm(dim_head, eps=eps)
        self.norm_k = LayerNorm(dim_head, eps=eps)
        self.to_q = Linear(query_dim, self.inner_dim, bias=bias)
        self.to_k = Linear(query_dim, self.inner_dim, bias=bias)
        self.to_v = Linear(query_dim, self.inner_dim, bias=bias)
        self.to_out = nn.ModuleList([Linear(self.inner_dim, query_dim, bias=out_bias), Dropout()])
        self.set_processor(processor if processor is not None else CogVideoXAttnProcessor2_0())

    def set_processor(self, processor) -> None:
        self.processor = processor

    def get_processor(self, return_deprecated_lora: bool = False):
        return self.processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **cross_attention_kwargs):
        # kwargs the processor does not declare are dropped, as in the reference (:479-488)
        params = set(inspect.signature(self.processor.__call__).parameters.keys())
        kw = {k: v for k, v in cross_attention_kwargs.items() if k in params}
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                              attention_mask=attention_mask, **kw)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """bf16 [B, N, D] rows with a contiguous last dim, at any row stride (the first columns of an x_aug buffer,
    lora.augmented_rows, stay in place)."""
    t = t.to(BF16)
    return t if t.stride(-1) == 1 else t.contiguous()


def keeps_all(keep: Optional[dict]) -> bool:
    """A forward's `keep` dict (CogVideoXBlock.forward_joint) is at the level "all"."""
    return keep is not None and keep["level"] == "all"


def _qkv(attn, x: torch.Tensor, norm_rope=None, keep: Optional[dict] = None) -> torch.Tensor:
    """The fused QKV projection; with norm_rope = (text_len, rope) q and k leave the GEMM already through norm_q /
    norm_k and RoPE (the epilogue EPI_BIAS_QKNORM_ROPE: bit-equal to the GEMM + vp_head_norm_rope_bf16 on each).
    keep, at the level "all", receives views of what the GEMM wrote under the names the backward reads them by
    (autograd): "v", the pre-norm "qpre" / "kpre" — the output's columns, or with norm_rope those of the fused
    epilogue's aux output (requested then only) beside the normed + rotated "q" / "k" — and, with train, the operand
    the GEMM read, "xq" (x, or its K-augmented form under unfused LoRA)."""
    B, Ntok, D = x.shape
    out = torch.empty(B, Ntok, 3 * attn.inner_dim if hasattr(attn, "inner_dim") else 3 * D, device=x.device,
                      dtype=BF16)
    ws = [attn.to_q.weight, attn.to_k.weight, attn.to_v.weight]
    bs = [attn.to_q.bias, attn.to_k.bias, attn.to_v.bias]
    a = x.reshape(-1, D)
    aug = AugmentedProjection.of((attn.to_q, attn.to_k, attn.to_v))
    kw = {}
    pre = out
    if norm_rope is not None:
        text_len, rope = norm_rope
        kw = dict(epilogue=NAT.EPI_BIAS_QKNORM_ROPE, qk_norm=(attn.norm_q, attn.norm_k), rope=rope,
                  tokens_per_batch=Ntok, text_len=text_len)
        if keeps_all(keep):
            pre = torch.empty(B, Ntok, 2 * D, device=x.device, dtype=BF16)
            kw["aux"] = pre.view(B * Ntok, 2 * D)
    if aug is not None:  # LoRA adapters, unfused (lora.AugmentedProjection)
        a = aug.input(a)
        aug.gemm(a, bs, out.view(B * Ntok, -1), **kw)
    else:
        K.gemm(a, ws, bs, out.view(B * Ntok, -1), **kw)
    if keeps_all(keep):
        keep["qpre"], keep["kpre"], keep["v"] = pre[..., :D], pre[..., D:2 * D], out[..., 2 * D:]
        if pre is not out:
            keep["q"], keep["k"] = out[..., :D], out[..., D:2 * D]
        if keep["train"]:
            keep["xq"] = a
    return out


def keep_handed_qkv(attn, qkv: torch.Tensor, text_len: int, rope, keep: dict):
    """A keep-all forward (or the backward's recompute) on a pre-norm `qkv` [B, N, 3D] the block handed over (its
    MX-FP8 projection): the two norm launches of the inference path, written beside qkv instead of over it, so the
    pre-norm q | k the LayerNorm backward reads survive.  Fills "qpre" / "kpre" / "v" / "q" / "k" as `_qkv` names
    them and returns (q, k, v), normed + rotated."""
    B, Ntok, D3 = qkv.shape
    D, H = D3 // 3, attn.heads
    nq, nk = attn.norm_q, attn.norm_k
    qk = torch.empty(B, Ntok, 2 * D, device=qkv.device, dtype=BF16)
    q, k, v = qk[..., :D], qk[..., D:], qkv[..., 2 * D:]
    K.head_norm_rope(qkv[..., :D], q, H, text_len, nq.weight, nq.bias, nq.eps, rope)
    K.head_norm_rope(qkv[..., D:2 * D], k, H, text_len, nk.weight, nk.bias, nk.eps, rope)
    keep.update(qpre=qkv[..., :D], kpre=qkv[..., D:2 * D], v=v, q=q, k=k)
    return q, k, v


def _kv(attn, x: torch.Tensor) -> torch.Tensor:
    B, Ntok, D = x.shape
    out = torch.empty(B, Ntok, 2 * D, device=x.device, dtype=BF16)
    a, ws = x.reshape(-1, D), [attn.to_k.weight, attn.to_v.weight]
    aug = AugmentedProjection.of((attn.to_k, attn.to_v))
    if aug is not None:
        aug.gemm(aug.input(a), [attn.to_k.bias, attn.to_v.bias], out.view(B * Ntok, -1))
    else:
        K.gemm(a, ws, [attn.to_k.bias, attn.to_v.bias], out.view(B * Ntok, -1))
    return out


def _prev_kv(attn, prev_hidden_states, prev_clip_weight):
    """(pk, pv, w) of the prev-clip blend: the previous window's pre-norm K / V projections [B, N, D] and the weight,
    or (None, None, 0.0) — nothing projected — without previous states or with a weight of None or <= 0."""
    if prev_hidden_states is None or prev_clip_weight is None or prev_clip_weight <= 0.0:
        return None, None, 0.0
    pkv = _kv(attn, _rows(prev_hidden_states))
    D = pkv.shape[-1] // 2
    return pkv[..., :D], pkv[..., D:], float(prev_clip_weight)


def project_out(lin, o2d: torch.Tensor, out2d: torch.Tensor, **gemm_kw) -> torch.Tensor:
    """to_out.0 on [M, D] rows with any GEMM epilogue (the block's gated residual), its LoRA adapters applied
    unfused (lora.AugmentedProjection) when it carries any."""
    aug = AugmentedProjection.of((lin,))
    if aug is not None:
        return aug.gemm(aug.input(o2d), [lin.bias], out2d, **gemm_kw)
    return K.gemm(o2d, [lin.weight], [lin.bias], out2d, **gemm_kw)


def _fusable_norms(attn) -> bool:
    """norm_q / norm_k are LayerNorm(64) with bf16 affine parameters (CogVideoX's qk_norm, the fused epilogue's
    contract); env VP_NO_QKV_FUSION=1 keeps the separate vp_head_norm_rope_bf16 launches (A/B)."""
    if _sw("VP_NO_QKV_FUSION", "0") == "1":
        return False
    for ln in (getattr(attn, "norm_q", None), getattr(attn, "norm_k", None)):
        if ln is None or getattr(ln, "weight", None) is None or getattr(ln, "bias", None) is None:
            return False
        if ln.weight.numel() != 64 or ln.weight.dtype != BF16 or ln.bias.dtype != BF16:
            return False
    return True


def bounded_scores(attn) -> bool:
    """True when the qk-LayerNorm weights bound every attention score of `attn` within the kernel's exact
    no-running-max range (kernels.score_bound_log2 <= SCORE_BOUND_LOG2).  Cached per layer on the weights' storage and
    version (one host sync per weight update); env VP_ATTN_BOUNDED=0 forces the running-max kernel (A/B)."""
    if _sw("VP_ATTN_BOUNDED", "1") == "0":
        return False
    nq, nk = attn.norm_q, attn.norm_k
    key = tuple((t.data_ptr(), t._version) for t in (nq.weight, nq.bias, nk.weight, nk.bias)) + (float(attn.scale),)
    cached = getattr(attn, "_vp_score_bound", None)
    if cached is None or cached[0] != key:
        cached = (key, K.score_bound_log2(nq, nk, float(attn.scale)) <= K.SCORE_BOUND_LOG2)
        attn._vp_score_bound = cached
    return cached[1]


def cfg_shared_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int,
                         text_len: int, *, scale: float, bounded_scores: bool = False) -> torch.Tensor:
    """Joint self-attention of two batch rows whose video rows (tokens >= text_len) are the same and whose text rows
    differ — the classifier-free-guidance halves in a model's first block.  q / k / v / out: [2, N, heads*64] views;
    of q / k / v only batch 0 and batch 1's text rows are read.  The softmax over the joint keys is composed from
    pieces over disjoint key sets (CogVideoXBlock._attend_cfg_shared): the video x video part once instead of twice."""
    T = text_len
    B, N, D = q.shape
    if B != 2 or not 0 < T < N:
        raise ValueError(f"cfg_shared_attention needs two batch rows with text and video rows, got {tuple(q.shape)}")
    Nv = N - T
    dev = q.device
    qv, kv, vv = q[:1, T:], k[:1, T:], v[:1, T:]  # batch 0's video rows
    kw = dict(scale=scale, bounded_scores=bounded_scores)
    # (a) video queries x video keys, once
    # (the partials stay fp32: the merge rounds to bf16 once, as a single call does)
    o_v = torch.empty(1, Nv, D, device=dev, dtype=torch.float32)
    lse_v = torch.empty(1, heads, Nv, device=dev, dtype=torch.float32)
    K.attention(qv, kv, vv, o_v, heads, lse=lse_v, **kw)
    # (b) the same queries x each half's text keys
    o_t = torch.empty(2, Nv, D, device=dev, dtype=torch.float32)
    lse_t = torch.empty(2, heads, Nv, device=dev, dtype=torch.float32)
    K.attention(qv.expand(2, -1, -1), k[:, :T], v[:, :T], o_t, heads, lse=lse_t, **kw)
    # (c) each half's text queries x (own text keys | the shared video keys)
    K.attention(q[:, :T], k[:, :T], v[:, :T], out[:, :T], heads, k2=kv.expand(2, -1, -1), v2=vv.expand(2, -1, -1),
                **kw)
    # (d) video rows of both halves = merge of (a) and (b)
    K.attention_merge(o_v.expand(2, -1, -1), lse_v.expand(2, -1, -1), o_t, lse_t, out[:, T:], heads)
    return out


class CogVideoXAttnProcessor2_0:
    """HIP restatement of `CogVideoXAttnProcessor2_0.__call__` (attention_processor.py:2107-2209)."""

    def attend(self, attn, x: torch.Tensor, text_len: int, image_rotary_emb=None, prev_hidden_states=None,
               prev_clip_weight=None, resample_mask=None, prev_resample_mask=None,
               qkv: Optional[torch.Tensor] = None, keep: Optional[dict] = None) -> torch.Tensor:
        """keep: a dict that receives the attention output "o" and its softmax statistics "lse" (fp32 [B, H, N]) —
        a training forward keeps them for the backward (autograd.SAVE_ATTENTION) — and at the level "all" what the
        projection keeps (_qkv; of a handed-over `qkv`, the block's fp8 projection: keep_handed_qkv); the
        single-segment bf16 attention only."""
        B, Ntok, D = x.shape
        H = attn.heads
        rope = _rope_dev(image_rotary_emb, x.device)
        fp8 = getattr(attn, "fp8_qk_exp", None)
        if keep is not None and (fp8 is not None or prev_hidden_states is not None):
            raise ValueError("keep: the single-segment bf16 attention only")
        # (the pre-norm q | k a keep-all forward stores are the fused epilogue's second output: it runs that epilogue
        # whatever VP_NO_QKV_FUSION says — the same bits as the separate launches)
        fused = qkv is None and fp8 is None and (keeps_all(keep) or _fusable_norms(attn))
        if qkv is None:  # (the block may hand over an fp8 projection)
            qkv = _qkv(attn, x, (text_len, rope) if fused else None, keep)
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        if not fused and keeps_all(keep):  # (a handed-over qkv: the norms out of place, the same launches otherwise)
            q, k, v = keep_handed_qkv(attn, qkv, text_len, rope, keep)
            fused = True
        if fp8 is None:
            o = augmented_rows((attn.to_out[0],), B, Ntok, D, x.device)
            lse = None
            if keep is not None:
                keep["o"], keep["lse"] = o, torch.empty(B, H, Ntok, device=x.device, dtype=torch.float32)
                lse = keep["lse"]
            return self.attend_heads(attn, q, k, v, text_len, rope, None, None, fused,
                                     *_prev_kv(attn, prev_hidden_states, prev_clip_weight), o, lse=lse)
        # fp8 attention (BASELINE config 5): qk-norm + RoPE written as e4m3 with the static power-of-two factors
        # chosen by `CogVideoXBlock.enable_fp8_attention` (Q's includes scale * log2 e), V packed to e4m3 V^T with
        # per-(d, 32 keys) scales, the block-scaled MFMA kernel
        q_exp, k_exp = fp8
        nq, nk = attn.norm_q, attn.norm_k
        q8 = K.head_norm_rope_fp8(q, H, text_len, nq.weight, nq.bias, nq.eps, rope,
                                  attn.scale * K.LOG2E * 2.0 ** q_exp)
        k8 = K.head_norm_rope_fp8(k, H, text_len, nk.weight, nk.bias, nk.eps, rope, 2.0 ** k_exp)
        return self.attend_heads_fp8(attn, q8, k8, v, text_len, rope,
                                     lambda: _prev_kv(attn, prev_hidden_states, prev_clip_weight),
                                     augmented_rows((attn.to_out[0],), B, Ntok, D, x.device))

    def attend_heads_fp8(self, attn, q8, k8, v, text_len: int, rope, prev, o) -> torch.Tensor:
        """The fp8 attention on operands quantised already: q8 / k8 e4m3 [B, Nq, h*64] / [B, N, h*64] (the bytes of
        `head_norm_rope_fp8` with the factors of `attn.fp8_qk_exp`), v bf16 [B, N, h*64] — views at any row and batch
        stride of every head, or of one head group (the Ulysses split, ulysses.py: views of its receive buffer; q8 may
        carry the last shard's padding rows past k8's N).  prev() -> (pk, pv, w): the previous window's pre-norm K / V
        projections on the same heads and the blend weight (`_prev_kv`'s return), asked for after this window's V is
        packed (the unsplit launch order: the pack, then the previous window's projection); o: the bf16 output
        [B, Nq, h*64], at any strides too.  text_len / rope: of the N rows (the previous window's keys are quantised
        here)."""
        H = k8.shape[-1] // 64
        q_exp, k_exp = attn.fp8_qk_exp
        nk = attn.norm_k

        def operands(k_, v_):
            return (K.head_norm_rope_fp8(k_, H, text_len, nk.weight, nk.bias, nk.eps, rope, 2.0 ** k_exp),
                    K.v_pack_fp8(v_, H))

        def attention(k_, v_, **kw):
            K.attention_fp8(q8, k_, v_, o, H, q_exp, k_exp, **kw)
        own = (k8, K.v_pack_fp8(v, H))
        self._blend(own, *prev(), operands, attention)
        return o

    def head_plan(self, attn, text_len: int, rope, prev: bool, resample_mask=None, prev_resample_mask=None):
        """(m, plan, fused) of an `attend_heads` call whose caller projects q / k / v itself (the Ulysses split): this
        processor reads no token mask and plans nothing; q / k leave the QKV GEMM normed + rotated (`fused`) where the
        norms fit its epilogue.  prev: the call blends the previous window in."""
        return None, None, _fusable_norms(attn)

    def attend_heads(self, attn, q, k, v, text_len: int, rope, m=None, plan=None, fused: bool = True, pk=None,
                     pv=None, w: float = 0.0, o=None, lse=None) -> torch.Tensor:
        """The processor's bf16 attention on [B, N, h*64] views of every head (or of one head group: the Ulysses
        split, videopainter_amd/ulysses.py; q may then carry the padding rows of the last shard past k's N rows) —
        q / k normed + rotated already when `fused`, pre-norm otherwise; pk / pv: the previous window's pre-norm K / V
        projections (prev-clip blend with weight w), or None.  m / plan: the resample processor's (unused here).
        lse: the unblended call's softmax statistics."""
        H = k.shape[-1] // 64
        nq, nk, bs = attn.norm_q, attn.norm_k, bounded_scores(attn)
        if not fused:
            qn = q[:, :k.shape[1]]  # (the RoPE table ends with the real rows; no key attends a padding query)
            K.head_norm_rope(qn, qn, H, text_len, nq.weight, nq.bias, nq.eps, rope)
            K.head_norm_rope(k, k, H, text_len, nk.weight, nk.bias, nk.eps, rope)

        def operands(k_, v_):
            return K.head_norm_rope(k_, k_, H, text_len, nk.weight, nk.bias, nk.eps, rope), v_

        def attention(k_, v_, **kw):
            K.attention(q, k_, v_, o, H, scale=attn.scale, bounded_scores=bs, **kw)
        self._blend((k, v), pk, pv, w, operands, attention, **({} if lse is None else {"lse": lse}))
        return o

    @staticmethod
    def _blend(own, pk, pv, w: float, operands, attention, **alone) -> None:
        """`attention(k, v, **kw)` over this window's keys `own`, or — with the previous window's K / V projections
        pk / pv (`_prev_kv`) — the prev-clip blend (1 - w) x that + w x the attention over `operands(pk, pv)`: two
        calls into one output.  alone: the unblended call's lse."""
        if pk is None:
            attention(*own, **alone)
            return
        prev = operands(pk, pv)
        del pk, pv
        attention(*own, out_scale=1.0 - w)
        attention(*prev, out_scale=w, accumulate=True)

    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor,
                 attention_mask: Optional[torch.Tensor] = None, resample_mask: Optional[torch.Tensor] = None,
                 image_rotary_emb=None, prev_hidden_states: Optional[torch.Tensor] = None,
                 prev_clip_weight: Optional[float] = None, prev_resample_mask: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is never set on the CogVideoX path (SURVEY.md §3.2)")
        t = encoder_hidden_states.size(1)
        x = torch.cat([encoder_hidden_states, hidden_states], dim=1).to(BF16).contiguous()
        o = self.attend(attn, x, t, image_rotary_emb, prev_hidden_states, prev_clip_weight, resample_mask,
                        prev_resample_mask)
        out = torch.empty_like(o)
        project_out(attn.to_out[0], o.view(-1, o.shape[-1]), out.view(-1, o.shape[-1]))
        return out[:, t:], out[:, :t]


class CogVideoXAttnProcessor2_0_wo_text(CogVideoXAttnProcessor2_0):
    """HIP restatement of `CogVideoXAttnProcessor2_0_wo_text.__call__` (attention_processor.py:2306-2366): the
    branch's text-free mode, self-attention over the video tokens alone with RoPE on every token — `attend` with
    text_len = 0.  Without RoPE the reference never runs its attention (the call sits inside its
    `if image_rotary_emb is not None:`, :2349-2356): its head merge (:2358, `transpose(1, 2).reshape(B, -1, D)`)
    then scrambles the processor's INPUT, which goes on to to_out — restated as that exact permutation (attend)."""

    def attend(self, attn, x: torch.Tensor, text_len: int, image_rotary_emb=None, *args, **kwargs) -> torch.Tensor:
        if image_rotary_emb is not None:
            return super().attend(attn, x, text_len, image_rotary_emb, *args, **kwargs)
        # no RoPE: o[b] = x[b]^T read back as [N, D] rows (the reference's transpose + reshape of a [B, N, D] tensor);
        # the Q / K / V it computes and drops are skipped
        B, N, D = x.shape
        o = torch.empty(B, N, D, device=x.device, dtype=BF16)
        for b in range(B):
            K.transpose(x[b], out=o[b].view(D, N))
        return o

    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, image_rotary_emb=None) -> torch.Tensor:
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is never set on the CogVideoX path (SURVEY.md §3.2)")
        x = hidden_states.to(BF16).contiguous()
        o = self.attend(attn, x, 0, image_rotary_emb)
        out = torch.empty_like(o)
        project_out(attn.to_out[0], o.view(-1, o.shape[-1]), out.view(-1, o.shape[-1]))
        return out


_MASK_PLANS: dict = {}


def _mask_plan(m: torch.Tensor, text_len: int, grid):
    """(dst_rows, counts, segments) of a resample mask — the stable partition (masked rows first) and, with a grid,
    the null-key segments (kernels.mask_null_segments) — computed once per mask and reused by every layer of the
    forward (the transformer hands all blocks the same mask tensor).  Keyed on the mask's storage and version; the
    entry holds the mask, so its address is not reused while cached; an event orders a reuse on another stream."""
    key = (m.data_ptr(), m._version, tuple(m.shape), text_len, grid)
    hit = _MASK_PLANS.get(key)
    if hit is not None and hit[0] is m:
        torch.cuda.current_stream(m.device).wait_event(hit[4])
        return hit[1], hit[2], hit[3]
    dst, cnt = K.partition_rows_index(m)
    segments = None
    if grid is not None:
        segments = K.mask_null_segments(m, text_len, grid)
        # only the masked rows are segment 2 now: the null rows' copies are skipped (dst -1)
        dst = torch.where(m.bool(), dst, torch.full_like(dst, -1))
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(m.device))
    if len(_MASK_PLANS) >= 8:
        _MASK_PLANS.pop(next(iter(_MASK_PLANS)))
    _MASK_PLANS[key] = (m, dst, cnt, segments, ev)
    return dst, cnt, segments


class CogVideoXAttnProcessor2_0_resample(CogVideoXAttnProcessor2_0):
    """HIP restatement of `CogVideoXAttnProcessor2_0_resample.__call__` (attention_processor.py:2223-2304).

    The doubled K/V (cat along the sequence, :2283-2284) is not materialised: the masked copy is built once
    (LN of the zero-masked projection -> the LN bias "null key", then RoPE) and passed to the flash kernel as a
    second K/V segment."""

    def attend(self, attn, x: torch.Tensor, text_len: int, image_rotary_emb=None, prev_hidden_states=None,
               prev_clip_weight=None, resample_mask=None, prev_resample_mask=None,
               qkv: Optional[torch.Tensor] = None, keep: Optional[dict] = None) -> torch.Tensor:
        """keep: a training forward's dict (autograd._BlockFn with the closed-form resample backward on): receives
        the attention output "o" and the statistics "lse" of the two-segment launch (the null-key mass included) —
        the same launches as without it; window 0's bf16 closed-form plan only (the projection may be a handed-over
        `qkv`, the block's fp8 one: the backward recomputes the pre-norm "qpre" / "kpre" / "v" and the normed "q" /
        "k" from the same stages, autograd._TwoSegment)."""
        B, Ntok, D = x.shape
        rope = _rope_dev(image_rotary_emb, x.device)
        prev = prev_hidden_states is not None and prev_clip_weight is not None and prev_clip_weight > 0.0
        m, plan, fused = self.head_plan(attn, text_len, rope, prev, resample_mask, prev_resample_mask)
        fp8 = self.fp8_exponents(attn, plan)
        if keep is not None and (prev or fp8 is not None or plan[3] is None):
            raise ValueError("keep: window 0's bf16 attention with the null keys in closed form only")
        # (the block may hand over an fp8 projection; the fp8 form quantises from the pre-norm q / k: no fused
        # epilogue in either case)
        fused = fused and qkv is None and fp8 is None
        if qkv is None:
            qkv = _qkv(attn, x, (text_len, rope) if fused else None)
        pk, pv, w = _prev_kv(attn, prev_hidden_states, prev_clip_weight)
        o = augmented_rows((attn.to_out[0],), B, Ntok, D, x.device)
        lse = None
        if keep is not None:
            keep["o"], keep["lse"] = o, torch.empty(B, attn.heads, Ntok, device=x.device, dtype=torch.float32)
            lse = keep["lse"]
        return self.attend_heads(attn, qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], text_len, rope, m, plan,
                                 fused, pk, pv, w, o, fp8=fp8, lse=lse)

    def head_plan(self, attn, text_len: int, rope, prev: bool, resample_mask=None, prev_resample_mask=None):
        """(m, plan, fused): the token mask of the call (the previous window's when it blends that window in) as
        uint8, its `plan`, and whether q / k leave the QKV GEMM normed + rotated — with the null keys in closed form
        segment 2 holds masked rows only, and those of window 0 are rows of the normed + rotated K itself."""
        m = _u8(prev_resample_mask if prev else resample_mask)
        if m is None:
            raise ValueError("the resample processor needs resample_mask (id_pool_resample needs masks)")
        plan = self.plan(attn, m, text_len, rope)
        return m, plan, plan[3] is not None and _fusable_norms(attn)

    @staticmethod
    def fp8_exponents(attn, plan):
        """(q_exp, k_exp) when this call runs the fp8 two-segment attention: the block opted in
        (enable_fp8_attention(resample=True)), its Q / K factors are set, and the null keys are summed in closed form
        (plan[3]: grid known, RoPE separable, VP_RESAMPLE_NULLMASS not 0).  None: today's bf16 code — the k2_full
        form, a plain rope tuple at the plug-in boundary, VP_RESAMPLE_PARTITION=0."""
        if not getattr(attn, "fp8_resample", False) or plan[3] is None:
            return None
        return getattr(attn, "fp8_qk_exp", None)

    @staticmethod
    def plan(attn, m: torch.Tensor, text_len: int, rope):
        """(dst_rows, counts, segments, axes) of the token mask m [B, N] (uint8).  The second segment in partitioned
        row order: the masked rows' keys / values first, then the null keys (LN of a zeroed row = the norm_k bias,
        rotated) whose values are zero — they only add to the row sums.  The order of keys does not change
        attention.  With the video grid known and the RoPE table separable, the null keys leave the segment (k2_len
        = the masked-row count) and their row mass is summed in closed form over the grid (null_key_mass ->
        l_extra, DESIGN_LOG.md §3.0; axes = the per-axis RoPE tables); otherwise they stay as row-sum-only keys
        (k2_full).  VP_RESAMPLE_NULLMASS=0: keep them as keys; VP_RESAMPLE_PARTITION=0: original order (A/B)."""
        dst = cnt = segments = axes = None
        grid = getattr(rope, "grid", None)
        if _sw("VP_RESAMPLE_PARTITION", "1") != "0":
            axes = CogVideoXAttnProcessor2_0_resample.closed_form_axes(attn, rope)
            dst, cnt, segments = _mask_plan(m, text_len, grid if axes is not None else None)
        return dst, cnt, segments, axes

    @staticmethod
    def closed_form_axes(attn, rope):
        """The per-axis RoPE tables when `plan` sums the null keys in closed form for this rope (the grid known and
        taken by vp_null_key_mass, the table separable, a bf16 norm_k bias, neither A/B switch at 0), else None.
        Host-side only: no launch, the mask plan is not built."""
        grid = getattr(rope, "grid", None)
        if (_sw("VP_RESAMPLE_PARTITION", "1") != "0" and grid is not None and _sw("VP_RESAMPLE_NULLMASS", "1") != "0"
                and attn.norm_k.bias is not None and attn.norm_k.bias.dtype == BF16
                and K.null_key_mass_supported(grid)):
            return K.rope_axis_tables(rope, grid)
        return None

    def attend_heads(self, attn, q, k, v, text_len: int, rope, m, plan, fused: bool, pk=None, pv=None,
                     w: float = 0.0, o=None, fp8=None, lse=None) -> torch.Tensor:
        """The processor's attention on [B, N, h*64] views of every head (or of one head group: the Ulysses split,
        videopainter_amd/ulysses.py) — q / k normed + rotated already when `fused`, pre-norm otherwise; pk / pv: the
        previous window's pre-norm K / V projections (prev-clip blend with weight w), or None.  fp8: `fp8_exponents`
        (needs pre-norm q / k and the closed-form plan).  lse: fp32 [B, h, N] receiving the bf16 launch's softmax
        statistics (with the closed-form plan they include the null-key mass)."""
        B, Ntok, D = k.shape
        H = D // 64
        # (the Ulysses split's padded last shard: q / o rows past the N the mask covers are padding, left alone)
        q, o = q[:, :Ntok], (o[:, :Ntok] if o is not None else None)
        dst, cnt, segments, axes = plan
        grid = getattr(rope, "grid", None)
        if fp8 is not None:
            if fused or axes is None:
                raise ValueError("the fp8 resample attention takes pre-norm q / k and the closed-form null-key plan")
            # the two-segment fp8 kernel: both segments' keys as e4m3 with one static factor, both V as packed V^T;
            # cnt stays on the device, so segment 2's buffers have N rows and the rows past cnt[b] are never read
            q_exp, k_exp = fp8
            nq, nk = attn.norm_q, attn.norm_k
            q8 = K.head_norm_rope_fp8(q, H, text_len, nq.weight, nq.bias, nq.eps, rope,
                                      attn.scale * K.LOG2E * 2.0 ** q_exp)
            k8 = K.head_norm_rope_fp8(k, H, text_len, nk.weight, nk.bias, nk.eps, rope, 2.0 ** k_exp)
            vp = K.v_pack_fp8(v, H)
            # segment 2: the masked rows of k (window 0) or of the previous window's K projection x w, in partition
            # order; its values the same rows of v / pv x w, packed with zeros from row cnt[b] on
            k2_8 = torch.empty(B, Ntok, D, device=q.device, dtype=torch.uint8)
            K.head_norm_rope_fp8(pk if pk is not None else k, H, text_len, nk.weight, nk.bias, nk.eps, rope,
                                 2.0 ** k_exp, out=k2_8, tok_mask=m, pre_scale=w if pk is not None else 1.0,
                                 dst_rows=dst)
            v2 = torch.empty(B, Ntok, D, device=q.device, dtype=BF16)
            K.mask_scale_rows(pv if pk is not None else v, v2, m, w if pk is not None else 1.0, dst_rows=dst)
            vp2 = K.v_pack_fp8(v2, H, lens=cnt)
            # the null-key mass reads the bf16 normed + rotated queries (after q8 took the pre-norm q)
            K.head_norm_rope(q, q, H, text_len, nq.weight, nq.bias, nq.eps, rope)
            lx = K.null_key_mass(q, H, text_len, grid, nk.bias, axes, m, segments, attn.scale)
            if o is None:
                o = torch.empty(B, Ntok, D, device=q.device, dtype=BF16)
            K.attention_fp8(q8, k8, vp, o, H, q_exp, k_exp, k2=k2_8, vp2=vp2, k2_len=cnt, l_extra=lx)
            return o
        # segment 2 with the row stride of the fused QKV output (3 D): the attention kernel then streams its full tiles
        # on the same precomputed lane offsets as segment 1 (DESIGN_LOG.md §3.R4)
        # (VP_RESAMPLE_K2_STRIDED=0: contiguous k2 / v2, the general per-lane DMA path; A/B)
        if _sw("VP_RESAMPLE_K2_STRIDED", "1") != "0":
            kv2 = torch.empty(B, Ntok, 3 * D, device=q.device, dtype=BF16)
            k2, v2 = kv2[..., :D], kv2[..., D:2 * D]
        else:
            k2 = torch.empty(B, Ntok, D, device=q.device, dtype=BF16)
            v2 = torch.empty(B, Ntok, D, device=q.device, dtype=BF16)
        if pk is not None:
            K.head_norm_rope(pk, k2, H, text_len, attn.norm_k.weight, attn.norm_k.bias, attn.norm_k.eps,
                             rope, tok_mask=m, pre_scale=w, dst_rows=dst)
            K.mask_scale_rows(pv, v2, m, w, dst_rows=dst)
        elif fused:  # LN(1 . k) + RoPE of a masked row is K's row (bit-equal: the epilogue's arithmetic)
            K.mask_scale_rows(k, k2, m, 1.0, dst_rows=dst)
            K.mask_scale_rows(v, v2, m, 1.0, dst_rows=dst)
        else:
            K.head_norm_rope(k, k2, H, text_len, attn.norm_k.weight, attn.norm_k.bias, attn.norm_k.eps, rope,
                             tok_mask=m, pre_scale=1.0, dst_rows=dst)
            K.mask_scale_rows(v, v2, m, 1.0, dst_rows=dst)
        if not fused:
            K.head_norm_rope(q, q, H, text_len, attn.norm_q.weight, attn.norm_q.bias, attn.norm_q.eps, rope)
            K.head_norm_rope(k, k, H, text_len, attn.norm_k.weight, attn.norm_k.bias, attn.norm_k.eps, rope)
        if o is None:
            o = torch.empty(B, Ntok, D, device=q.device, dtype=BF16)
        if axes is not None:
            lx = K.null_key_mass(q, H, text_len, grid, attn.norm_k.bias, axes, m, segments, attn.scale)
            K.attention(q, k, v, o, H, k2=k2, v2=v2, scale=attn.scale, bounded_scores=bounded_scores(attn),
                        k2_len=cnt, l_extra=lx, lse=lse)
        else:
            K.attention(q, k, v, o, H, k2=k2, v2=v2, scale=attn.scale, bounded_scores=bounded_scores(attn),
                        k2_full=cnt, lse=lse)
        return o
