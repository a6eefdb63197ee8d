"""Training backward of the CogVideoX transformer + VideoPainter branch on the HIP kernels.

The caller is the reference's training step (train/train_cogvideox_inpainting_i2v_video.py:1857-1892): the branch
(trainable) runs on the noisy latents + masked-video condition, its per-block samples are injected into the frozen
42-layer transformer, the v-prediction loss is backpropagated (`accelerator.backward(loss)`) through the frozen
transformer into the branch's parameters.  Each piece is a `torch.autograd.Function` whose forward is the inference
path itself (same launches, same rounding points) and whose backward runs only native kernels:

  * `_BlockFn` — one CogVideoXBlock (cogvideox_transformer_3d.py:125-184), gradient-checkpointed.  Its forward IS
    `block.forward_joint`, with a `keep` dict that the block's stages fill (transformer.py): level "all" while the
    device has room (SAVE_ACTIVATIONS: mod1 / mod2, q | k | v normed and pre-norm, the attention output + softmax
    statistics, the gated residual, the FF1 pre-activation; with trainable parameters also the AdaLN outputs, the QKV
    operand and h), else "attention" (SAVE_ATTENTION: the attention output + statistics), else nothing.  What was not
    kept the backward recomputes with the same stages (`_block_front`: stopping after the FF front, skipping the
    attention call when its output was kept).  `block_backward` is the forward's stages in reverse, one function each:
      `_ff_bwd`           FF2 dgrad -> GELU' -> FF1 dgrad -> AdaLN2' (+ residual)
      `_attn_output_bwd`  gate1 row-scale -> to_out dgrad
      the attention form  flash-attention backward -> (LayerNorm(64) + RoPE)' for q, k: the pre-norm d(q | k | v)
      `_qkv_bwd`          fused QKV dgrad
      `_attn_input_bwd`   AdaLN1' (+ residual) -> both modulation linears' backward into the time embedding
    with the dgrad GEMMs against cached transposed weights; `_AdaLNBwd` is the AdaLN' of both sites.  Trainable blocks
    add the weight gradients (one GEMM over the token dimension per weight, `kernels.wgrad`) and the bias /
    LayerNorm-affine / modulation sums (`kernels.colsum`).  The stages hand tensors on through the kept dict and pop
    what they read last: the block's backward runs near the memory peak, and a caller's local would hold a tensor
    until the stage returned.  Everything that depends on the attention processor is one of three forms with one
    interface, chosen once per block call (`_attention_form`: `_SingleSegment`, and for the resample processor
    `_Explicit2N` or `_ClosedForm`, below).
  * `_HeadFn` — norm_final + norm_out (AdaLN, shift|scale) + proj_out + unpatchify (:613-637), input gradient only
    (the transformer is frozen in the reference's training; trainable head parameters raise).
  * `_PatchEmbedFn` (embeddings.py:400-454), `_TimeEmbedFn` (embeddings.py:729-774), `_RowLinearFn` (the branch's
    zero-initialised output linears, branch_cogvideox.py:418-426): parameter gradients (inputs are data).

Grad tensors are bf16 like the parameters (fp32 accumulation inside every kernel; the per-column sums are fp32 until
the final cast).

VideoPainterID training (train/train_cogvideox_inpainting_i2v_video_resample.py:1520-1526, 1951-1961): the blocks'
resample processor (window 0: attention over [K; LN(mask . k) + RoPE] and [V; mask . v],
attention_processor.py:2223-2304) is differentiable — the backward recomputes both segments explicitly, runs the
flash backward over all 2N keys and routes the second segment's gradients back through the masked copy (masked rows
to k / v, the null keys' to the norm_k affine) — and trainable LoRA factors on to_q / to_k / to_v / to_out.0
(`transformer.add_adapter`, lora.py) run unfused like PEFT's, on K-augmented operands (lora.AugmentedProjection):
dA = dT^T x and dB = s dy^T T from the augmented projection's gradients (dT = s dy B, T = x A^T).
With `enable_closed_form_resample_backward` (opt-in, norm_k.bias frozen) the backward differentiates the forward's
compact plan instead: the forward keeps o / lse of its two-segment launch, and with c = scale log2 e,
lse_i = log2(sum_real 2^s_ij + 2^lx_i) (lx: the null keys' closed-form mass), D_i = rowsum(dO_i o O_i):
  real keys (K's N rows + the cnt[b] masked rows behind them, attention_bwd's k_len): dS_ij = P_ij (dP_ij - D_i);
  null keys (V = 0, so dP = 0): dS_ij = -P_ij D_i, which reaches only dq — dq_i += -scale D_i G_i with
  G_i = sum_{j null} 2^(c q_i.k_j - lse_i) k_j, summed over the grid (kernels.null_key_mass_bwd) — and the norm_k
  bias, which is not built;
  dK_normed[n] = dK1[n] + dK2c[dst[n]] and dV[n] += dV2c[dst[n]] on the masked rows (kernels.gather_add_rows: a
  masked row's K2 / V2 row is the same function of the same k / v row), then ONE (LN + RoPE)' for k.
Frozen blocks on the MX-FP8 GEMMs (`enable_fp8_ffn / _qkv / _out`): the forward is the fp8 inference forward (FF1's
aux output z the one addition), and the four dgrad GEMMs — the same projections against constant weights — run on
vp_gemm_mx_fp8 too, against transposed weights quantised along the forward's output dimension (`_wt_mx`, `_qkv_t_mx`:
built at the first backward), each dY quantised after its gate row-scale (kernels.rowscale_mx), the FF2 dgrad handing
dz to the FF1 dgrad in MX (EPI_GELU_BWD_MXFP8).  FP8_DGRAD names the dgrads that do; the attention stays bf16 both ways.
Such a block is refused with a trainable base parameter or a wanted temb gradient (weight gradients and the modulation
path are bf16-only); LoRA factors on to_q / to_k / to_v / to_out.0 train on it: their forward delta runs beside the
fp8 base as low-rank bf16 launches (transformer.py), `_aug_dgrad` follows each base dgrad on the bf16 GEMM, and a
block that trains q / k / v factors keeps the to_out dgrad in bf16 (FP8_DGRAD_LORA_OFF).  All three attention forms
take the fp8 QKV / out projections of a block with adapters: their recompute reads the handed-over pre-norm qkv.
Out of scope for the backward (NotImplementedError): the fp8 attention, the previous-clip blend (windows > 0) and
`return_hidden_states` — inference-only in the reference.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import _native as NAT
from . import kernels as K
from .attention_processor import (CogVideoXAttnProcessor2_0, CogVideoXAttnProcessor2_0_resample, _qkv,
                                  bounded_scores, keep_handed_qkv, keeps_all, project_out)
from .lora import AugmentedProjection, augmented_rows, module_pairs

BF16 = torch.bfloat16
F32 = torch.float32


# ------------------------------------------------------------------------------------------------------------------
# transposed weights for the dgrad GEMMs (cached on the parameter, keyed on storage + version)
# ------------------------------------------------------------------------------------------------------------------

def _wt(w: torch.Tensor) -> torch.Tensor:
    key = (w.data_ptr(), w._version, tuple(w.shape))
    c = getattr(w, "_vp_wt", None)
    if c is None or c[0] != key:
        c = (key, K.transpose(w.detach()))
        w._vp_wt = c
    return c[1]


def _qkv_t(attn) -> torch.Tensor:
    """[D, 3D] = cat(W_q, W_k, W_v)^T: the fused QKV dgrad's weight."""
    ws = (attn.to_q.weight, attn.to_k.weight, attn.to_v.weight)
    key = tuple((w.data_ptr(), w._version) for w in ws)
    c = getattr(attn, "_vp_qkv_t", None)
    if c is None or c[0] != key:
        D = ws[0].shape[1]
        n = ws[0].shape[0]
        wt = torch.empty(D, 3 * n, device=ws[0].device, dtype=BF16)
        for s, w in enumerate(ws):
            K.transpose(w.detach(), out=wt[:, s * n:(s + 1) * n])
        c = (key, wt)
        attn._vp_qkv_t = c
    return c[1]


# The dgrad GEMMs of a block's MX-FP8 projections that run on the fp8 GEMM too: "ff2" (with GELU'), "ff1", "out",
# "qkv".  A name taken out keeps that dgrad on the bf16 GEMM against the bf16 transposed weight, while the forward
# stays fp8 (the A/B arm, and the fallback should one GEMM's e4m3 dgrad cost too much accuracy).
FP8_DGRAD = {"ff2", "ff1", "out", "qkv"}
# A block that trains LoRA factors on q / k / v keeps the to_out dgrad on the bf16 GEMM whatever FP8_DGRAD says: its
# e4m3 cost goes through the attention's backward into d(q | k | v), which those factors' gradients are sums of, and
# alone pushes them outside the 5x band of one block (5.5 - 6.4x with it, <= 4.9x without; dx, which
# averages over 3D columns more, stays inside either way).
FP8_DGRAD_LORA_OFF = {"out"}


def _out_dgrad_mx(block, train: bool) -> bool:
    """The to_out dgrad of this backward runs on the fp8 GEMM."""
    a = block.attn1
    if block.out_mx is None or "out" not in FP8_DGRAD:
        return False
    return not (train and "out" in FP8_DGRAD_LORA_OFF and AugmentedProjection.of((a.to_q, a.to_k, a.to_v)) is not None)


def _wt_mx(w: torch.Tensor) -> "K.MXTensor":
    """MX-quantise(W^T): the fp8 dgrad's weight, quantised along the forward's OUTPUT dimension (the dgrad's K) —
    another quantisation than the forward's weight, not a re-layout of it.  Cached like `_wt`."""
    key = (w.data_ptr(), w._version, tuple(w.shape))
    c = getattr(w, "_vp_wt_mx", None)
    if c is None or c[0] != key:
        c = (key, K.mx_quantize(K.transpose(w.detach())))
        w._vp_wt_mx = c
    return c[1]


def _qkv_t_mx(attn) -> "K.MXTensor":
    """MX-quantise(cat(W_q, W_k, W_v)^T) [D, 3D]: the fused QKV dgrad's fp8 weight (cached like `_qkv_t`)."""
    ws = (attn.to_q.weight, attn.to_k.weight, attn.to_v.weight)
    key = tuple((w.data_ptr(), w._version) for w in ws)
    c = getattr(attn, "_vp_qkv_t_mx", None)
    if c is None or c[0] != key:
        n = ws[0].shape[0]
        wt = torch.empty(ws[0].shape[1], 3 * n, device=ws[0].device, dtype=BF16)
        for s, w in enumerate(ws):
            K.transpose(w.detach(), out=wt[:, s * n:(s + 1) * n])
        c = (key, K.mx_quantize(wt))
        attn._vp_qkv_t_mx = c
    return c[1]


def _aug_tail_t(aug: AugmentedProjection, side: bool = False) -> torch.Tensor:
    """[R, sum out_i]: the transposed block-diagonal tail of the augmented weights — rows i r .. of projection i's
    columns hold W_aug_i[:, K:]^T = (s B_i)^T, zero elsewhere (cached on the first Linear, keyed like them).  side:
    built from the rank blocks alone (aug.tails(): the adapters beside an MX-FP8 base, which build no W_aug)."""
    ws = aug.tails() if side else aug.weights()
    key = tuple(id(l) for l in aug.lins) + aug._key() + (side,)
    owner = aug.lins[0]
    c = owner.__dict__.get("_vp_aug_tail_t")
    if c is None or c[0] != key:
        n = sum(w.shape[0] for w in ws)
        wt = torch.zeros(aug.R, n, device=ws[0].device, dtype=BF16)
        off = 0
        for i, w in enumerate(ws):
            c0 = 0 if side else aug.block_col(i)
            K.transpose(w[:, c0:c0 + aug.r], out=wt[i * aug.r:(i + 1) * aug.r, off:off + w.shape[0]])
            off += w.shape[0]
        c = (key, wt)
        owner.__dict__["_vp_aug_tail_t"] = c
    return c[1]


def _aug_dgrad(aug: AugmentedProjection, dy2: torch.Tensor, x2: Optional[torch.Tensor], out2: torch.Tensor, train: bool,
               G: "_Grads", x_aug: Optional[torch.Tensor] = None, side: bool = False) -> None:
    """Backward of the unfused-LoRA projections y_i = x_aug W_aug_i^T (lora.AugmentedProjection; segment i reads
    rank block i of T = x A_cat^T), given out2 = dy W0 (the base dgrad): out2 += dT A_cat with dT = dy W_tail
    (block i = s dy_i B_i).  With train: W0_i's gradient only when it trains (dy_i^T x), dB = s (dy_i^T T_i) from
    the GEMM over rank block i of x_aug alone, dA = dT^T x — no full [N, K + R] weight gradient for frozen bases.
    side: the adapters ran beside an MX-FP8 base projection (`_aug_tail_t`); the same launches on the same operands."""
    Kd, r = aug.K, aug.r
    M = dy2.shape[0]
    dT = torch.empty(M, aug.R, device=dy2.device, dtype=BF16)
    K.gemm(dy2, [_aug_tail_t(aug, side)], [None], dT)
    dxl = torch.empty(M, Kd, device=dy2.device, dtype=BF16)
    K.gemm(dT, [aug.a_cat_t()], [None], dxl)  # dT A_cat
    K.axpy(out2, dxl, out=out2)
    if not train:
        return
    dA = None
    row = 0
    for i, (lin, ps) in enumerate(zip(aug.lins, aug.pairs)):
        n = lin.weight.shape[0]
        dyi = dy2[:, row:row + n]
        if lin.weight.requires_grad:
            G.put(lin.weight, K.wgrad(dyi, x2))
        if any(B.requires_grad for _, B, _ in ps):
            dbt = K.wgrad(dyi, x_aug[:, Kd + i * r:Kd + (i + 1) * r])  # [n, r] = dy_i^T T_i
        o = 0
        for A, B, sc in ps:
            ra = A.shape[0]
            if B.requires_grad:
                G.put(B, dbt[:, o:o + ra].float() * sc)
            if A.requires_grad:
                if dA is None:
                    dA = K.wgrad(dT, x2)  # [R, K]
                G.put(A, dA[i * r + o:i * r + o + ra])
            o += ra
        row += n


def _dgrad(dy2: torch.Tensor, w: torch.Tensor, out2: torch.Tensor) -> torch.Tensor:
    """out = dy W for y = x W^T: the GEMM C = A B^T with B = W^T."""
    return K.gemm(dy2, [_wt(w)], [None], out2)


def _total(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 column sum over every row of a 2-D view (of a * b)."""
    return K.colsum(a, b)[0, 0]


class _Grads:
    """Collects parameter gradients (bf16, the parameter's shape) for parameters that require them."""

    def __init__(self):
        self.g: Dict[int, torch.Tensor] = {}

    def put(self, p: Optional[torch.Tensor], g: torch.Tensor) -> None:
        if p is None or not p.requires_grad:
            return
        g = g.reshape(p.shape).to(p.dtype)
        if id(p) in self.g:
            self.g[id(p)] = self.g[id(p)] + g
        else:
            self.g[id(p)] = g

    def out(self, params: Sequence[torch.Tensor]) -> List[Optional[torch.Tensor]]:
        return [self.g.get(id(p)) for p in params]


def _mod_grad(shift: torch.Tensor, scale: torch.Tensor, gate: torch.Tensor) -> torch.Tensor:
    """[B, 6D] bf16 gradient of the CogVideoXLayerNormZero modulation (shift|scale|gate|enc_shift|enc_scale|enc_gate)
    from the per-(batch, video/text) column sums [B, 2, D]."""
    B, _, D = shift.shape
    return torch.stack((shift[:, 0], scale[:, 0], gate[:, 0], shift[:, 1], scale[:, 1], gate[:, 1]), 1) \
        .reshape(B, 6 * D).to(BF16)


def _small_linear_bwd(G: _Grads, lin, x_in: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Backward of y = x_in W^T + b on a few rows (the modulation / time-embedding linears): parameter grads into G,
    returns d x_in (bf16 [rows, in])."""
    G.put(lin.weight, K.wgrad(dy, x_in))
    if lin.bias is not None:
        G.put(lin.bias, _total(dy))
    return K.linear_small(dy, _wt(lin.weight), None)


# ------------------------------------------------------------------------------------------------------------------
# the block
# ------------------------------------------------------------------------------------------------------------------

def closed_form_resample(a) -> bool:
    """The attention runs the resample processor and opted in to its closed-form backward
    (CogVideoXBlock.enable_closed_form_resample_backward)."""
    return (isinstance(a.processor, CogVideoXAttnProcessor2_0_resample)
            and bool(getattr(a, "closed_form_resample_backward", False)))


def _check_closed_form_plan(a, rope) -> None:
    """ValueError naming what keeps the forward's plan from being the closed-form one: the opt-in does not fall back
    to the explicit form.  Host-side only (no launch: the forward's trace stays the inference plan's)."""
    grid = getattr(rope, "grid", None)
    if grid is None:
        raise ValueError("the closed-form resample backward needs the video grid on the rope tables "
                         "(attention_processor._rope_dev(rope, device, grid)); the model's training forward sets it")
    if a.processor.closed_form_axes(a, rope) is None:
        raise ValueError("the closed-form resample backward needs the closed-form null-key plan: a separable RoPE "
                         "table, a grid vp_null_key_mass takes, a bf16 norm_k bias, and VP_RESAMPLE_PARTITION / "
                         "VP_RESAMPLE_NULLMASS not 0")
    if not K.null_key_mass_bwd_supported(grid):
        raise ValueError(f"the closed-form resample backward does not take the grid {tuple(grid)}")


def _closed_form_plan(a, T: int, rope, resample_mask):
    """(m, dst_rows, counts, segments, axes, grid) of the forward's compact plan (cached per mask: no launch when
    the forward built it)."""
    _check_closed_form_plan(a, rope)
    m, (dst, cnt, segments, axes), _ = a.processor.head_plan(a, T, rope, False, resample_mask)
    return m, dst, cnt, segments, axes, rope.grid


# ---- the attention's backward, per form --------------------------------------------------------------------------
# One form per block call (`_attention_form`), with one interface: `check` (what it refuses), `keep_level` (what a
# training forward may keep for it), `recompute` (fills the kept set from xn) and `backward` (the pre-norm d(q | k | v)
# from the kept set).  The kept set — a keep-all dict, filled by the forward's stages or by `_block_front` — names
# the attention's operands alike in all forms: "q" / "k" / "v" as attention_bwd reads them (normed + rotated queries,
# keys and values), the pre-norm "qpre" / "kpre", "o", "lse", and "plan" where there is one; `_attn_output_bwd` adds
# "do".

def _attention_operands(s: dict):
    """(q, k, v, o, do, lse) popped from the kept set, and a fresh d(q | k | v) [B, N, 3D]."""
    q, k, v, o, do, lse = (s.pop(n) for n in ("q", "k", "v", "o", "do", "lse"))
    B, Ntok, D = do.shape
    return q, k, v, o, do, lse, torch.empty(B, Ntok, 3 * D, device=do.device, dtype=BF16)


def _qk_norm_bwd(a, qpre, kpre, dk, dqkv: torch.Tensor, T: int, rope, train: bool):
    """(LayerNorm(64) + RoPE)' for q (in place in dqkv's q columns) and k (dk -> dqkv's k columns).  Returns the
    affine gradients' fp32 accumulators (dlnq, dlnk), (None, None) when neither norm trains."""
    D = dqkv.shape[-1] // 3
    dlnq = dlnk = None
    if train and (a.norm_q.weight.requires_grad or a.norm_k.weight.requires_grad):
        dlnq, dlnk = (tuple(torch.zeros(64, device=dqkv.device, dtype=F32) for _ in range(2)) for _ in range(2))
    K.head_norm_rope_bwd(qpre, dqkv[..., :D], dqkv[..., :D], a.heads, T, a.norm_q, rope, dlnq)
    K.head_norm_rope_bwd(kpre, dk, dqkv[..., D:2 * D], a.heads, T, a.norm_k, rope, dlnk)
    return dlnq, dlnk


def _qk_norm_grads(a, dln, G: _Grads) -> None:
    if dln[0] is not None:
        for ln, (dw, db) in zip((a.norm_q, a.norm_k), dln):
            G.put(ln.weight, dw)
            G.put(ln.bias, db)


class _AttentionForm:
    def __init__(self, a, mask=None):
        self.a, self.mask = a, mask  # the attention module; the resample processor's token mask

    def check(self, rope) -> None:
        """Raises what the form refuses beyond `_trainable_form`'s own refusals."""


class _SingleSegment(_AttentionForm):
    """The standard processor (and its text-free form): one key segment, q / k normed in the QKV GEMM's epilogue."""

    def keep_level(self, block, x: torch.Tensor, train: bool) -> Optional[str]:
        """"all" while the device has room, else the attention output + statistics (SAVE_ATTENTION), else nothing."""
        a = self.a
        qaug = AugmentedProjection.of((a.to_q, a.to_k, a.to_v)) if train else None
        if SAVE_ACTIVATIONS and _room_for(x, block.ff.net[0].proj.weight.shape[0], train,
                                          qaug.R if qaug is not None else 0):
            return "all"
        if SAVE_ATTENTION and type(a.processor) is CogVideoXAttnProcessor2_0:
            return "attention"
        return None

    def recompute(self, block, xn: torch.Tensor, T: int, rope, keep: dict, qkv=None) -> None:
        """The block's attention stage — its projection alone where the forward kept "o" / "lse".  qkv: the block's
        fp8 projection's output (xn is then any [B, N, D] tensor, for its shape)."""
        if "o" not in keep:
            block._attention(xn, T, rope, qkv=qkv, keep=keep)
        elif qkv is not None:
            keep_handed_qkv(self.a, qkv, T, rope, keep)
        else:
            _qkv(self.a, xn, (T, rope), keep)

    def backward(self, s: dict, T: int, rope, train: bool, G: _Grads) -> torch.Tensor:
        a = self.a
        q, k, v, o, do, lse, dqkv = _attention_operands(s)
        D = do.shape[-1]
        K.attention_bwd(q, k, v, o, do, lse, a.heads, scale=a.scale, dq=dqkv[..., :D], dk=dqkv[..., D:2 * D],
                        dv=dqkv[..., 2 * D:])
        del q, k, v, o, do, lse
        _qk_norm_grads(a, _qk_norm_bwd(a, s.pop("qpre"), s.pop("kpre"), dqkv[..., D:2 * D], dqkv, T, rope, train), G)
        return dqkv


class _TwoSegment(_AttentionForm):
    """The resample processor (window 0) as the backward differentiates it: keys / values as ONE buffer each,
    [B, 2N, D] — K / V in rows [0, N), the second segment behind them — so one flash backward covers both."""

    def _recompute_operands(self, xn: torch.Tensor, T: int, rope, keep: dict, second=None, qkv=None):
        """What both forms recompute alike: the pre-norm projections ("qpre" / "kpre"; `_qkv`, or the columns of a
        handed-over `qkv`, the block's fp8 projection), the buffers "q" [B, N, D] and "k" / "v" [B, 2N, D], and the q
        and K norm launches into them — after `second(k, v, kc, vc)`, the launches of a second segment built from the
        pre-norm projections.  Returns (v, kc, vc)."""
        a = self.a
        B, Ntok, D = xn.shape
        H, dev, nq, nk = a.heads, xn.device, a.norm_q, a.norm_k
        if qkv is None:
            qkv = _qkv(a, xn, None, keep)
        else:
            keep.update(qpre=qkv[..., :D], kpre=qkv[..., D:2 * D])
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        qn = torch.empty(B, Ntok, D, device=dev, dtype=BF16)
        kc = torch.empty(B, 2 * Ntok, D, device=dev, dtype=BF16)
        vc = torch.empty(B, 2 * Ntok, D, device=dev, dtype=BF16)
        if second is not None:
            second(k, v, kc, vc)
        K.head_norm_rope(q, qn, H, T, nq.weight, nq.bias, nq.eps, rope)
        K.head_norm_rope(k, kc[:, :Ntok], H, T, nk.weight, nk.bias, nk.eps, rope)
        keep.update(q=qn, k=kc, v=vc)
        return v, kc, vc


class _Explicit2N(_TwoSegment):
    """The explicit form: K2 = LN(mask . k) + RoPE (masked rows: = K's rows; null rows: the norm_k bias, rotated) and
    V2 = mask . v, all N rows of each; the second segment's gradients go back through the masked copy (masked rows
    to k / v, the null keys' to the norm_k affine)."""

    def keep_level(self, block, x, train):
        return None  # (its backward recomputes the attention over the 2N keys)

    def recompute(self, block, xn, T, rope, keep, qkv=None):
        a, nk, Ntok = self.a, self.a.norm_k, xn.shape[1]

        def second(k, v, kc, vc):
            K.head_norm_rope(k, kc[:, Ntok:], a.heads, T, nk.weight, nk.bias, nk.eps, rope, tok_mask=self.mask,
                             pre_scale=1.0)
            vc[:, :Ntok].copy_(v)
            K.mask_scale_rows(v, vc[:, Ntok:], self.mask, 1.0)
        self._recompute_operands(xn, T, rope, keep, second, qkv)
        o = augmented_rows((a.to_out[0],), *xn.shape, xn.device)
        lse = torch.empty(xn.shape[0], a.heads, Ntok, device=xn.device, dtype=F32)
        K.attention(keep["q"], keep["k"], keep["v"], o, a.heads, scale=a.scale, bounded_scores=bounded_scores(a),
                    lse=lse)
        keep.update(o=o, lse=lse)

    def backward(self, s, T, rope, train, G):
        a, mask = self.a, self.mask
        q, k, v, o, do, lse, dqkv = _attention_operands(s)
        B, Ntok, D = do.shape
        dkc, dvc = torch.empty_like(k), torch.empty_like(k)  # d "k", d "v" [B, 2N, D]
        K.attention_bwd(q, k, v, o, do, lse, a.heads, scale=a.scale, dq=dqkv[..., :D], dk=dkc, dv=dvc)
        dqkv[..., D:2 * D].copy_(dkc[:, :Ntok])
        dv2 = torch.empty(B, Ntok, D, device=do.device, dtype=BF16)
        K.mask_scale_rows(dvc[:, Ntok:], dv2, mask, 1.0)  # V2 = mask . v
        torch.add(dvc[:, :Ntok], dv2, out=dv2)
        dqkv[..., 2 * D:].copy_(dv2)
        del dvc, dv2, q, k, v, o, do, lse
        kpre = s.pop("kpre")
        dln = _qk_norm_bwd(a, s.pop("qpre"), kpre, dqkv[..., D:2 * D], dqkv, T, rope, train)
        # K2 = LN(mask . k) + RoPE: (LN + RoPE)' at the masked input, then x mask (null rows: LN of a zero row,
        # whose input gradient the mask cancels; their d beta stays in dlnk)
        km = torch.empty(B, Ntok, D, device=dqkv.device, dtype=BF16)
        K.mask_scale_rows(kpre, km, mask, 1.0)
        dkm = K.head_norm_rope_bwd(km, dkc[:, Ntok:], torch.empty(B, Ntok, D, device=km.device, dtype=BF16), a.heads,
                                   T, a.norm_k, rope, dln[1])
        K.mask_scale_rows(dkm, km, mask, 1.0)
        dqkv[..., D:2 * D].add_(km)
        _qk_norm_grads(a, dln, G)
        return dqkv


class _ClosedForm(_TwoSegment):
    """The forward's compact plan (opt-in; the module docstring has the derivation): the second segment holds the
    masked rows of K / V alone, in partition order, `cnt[b]` of them (the rows past N + cnt[b] are never read:
    attention_bwd's k_len); the null keys reach only dq, in closed form."""

    def check(self, rope) -> None:
        a = self.a
        # the null keys' dS reaches only the norm_k bias (the mask cancels the path into k): not built
        if a.norm_k.bias is not None and a.norm_k.bias.requires_grad:
            raise NotImplementedError("the closed-form resample backward builds no norm_k bias gradient: freeze "
                                      "norm_k.bias or disable it (enable_closed_form_resample_backward(False))")
        _check_closed_form_plan(a, rope)

    def keep_level(self, block, x, train):
        return "attention"  # (the two-segment launch's o / lse, the null-key mass included)

    def recompute(self, block, xn, T, rope, keep, qkv=None):
        """No attention launch (the forward kept "o" / "lse"): compact copies, as the fused forward makes them."""
        Ntok = xn.shape[1]
        keep["plan"] = m, dst, _, _, _, _ = _closed_form_plan(self.a, T, rope, self.mask)
        v, kc, vc = self._recompute_operands(xn, T, rope, keep, qkv=qkv)
        # LN(1 . k) + RoPE of a masked row is K's row, and V2 = v there
        K.mask_scale_rows(kc[:, :Ntok], kc[:, Ntok:], m, 1.0, dst_rows=dst)
        vc[:, :Ntok].copy_(v)
        K.mask_scale_rows(v, vc[:, Ntok:], m, 1.0, dst_rows=dst)

    def backward(self, s, T, rope, train, G):
        a = self.a
        m, dst, cnt, segments, axes, grid = s.pop("plan")
        q, k, v, o, do, lse, dqkv = _attention_operands(s)
        B, Ntok, D = do.shape
        dkc, dvc = torch.empty_like(k), torch.empty_like(k)  # d "k", d "v" [B, 2N, D]
        delta = torch.empty(B, a.heads, Ntok, device=do.device, dtype=F32)
        K.attention_bwd(q, k, v, o, do, lse, a.heads, scale=a.scale, dq=dqkv[..., :D], dk=dkc, dv=dvc,
                        k_len=cnt + Ntok, delta=delta)
        K.null_key_mass_bwd(q, a.heads, T, grid, a.norm_k.bias, axes, m, segments, a.scale, lse, delta, dqkv[..., :D])
        K.gather_add_rows(dkc[:, Ntok:], dkc[:, :Ntok], m, dst)
        K.gather_add_rows(dvc[:, Ntok:], dvc[:, :Ntok], m, dst)
        dqkv[..., 2 * D:].copy_(dvc[:, :Ntok])
        del dvc, delta, q, k, v, o, do, lse
        _qk_norm_grads(a, _qk_norm_bwd(a, s.pop("qpre"), s.pop("kpre"), dkc[:, :Ntok], dqkv, T, rope, train), G)
        return dqkv


def _attention_form(a, resample_mask=None):
    """The form of the attention's backward for one block call: by the processor, the mask and the opt-in."""
    if isinstance(a.processor, CogVideoXAttnProcessor2_0_resample):
        if resample_mask is None:
            raise ValueError("the resample processor needs resample_mask (id_pool_resample needs masks)")
        return (_ClosedForm if closed_form_resample(a) else _Explicit2N)(a, resample_mask)
    if resample_mask is not None:
        # (such a block's forward ignores the mask, while the backward would differentiate the resample attention)
        raise NotImplementedError("resample_mask on a block without the resample processor has no backward")
    return _SingleSegment(a)


def _mx_gemms(block) -> bool:
    """The block runs a projection on the MX-FP8 GEMM (enable_fp8_ffn / _qkv / _out)."""
    return block.ff_mx is not None or block.qkv_mx is not None or getattr(block, "out_mx", None) is not None


def _lora_factors(a) -> set:
    """ids of the unfused LoRA factors on to_q / to_k / to_v / to_out.0: what a block on the MX-FP8 GEMMs may train."""
    return {id(p) for lin in (a.to_q, a.to_k, a.to_v, a.to_out[0]) for A, B, _ in module_pairs(lin) for p in (A, B)}


def _trainable_form(block, resample_mask=None, rope=None, temb=None):
    """The attention form of a block call the backward can run; raises what it refuses.  temb: the call's time
    embedding (whether its gradient is wanted)."""
    a = block.attn1
    if getattr(a, "fp8_qk_exp", None) is not None:
        raise NotImplementedError("the backward runs the bf16 path: disable the fp8 modes for training")
    form = _attention_form(a, resample_mask)
    if _mx_gemms(block):
        # the dgrad GEMMs run against constant weights; weight gradients and the modulation path are bf16-only.  The
        # LoRA factors on the attention projections train: their low-rank backward runs on the bf16 GEMM (_aug_dgrad)
        lora = _lora_factors(a)
        if any(p.requires_grad and id(p) not in lora for p in block.parameters()):
            raise NotImplementedError("a block on the fp8 GEMMs trains no parameter of its own (its weight gradients "
                                      "are bf16-only) but LoRA factors on to_q / to_k / to_v / to_out.0: freeze the "
                                      "rest, or disable enable_fp8_ffn / _qkv / _out on it")
        if temb is not None and temb.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("a block on the fp8 GEMMs builds no time-embedding gradient (the modulation "
                                      "path is bf16-only): detach temb, or disable enable_fp8_ffn / _qkv / _out on it")
        if ((block.qkv_mx is not None or block.out_mx is not None) and not isinstance(form, _SingleSegment)
                and not lora and AugmentedProjection.of((a.to_q, a.to_k, a.to_v, a.to_out[0])) is None):
            # (as before the LoRA side path: lifted for the blocks that carry adapters, the ID training's)
            raise NotImplementedError("the fp8 QKV / output projections have no backward with the resample "
                                      "processor on a block without LoRA adapters: enable_fp8_ffn alone trains "
                                      "with it")
    form.check(rope)
    return form


# ---- the block's stages, backward --------------------------------------------------------------------------------

def _block_front(block, x: torch.Tensor, T: int, temb: torch.Tensor, rope, resample_mask, attn_saved=None,
                 with_h: bool = False, form=None) -> dict:
    """The backward's recompute: forward_joint's stages (CogVideoXBlock) up to the FF front with a keep-all dict,
    which it returns — the attention stage as `form` recomputes it (block_backward hands over the block call's;
    a caller without one gets it from resample_mask).  attn_saved: the forward's (attention output, lse); then no
    attention is launched.  with_h: FF1 runs its GELU epilogue (h, and z as its aux output: the same bits as FF1 +
    vp_gelu_bf16); without, it stores z alone.  Both modulations are computed up front."""
    if form is None:
        form = _attention_form(block.attn1, resample_mask)
    keep = dict(level="all", train=True)
    keep["mod1"], keep["mod2"] = mod1, mod2 = block.norm1.modulation(temb), block.norm2.modulation(temb)
    xn, qkv, _ = block._attn_input(x, T, mod1, keep=keep)
    if attn_saved is not None:
        keep["o"], keep["lse"] = attn_saved
    form.recompute(block, xn if xn is not None else x, T, rope, keep, qkv)
    del xn, qkv
    block._ff_front(block._attn_output(x, keep["o"], mod1, T, keep), mod2, T, keep, activate=with_h)
    return keep


class _AdaLNBwd:
    """AdaLN' at one of the block's two sites (norm2 on x_mid, norm1 on x), in the three steps both share and between
    which a site runs its own launches: the constructor adds LN'(dy (1 + scale) w) into g — with need_dmod it also
    stores the LayerNorm's output, that output's gradient and x-hat; `mod_grad` sums the modulation's gradient;
    `affine_grads` the LayerNorm weight's and bias's."""

    def __init__(self, nz, x: torch.Tensor, dy: torch.Tensor, g: torch.Tensor, T: int, mod: torch.Tensor,
                 need_dmod: bool):
        self.ln, self.dy, self.T = nz.norm, dy, T
        self.n = self.dn = self.xhat = None
        if need_dmod:
            self.n, self.dn, self.xhat = (torch.empty_like(x) for _ in range(3))
        K.adaln_bwd(x, dy, g, T, self.ln.weight, self.ln.bias, self.ln.eps, mod, n_out=self.n, dn_out=self.dn,
                    xhat_out=self.xhat)

    def mod_grad(self, gate) -> torch.Tensor:
        """[B, 6D] (_mod_grad) from the shift and scale column sums and the gate's: `gate` [B, 2, D], or the pair
        (d out, branch output) to sum it from."""
        _, Ntok, D = self.dy.shape
        kw = dict(tokens_per_batch=Ntok, text_len=self.T)
        shift = K.colsum(self.dy.view(-1, D), **kw)
        scale = K.colsum(self.dy.view(-1, D), self.n.view(-1, D), **kw)
        return _mod_grad(shift, scale, K.colsum(*gate, **kw) if isinstance(gate, tuple) else gate)

    def affine_grads(self, G: _Grads) -> None:
        D = self.dy.shape[-1]
        G.put(self.ln.weight, _total(self.dn.view(-1, D), self.xhat.view(-1, D)))
        G.put(self.ln.bias, _total(self.dn.view(-1, D)))


def _ff_bwd(block, s: dict, dout: torch.Tensor, g: torch.Tensor, T: int, mod2: torch.Tensor, need_dmod: bool,
            train: bool, G: _Grads) -> Optional[torch.Tensor]:
    """FeedForward + gated residual 2: FF2 dgrad -> GELU' -> FF1 dgrad -> AdaLN2' added into g (= dout: the residual).
    Returns the norm2 modulation's gradient (need_dmod)."""
    B, Ntok, D = dout.shape
    M = B * Ntok
    ff0, ff2 = block.ff.net[0].proj, block.ff.net[2]
    x_mid, z, xn2, h = s.pop("x_mid"), s.pop("z"), s.pop("xn2", None), s.pop("h", None)
    dout2 = dout.view(M, D)
    F4 = ff0.weight.shape[0]
    mx2, mx1 = (block.ff_mx is not None and n in FP8_DGRAD for n in ("ff2", "ff1"))
    df = None
    if mx2:
        # dY quantised after its gate row-scale, in one pass; dz stays in MX where the FF1 dgrad takes it
        dfq = K.rowscale_mx(dout2, Ntok, T, mod2, 2, 5)
        if mx1:
            dz = K.gemm_mx(dfq, [_wt_mx(ff2.weight)], [None], K.MXTensor(M, F4, dout.device, zero=False),
                           epilogue=NAT.EPI_GELU_BWD_MXFP8, z=z)
        else:
            dh = torch.empty(M, F4, device=dout.device, dtype=BF16)
            K.gemm_mx(dfq, [_wt_mx(ff2.weight)], [None], dh)
            dz = K.gelu_bwd(dh, z)
            del dh
        del dfq
    else:
        df = torch.empty(M, D, device=dout.device, dtype=BF16)
        K.rowscale(dout2, df, Ntok, T, mod2, 2, 5)
        dz = torch.empty(M, F4, device=dout.device, dtype=BF16)
        K.gemm(df, [_wt(ff2.weight)], [None], dz, epilogue=NAT.EPI_GELU_BWD, z=z)  # (df W2) * GELU'(z), one pass
        if mx1:
            dz = K.mx_quantize(dz, out=K.MXTensor(M, F4, dout.device, zero=False))
    dxn2 = torch.empty(B, Ntok, D, device=dout.device, dtype=BF16)
    if mx1:
        K.gemm_mx(dz, [_wt_mx(ff0.weight)], [None], dxn2.view(M, D))
    else:
        _dgrad(dz, ff0.weight, dxn2.view(M, D))
    ad = _AdaLNBwd(block.norm2, x_mid, dxn2, g, T, mod2, need_dmod)
    if not need_dmod:
        return None
    # h exactly as the forward made it: GELU applied in the FF1 GEMM epilogue on the fp32 accumulator (a GELU of the
    # bf16-rounded z would differ by one rounding, and so would ff2's weight and gate-2 gradients)
    if h is None:
        h = K.linear(xn2.view(M, D), ff0.weight, ff0.bias, gelu=True)
    f = torch.empty(M, D, device=dout.device, dtype=BF16)
    K.gemm(h, [ff2.weight], [ff2.bias], f)
    dmod2 = ad.mod_grad((dout2, f))
    del f
    if train:
        G.put(ff2.weight, K.wgrad(df, h))
        G.put(ff2.bias, _total(df))
        G.put(ff0.weight, K.wgrad(dz, xn2.view(M, D)))
        G.put(ff0.bias, _total(dz))
        ad.affine_grads(G)
    return dmod2


def _attn_output_bwd(block, s: dict, g: torch.Tensor, T: int, mod1: torch.Tensor, need_dmod: bool, train: bool,
                     G: _Grads) -> Optional[torch.Tensor]:
    """to_out + gated residual 1: gate-1 row-scale -> to_out dgrad, "do" into s (from its "o", which stays for the
    attention).  Returns the gate-1 column sums (need_dmod)."""
    B, Ntok, D = g.shape
    M = B * Ntok
    to_out = block.attn1.to_out[0]
    oaug = AugmentedProjection.of((to_out,))
    o2 = s["o"].view(M, D)
    side = block.out_mx is not None and oaug is not None  # (the adapter ran beside the fp8 projection)
    if _out_dgrad_mx(block, train):
        # (`_trainable_form`: the base is frozen — the dgrad, and under an adapter its low-rank backward in bf16)
        s["do"] = do = torch.empty(B, Ntok, D, device=g.device, dtype=BF16)
        if oaug is None:
            K.gemm_mx(K.rowscale_mx(g.view(M, D), Ntok, T, mod1, 2, 5), [_wt_mx(to_out.weight)], [None], do.view(M, D))
            return None
        # the gate row-scale in bf16 (the adapter's dy), quantised from there: rowscale_mx's bytes
        dao = torch.empty(M, D, device=g.device, dtype=BF16)
        K.rowscale(g.view(M, D), dao, Ntok, T, mod1, 2, 5)
        K.gemm_mx(K.mx_quantize(dao, out=K.MXTensor(M, D, g.device, zero=False)), [_wt_mx(to_out.weight)], [None],
                  do.view(M, D))
        _aug_dgrad(oaug, dao, o2, do.view(M, D), train, G, oaug.input(o2) if train else None, side=True)
        return None
    dao = torch.empty(M, D, device=g.device, dtype=BF16)
    K.rowscale(g.view(M, D), dao, Ntok, T, mod1, 2, 5)
    o_aug = gate1 = None
    if need_dmod:
        ao = torch.empty(M, D, device=g.device, dtype=BF16)
        project_out(to_out, o2, ao)
        gate1 = K.colsum(g.view(M, D), ao, tokens_per_batch=Ntok, text_len=T)
        del ao
        if train:
            if oaug is not None:
                o_aug = oaug.input(o2)
            elif to_out.weight.requires_grad:
                G.put(to_out.weight, K.wgrad(dao, o2))
            G.put(to_out.bias, _total(dao))
    if train and oaug is not None and o_aug is None:  # (a block whose modulation path is off: need_dmod False)
        o_aug = oaug.input(o2)
    do = torch.empty(B, Ntok, D, device=g.device, dtype=BF16)
    _dgrad(dao, to_out.weight, do.view(M, D))
    if oaug is not None:
        _aug_dgrad(oaug, dao, o2, do.view(M, D), train, G, o_aug, side=side)
    s["do"] = do
    return gate1


def _qkv_bwd(a, s: dict, train: bool, G: _Grads, mx: bool = False, side: bool = False) -> torch.Tensor:
    """The fused QKV projection: "dqkv" -> d xn [B, N, D], and the weight / bias / LoRA gradients.  mx: the dgrad on
    the fp8 GEMM (the base is frozen: the dgrad alone, and under adapters their low-rank backward in bf16)."""
    dqkv, xn, xq = s.pop("dqkv"), s.pop("xn", None), s.pop("xq", None)
    B, Ntok, D3 = dqkv.shape
    D, M = D3 // 3, B * Ntok
    lins = (a.to_q, a.to_k, a.to_v)
    qaug = AugmentedProjection.of(lins)
    dxn = torch.empty(B, Ntok, D, device=dqkv.device, dtype=BF16)
    if mx:
        dq8 = K.mx_quantize(dqkv.view(M, D3), out=K.MXTensor(M, D3, dqkv.device, zero=False))
        K.gemm_mx(dq8, [_qkv_t_mx(a)], [None], dxn.view(M, D))
        if qaug is not None:
            _aug_dgrad(qaug, dqkv.view(M, D3), xn.view(M, D) if train else None, dxn.view(M, D), train, G, xq, side=True)
        return dxn
    side = side and qaug is not None  # (fp8 forward, this dgrad on the bf16 GEMM: the adapters ran beside the base)
    K.gemm(dqkv.view(M, D3), [_qkv_t(a)], [None], dxn.view(M, D))
    if side:
        _aug_dgrad(qaug, dqkv.view(M, D3), xn.view(M, D) if train else None, dxn.view(M, D), train, G, xq, side=True)
        return dxn
    if train:
        db = _total(dqkv.view(M, D3))
        if qaug is None and any(l.weight.requires_grad for l in lins):
            dw = K.wgrad(dqkv.view(M, D3), xq)
            for i, lin in enumerate(lins):
                G.put(lin.weight, dw[i * D:(i + 1) * D])
        for i, lin in enumerate(lins):
            G.put(lin.bias, db[i * D:(i + 1) * D])
        if qaug is not None:
            _aug_dgrad(qaug, dqkv.view(M, D3), xn.view(M, D), dxn.view(M, D), True, G, xq)
    elif qaug is not None:
        # (no parameter gradients: x2 is not read — and a frozen block's saving forward keeps no xn)
        _aug_dgrad(qaug, dqkv.view(M, D3), None, dxn.view(M, D), False, G)
    return dxn


def _attn_input_bwd(block, x: torch.Tensor, dxn: torch.Tensor, g: torch.Tensor, T: int, temb: torch.Tensor,
                    mod1: torch.Tensor, gate1, dmod2, need_dmod: bool, want_dtemb: bool, train: bool,
                    G: _Grads) -> Optional[torch.Tensor]:
    """AdaLN1' added into g (now d x), then both modulation linears' backward into the time embedding: dtemb."""
    ad = _AdaLNBwd(block.norm1, x, dxn, g, T, mod1, need_dmod)
    if not need_dmod:
        return None
    dmod1 = ad.mod_grad(gate1)
    if train:
        ad.affine_grads(G)
    st = K.silu(temb.contiguous())
    ds = K.axpy(_small_linear_bwd(G, block.norm1.linear, st, dmod1),
                _small_linear_bwd(G, block.norm2.linear, st, dmod2))
    return K.silu_bwd(ds, temb.contiguous()) if want_dtemb else None


def block_backward(block, form, x: torch.Tensor, T: int, temb: torch.Tensor, rope,
                   inject_mask: Optional[torch.Tensor], dout: torch.Tensor, want_dtemb: bool, want_dinject: bool,
                   train: bool, attn_saved=None, front: Optional[dict] = None):
    """Gradient-checkpointed backward of `block.forward_joint(x, T, temb, rope, resample_mask=.., inject=..,
    inject_mask=..)`, the forward's stages in reverse.  Returns (dx [B, Ntok, D], dtemb or None, dinject [B, Nv, D]
    or None, _Grads).  form: the attention's (`_attention_form`); attn_saved: the forward's (attention output, lse) —
    then the attention is not recomputed; front: the training forward's keep-all dict (_BlockFn.forward) — then
    nothing is recomputed."""
    B, Ntok, D = x.shape
    # (a block on the MX-FP8 GEMMs trains LoRA factors at most and builds no temb gradient, `_trainable_form`: its
    # modulation path — the gate sums, h, the AdaLN affine sums — is off)
    need_dmod = (train or want_dtemb) and not _mx_gemms(block)
    G = _Grads()
    # the forward's intermediates: kept by the training forward (the `keep` level "all") or recomputed here by
    # forward_joint's own stages; the stages below pop them, and hand "do" / "dqkv" on, through this dict
    s = front if front is not None else _block_front(block, x, T, temb, rope, form.mask, attn_saved, need_dmod, form)
    del front
    mod1, mod2 = s.pop("mod1"), s.pop("mod2")

    dout = dout.contiguous()
    dinj = None
    if want_dinject:
        if inject_mask is None:
            dinj = dout[:, T:].clone()
        else:
            dinj = torch.empty(B, Ntok - T, D, device=x.device, dtype=BF16)
            K.mask_scale_rows(dout[:, T:], dinj, (inject_mask == 0).to(torch.uint8), 1.0)

    g = dout.clone()  # d x_mid, then d x
    dmod2 = _ff_bwd(block, s, dout, g, T, mod2, need_dmod, train, G)
    gate1 = _attn_output_bwd(block, s, g, T, mod1, need_dmod, train, G)
    s["dqkv"] = form.backward(s, T, rope, train, G)
    dxn = _qkv_bwd(block.attn1, s, train, G, block.qkv_mx is not None and "qkv" in FP8_DGRAD,
                   block.qkv_mx is not None)
    dtemb = _attn_input_bwd(block, x, dxn, g, T, temb, mod1, gate1, dmod2, need_dmod, want_dtemb, train, G)
    return g, dtemb, dinj, G


# The block forward keeps its attention output and softmax statistics for the backward (~113 MB per block at B = 1,
# N = 17 776: 5 GB for the 44 blocks of a training step, against 288 GB of HBM), so the backward recomputes the
# projections and norms but not the attention — the checkpointing otherwise stays as the reference's
# --gradient_checkpointing has it.  The same kernel call produces both (bit-identical to the recompute: the fused QKV
# epilogue equals the separate norm launches).  False: recompute the attention too.
SAVE_ATTENTION = True
# Beyond that, while the device has room (SAVE_ACTIVATIONS = True; the budget below), the training forward keeps
# every intermediate the backward reads (forward_joint's `keep` level "all"), so the backward recomputes nothing: ~1.2 GB per frozen 5b block at B = 1, N = 17 776 (q | k | v, the normed q | k, O, x_mid, the FF1
# pre-activation z).
# A block whose kept set would leave less than SAVE_RESERVE_BYTES free (or four times its own size) falls back to
# the attention-only form, so a larger batch degrades to recompute instead of running out of memory.
SAVE_ACTIVATIONS = True
SAVE_RESERVE_BYTES = 16 << 30


def _room_for(x: torch.Tensor, F4: int, keep_train: bool = False, R: int = 0) -> bool:
    B, Ntok, D = x.shape
    per_row = 5 * D + D + D + F4  # q | k | v, normed q | k, O, x_mid, z (bf16)
    if keep_train:  # + h [F4], the AdaLN outputs xn / xn2 and xq (with the adapters' rank tail R)
        per_row += F4 + 3 * D + R
    need = B * Ntok * per_row * 2
    free, _ = torch.cuda.mem_get_info(x.device)
    return free - need > max(SAVE_RESERVE_BYTES, 4 * need)


class _BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, block, T, rope, inject_mask, form, x, temb, inject, *params):
        """forward_joint with a `keep` dict at the level the attention's form states (`keep_level`): "all" (then
        nothing is recomputed; a frozen block drops xn / xq / xn2 / h, train=False), "attention", or none."""
        train = any(p.requires_grad for p in params) or temb.requires_grad
        level = form.keep_level(block, x, train)
        keep = mod1 = mod2 = None
        if level is not None:
            keep = dict(level=level, train=train)
        if level == "all":
            mod1, mod2 = block.norm1.modulation(temb), block.norm2.modulation(temb)  # (as _block_front)
        out = block.forward_joint(x, T, temb, rope, resample_mask=form.mask, inject=inject,
                                  inject_mask=inject_mask if inject is not None else None, keep=keep, mod1=mod1,
                                  mod2=mod2)
        ctx.front = keep if keeps_all(keep) else None
        ctx.attn_saved = (keep["o"], keep["lse"]) if keep is not None and ctx.front is None else None
        ctx.block, ctx.T, ctx.rope, ctx.inject_mask, ctx.form = block, T, rope, inject_mask, form
        ctx.has_inject = inject is not None
        ctx.params = params
        ctx.save_for_backward(x, temb)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, temb = ctx.saved_tensors
        need = ctx.needs_input_grad
        train = any(need[8:])
        front, ctx.front = ctx.front, None  # (the backward pops it: each intermediate is freed as it is used)
        attn_saved, ctx.attn_saved = ctx.attn_saved, None
        dx, dtemb, dinj, G = block_backward(ctx.block, ctx.form, x, ctx.T, temb, ctx.rope,
                                            ctx.inject_mask if ctx.has_inject else None, dout, need[6],
                                            need[7] and ctx.has_inject, train, attn_saved, front)
        return (None, None, None, None, None, dx if need[5] else None, dtemb, dinj, *G.out(ctx.params))


def block_apply(block, x: torch.Tensor, T: int, temb: torch.Tensor, rope, inject: Optional[torch.Tensor] = None,
                inject_mask: Optional[torch.Tensor] = None,
                resample_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable `block.forward_joint` (gradient-checkpointed).  resample_mask: the uint8 token mask of the
    blocks' resample processor (window 0 of VideoPainterID training)."""
    form = _trainable_form(block, resample_mask, rope, temb)
    params = [p for p in block.parameters()]
    return _BlockFn.apply(block, T, rope, inject_mask, form, x, temb, inject, *params)


# ------------------------------------------------------------------------------------------------------------------
# head, embeddings, branch output linears
# ------------------------------------------------------------------------------------------------------------------

class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, dims, x, emb):
        ctx.model, ctx.dims = model, dims
        ctx.save_for_backward(x, emb)
        return model._head(x, emb, dims[4], dims[:4])  # (the inference forward's head)

    @staticmethod
    def backward(ctx, dout):
        x, emb = ctx.saved_tensors
        m = ctx.model
        B, F, H, W, T = ctx.dims
        cfg = m.config
        p = cfg.patch_size
        _, Ntok, D = x.shape
        Nv = Ntok - T
        if ctx.needs_input_grad[3]:
            raise NotImplementedError("the head's time-embedding gradient (a trainable transformer time embedding) "
                                      "is not implemented: the reference trains the branch only")
        mod = K.linear_small(emb, m.norm_out.linear.weight, m.norm_out.linear.bias, act_in=K.ACT_SILU)
        dproj = K.patchify(dout.to(BF16).contiguous(), None, p, p * p * cfg.out_channels)
        dy = torch.empty(B * Nv, D, device=x.device, dtype=BF16)
        _dgrad(dproj, m.proj_out.weight, dy)
        zero_mod = torch.zeros(B, 6 * D, device=x.device, dtype=BF16)
        n1 = K.adaln_modulate(x, m.norm_final.weight, m.norm_final.bias, zero_mod, T, m.norm_final.eps)
        dx = torch.zeros_like(x)
        dn1 = torch.empty(1, Nv, D, device=x.device, dtype=BF16)
        for b in range(B):
            dn1.zero_()
            K.adaln_bwd(n1[b:b + 1, T:], dy[b * Nv:(b + 1) * Nv].view(1, Nv, D), dn1, 0, m.norm_out.norm.weight,
                        m.norm_out.norm.bias, m.norm_out.norm.eps, mod[b:b + 1], chunks=(0, 1, 0, 1))
            K.adaln_bwd(x[b:b + 1, T:], dn1, dx[b:b + 1, T:], 0, m.norm_final.weight, m.norm_final.bias,
                        m.norm_final.eps, zero_mod[b:b + 1], chunks=(0, 1, 0, 1))
        return None, None, dx, None


def head_apply(model, x: torch.Tensor, emb: torch.Tensor, dims) -> torch.Tensor:
    head = [model.norm_final.weight, model.norm_final.bias, model.norm_out.linear.weight, model.norm_out.linear.bias,
            model.norm_out.norm.weight, model.norm_out.norm.bias, model.proj_out.weight, model.proj_out.bias]
    if any(t is not None and t.requires_grad for t in head):
        raise NotImplementedError("trainable transformer head parameters: the reference trains the branch only")
    return _HeadFn.apply(model, dims, x, emb)


class _PatchEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pe, text, video, video2, *params):
        ctx.pe = pe
        ctx.params = params
        ctx.save_for_backward(text, video, video2)
        return pe.embed(text, video, video2)

    @staticmethod
    def backward(ctx, dx):
        text, video, video2 = ctx.saved_tensors
        pe = ctx.pe
        G = _Grads()
        dx = dx.contiguous()
        B, Ntok, D = dx.shape
        T = text.shape[1]
        G.put(pe.text_proj.weight, K.wgrad(dx[:, :T], text))
        wp, kpad = pe._padded_conv_weight()
        cols = K.patchify(video, video2, pe.patch_size, kpad)
        w = pe.proj.weight
        kk = w.shape[1] * w.shape[2] * w.shape[3]
        dwp = K.wgrad(dx[:, T:], cols)
        G.put(w, dwp[:, :kk].contiguous())
        if pe.text_proj.bias is not None or pe.proj.bias is not None:
            st = torch.zeros(1, 2, D, device=dx.device, dtype=F32)
            sv = torch.zeros(1, 2, D, device=dx.device, dtype=F32)
            for b in range(B):
                K.colsum(dx[b, :T], out=st)
                K.colsum(dx[b, T:], out=sv)
            G.put(pe.text_proj.bias, st[0, 0])
            G.put(pe.proj.bias, sv[0, 0])
        return (None, None, None, None, *G.out(ctx.params))


def patch_embed_apply(pe, text: torch.Tensor, video: torch.Tensor, video2: Optional[torch.Tensor] = None):
    if any(t is not None and t.requires_grad for t in (text, video, video2)):
        raise NotImplementedError("gradients w.r.t. the latents / prompt embeddings are not implemented (the "
                                  "reference's training feeds them as data)")
    params = [pe.text_proj.weight, pe.text_proj.bias, pe.proj.weight, pe.proj.bias]
    if not any(p is not None and p.requires_grad for p in params):
        return pe.embed(text, video, video2)
    return _PatchEmbedFn.apply(pe, text, video, video2, *[p for p in params if p is not None])


class _TimeEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, te, t0, *params):
        h = K.linear_small(t0, te.linear_1.weight, te.linear_1.bias, act_out=K.ACT_SILU)
        ctx.te, ctx.params = te, params
        ctx.save_for_backward(t0)
        return K.linear_small(h, te.linear_2.weight, te.linear_2.bias)

    @staticmethod
    def backward(ctx, demb):
        (t0,) = ctx.saved_tensors
        te = ctx.te
        G = _Grads()
        a1 = K.linear_small(t0, te.linear_1.weight, te.linear_1.bias)
        h = K.silu(a1)
        dh = _small_linear_bwd(G, te.linear_2, h, demb.to(BF16).contiguous())
        _small_linear_bwd(G, te.linear_1, t0, K.silu_bwd(dh, a1))
        return (None, None, *G.out(ctx.params))


def time_embed_apply(te, t0: torch.Tensor) -> torch.Tensor:
    params = [p for p in te.parameters()]
    if not any(p.requires_grad for p in params):
        h = K.linear_small(t0, te.linear_1.weight, te.linear_1.bias, act_out=K.ACT_SILU)
        return K.linear_small(h, te.linear_2.weight, te.linear_2.bias)
    return _TimeEmbedFn.apply(te, t0, *params)


class _RowLinearFn(torch.autograd.Function):
    """y = (x W^T + b) * scale over every row of the joint buffer (the branch's output linears)."""

    @staticmethod
    def forward(ctx, x, w, b, scale):
        B, Ntok, D = x.shape
        o = torch.empty(B, Ntok, w.shape[0], device=x.device, dtype=BF16)
        epi = NAT.EPI_BIAS if scale == 1.0 else NAT.EPI_BIAS_SCALE
        K.gemm(x.reshape(B * Ntok, D), [w], [b], o.view(B * Ntok, -1), epilogue=epi, alpha=scale)
        ctx.scale = scale
        ctx.save_for_backward(x, w, b)
        return o

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        B, Ntok, D = x.shape
        dy = dy.to(BF16).contiguous()
        if ctx.scale != 1.0:
            dy = K.scale_bf16(dy, ctx.scale)
        dy2 = dy.view(B * Ntok, -1)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _dgrad(dy2, w, dx.view(B * Ntok, D))
        if ctx.needs_input_grad[1]:
            dw = K.wgrad(dy2, x.reshape(B * Ntok, D)).to(w.dtype)
        if b is not None and ctx.needs_input_grad[2]:
            db = _total(dy2).to(b.dtype)
        return dx, dw, db, None


def row_linear_apply(x: torch.Tensor, lin, scale: float) -> torch.Tensor:
    return _RowLinearFn.apply(x, lin.weight, lin.bias, float(scale))


def needs_grad(module, *tensors) -> bool:
    """The training path is taken when autograd is on and a parameter or an input requires grad."""
    if not torch.is_grad_enabled():
        return False
    if any(p.requires_grad for p in module.parameters()):
        return True
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            return True
        if isinstance(t, (list, tuple)) and any(isinstance(s, torch.Tensor) and s.requires_grad for s in t):
            return True
    return False
