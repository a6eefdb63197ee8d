"""CogVideoX-5b-I2V DiT on the HIP kernels — drop-in for the reference `CogVideoXTransformer3DModel` /
`CogVideoXBlock` (DF/models/transformers/cogvideox_transformer_3d.py:38-646): same constructor kwargs, same
state-dict keys, same `forward` signature and return forms.

MI355X data layout: the text and video token streams live in ONE resident bf16 buffer [B, T + Nv, D] (text first),
which is exactly the reference's `cat([encoder_hidden_states, hidden_states], dim=1)`, so every per-block
`cat`/`split` of the reference disappears; per-segment behaviour (text vs video modulation, gates, RoPE only on
video tokens, injection only on video tokens) is selected per row inside the kernels.  Each block is 10 launches:

  norm1 linear (small-M) -> AdaLN modulate -> fused QKV GEMM -> qk-LN+RoPE (q, k) -> flash attention
  -> to_out GEMM (+ gate * . + residual) -> norm2 linear -> AdaLN modulate -> FF1 GEMM (+GELU-tanh)
  -> FF2 GEMM (+ gate * . + residual + masked branch injection)

(The norm linears of all blocks read silu(temb) alone: a model's forward runs them as one batched launch,
`batched_modulations`.  With `forward(cfg_shared_video=True)` the first block computes the work its two batch rows —
the classifier-free-guidance halves — share once, `CogVideoXBlock._attend_cfg_shared`.)

The block's forward is written once, as five stages (`CogVideoXBlock._attn_input`, `_attention`, `_attn_output`,
`_ff_front`, `_ff_back`): `forward_joint` composes them, a training forward is the same call with a `keep` dict the
stages fill for the backward, the backward's recompute (autograd._block_front) runs the same stages, and the backward
itself (autograd.block_backward) is one function per stage, in reverse.  Whether a training forward passes `keep`, and
at what level, is the rule of its attention's backward form (autograd._attention_form); the attention stage hands it
to the processor's `attend` in one call.

A model's inference forward is written once too (`_forward_infer`, the head `_head`): `forward` parses the call and
shapes the return; the Ulysses head-parallel split (ulysses.py) runs the same body on a rank's row shard by passing a
split context — a handful of `split is not None` lines shard x, cut the row-local operands at the shard's first video
row and gather the head's rows; the training forward's head (autograd._HeadFn) is `_head` as well.

With `return_hidden_states=True` every block writes its output into a fresh buffer that IS the returned
`hidden_states_list[i]` (no copies).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import kernels as K
from . import _native as NAT
from .attention_processor import (Attention, CogVideoXAttnProcessor2_0, CogVideoXAttnProcessor2_0_resample,
                                  CogVideoXAttnProcessor2_0_wo_text, _fusable_norms, _rope_dev, _u8,
                                  bounded_scores, cfg_shared_attention, keeps_all, project_out)
from .embeddings import joint_sincos_pos_embedding
from .lora import AugmentedProjection, augmented_rows
from .modules import Conv2dPatch, Dropout, LayerNorm, Linear, ModelMixin, _empty

BF16 = torch.bfloat16


@dataclass
class Transformer2DModelOutput:
    sample: torch.Tensor


def _bf(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != BF16:
        t = t.to(BF16)
    return t.contiguous()


# ------------------------------------------------------------------------------------------------------------------
# sub-modules with the reference's parameter names
# ------------------------------------------------------------------------------------------------------------------

class CogVideoXLayerNormZero(nn.Module):
    """DF/models/normalization.py:358-386 — linear: 6*D x temb, norm: LayerNorm(D)."""

    def __init__(self, conditioning_dim: int, embedding_dim: int, elementwise_affine: bool = True, eps: float = 1e-5,
                 bias: bool = True):
        super().__init__()
        self.linear = Linear(conditioning_dim, 6 * embedding_dim, bias=bias)
        self.norm = LayerNorm(embedding_dim, eps=eps, elementwise_affine=elementwise_affine)

    def modulation(self, temb: torch.Tensor) -> torch.Tensor:
        """silu(temb) @ W + b -> bf16 [B, 6D] = shift|scale|gate|enc_shift|enc_scale|enc_gate."""
        return K.linear_small(temb, self.linear.weight, self.linear.bias, act_in=K.ACT_SILU)


class GELUProj(nn.Module):
    def __init__(self, dim_in, dim_out, bias=True):
        super().__init__()
        self.proj = Linear(dim_in, dim_out, bias=bias)
        self.approximate = "tanh"


class FeedForward(nn.Module):
    """DF/models/attention.py:1144-1202 with activation_fn="gelu-approximate": net = [GELU(proj), Dropout, Linear,
    Dropout] (non-gated; SURVEY.md finding 1)."""

    def __init__(self, dim: int, inner_dim: Optional[int] = None, bias: bool = True, final_dropout: bool = True):
        super().__init__()
        inner_dim = inner_dim or 4 * dim
        mods = [GELUProj(dim, inner_dim, bias=bias), Dropout(), Linear(inner_dim, dim, bias=bias)]
        if final_dropout:
            mods.append(Dropout())
        self.net = nn.ModuleList(mods)


class TimestepEmbedding(nn.Module):
    """DF/models/embeddings.py:729-774 (linear_1 -> SiLU -> linear_2)."""

    def __init__(self, in_channels: int, time_embed_dim: int):
        super().__init__()
        self.linear_1 = Linear(in_channels, time_embed_dim)
        self.linear_2 = Linear(time_embed_dim, time_embed_dim)


class CogVideoXPatchEmbed(nn.Module):
    """DF/models/embeddings.py:337-454 — parameters only; `embed()` runs im2col + two GEMMs with fused bias and
    positional-embedding add, writing text rows then video rows of the joint buffer."""

    def __init__(self, patch_size: int, in_channels: int, embed_dim: int, text_embed_dim: int, sample_width: int,
                 sample_height: int, sample_frames: int, temporal_compression_ratio: int, max_text_seq_length: int,
                 spatial_interpolation_scale: float, temporal_interpolation_scale: float,
                 use_positional_embeddings: bool, use_learned_positional_embeddings: bool):
        super().__init__()
        self.patch_size = patch_size
        self.embed_dim = embed_dim
        self.sample_height, self.sample_width, self.sample_frames = sample_height, sample_width, sample_frames
        self.temporal_compression_ratio = temporal_compression_ratio
        self.max_text_seq_length = max_text_seq_length
        self.spatial_interpolation_scale = spatial_interpolation_scale
        self.temporal_interpolation_scale = temporal_interpolation_scale
        self.use_positional_embeddings = use_positional_embeddings
        self.use_learned_positional_embeddings = use_learned_positional_embeddings
        self.proj = Conv2dPatch(in_channels, embed_dim, patch_size)
        self.text_proj = Linear(text_embed_dim, embed_dim)
        self._pos_cache = {}
        self._wpad = None
        if use_positional_embeddings or use_learned_positional_embeddings:
            pe = self._sincos(sample_height, sample_width, sample_frames)
            if use_learned_positional_embeddings:
                self.register_buffer("pos_embedding", _empty(*pe.shape).data, persistent=True)
                with torch.no_grad():
                    self.pos_embedding.copy_(pe)
            else:
                self.register_buffer("pos_embedding", pe.to(self.proj.weight.device, BF16), persistent=False)

    def _sincos(self, h, w, frames):
        return joint_sincos_pos_embedding(self.embed_dim, self.patch_size, self.max_text_seq_length, h, w, frames,
                                          self.temporal_compression_ratio, self.spatial_interpolation_scale,
                                          self.temporal_interpolation_scale)

    def _padded_conv_weight(self) -> Tuple[torch.Tensor, int]:
        w = self.proj.weight
        kk = w.shape[1] * w.shape[2] * w.shape[3]
        kpad = (kk + 63) // 64 * 64
        key = (w.data_ptr(), w._version, kpad)
        if self._wpad is None or self._wpad[0] != key:
            wp = torch.zeros(w.shape[0], kpad, device=w.device, dtype=BF16)
            wp[:, :kk] = w.reshape(w.shape[0], kk)
            self._wpad = (key, wp)
        return self._wpad[1], kpad

    def _pos_for(self, h: int, w: int, frames_latent: int, device) -> Optional[torch.Tensor]:
        """Reference :431-450: learned buffer at the sample resolution / frame count; 3D sin-cos recomputed for
        other frame counts; ValueError for another resolution with learned embeddings."""
        if not (self.use_positional_embeddings or self.use_learned_positional_embeddings):
            return None
        if self.use_learned_positional_embeddings and (self.sample_width != w or self.sample_height != h):
            raise ValueError(
                "It is currently not possible to generate videos at a different resolution that the defaults. This "
                "should only be the case with 'THUDM/CogVideoX-5b-I2V'.If you think this is incorrect, please open "
                "an issue at https://github.com/huggingface/diffusers/issues.")
        pre = (frames_latent - 1) * self.temporal_compression_ratio + 1
        if self.sample_height != h or self.sample_width != w or self.sample_frames != pre:
            key = (h, w, pre, str(device))
            if key not in self._pos_cache:
                self._pos_cache[key] = self._sincos(h, w, pre)[0].to(device=device, dtype=BF16).contiguous()
            return self._pos_cache[key]
        return self.pos_embedding[0]

    def embed(self, text: torch.Tensor, video: torch.Tensor, video2: Optional[torch.Tensor] = None) -> torch.Tensor:
        """text [B, T, Ct], video [B, F, C1, H, W] (+ video2 [B, F, C2, H, W] concatenated on channels)
        -> joint bf16 [B, T + F*(H/p)*(W/p), D]."""
        B, T, _ = text.shape
        _, F, _, H, W = video.shape
        p = self.patch_size
        Nv = F * (H // p) * (W // p)
        Ntok = T + Nv
        D = self.embed_dim
        if T != self.max_text_seq_length and (self.use_learned_positional_embeddings or self.use_positional_embeddings):
            raise ValueError(f"text length {T} != max_text_seq_length {self.max_text_seq_length}")
        pos = self._pos_for(H, W, F, video.device)
        x = torch.empty(B, Ntok, D, device=video.device, dtype=BF16)
        xf = x.view(B * Ntok, D)
        epi = NAT.EPI_BIAS_ADDROWS if pos is not None else NAT.EPI_BIAS
        K.gemm(text.reshape(B * T, -1), [self.text_proj.weight], [self.text_proj.bias], xf, epilogue=epi,
               rows_per_group=T, group_stride=Ntok, row_offset=0, addrows=pos, addrows_offset=0)
        wp, kpad = self._padded_conv_weight()
        cols = K.patchify(video, video2, p, kpad)
        K.gemm(cols, [wp], [self.proj.bias], xf, epilogue=epi, rows_per_group=Nv, group_stride=Ntok, row_offset=T,
               addrows=pos, addrows_offset=T)
        return x


class CogVideoXBlock(nn.Module):
    """DF/models/transformers/cogvideox_transformer_3d.py:38-216."""

    def __init__(self, dim: int, num_attention_heads: int, attention_head_dim: int, time_embed_dim: int,
                 dropout: float = 0.0, activation_fn: str = "gelu-approximate", attention_bias: bool = False,
                 qk_norm: bool = True, norm_elementwise_affine: bool = True, norm_eps: float = 1e-5,
                 final_dropout: bool = True, ff_inner_dim: Optional[int] = None, ff_bias: bool = True,
                 attention_out_bias: bool = True, wo_text: bool = False, id_pool_resample_learnable: bool = False):
        super().__init__()
        if activation_fn != "gelu-approximate":
            raise NotImplementedError(f"activation_fn={activation_fn!r}: CogVideoX uses gelu-approximate")
        if not qk_norm:
            raise NotImplementedError("CogVideoX uses qk_norm=True")
        self.norm1 = CogVideoXLayerNormZero(time_embed_dim, dim, norm_elementwise_affine, norm_eps, bias=True)
        # wo_text (the branch's text-free mode, :96-97): the blocks run `forward_joint` with no text rows
        self.wo_text = bool(wo_text)
        self.processor = CogVideoXAttnProcessor2_0_wo_text() if wo_text else \
            CogVideoXAttnProcessor2_0_resample() if id_pool_resample_learnable else CogVideoXAttnProcessor2_0()
        self.attn1 = Attention(query_dim=dim, dim_head=attention_head_dim, heads=num_attention_heads, eps=1e-6,
                               bias=attention_bias, out_bias=attention_out_bias, processor=self.processor)
        self.norm2 = CogVideoXLayerNormZero(time_embed_dim, dim, norm_elementwise_affine, norm_eps, bias=True)
        self.ff = FeedForward(dim, inner_dim=ff_inner_dim, bias=ff_bias, final_dropout=final_dropout)
        self.dim = dim
        self.ff_mx = None  # (W1, W2) as MX-FP8 when the fp8 FeedForward is enabled (BASELINE config 5)
        self.qkv_mx = None  # (Wq, Wk, Wv) as MX-FP8 when the fp8 QKV projection is enabled
        self.out_mx = None  # W_out as MX-FP8 when the fp8 attention output projection is enabled

    def enable_fp8_ffn(self, enabled: bool = True) -> None:
        """Run the FeedForward on the block-scaled fp8 MFMA: both weights quantised once to MX-FP8 (e4m3 + one
        E8M0 scale per 32 inputs), the norm2 AdaLN output written in MX-FP8, FF1's GELU output re-quantised in its
        epilogue, FF2 accumulating in fp32 into the bf16 gated residual.  The state dict is unchanged."""
        if not enabled:
            self.ff_mx = None
            return
        w1, w2 = self.ff.net[0].proj.weight, self.ff.net[2].weight
        if w1.shape[0] % 256 or w2.shape[0] % 256 or w1.shape[1] % 128 or w2.shape[1] % 128:
            raise ValueError(f"fp8 FeedForward needs widths that are multiples of 256, got {tuple(w1.shape)}")
        self.ff_mx = (K.mx_quantize(w1), K.mx_quantize(w2))

    def enable_fp8_qkv(self, enabled: bool = True) -> None:
        """Fused QKV projection on the block-scaled fp8 MFMA: the three weights quantised once to MX-FP8, the norm1
        AdaLN writing MX-FP8 directly, bf16 q/k/v out (the prev-clip K/V projection stays bf16).  Unfused LoRA adapters
        on q / k / v (loaded ones attached before or after this call, trainable ones before it) run beside it as low-rank bf16 launches (`_attn_input`)."""
        if not enabled:
            self.qkv_mx = None
            return
        a = self.attn1
        ws = (a.to_q.weight, a.to_k.weight, a.to_v.weight)
        if any(w.shape[0] % 256 or w.shape[1] % 128 for w in ws):
            raise ValueError("fp8 QKV needs widths that are multiples of 256")
        self.qkv_mx = tuple(K.mx_quantize(w) for w in ws)

    def enable_fp8_out(self, enabled: bool = True) -> None:
        """The attention's output projection (to_out[0], attention_processor.py:2202) on the block-scaled fp8 MFMA:
        the weight quantised once to MX-FP8, the attention output quantised per call (vp_mx_quantize_bf16), the gated
        residual in the fp8 GEMM's epilogue as in the bf16 path.  An unfused LoRA adapter on to_out (attached before
        or after this call) runs beside it as low-rank bf16 launches (`_attn_output`)."""
        if not enabled:
            self.out_mx = None
            return
        lin = self.attn1.to_out[0]
        if lin.weight.shape[0] % 256 or lin.weight.shape[1] % 128:
            raise ValueError("fp8 output projection needs widths that are multiples of 256")
        self.out_mx = K.mx_quantize(lin.weight)

    def enable_fp8_attention(self, enabled: bool = True, resample: bool = False) -> None:
        """Run self-attention on the block-scaled fp8 MFMA (vp_attention_fwd_fp8): Q and K leave the qk-norm + RoPE
        kernel as e4m3 with one static power-of-two factor each, chosen from the LayerNorm's bound on its outputs
        (kernels.qk_fp8_exponent: nothing can saturate), V is packed to e4m3 with per-(channel, 32 keys) scales,
        and P is rounded to e4m3 inside the kernel.  The resample processor (two K/V segments) stays bf16 unless
        `resample` opts in: then, when its null keys are summed in closed form (the video grid known, the RoPE table
        separable), its masked keys run as the fp8 kernel's second segment (K rows through the masked fp8 norm, V
        through a length-aware pack) and the null-key mass as its l_extra; every other form of that processor stays
        bf16.  Accuracy at full length (inside the 5x block band) and speed against bf16: DESIGN.md §4.  enabled=False
        clears both switches."""
        attn = self.attn1
        attn.fp8_resample = bool(enabled and resample)
        if not enabled:
            attn.fp8_qk_exp = None
            return
        attn.fp8_qk_exp = (K.qk_fp8_exponent(attn.norm_q.weight, attn.norm_q.bias, attn.scale * K.LOG2E),
                           K.qk_fp8_exponent(attn.norm_k.weight, attn.norm_k.bias))

    def enable_closed_form_resample_backward(self, enabled: bool = True) -> None:
        """The ID-resample processor's training backward on the forward's compact plan (autograd.block_backward): the
        training forward keeps the two-segment launch's o / lse, the flash backward runs over the N own keys plus the
        masked rows (a per-batch key length), and the null keys' share of dq comes from the closed form
        (kernels.null_key_mass_bwd).  Needs the video grid on the rope, a separable table and a frozen norm_k bias;
        an unmet condition raises when the block is applied.  No effect on a block without that processor."""
        if isinstance(self.attn1.processor, CogVideoXAttnProcessor2_0_resample):
            self.attn1.closed_form_resample_backward = bool(enabled)

    # -- the CFG halves' shared first-block work --
    def _cfg_shared_ok(self, x: torch.Tensor, text_len: int) -> bool:
        """The shared path restates the plain bf16 block only: two batch rows with text, the standard processor with
        the fused qk-norm + RoPE epilogue, no fp8 form and no unfused LoRA operand on the projections.  Anything else
        (and VP_CFG_SHARED=0, the A/B knob) runs the plain path."""
        a = self.attn1
        return (NAT.knob_values.get("VP_CFG_SHARED") != "0" and x.shape[0] == 2 and 0 < text_len < x.shape[1]
                and type(a.processor) is CogVideoXAttnProcessor2_0 and self.qkv_mx is None
                and getattr(a, "fp8_qk_exp", None) is None and hasattr(a, "inner_dim") and a.inner_dim == x.shape[2]
                and _fusable_norms(a) and AugmentedProjection.of((a.to_q, a.to_k, a.to_v, a.to_out[0])) is None)

    def _attend_cfg_shared(self, x: torch.Tensor, text_len: int, mod1: torch.Tensor, rope) -> torch.Tensor:
        """norm1 modulate -> QKV -> attention of a block whose two batch rows (the classifier-free-guidance halves)
        hold the same video rows and differ in their text rows only: what the halves share is computed once.

        The first N + T rows of the flat [2 N, D] view are batch 0 whole plus batch 1's text rows: the modulate and
        the QKV GEMM (M = N + T; its epilogue takes text / video and the RoPE row from m % N) run on exactly those,
        bit-equal to the plain path there; batch 1's video rows of xn / qkv are never written nor read.  The attention
        over the joint keys is composed from pieces over disjoint key sets, all through strides (no copies):
          (a) video queries x video keys of batch 0, B = 1                 -> O_v, lse_v   (the shared 97 %)
          (b) the same queries (batch stride 0) x each half's text keys    -> O_t, lse_t
          (c) each half's text queries x (own text keys | batch 0's video keys) -> o's text rows
          (d) merge of (a) and (b) (vp_attention_merge_bf16)               -> o's video rows of both halves."""
        B, N_, D = x.shape
        T, a, H = text_len, self.attn1, self.attn1.heads
        xn = torch.empty_like(x)
        self._norm1(x[:1], mod1[:1], T, out=xn[0])
        self._norm1(x[1:, :T], mod1[1:], T, out=xn[1, :T])
        # (the QKV GEMM on a row slice of the two halves: _qkv projects whole [B, N, D] operands, so this one call
        # stays apart from it; _cfg_shared_ok admits no LoRA operand here)
        qkv = torch.empty(B, N_, 3 * D, device=x.device, dtype=BF16)
        M = N_ + T
        K.gemm(xn.view(B * N_, D)[:M], [a.to_q.weight, a.to_k.weight, a.to_v.weight],
               [a.to_q.bias, a.to_k.bias, a.to_v.bias], qkv.view(B * N_, 3 * D)[:M],
               epilogue=NAT.EPI_BIAS_QKNORM_ROPE, qk_norm=(a.norm_q, a.norm_k), rope=rope, tokens_per_batch=N_,
               text_len=T)
        del xn
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        o = torch.empty(B, N_, D, device=x.device, dtype=BF16)
        cfg_shared_attention(q, k, v, o, H, T, scale=a.scale, bounded_scores=bounded_scores(a))
        return o

    # -- the block's forward as stages; the modulation vectors are their inputs --
    def _norm1(self, x: torch.Tensor, mod1: torch.Tensor, text_len: int, out=None) -> torch.Tensor:
        n = self.norm1.norm
        return K.adaln_modulate(x, n.weight, n.bias, mod1, text_len, n.eps, out=out)

    def _attn_input(self, x: torch.Tensor, text_len: int, mod1: torch.Tensor, prev_joint=None, augment: bool = True,
                    keep: Optional[dict] = None):
        """norm1 AdaLN -> (xn, qkv, pn): the attention's bf16 operand xn (written straight into the projection's
        K-augmented operand under unfused LoRA, unless an `attend` hook takes it: augment=False), or with the fp8 QKV
        projection the MX-FP8 modulate + GEMM's output qkv; pn: the previous window's states through the same norm1
        (reference :141-146), the prev-clip K / V operand.

        The fp8 QKV projection under unfused LoRA on q / k / v is PEFT's base(x) + lora_B(lora_A(x)) * scaling as
        launches: the dual modulate writes the MX rows and, into the K-augmented operand, the bf16 rows; the MX GEMM
        writes the base qkv; T = x A_cat^T (lora.AugmentedProjection.input) and one low-rank bf16 GEMM per adapted
        projection add the delta onto it in place, qkv = rnd(rnd(T_i (s B_i)^T) + qkv) (`side_delta`).  xn is then
        returned beside qkv, and a keep-all training forward keeps it and the operand ("xn", "xq")."""
        B, Ntok, D = x.shape
        a, n1 = self.attn1, self.norm1.norm
        xn = qkv = pn = None
        if self.qkv_mx is not None:
            lins = (a.to_q, a.to_k, a.to_v)
            qaug = AugmentedProjection.of(lins)
            if qaug is None:
                xq = K.adaln_modulate_mx(x, n1.weight, n1.bias, mod1, text_len, n1.eps)
            else:
                xn, xq = K.adaln_modulate_dual(x, n1.weight, n1.bias, mod1, text_len, n1.eps,
                                               out=augmented_rows(lins, B, Ntok, D, x.device))
            qkv = torch.empty(B, Ntok, 3 * D, device=x.device, dtype=x.dtype)
            K.gemm_mx(xq, list(self.qkv_mx), [a.to_q.bias, a.to_k.bias, a.to_v.bias], qkv.view(B * Ntok, 3 * D))
            if qaug is not None:
                x_aug = qaug.input(xn.reshape(-1, D))
                qaug.side_delta(x_aug, qkv.view(B * Ntok, 3 * D))
                if keeps_all(keep) and keep["train"]:
                    keep["xn"], keep["xq"] = xn, x_aug
        else:
            xn = self._norm1(x, mod1, text_len,
                             augmented_rows((a.to_q, a.to_k, a.to_v), B, Ntok, D, x.device) if augment else None)
            if keeps_all(keep) and keep["train"]:
                keep["xn"] = xn
        if prev_joint is not None:
            pn = self._norm1(_bf(prev_joint), mod1, text_len,
                             augmented_rows((a.to_k, a.to_v), prev_joint.shape[0], prev_joint.shape[1], D, x.device))
        return xn, qkv, pn

    def _attention(self, x: torch.Tensor, text_len: int, rope, pn=None, prev_clip_weight=None, resample_mask=None,
                   prev_resample_mask=None, qkv=None, attend=None, keep: Optional[dict] = None) -> torch.Tensor:
        """x: the attention-input stage's xn (with an fp8 projection `qkv`: any [B, N, D] tensor, for its shape)
        -> o [B, N, D], through the `attend` hook or the processor.  The hook also gets the fp8 projection's `qkv` and
        whether the output projection is the fp8 one (it may then return o as the MXTensor `_attn_output` takes).
        keep: handed to the processor, which fills it (`attend` of either processor; a ValueError where it keeps
        nothing: the fp8 attention, the prev-clip blend, the resample processor with a handed-over qkv).  Whether a training forward passes one is the
        rule of its attention's backward form (autograd: `keep_level`)."""
        a = self.attn1
        if attend is not None:
            # (an unfused adapter on to_out reads the bf16 o: the hook then hands that back, not the MX operand)
            return attend(a, x, text_len, rope, pn, prev_clip_weight, resample_mask, prev_resample_mask, qkv,
                          self.out_mx is not None and AugmentedProjection.of((a.to_out[0],)) is None)
        return a.processor.attend(a, x, text_len, rope, pn, prev_clip_weight, resample_mask, prev_resample_mask,
                                  qkv=qkv, keep=keep)

    def _attn_output(self, x: torch.Tensor, o, mod1: torch.Tensor, text_len: int,
                     keep: Optional[dict] = None) -> torch.Tensor:
        """to_out (bf16, or the fp8 projection of the re-quantised o) with the gated residual on x -> x_mid.  o: bf16
        [B, N, D], or with the fp8 projection its MX-FP8 operand already (an MXTensor [B N, D]: the head-parallel
        split quantises while it gathers the heads, kernels.mx_quantize_heads).

        The fp8 projection under an unfused LoRA adapter on to_out: the adapter's low-rank bf16 GEMM runs first, under
        the gated epilogue without a bias onto the residual, R' = rnd(x + rnd(gate rnd(T (s B)^T))) into a buffer of
        its own, and the MX GEMM then takes R' as its residual: x + gate (base + bias + delta) up to those roundings."""
        B, Ntok, D = x.shape
        M = B * Ntok
        x_mid = torch.empty_like(x)
        kw = dict(epilogue=NAT.EPI_GATED, resid=x.view(M, D), mod=mod1, tokens_per_batch=Ntok, text_len=text_len)
        if self.out_mx is not None:
            oaug = AugmentedProjection.of((self.attn1.to_out[0],))
            if oaug is not None:
                if isinstance(o, K.MXTensor):
                    raise ValueError("an unfused LoRA adapter on to_out reads the bf16 attention output")
                kw["resid"] = oaug.side_delta(oaug.input(o.view(M, D)), torch.empty(M, D, device=x.device, dtype=BF16),
                                              gate_chunk=2, gate_text_chunk=5, **kw)
            om = o if isinstance(o, K.MXTensor) else \
                K.mx_quantize(o.view(M, D), out=K.MXTensor(M, D, x.device, zero=False))
            K.gemm_mx(om, [self.out_mx], [self.attn1.to_out[0].bias], x_mid.view(M, D), **kw)
        else:
            project_out(self.attn1.to_out[0], o.view(M, D), x_mid.view(M, D), gate_chunk=2, gate_text_chunk=5, **kw)
        if keeps_all(keep):
            keep["x_mid"] = x_mid
        return x_mid

    def _ff_front(self, x_mid: torch.Tensor, mod2: torch.Tensor, text_len: int, keep: Optional[dict] = None,
                  activate: bool = True):
        """norm2 AdaLN + FF1 with its GELU epilogue -> h (bf16 [B, N, 4D], or MX-FP8 rows with the fp8 FeedForward).
        keep, at the level "all", receives the pre-activation "z" — the epilogue's aux output (of either GEMM),
        requested then only; a backward that needs no h passes activate=False: FF1 then stores z alone (the fp8 FF1
        under EPI_BIAS: the same bits), nothing is returned — and, for trainable parameters, "xn2" and "h" (bf16
        FeedForward only: a block on the fp8 GEMMs trains LoRA factors at most, autograd._trainable_form)."""
        B, Ntok, D = x_mid.shape
        M = B * Ntok
        n2, ff0 = self.norm2.norm, self.ff.net[0].proj
        if self.ff_mx is not None:
            w1 = self.ff_mx[0]
            xq = K.adaln_modulate_mx(x_mid, n2.weight, n2.bias, mod2, text_len, n2.eps)
            # (autograd refuses trainable FeedForward parameters beside the MX GEMMs): z is all its backward reads
            z = None
            if keeps_all(keep):
                keep["z"] = z = torch.empty(M, w1.rows, device=x_mid.device, dtype=BF16)
            if not activate:
                K.gemm_mx(xq, [w1], [ff0.bias], z)
                return None
            h = K.MXTensor(M, w1.rows, x_mid.device, zero=False)
            K.gemm_mx(xq, [w1], [ff0.bias], h, epilogue=NAT.EPI_BIAS_GELU_MXFP8, aux=z)
            return h
        xn2 = K.adaln_modulate(x_mid, n2.weight, n2.bias, mod2, text_len, n2.eps)
        F4 = ff0.weight.shape[0]
        h = z = None
        if keeps_all(keep):
            keep["z"] = z = torch.empty(M, F4, device=x_mid.device, dtype=BF16)
        if activate:
            h = torch.empty(B, Ntok, F4, device=x_mid.device, dtype=BF16)
            K.gemm(xn2.view(M, D), [ff0.weight], [ff0.bias], h.view(M, F4), epilogue=NAT.EPI_BIAS_GELU, aux=z)
        else:
            K.gemm(xn2.view(M, D), [ff0.weight], [ff0.bias], z)
        if keeps_all(keep) and keep["train"]:
            keep["xn2"] = xn2
            if activate:
                keep["h"] = h.view(M, F4)
        return h

    def _ff_back(self, x_mid: torch.Tensor, h, mod2: torch.Tensor, text_len: int, inject=None, inject_mask=None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """FF2 with the gated residual on x_mid and the masked branch injection -> out."""
        B, Ntok, D = x_mid.shape
        M = B * Ntok
        ff2 = self.ff.net[2]
        if out is None:
            out = torch.empty_like(x_mid)
        kw = dict(epilogue=NAT.EPI_GATED, resid=x_mid.view(M, D), mod=mod2, tokens_per_batch=Ntok, text_len=text_len)
        if self.ff_mx is not None:
            K.gemm_mx(h, [self.ff_mx[1]], [ff2.bias], out.view(M, D), inject=inject, inject_mask=inject_mask, **kw)
            return out
        if inject is not None:
            kw.update(inject=inject, inject_ld=inject.stride(1), inject_bstride=inject.stride(0),
                      inject_mask=inject_mask)
        K.gemm(h.view(M, -1), [ff2.weight], [ff2.bias], out.view(M, D), gate_chunk=2, gate_text_chunk=5, **kw)
        return out

    # -- joint-buffer fast path used by the models --
    def forward_joint(self, x: torch.Tensor, text_len: int, temb: torch.Tensor, rope=None,
                      resample_mask: Optional[torch.Tensor] = None, prev_joint: Optional[torch.Tensor] = None,
                      prev_clip_weight: Optional[float] = None, prev_resample_mask: Optional[torch.Tensor] = None,
                      inject: Optional[torch.Tensor] = None, inject_mask: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, attend=None, keep: Optional[dict] = None,
                      mod1: Optional[torch.Tensor] = None, mod2: Optional[torch.Tensor] = None,
                      cfg_shared_video: bool = False) -> torch.Tensor:
        """mod1 / mod2: the norm1 / norm2 modulation vectors [B, 6D] when the model computed every block's in one
        launch (batched_modulations); absent, the block computes its own.  cfg_shared_video: the caller's promise that
        the two batch rows of x hold the same video rows (the CFG halves entering the model's first block) — the
        block then computes their shared work once (_attend_cfg_shared) where it runs the plain bf16 path.
        attend: optional replacement of the processor's attention, `attend(attn, xn, text_len, rope, pn,
        prev_clip_weight, resample_mask, prev_resample_mask, qkv, mx_out) -> o` [B, N, D] (the Ulysses head-parallel
        split, ulysses._Ctx.attend: x and rope are then a rank's rows, the masks the whole ones; qkv: the fp8 QKV
        projection's pre-norm output in place of xn, or None; mx_out: the output projection is the fp8 one, o may come
        back as its MX-FP8 operand).
        keep: {"level": "attention" | "all", "train": bool}, a training forward's dict that the stages fill for its
        backward (autograd._BlockFn) without changing a launch.  "attention": the attention output "o" and its softmax
        statistics "lse" (the single-segment bf16 attention, or the resample processor's closed-form plan).  "all":
        also "mod1", "mod2", the normed "q" / "k" and "v", the pre-norm "qpre" / "kpre", "x_mid" and the FF1
        pre-activation "z" (the two GEMMs' aux outputs, requested at this level only) and, with train, "xn", "xq",
        "xn2" and "h"."""
        processor = self.attn1.processor
        if not isinstance(processor, CogVideoXAttnProcessor2_0):
            raise ValueError(f"Unsupported processor type: {type(processor)}")
        if mod1 is None:
            mod1 = self.norm1.modulation(temb)
        if (cfg_shared_video and attend is None and keep is None and prev_joint is None
                and self._cfg_shared_ok(x, text_len)):
            o = self._attend_cfg_shared(x, text_len, mod1, rope)
        else:
            xn, qkv, pn = self._attn_input(x, text_len, mod1, prev_joint, attend is None, keep)
            o = self._attention(xn if xn is not None else x, text_len, rope, pn, prev_clip_weight, resample_mask,
                                prev_resample_mask, qkv, attend, keep)
            del xn, qkv, pn
        x_mid = self._attn_output(x, o, mod1, text_len, keep)
        del o
        if mod2 is None:
            mod2 = self.norm2.modulation(temb)
        if keeps_all(keep):
            keep["mod1"], keep["mod2"] = mod1, mod2
        return self._ff_back(x_mid, self._ff_front(x_mid, mod2, text_len, keep), mod2, text_len, inject, inject_mask,
                             out)

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor, temb: torch.Tensor,
                image_rotary_emb=None, attention_mask=None, resample_mask=None,
                attention_kwargs: Optional[Dict[str, Any]] = None):
        """Reference signature (:125-134); returns (hidden_states, encoder_hidden_states)."""
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is never set on the CogVideoX path")
        t = encoder_hidden_states.size(1)
        x = torch.cat([_bf(encoder_hidden_states), _bf(hidden_states)], dim=1).contiguous()
        kw = attention_kwargs or {}
        prev = kw.get("prev_hidden_states")
        prev = prev if isinstance(prev, torch.Tensor) else None
        out = self.forward_joint(x, t, _bf(temb), _rope_dev(image_rotary_emb, x.device), _u8(resample_mask), prev,
                                 kw.get("prev_clip_weight"), _u8(kw.get("prev_resample_mask")))
        return out[:, t:], out[:, :t]


class CogVideoXTransformer3DModel(ModelMixin):
    """Drop-in for DF/models/transformers/cogvideox_transformer_3d.py:218-646."""

    _is_branch = False
    takes_cfg_shared_video = True  # forward() accepts the hint (the harness passes it only to models that say so)

    def __init__(self, num_attention_heads: int = 30, attention_head_dim: int = 64, in_channels: int = 16,
                 out_channels: Optional[int] = 16, flip_sin_to_cos: bool = True, freq_shift: int = 0,
                 time_embed_dim: int = 512, text_embed_dim: int = 4096, num_layers: int = 30, dropout: float = 0.0,
                 attention_bias: bool = True, sample_width: int = 90, sample_height: int = 60,
                 sample_frames: int = 49, patch_size: int = 2, temporal_compression_ratio: int = 4,
                 max_text_seq_length: int = 226, activation_fn: str = "gelu-approximate",
                 timestep_activation_fn: str = "silu", norm_elementwise_affine: bool = True, norm_eps: float = 1e-5,
                 spatial_interpolation_scale: float = 1.875, temporal_interpolation_scale: float = 1.0,
                 use_rotary_positional_embeddings: bool = False, use_learned_positional_embeddings: bool = False,
                 id_pool_resample_learnable: Optional[bool] = False):
        super().__init__()
        self._init_config(dict(locals_without_self(locals())))
        inner_dim = num_attention_heads * attention_head_dim
        if not use_rotary_positional_embeddings and use_learned_positional_embeddings:
            raise ValueError(
                "There are no CogVideoX checkpoints available with disable rotary embeddings and learned positional "
                "embeddings. If you're using a custom model and/or believe this should be supported, please open an "
                "issue at https://github.com/huggingface/diffusers/issues.")
        if timestep_activation_fn != "silu" or not flip_sin_to_cos:
            raise NotImplementedError("CogVideoX uses silu time embedding with flip_sin_to_cos=True")
        self.patch_embed = CogVideoXPatchEmbed(
            patch_size, self._patch_channels(), inner_dim, text_embed_dim, sample_width, sample_height,
            sample_frames, temporal_compression_ratio, max_text_seq_length, spatial_interpolation_scale,
            temporal_interpolation_scale, not use_rotary_positional_embeddings, use_learned_positional_embeddings)
        self.embedding_dropout = Dropout()
        self.time_embedding = TimestepEmbedding(inner_dim, time_embed_dim)
        self.transformer_blocks = nn.ModuleList([
            CogVideoXBlock(dim=inner_dim, num_attention_heads=num_attention_heads,
                           attention_head_dim=attention_head_dim, time_embed_dim=time_embed_dim, dropout=dropout,
                           activation_fn=activation_fn, attention_bias=attention_bias,
                           norm_elementwise_affine=norm_elementwise_affine, norm_eps=norm_eps,
                           id_pool_resample_learnable=self._block_resample())
            for _ in range(num_layers)])
        self.norm_final = LayerNorm(inner_dim, norm_eps, norm_elementwise_affine)
        self._build_head(inner_dim, time_embed_dim, norm_elementwise_affine, norm_eps, patch_size, out_channels)

    def load_lora_weights(self, path: str, weight_name: str = "pytorch_lora_weights.safetensors",
                          adapter_name: Optional[str] = None, lora_scale: Optional[float] = None, **_):
        """The VideoPainterID adapter (PEFT safetensors) on to_q/to_k/to_v/to_out.0, applied UNFUSED as the
        reference's PEFT does (infer/inpaint.py:310-316; videopainter_amd/lora.py): the projections run on K-augmented
        operands, W0 untouched.  Every forward applies its own `attention_kwargs["scale"]` (default 1.0);
        `lora_scale` sets it now.  `fuse_lora` folds explicitly."""
        from .lora import attach_lora_, load_lora_state_dict
        sd = load_lora_state_dict(path, weight_name)
        if any(k.startswith("transformer.") for k in sd):  # the pipeline-level file (lora_pipeline.py:2653-2656)
            sd = {k: v for k, v in sd.items() if k.startswith("transformer.")}
        attach_lora_(self, sd, lora_scale, adapter_name)
        return self

    def get_list_adapters(self):
        from .lora import lora_state
        st = lora_state(self)
        return [n for n, _ in st.adapters] if st is not None else []

    def set_lora_scale(self, scale: float):
        """The per-call LoRA scale (what a call with attention_kwargs={"scale": scale} does): unfused adapters take
        it in their augmented operands; weights holding a fold are rebuilt exactly from their kept base."""
        from .lora import lora_state, refold_lora_
        st = lora_state(self)
        if st is not None and st.scale != float(scale):
            refold_lora_(self, float(scale))
        return self

    def set_adapters(self, adapter_names, weights=None):
        """PEFT's set_adapters on the folded adapters: the listed ones active with these weights, the rest off."""
        from .lora import set_adapter_weights_
        set_adapter_weights_(self, adapter_names, weights)
        return self

    def fuse_lora(self, lora_scale: float = 1.0):
        """The pipeline's `fuse_lora(lora_scale=...)`: the loaded adapters folded into W0 + s B A at `lora_scale`
        (base kept), no longer following per-call scales (PEFT's merged layers no longer see `scale_lora_layers`)."""
        from .lora import fuse_lora_
        fuse_lora_(self, lora_scale)
        return self

    def unfuse_lora(self):
        """PEFT's `unfuse_lora`: back to W0 (exact, from the kept base) with the adapters applied unfused."""
        from .lora import unfuse_lora_
        unfuse_lora_(self)
        return self

    def add_adapter(self, adapter_config, adapter_name: str = "default"):
        """PEFT's `transformer.add_adapter(LoraConfig(r=..., lora_alpha=..., init_lora_weights=True,
        target_modules=["to_q", "to_k", "to_v", "to_out.0"]))` (train/train_cogvideox_inpainting_i2v_video_resample.py
        :1520-1526): trainable lora_A / lora_B factors on the target Linears, everything else frozen
        (videopainter_amd/lora.py add_trainable_adapter_).  `adapter_config`: any object (or dict) with r,
        lora_alpha and optionally target_modules / init_lora_weights — peft's LoraConfig itself qualifies."""
        from .lora import TARGETS, add_trainable_adapter_
        get = (lambda k, d=None: adapter_config.get(k, d)) if isinstance(adapter_config, dict) else (
            lambda k, d=None: getattr(adapter_config, k, d))
        tm = get("target_modules") or TARGETS
        if isinstance(tm, str):
            tm = [tm]
        add_trainable_adapter_(self, int(get("r")), float(get("lora_alpha", get("r"))), tuple(tm), adapter_name,
                               bool(get("init_lora_weights", True)))
        return self

    def get_lora_state_dict(self):
        """The trainable factors under PEFT's saved names (`get_peft_model_state_dict(transformer)`), for
        `save_lora_weights(transformer_lora_layers=...)`."""
        from .lora import trainable_lora_state_dict
        return trainable_lora_state_dict(self)

    def _call_lora_scale(self, attention_kwargs):
        from .lora import lora_state
        st = lora_state(self)
        if st is None:
            return
        s = attention_kwargs.get("scale", 1.0) if attention_kwargs else 1.0
        self.set_lora_scale(1.0 if s is None else s)

    def enable_fp8_ffn(self, enabled: bool = True):
        """fp8 FeedForward in every block (BASELINE config 5; see CogVideoXBlock.enable_fp8_ffn).  Call after the
        weights are loaded; re-call after changing them."""
        for blk in self.transformer_blocks:
            blk.enable_fp8_ffn(enabled)
        return self

    def enable_fp8_attention(self, enabled: bool = True, resample: bool = False):
        """fp8 self-attention in every block (BASELINE config 5; see CogVideoXBlock.enable_fp8_attention).  Call
        after the weights are loaded (the Q/K factors come from the qk-norm affine).  resample: also the ID-resample
        processor's two-segment attention (off by default: that processor then stays bf16)."""
        for blk in self.transformer_blocks:
            blk.enable_fp8_attention(enabled, resample)
        return self

    def enable_closed_form_resample_backward(self, enabled: bool = True):
        """Opt in (default off) to the closed-form backward of the ID-resample processor in every block that carries
        it (VideoPainterID LoRA training, window 0): the backward differentiates the forward's compact plan — no
        attention recompute, the flash backward over N + masked-row keys instead of 2 N, the null keys' query
        gradient in closed form (CogVideoXBlock.enable_closed_form_resample_backward; INTEGRATION.md, training).
        Off, the backward stays the explicit 2 N-key form."""
        for blk in self.transformer_blocks:
            blk.enable_closed_form_resample_backward(enabled)
        return self

    def enable_fp8_qkv(self, enabled: bool = True):
        """fp8 fused QKV projection in every block (see CogVideoXBlock.enable_fp8_qkv)."""
        for blk in self.transformer_blocks:
            blk.enable_fp8_qkv(enabled)
        return self

    def enable_fp8_out(self, enabled: bool = True):
        """fp8 attention output projection in every block (see CogVideoXBlock.enable_fp8_out)."""
        for blk in self.transformer_blocks:
            blk.enable_fp8_out(enabled)
        return self

    def enable_fp8(self, ffn: bool = True, attention: bool = True, qkv: bool = True, out: bool = True,
                   resample_attention: bool = False):
        """BASELINE config 5: "attn + FFN in fp8" (the QKV projection, the attention products, the attention's output
        projection, the FeedForward).  resample_attention: with `attention`, also the ID-resample processor's
        attention (enable_fp8_attention(resample=True))."""
        self.enable_fp8_ffn(ffn)
        self.enable_fp8_qkv(qkv)
        self.enable_fp8_out(out)
        return self.enable_fp8_attention(attention, resample_attention)

    def _patch_channels(self):
        return self.config.in_channels

    def _block_resample(self):
        return bool(self.config.id_pool_resample_learnable)

    def _build_head(self, inner_dim, time_embed_dim, affine, eps, patch_size, out_channels):
        self.norm_out = AdaLayerNorm(time_embed_dim, 2 * inner_dim, affine, eps)
        self.proj_out = Linear(inner_dim, patch_size * patch_size * out_channels)

    # -- processor plumbing (reference :372-430) --
    @property
    def attn_processors(self):
        procs = {}
        for name, m in self.named_modules():
            if hasattr(m, "get_processor"):
                procs[f"{name}.processor"] = m.get_processor()
        return procs

    def set_attn_processor(self, processor):
        count = len(self.attn_processors)
        if isinstance(processor, dict) and len(processor) != count:
            raise ValueError(f"A dict of processors was passed, but the number of processors {len(processor)} does "
                             f"not match the number of attention layers: {count}.")
        processor = dict(processor) if isinstance(processor, dict) else processor
        for name, m in self.named_modules():
            if hasattr(m, "set_processor"):
                m.set_processor(processor.pop(f"{name}.processor") if isinstance(processor, dict) else processor)

    # -- QKV fusion switches (reference :431-470) --
    def fuse_qkv_projections(self):
        """Reference :432-456 fuses to_q / to_k / to_v of every Attention into one projection and installs
        FusedCogVideoXAttnProcessor2_0.  Here Q, K and V always run as ONE GEMM over the three weight segments with
        the qk-norm + RoPE epilogue (CogVideoXBlock.forward_joint), so there is nothing to fuse: the call records
        the processors like the reference (for unfuse) and leaves weights, state-dict keys and outputs unchanged."""
        for _, proc in self.attn_processors.items():
            if "Added" in type(proc).__name__:
                raise ValueError("`fuse_qkv_projections()` is not supported for models having added KV projections.")
        self.original_attn_processors = self.attn_processors
        self._qkv_fused = True

    def unfuse_qkv_projections(self):
        """Reference :459-470: restores the processors recorded by fuse_qkv_projections (a no-op for the math, as
        fusing is)."""
        if getattr(self, "original_attn_processors", None) is not None:
            self.set_attn_processor(self.original_attn_processors)
        self._qkv_fused = False

    # -- shared pieces --
    def _time_embed(self, timestep, batch: int, device) -> torch.Tensor:
        if not torch.is_tensor(timestep):
            timestep = torch.tensor([timestep] * batch, device=device)
        timestep = timestep.to(device)
        if timestep.dim() == 0:
            timestep = timestep.expand(batch)
        temb0 = K.timestep_embedding(timestep, self.config.num_attention_heads * self.config.attention_head_dim,
                                     float(self.config.freq_shift))
        from .autograd import time_embed_apply
        return time_embed_apply(self.time_embedding, temb0)

    def _token_masks(self, masks: Optional[torch.Tensor], resample: bool, text_len: int):
        """(tok_mask, resample_mask, its uint8 form) of a forward: the latent masks patchified to one byte per video
        token [B, Nv] (None without masks), and with `resample` (id_pool_resample_learnable / return_resample_mask)
        the bool joint-token mask [B, T + Nv] of the resample processor, text rows clear."""
        tok_mask = resample_mask = None
        if masks is not None:
            tok_mask = K.patch_mask(masks.detach().to(self.proj_out.weight.device), self.config.patch_size)
        if resample:
            if tok_mask is None:
                # the reference reads an unbound `masks` here (UnboundLocalError); we fail explicitly
                raise ValueError("id_pool_resample needs masks")
            resample_mask = torch.zeros(tok_mask.shape[0], text_len + tok_mask.shape[1], device=tok_mask.device,
                                        dtype=torch.bool)
            resample_mask[:, text_len:] = tok_mask.bool()
        return tok_mask, resample_mask, _u8(resample_mask)

    def _branch_sample(self, samples: Optional[list], i: int, add_first) -> Optional[torch.Tensor]:
        """The branch sample injected after block i (reference :579-591): each sample serves a run of
        ceil(L / n) consecutive blocks, or with add_first the first n blocks take one each."""
        if not samples:
            return None
        if not add_first:
            return samples[i // int(np.ceil(len(self.transformer_blocks) / len(samples)))]
        return samples[i] if i < len(samples) else None

    def batched_modulations(self, emb: torch.Tensor) -> Optional[torch.Tensor]:
        """Every block's norm1 / norm2 modulation vectors in one launch: bf16 [2 L, B, 6 D], entry 2 i the norm1 and
        2 i + 1 the norm2 modulation of block i, bit-equal to the blocks' own `modulation(emb)` calls — they all read
        silu(emb), and one by one each is a latency-bound launch on the dependency chain between the big kernels.
        The pointer table is cached on the model and rebuilt when a parameter's storage moves.  None (the blocks then
        compute their own): VP_MOD_BATCHED=0 (A/B), or a shape outside the weight-streaming kernel's."""
        blocks = self.transformer_blocks
        if NAT.knob_values.get("VP_MOD_BATCHED") == "0" or len(blocks) == 0:
            return None
        if emb.shape[0] > 2 or emb.shape[1] > 512 or emb.shape[1] % 8 or emb.stride(0) % 8 or emb.data_ptr() % 16:
            return None
        lins = [lin for blk in blocks for lin in (blk.norm1.linear, blk.norm2.linear)]
        return K.linear_small_batched(emb, K.LinearGroupTable.cached(self.__dict__, lins), act_in=K.ACT_SILU)

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor,
                timestep: Union[int, float, torch.LongTensor], timestep_cond: Optional[torch.Tensor] = None,
                image_rotary_emb: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                attention_kwargs: Optional[Dict[str, Any]] = None, branch_block_samples=None,
                branch_block_masks: Optional[torch.Tensor] = None, add_first: Optional[bool] = False,
                self_guidance_hidden_states=None, self_guidance_masks=None,
                return_hidden_states: Optional[bool] = False, return_resample_mask: Optional[bool] = False,
                id_pool_resample_learnable: Optional[bool] = False, return_dict: bool = True,
                cfg_shared_video: bool = False):
        """Reference :472-646.  With autograd on and a parameter or input requiring grad, the differentiable path
        (videopainter_amd/autograd.py: gradient-checkpointed blocks on the HIP backward kernels) runs instead.
        cfg_shared_video (no reference counterpart): the caller's promise that the two batch rows are the
        classifier-free-guidance halves of one sample — equal hidden_states and timestep, only the text differs — so
        the first block computes their shared work once (CogVideoXBlock._attend_cfg_shared); same result up to the
        rounding of that block's attention."""
        from . import autograd as AG
        if AG.needs_grad(self, hidden_states, encoder_hidden_states, branch_block_samples):
            if self_guidance_hidden_states is not None or self_guidance_masks is not None:
                raise NotImplementedError("self-guidance is inference-only (no training script passes it)")
            return self._forward_train(hidden_states, encoder_hidden_states, timestep, image_rotary_emb,
                                       attention_kwargs, branch_block_samples, branch_block_masks, add_first,
                                       self_guidance_hidden_states, return_hidden_states, return_resample_mask,
                                       id_pool_resample_learnable, timestep_cond, return_dict)
        if timestep_cond is not None:
            raise ValueError("timestep_cond requires a cond_proj, which CogVideoX's TimestepEmbedding does not have")
        # LoRA scale per call, default 1.0 (reference :490-499): the folded adapters are re-folded when it changes
        self._call_lora_scale(attention_kwargs)
        prev = (None, None, None)
        if attention_kwargs and "prev_hidden_states" in attention_kwargs:
            prev = (attention_kwargs["prev_hidden_states"], attention_kwargs.get("prev_clip_weight"),
                    attention_kwargs.get("prev_resample_mask"))
        output, hidden_states_list, resample_mask = self._forward_infer(
            hidden_states, encoder_hidden_states, timestep, image_rotary_emb, prev, branch_block_samples,
            branch_block_masks, add_first, self_guidance_hidden_states, self_guidance_masks, return_hidden_states,
            return_resample_mask, id_pool_resample_learnable, cfg_shared_video)
        if not return_dict:
            if return_hidden_states:
                if return_resample_mask:
                    return (output, hidden_states_list, resample_mask)
                return (output, hidden_states_list)
            return (output,)
        return Transformer2DModelOutput(sample=output)

    def _forward_infer(self, hidden_states, encoder_hidden_states, timestep, image_rotary_emb=None,
                       prev=(None, None, None), branch_block_samples=None, branch_block_masks=None, add_first=False,
                       self_guidance_hidden_states=None, self_guidance_masks=None, return_hidden_states=False,
                       return_resample_mask=False, id_pool_resample_learnable=False, cfg_shared_video=False,
                       split=None):
        """The inference forward, written once -> (output, hidden_states_list, resample_mask).  prev: (states, weight,
        resample mask) of the any-length pipeline's previous window (anyl.py:962-988), the states one tensor or
        {layer: tensor}.

        split: one rank's context of the Ulysses head-parallel split (ulysses._Ctx: the shard geometry `sh`, the
        `attend` hook, `gather_rows`).  The forward then runs on the rank's rows of the joint buffer: the row-local
        operands (RoPE table, injection mask; branch_block_samples and prev states are the rank's own) are cut at the
        shard's first video row, the text length is the shard's, the attention goes through the hook — which keeps the
        whole RoPE table and gets the whole masks — and the head gathers every rank's proj_out rows, so each rank
        returns the whole prediction (and its shard's hidden states).  What the split does not do, each marked
        `split is None` below: the batched modulations, the ping-pong output buffers and the bf16 / contiguous copy of
        the branch samples; the callers in ulysses.py pass no self-guidance and no cfg_shared_video."""
        dev = self.proj_out.weight.device
        B, F, C, H, W = hidden_states.shape
        cfg = self.config
        p = cfg.patch_size
        hs = _bf(hidden_states.to(dev))
        enc = _bf(encoder_hidden_states.to(dev))
        T = enc.shape[1]

        emb = self._time_embed(timestep, B, dev)
        x = self.patch_embed.embed(enc, hs)
        if split is not None:
            x = split.shard(x, T)  # (the whole buffer is freed here)
        if self_guidance_hidden_states is not None and self_guidance_masks is None and branch_block_masks is None:
            # the reference reads an unbound `masks` here; we fail explicitly
            raise ValueError("self_guidance_hidden_states need self_guidance_masks or branch_block_masks")
        # the token mask: from self_guidance_masks when given, else from branch_block_masks (reference :518-523); it
        # is the injection mask (when branch_block_masks is given), the resample mask and the self-guidance mask
        tok_mask, resample_mask, rm_u8 = self._token_masks(
            self_guidance_masks if self_guidance_masks is not None else branch_block_masks,
            id_pool_resample_learnable or return_resample_mask, T)
        rope = _rope_dev(image_rotary_emb, dev, grid=(F, H // p, W // p))
        tl, attend = T, None
        if split is not None:
            split.rope_full = rope
            rope, tl, attend = split.sh.rope(rope), split.sh.tl, split.attend
            if tok_mask is not None:
                tok_mask = split.sh.video_rows(tok_mask).contiguous()

        prev_states, prev_w, prev_mask = prev[0], prev[1], _u8(prev[2])
        bs = None
        if branch_block_samples is not None:
            bs = [_bf(s.to(dev)) for s in branch_block_samples] if split is None else list(branch_block_samples)
        hidden_states_list: List[torch.Tensor] = []
        ping = None
        mods = self.batched_modulations(emb) if split is None else None
        for i, block in enumerate(self.transformer_blocks):
            inj = self._branch_sample(bs, i, add_first)
            pj = None
            if prev_states is not None:
                pj = prev_states.get(i) if isinstance(prev_states, dict) else prev_states
            out = None  # (split: the block allocates its own output)
            if split is None and return_hidden_states:
                out = torch.empty_like(x)
            elif split is None:
                out = ping if (ping is not None and ping.data_ptr() != x.data_ptr()) else torch.empty_like(x)
                ping = x
            guide = None
            if self_guidance_hidden_states is not None:
                guide = _bf(self_guidance_hidden_states[i].to(dev))
            # (self-guidance replaces the unmasked video rows BEFORE the injection, reference :593-608: the block then
            # runs without its fused injection, and vp_guide_rows_bf16 applies both)
            x = block.forward_joint(x, tl, emb, rope, rm_u8, pj, prev_w if pj is not None else None,
                                    prev_mask if pj is not None else None, inj if guide is None else None,
                                    tok_mask if (inj is not None and branch_block_masks is not None) else None, out,
                                    attend, mod1=mods[2 * i] if mods is not None else None,
                                    mod2=mods[2 * i + 1] if mods is not None else None,
                                    cfg_shared_video=bool(cfg_shared_video) and i == 0)
            if guide is not None:
                xv = x[:, tl:]
                K.guide_rows(xv, guide.expand_as(xv), tok_mask, inj, inject_all=branch_block_masks is None)
            if return_hidden_states:
                hidden_states_list.append(x)
        output = self._head(x, emb, tl, (B, F, H, W), split.gather_rows if split is not None else None)
        return output, hidden_states_list, resample_mask

    def _head(self, x: torch.Tensor, emb: torch.Tensor, text_len: int, dims, gather=None) -> torch.Tensor:
        """norm_final + norm_out (AdaLN on silu(emb): shift | scale) on the video rows of x, proj_out, then the
        patches back to [B, F, C, H, W] (reference :613-637).  gather: the split's exchange from this rank's proj_out
        rows [B * nv, pc] to every video row [B * Nv, pc]."""
        B, F, H, W = dims
        cfg = self.config
        if not cfg.use_rotary_positional_embeddings:
            raise NotImplementedError("CogVideoX-2B head (norm_final on video rows only) is not on the 5B-I2V path")
        mod = K.linear_small(emb, self.norm_out.linear.weight, self.norm_out.linear.bias, act_in=K.ACT_SILU)
        y = K.final_norm(x, text_len, self.norm_final.weight, self.norm_final.bias, self.norm_out.norm.weight,
                         self.norm_out.norm.bias, self.norm_out.norm.eps, mod)
        proj = K.linear(y.view(-1, y.shape[-1]), self.proj_out.weight, self.proj_out.bias)
        if gather is not None:
            proj = gather(proj, B)
        return K.unpatchify(proj, B, F, cfg.out_channels, H, W, cfg.patch_size)

    def _forward_train(self, hidden_states, encoder_hidden_states, timestep, image_rotary_emb, attention_kwargs,
                       branch_block_samples, branch_block_masks, add_first, self_guidance_hidden_states,
                       return_hidden_states, return_resample_mask, id_pool_resample_learnable, timestep_cond,
                       return_dict):
        """The training step's transformer call (train_cogvideox_inpainting_i2v_video.py:1867-1876): the same
        forward launches, every block a gradient-checkpointed autograd node."""
        from . import autograd as AG
        if timestep_cond is not None or self_guidance_hidden_states is not None:
            raise NotImplementedError("timestep_cond / self-guidance are not on the training path")
        if attention_kwargs and attention_kwargs.get("prev_hidden_states") is not None:
            raise NotImplementedError("the previous-clip blend is inference-only (no backward)")
        if return_hidden_states:
            raise NotImplementedError("return_hidden_states is inference-only (no backward)")
        self._call_lora_scale(attention_kwargs)
        dev = self.proj_out.weight.device
        B, F, C, H, W = hidden_states.shape
        cfg = self.config
        p = cfg.patch_size
        if not cfg.use_rotary_positional_embeddings:
            raise NotImplementedError("CogVideoX-2B head (norm_final on video rows only) is not on the 5B-I2V path")
        hs = _bf(hidden_states.to(dev))
        enc = _bf(encoder_hidden_states.to(dev))
        T = enc.shape[1]
        emb = self._time_embed(timestep, B, dev)
        x = AG.patch_embed_apply(self.patch_embed, enc, hs)
        # (with id_pool_resample: the VideoPainterID training step, train_cogvideox_inpainting_i2v_video_resample.py
        # :1951-1961 — window 0's resample processor, differentiable, autograd.block_backward)
        tok_mask, _, rm_u8 = self._token_masks(branch_block_masks, id_pool_resample_learnable or return_resample_mask,
                                               T)
        rope = _rope_dev(image_rotary_emb, dev, grid=(F, H // p, W // p))
        bs = None
        if branch_block_samples is not None:
            bs = [s.to(dev, BF16) for s in branch_block_samples]
        for i, block in enumerate(self.transformer_blocks):
            inj = self._branch_sample(bs, i, add_first)
            x = AG.block_apply(block, x, T, emb, rope, inj, tok_mask if inj is not None else None, rm_u8)
        output = AG.head_apply(self, x, emb, (B, F, H, W, T))
        if not return_dict:
            return (output,)  # (the reference returns the mask only together with the hidden states)
        return Transformer2DModelOutput(sample=output)


class AdaLayerNorm(nn.Module):
    """DF/models/normalization.py:31-85 with chunk_dim=1 (shift, scale order)."""

    def __init__(self, embedding_dim: int, output_dim: int, norm_elementwise_affine: bool, norm_eps: float):
        super().__init__()
        self.linear = Linear(embedding_dim, output_dim)
        self.norm = LayerNorm(output_dim // 2, norm_eps, norm_elementwise_affine)


def locals_without_self(loc: dict) -> dict:
    return {k: v for k, v in loc.items() if k not in ("self", "__class__")}
