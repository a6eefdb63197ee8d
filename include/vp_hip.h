/* vp_hip.h — C ABI of the MI355X (gfx950) VideoPainter denoising hot path (libvp_hip.so).
 *
 * Every entry point takes plain device pointers, sizes and element strides, plus the HIP stream to launch on
 * (`void* stream` = hipStream_t; NULL = default stream).  No torch types cross this boundary.
 *   - Ownership: the caller allocates every output and workspace; no entry point allocates or frees.
 *   - Errors: return 0 on success, VP_ERR_* (>= 1000) for an argument error detected on the host, or the
 *     hipError_t of the failed launch.  Nothing is printed.
 *   - Threading: stateless and re-entrant; each call is asynchronous on `stream` and may be captured in a graph.
 *   - Storage dtype: bf16 (`__bf16` / torch.bfloat16) unless stated; accumulation is fp32.
 *
 *   - Multi-GPU: the library launches no collective.  The head-parallel (Ulysses) split of one clip
 *     (videopainter_amd/ulysses.py) exchanges buffers these kernels write and read in place: in bf16 the pre-norm
 *     q | k | v, and on the fp8 path (ABI 25) vp_qkv_heads_pack_fp8's send buffer [P, n, B, 4 Dp] — q and k as the
 *     e4m3 operands of vp_attention_fwd_fp8, v in bf16 — whose received form is that kernel's and vp_v_pack_fp8's
 *     operands through strides, and an attention output [P, n, B, Dp] that vp_mx_quantize_heads_bf16 gathers into the
 *     fp8 output projection's MX operand.
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/diffusers/src/diffusers/, abbreviated DF/).  The Python host mirror that binds them by ctypes is
 * videopainter_amd/_native.py; the reference-side binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef VP_HIP_H
#define VP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_OK 0
#define VP_ERR_ARG 1000      /* invalid size / stride / pointer combination */
#define VP_ERR_UNSUPPORTED 1001

/* ABI version: bump when any struct layout or signature below changes. */
#define VP_ABI_VERSION 32
int vp_abi_version(void);
/* "<sha256 of sources + flags>:<sha256 of the compiler version>" of the build (no reference counterpart) */
const char* vp_build_digest(void);
/* A/B switches of the library (kernel-variant selection only, never numerics of the default path; DESIGN_LOG.md §5):
 * VP_GEMM_VARIANT, VP_GEMM_NO_TAIL, VP_GEMM_GROUP, VP_GEMM8_VARIANT, VP_ATTN_BOUNDED_MODE, VP_ATTN_UNBOUNDED_MODE,
 * VP_ATTN_NO_SPLIT, VP_ATTN8_VARIANT, VP_T5_ATTN, VP_CONV_HOIST, VP_CONV_PIPE,
 * VP_ATTN_BWD_VARIANT, VP_ATTN_TAIL, VP_ATTN_PERSIST, and two that the library only stores for its Python front end
 * ("0" = off): VP_CFG_SHARED (the CFG halves' shared first-block work) and VP_MOD_BATCHED (one launch for a forward's
 * AdaLN modulation linears).  Each is read from the environment
 * once, when the library is loaded; afterwards only vp_set_knob changes it (value NULL = unset), e.g. a test that
 * runs two variants on the same operands.  Returns VP_ERR_ARG for an unknown name or a value over 31 bytes.  Host
 * only; not thread-safe against launches in flight on other host threads.  (ABI 14.) */
int vp_set_knob(const char* name, const char* value);
/* sizeof of the descriptor structs as compiled into the library: out[0..14] = gemm, attn, dpm, gemm_mx, attn_fp8,
 * conv3d, attn_bwd, mt_tensor, mt_chunk, optim_scalars, zero_range, zero_record, attn_merge, linear_group,
 * prodigy_scalars (ABI check) */
void vp_struct_sizes(int64_t* out);

/* ---------------------------------------------------------------------------------------------------------------
 * GEMM  C = epilogue(A · Wᵀ)   — replaces every nn.Linear / patch-embed conv on the path:
 *   attn.to_q/to_k/to_v/to_out.0 (DF/models/attention_processor.py:2132-2134,2202), FeedForward net.0.proj + GELU
 *   and net.2 (DF/models/attention.py:1177,1191; activations.py:65-90), the gated residuals
 *   (DF/models/transformers/cogvideox_transformer_3d.py:169-170,181-182), the branch injection (:596-609), the
 *   patch-embed conv + text_proj + pos-emb (DF/models/embeddings.py:400-454), the branch zero-linears
 *   (DF/models/branch_cogvideox.py:415-421) and proj_out (cogvideox_transformer_3d.py:624).
 * A: bf16 [M, K] (row stride lda); W: up to 3 weight segments, each bf16 [n_seg, K] (nn.Linear layout), columns
 * [s*n_seg, (s+1)*n_seg) of C come from segment s (fused QKV without packing the weights).  K % 8 == 0
 * (a K tail is zero-filled on the device), N % 8 == 0 and n_seg % 8 == 0 (VP_ERR_ARG otherwise, from vp_gemm_bf16 and
 * vp_gemm_bf16_ws alike: two segments of n_seg % 8 == 4 have N % 8 == 0, but an 8-row weight block and an 8-column
 * output chunk would straddle the segment boundary).
 * Output row remap: C row of GEMM row m = (m / rows_per_group) * group_stride + row_offset + (m % rows_per_group).
 * ------------------------------------------------------------------------------------------------------------- */
enum {
  VP_EPI_BIAS = 0,        /* C = rnd(acc + bias)                                                            */
  VP_EPI_BIAS_GELU = 1,   /* C = rnd(gelu_tanh(rnd(acc + bias)))                                             */
  VP_EPI_BIAS_SCALE = 2,  /* C = rnd(rnd(acc + bias) * alpha)            (branch conditioning_scale)         */
  VP_EPI_GATED = 3,       /* C = rnd(R + rnd(gate * rnd(acc + bias))) [then rnd(C + inject) on video rows]   */
  VP_EPI_BIAS_ADDROWS = 4, /* C = rnd(rnd(acc + bias) + addrows[(m % rows_per_group) + addrows_offset, n])  */
  /* 5 = VP_EPI_BIAS_GELU_MXFP8 (vp_gemm_mx_fp8 only, below) */
  VP_EPI_BIAS_QKNORM_ROPE = 6, /* fused QKV projection: segments 0 / 1 (q / k): every 64-column head of
                               * y = rnd(acc + bias) -> rnd(LayerNorm64(y; qk_ln_w[s], qk_ln_b[s], qk_eps[s])), then on
                               * video rows (m % tokens_per_batch >= text_len) the interleaved-pair RoPE from
                               * rope_cos / rope_sin (fp32 [tokens_per_batch - text_len][64]) -> rnd; segment 2 (v) as
                               * VP_EPI_BIAS.  = vp_gemm_bf16 + vp_head_norm_rope_bf16 on q and k, bit for bit. */
  VP_EPI_GELU_BWD = 7     /* C = rnd(rnd(acc + bias) * gelu_tanh'(Z[m, n])), Z = R (bf16 [M][N], row m at ldr; no
                           * row remap): the FeedForward's dgrad through its GELU — the dgrad GEMM of net.2 followed
                           * by vp_gelu_bwd_bf16, bit for bit, in one pass (ABI 17) */
};

typedef struct vp_gemm_desc {
  int32_t M, N, K, epilogue;
  const void* A;
  int64_t lda;
  const void* W[3];
  const void* bias[3]; /* bf16 [n_seg] per segment, or NULL */
  int32_t n_seg, pad0;
  void* C;
  int64_t ldc;
  int32_t rows_per_group, pad1;
  int64_t group_stride, row_offset;
  float alpha;
  int32_t pad2;
  /* VP_EPI_GATED: rows are (batch, token) of a [B, tokens_per_batch, N] stream; text tokens (token < text_len)
   * take gate_text[b], video tokens gate[b]; gate vectors bf16 [N] at batch stride gate_bstride.  R may alias C. */
  const void* R;
  int64_t ldr;
  const void* gate;
  const void* gate_text;
  int64_t gate_bstride;
  int32_t tokens_per_batch, text_len;
  /* optional branch injection on video rows: C += inject[b, token - text_len, :] where inject_mask[b, v] == 0
   * (or always when inject_mask == NULL) */
  const void* inject;
  int64_t inject_ld, inject_bstride;
  const uint8_t* inject_mask;
  int64_t inject_mask_bstride;
  /* VP_EPI_BIAS_ADDROWS */
  const void* addrows;
  int64_t addrows_ld, addrows_offset;
  /* VP_EPI_BIAS_QKNORM_ROPE (norm_q / norm_k are LayerNorm(64) with affine bf16 weights; rows_per_group == M) */
  const void* qk_ln_w[2];
  const void* qk_ln_b[2];
  float qk_eps[2];
  const float* rope_cos; /* NULL: no RoPE (image_rotary_emb None) */
  const float* rope_sin;
  /* Per-segment A tail (unfused LoRA, PEFT's y = x W^T + s (x A^T) B^T as ONE GEMM on K-augmented operands;
   * DF/loaders/lora_pipeline.py:2632-2705 load_lora_into_transformer, infer/inpaint.py:310-316): a_tail_k > 0 splits
   * K at a_tail_k; for k >= a_tail_k, segment s reads A column k + a_tail_off[s] (its own rank block of
   * T = x [A_0; A_1; ...]^T stored after x in the same rows), so every weight segment carries only its own rank
   * (W_s = [W0_s | s B_s], K = a_tail_k + r).  Needs K % 64 == a_tail_k % 64 == 0, n_seg % 256 == 0 with more than one
   * segment, the default
   * main loop (VP_ERR_UNSUPPORTED otherwise) and epilogue BIAS, GATED or BIAS_QKNORM_ROPE.  0: no tail.  (ABI 14.) */
  int32_t a_tail_k, pad3;
  int64_t a_tail_off[3];
  /* VP_EPI_BIAS_QKNORM_ROPE with a separable 3D RoPE table (ABI 16; NULL rope_ax[0]: the full table): rope_ax = the
   * per-axis factors of rope_cos / rope_sin — cos_t, sin_t [F][16], cos_y, sin_y [Hh][24], cos_x, sin_x [Ww][24] fp32,
   * exact slices of the full table (CogVideoX's 3D RoPE, DF/models/embeddings.py:457-530: dims 0-15 by frame, 16-39 by
   * row, 40-63 by column) — with rope_hw = Hh * Ww, rope_w = Ww and their division magics rope_mhw / rope_mw
   * (ceil(2^32 / d)); the epilogue reads those rows (a few KB, cache-resident) instead of the token's row of the
   * [F*Hh*Ww][64] table: the same values, bit-identical output.  rope_cos / rope_sin stay set. */
  const float* rope_ax[6];
  int32_t rope_hw, rope_w;
  uint32_t rope_mhw, rope_mw;
  /* Optional second output for the training forward (ABI 17; NULL: none), bf16, row m of the GEMM at aux + m * ld_aux
   * (no row remap): VP_EPI_BIAS_GELU writes the pre-activation rnd(acc + bias) there (the GELU's backward input, so
   * no separate vp_gelu_bf16 pass); VP_EPI_BIAS_QKNORM_ROPE writes the pre-norm rnd(acc + bias) of segments 0 / 1
   * (q | k, columns [0, 2 n_seg)) there (the LayerNorm backward's input); vp_gemm_mx_fp8's VP_EPI_BIAS_GELU_MXFP8
   * writes the pre-activation as VP_EPI_BIAS_GELU does (ABI 28).  Other epilogues: VP_ERR_ARG. */
  void* aux;
  int64_t ld_aux;
} vp_gemm_desc;

int vp_gemm_bf16(const vp_gemm_desc* d, void* stream);

/* 1 when the GEMM main loop VP_GEMM_VARIANT = variant (1, 5, 11, 13 = the default; 12, 20, 30 only in a
 * VP_GEMM_EXTRA_VARIANTS build: the rejected A/B loops) is in this library, else 0.  Host-only.  vp_gemm_bf16 returns
 * VP_ERR_UNSUPPORTED for a variant outside the build.  (ABI 13.) */
int vp_gemm_variant_built(int variant);

/* Split-K form for GEMMs too small to fill the chip (fewer than 128 output tiles of 256 x 256, e.g. the T5 encoder's
 * projections at M = 2 x 226 token rows; reference callers: transformers T5EncoderModel, anyl.py:216-256): the K
 * range is cut into chunks of >= 512, each (tile, chunk) workgroup writes its fp32 partial tile to `workspace`, and a
 * reduce pass sums the chunks in a fixed order (deterministic) and applies the epilogue (VP_EPI_BIAS, _GELU, _SCALE,
 * _GATED, _BIAS_ADDROWS, _GELU_BWD; VP_EPI_BIAS_QKNORM_ROPE and a_tail_k > 0 never split).
 * vp_gemm_bf16_workspace_bytes: bytes this descriptor needs (0: no split, and vp_gemm_bf16_ws then runs
 * vp_gemm_bf16).  vp_gemm_bf16 never splits. */
int64_t vp_gemm_bf16_workspace_bytes(const vp_gemm_desc* d);
int vp_gemm_bf16_ws(const vp_gemm_desc* d, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * MX-FP8 (OCP e4m3 elements, one E8M0 power-of-two scale per 32 consecutive K elements) — the fp8 path of
 * BASELINE config 5.  The same projections as vp_gemm_bf16 (FeedForward net.0.proj / net.2,
 * DF/models/attention.py:1177,1191), on gfx950's block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4: 2x the
 * bf16 MFMA rate; the hardware applies the scales, so the accumulator is the dequantised dot product).
 *
 * Data layout of an MX tensor with R rows and K columns (K % 128 == 0):
 *   elements: uint8 e4m3 [R][K] at row stride ld (bytes);
 *   scales:   uint8 E8M0 (value 2^(s-127)) in 256-row x 128-column tiles of 1 KiB, tile (R/256, K/128) at
 *             byte ((r >> 8) * (K / 128) + (k >> 7)) * 1024, and inside it block b = (k >> 5) & 3 of row r at
 *             b * 256 + (r & 15) * 16 + ((r >> 4) & 15) — one GEMM K-step's scales are one contiguous 1 KiB
 *             LDS-DMA, and a lane's scales for 4 consecutive 16-row fragments are one aligned dword.
 *             Size: ceil(R / 256) * (K / 128) * 1024 bytes.
 * Quantisation of a 32-element block x: s = ceil(log2(amax|x| / 448)) (clamped to [-127, 127]),
 * q = RNE_e4m3(x * 2^-s) (|q| <= 448, no clipping), scale byte s + 127 (0 for an all-zero block).
 * ------------------------------------------------------------------------------------------------------------- */
#define VP_MX_BLOCK 32
int64_t vp_mx_scale_bytes(int64_t rows, int64_t K);

/* rows x K bf16 (row stride ld_in elements) -> MX e4m3 (row stride ld_out bytes) + scales (layout above) */
int vp_mx_quantize_bf16(const void* x, int64_t ld_in, void* q, int64_t ld_out, void* scales, int32_t rows, int32_t K,
                        void* stream);

/* The same quantiser reading the head-parallel (Ulysses) split's second receive buffer (ABI 25): x bf16
 * [P, n, B, Dp] contiguous (head group, row, batch; 16-byte aligned) -> the MX tensor of B * n rows and K = P * Dp
 * columns whose row b * n + i, columns [j * Dp, (j + 1) * Dp) are x[j, i, b, :] — the fp8 output projection's operand
 * without the re-layout copy; byte for byte vp_mx_quantize_bf16 of the re-laid-out [B * n, K] tensor.  Dp % 64 == 0
 * (whole heads: a 32-element block never straddles two head groups), K % 128 == 0, ld_out >= K bytes. */
int vp_mx_quantize_heads_bf16(const void* x, void* q, int64_t ld_out, void* scales, int32_t B, int32_t n, int32_t P,
                              int32_t Dp, void* stream);

/* out = epilogue(A · Wᵀ) with A and W in MX-FP8.  base: as vp_gemm_desc with A / W[] pointing at the e4m3
 * elements (lda in BYTES; W rows are K bytes), epilogues VP_EPI_BIAS .. VP_EPI_BIAS_ADDROWS writing bf16 C, or
 * VP_EPI_BIAS_GELU_MXFP8: C = MX-quantise(rnd(gelu_tanh(rnd(acc + bias)))) written as e4m3 [M][N] (ldc in bytes)
 * plus c_scale (the FF1 -> FF2 hand-off stays in fp8).  K % 128 == 0, N % 256 == 0.
 * ABI 28, the training step through frozen fp8 blocks (forward and dgrad run against constant weights):
 *   - VP_EPI_BIAS_GELU_MXFP8 with base.aux / ld_aux set also stores the bf16 pre-activation z = rnd(acc + bias) to
 *     aux (ld_aux >= N, % 8), bit-equal to what VP_EPI_BIAS writes; the MX C / c_scale bytes are those without aux.
 *     aux with any other epilogue: VP_ERR_ARG.
 *   - VP_EPI_GELU_BWD_MXFP8: C = MX-quantise(rnd(rnd(acc + bias) * gelu_tanh'(Z[m, n]))) as e4m3 [M][N] plus c_scale,
 *     Z = base.R (bf16 [M][N], row m at ldr >= N, % 8; no row remap) as VP_EPI_GELU_BWD reads it: the FF2 dgrad whose
 *     output is the FF1 dgrad's MX operand, byte for byte vp_mx_quantize_bf16 of the bf16 VP_EPI_GELU_BWD result. */
#define VP_EPI_BIAS_GELU_MXFP8 5
#define VP_EPI_GELU_BWD_MXFP8 8
typedef struct vp_gemm_mx_desc {
  vp_gemm_desc base;
  const void* a_scale;
  const void* w_scale[3];
  void* c_scale;
} vp_gemm_mx_desc;

int vp_gemm_mx_fp8(const vp_gemm_mx_desc* d, void* stream);


/* ---------------------------------------------------------------------------------------------------------------
 * Flash attention forward, head_dim 64, non-causal, no mask — replaces F.scaled_dot_product_attention in
 * CogVideoXAttnProcessor2_0 (DF/models/attention_processor.py:2177-2197) and CogVideoXAttnProcessor2_0_resample
 * (:2283-2290; the doubled K/V is passed as two segments instead of being concatenated).
 * Element (b, h, n, d) of Q is Q[b*q_sb + n*q_sn + h*64 + d]; likewise K, V, K2, V2, O.
 * O = rnd(out_scale * rnd(softmax(scale Q Kᵀ) V)) (+ O_old when accumulate) — the prev-clip blend.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct vp_attn_desc {
  int32_t B, H, Nq, head_dim;
  const void* Q;
  int64_t q_sb, q_sn;
  const void* K;
  const void* V;
  int64_t k_sb, k_sn, v_sb, v_sn;
  int32_t Nk, Nk2;
  const void* K2; /* optional second key/value segment (Nk2 == 0: none) */
  const void* V2;
  int64_t k2_sb, k2_sn, v2_sb, v2_sn;
  void* O;
  int64_t o_sb, o_sn;
  float scale, out_scale;
  int32_t accumulate;
  int32_t flags; /* VP_ATTN_BOUNDED_SCORES: the caller guarantees |scale * q.k| * log2(e) <= VP_ATTN_SCORE_BOUND for
                    every (query, key) pair, so the kernel runs without a reference point (p2: exact, bf16/fp32 hold
                    2^+-60 and O / l is invariant to the reference point).  CogVideoX's qk-LayerNorm gives the bound
                    from the norm weights: videopainter_amd.kernels.score_bound_log2.  Without the flag (any
                    scores): p2a, the same pipeline with an anchored reference point, plus a re-run of the blocks it
                    flags by the exact anchored 16x16x32 kernel — which needs the workspace of
                    vp_attention_fwd_bf16_ws (without one the 16x16x32 kernel runs alone). */
  float* lse;     /* optional fp32 [B, H, Nq]: per query log2-sum-exp2 of the scaled log2-unit scores (m + log2 l), the
                     softmax statistics vp_attention_bwd_bf16 recomputes P from (bf16 kernel only; NULL: not written) */
  const int32_t* k2_full; /* optional int32 [B] (device), a hint: segment-2 rows n >= k2_full[b] of V2 are zero
                             (the caller guarantees it), so those keys enter only the row sums — the resample
                             processor's null keys, partitioned behind its masked keys by vp_partition_rows_index.
                             The 16x16x32 kernels skip their V^T DMA, reads and PV products for whole tiles past
                             k2_full[b]; the other kernels read the zeros.  NULL: no hint. */
  const int32_t* k2_len;  /* optional int32 [B] (device): segment 2 holds only its first min(k2_len[b], Nk2) keys for
                             batch row b (the rest are not read) — the resample processor's masked rows when its null
                             keys are summed in closed form (vp_null_key_mass).  NULL: Nk2 keys for every row. */
  const float* l_extra;   /* optional fp32 [B, H, Nq] (device): log2 of extra row-sum mass per query, in the kernel's
                             score units (scale * log2 e * q.k), added to the softmax denominator — the null keys'
                             total exp2(score) (their values are zero).  -inf: none.  NULL: nothing added.
                             k2_len / l_extra are taken by the s16 / a16 and the p2 / p2a kernels, k2_full by the
                             16x16x32 kernels only (a k2_full launch runs s16 / a16). */
} vp_attn_desc;
#define VP_ATTN_BOUNDED_SCORES 1
/* flags bit (ABI 23): O is fp32 [B, Nq, H*64] (o_sb / o_sn in fp32 elements, multiples of 4; base 16-byte aligned) and
 * receives softmax(...) V unrounded — a partial for vp_attention_merge_bf16, which then rounds once.  Needs
 * out_scale == 1 and no accumulate.  Every bf16 kernel variant, the tail-piece combine and the a16 redo take it. */
#define VP_ATTN_OUT_F32 2
#define VP_ATTN_SCORE_BOUND 60.0f

int vp_attention_fwd_bf16(const vp_attn_desc* d, void* stream);

/* The same with a caller-provided workspace for the grid-tail split: when the last round of workgroups would run
 * on a mostly idle chip (blocks mod resident slots <= half the slots), those blocks run as several key-range
 * workgroups each plus a merge pass.  vp_attention_workspace_bytes: bytes needed for this descriptor (0: no split;
 * -1: invalid descriptor).  A null or too small workspace runs the unsplit grid. */
int64_t vp_attention_workspace_bytes(const vp_attn_desc* d);
int vp_attention_fwd_bf16_ws(const vp_attn_desc* d, void* workspace, int64_t workspace_bytes, void* stream);

/* 1 when the attention kernel variant `name` (the values of the A/B environment switches VP_ATTN_BOUNDED_MODE /
 * VP_ATTN_UNBOUNDED_MODE: "p2", "p2a", "s16", "a16", and with a VP_ATTN_EXTRA_VARIANTS build "lazy", "w32", "w64",
 * "w64f", "s16i", "p1"; "fp8:N" for the fp8 kernel's VP_ATTN8_VARIANT = N: 2 and 3, and 1 and 4 with that build) is
 * in this library, else 0.  Host-only.  A launch that names a variant outside the build returns VP_ERR_UNSUPPORTED. */
int vp_attention_variant_built(const char* name);

/* Merge of two attention partials over disjoint key sets (ABI 23): given (O_a, lse_a) and (O_b, lse_b) of the same
 * queries, O = rnd((2^lse_a O_a + 2^lse_b O_b) / (2^lse_a + 2^lse_b)) per (batch, head, query) — the attention over
 * the union of the two key sets.  O_a / O_b: bf16 [B, Nq, H*64], or with flags & VP_MERGE_IN_F32 both fp32 (the
 * VP_ATTN_OUT_F32 outputs: the merged result is then rounded once, like a single attention call's; with bf16 partials
 * it carries their rounding too).  O: bf16 [B, Nq, H*64].
 * Element (b, h, n, d) at X[b*x_sb + n*x_sn + h*64 + d] (strides in elements, multiples of 8; bases 16-byte aligned);
 * lse_a / lse_b: fp32 [B, H, Nq] in the log2 units of vp_attn_desc.lse, batch stride la_sb / lb_sb (elements).  A
 * batch stride of 0 is allowed on either input: one partial read by every batch row (the video-query x video-key
 * part the two classifier-free-guidance halves share).  The weights are taken relative to max(lse_a, lse_b), so
 * nothing overflows; an input whose lse is -inf contributes nothing (its values are not read); both -inf: zeros. */
typedef struct vp_attn_merge_desc {
  int32_t B, H, Nq, head_dim;
  const void* Oa;
  int64_t oa_sb, oa_sn;
  const float* lse_a;
  int64_t la_sb;
  const void* Ob;
  int64_t ob_sb, ob_sn;
  const float* lse_b;
  int64_t lb_sb;
  void* O;
  int64_t o_sb, o_sn;
  int32_t flags; /* VP_MERGE_IN_F32 */
  int32_t pad0;
} vp_attn_merge_desc;
#define VP_MERGE_IN_F32 1
int vp_attention_merge_bf16(const vp_attn_merge_desc* d, void* stream);

/* fp8 attention (BASELINE config 5 "attn + FFN in fp8"; same math as vp_attention_fwd_bf16).
 * base.Q / base.K: e4m3 [B, N, H*64] written by vp_head_norm_rope_fp8 (strides in bytes, multiples of 16), each
 * carrying one power-of-two factor undone by the E8M0 bytes in qk_scale (bits 0-7: Q, bits 8-15: K; Q's factor
 * also includes scale * log2 e, so base.scale is ignored).  base.V: V^T e4m3 [B, H, 64, npad] and vs: its scales,
 * both from vp_v_pack_fp8.  base.O / out_scale / accumulate as in the bf16 kernel.  The probabilities P enter the
 * PV product (and the row sums) as e4m3 codes of p * 2^7 made by linear mantissa interpolation of exp2 (relative
 * error 3.2 % rms) — DESIGN_LOG.md §3.1.  env VP_ATTN8_VARIANT (A/B): 2, 3 and 5 (the default) are the valid values;
 * variant 1 (exp2 + round-to-nearest e4m3) and variant 4 were pruned and return VP_ERR_UNSUPPORTED.
 *
 * A second key segment (ABI 24; the resample processor's masked keys; base.Nk2 == 0: none, ABI 23's behaviour).  The
 * keys of batch row b are segment 1 followed by the first min(base.k2_len[b], Nk2) keys of segment 2 (k2_len NULL: all
 * Nk2; a row with 0 reads nothing of K2 / V2).  base.K2: e4m3 [B, Nk2, H*64] (k2_sb / k2_sn in bytes, multiples of
 * 16) with K's static factor, so qk_scale serves both; base.V2: a second V^T pack [B, H, 64, npad2] with scales vs2
 * (vp_v_pack_fp8_lens with the same lengths: the kernel reads whole 64-key tiles of the pack, so V rows past the
 * length must be packed as zeros, not left as they are).  Same scores, P codes, rescale rule and order of accumulation,
 * tile after tile over segment 1 and then segment 2, each segment's last partial tile masked against its own length.
 * base.l_extra (score units, as in vp_attn_desc): exp2(l_extra - m) is added to the fp32 row sum once after the last
 * tile, m the kernel's final reference; -inf adds nothing, a huge value takes the output row to 0, never NaN.
 * base.k2_full: VP_ERR_UNSUPPORTED.  A second segment, k2_len or l_extra with VP_ATTN8_VARIANT 2 or 3:
 * VP_ERR_UNSUPPORTED (the default kernel alone has the two-segment instance). */
typedef struct vp_attn_fp8_desc {
  vp_attn_desc base;
  const void* vs;
  int32_t npad;     /* ceil(Nk / 64) * 64 */
  int32_t qk_scale; /* E8M0 bytes: Q | K << 8 */
  const void* vs2;  /* scales of the V^T pack base.V2 (ABI 24; NULL with Nk2 == 0) */
  int32_t npad2;    /* ceil(Nk2 / 64) * 64 */
  int32_t pad0;
} vp_attn_fp8_desc;

int vp_attention_fwd_fp8(const vp_attn_fp8_desc* d, void* stream);
/* The same with a workspace (ABI 20): the default kernel runs persistent — resident workgroups take the query blocks
 * by per-XCD ticket — when vp_attention_fp8_workspace_bytes (0: none needed, -1: invalid) bytes are given; a smaller
 * or NULL workspace runs one workgroup per block (same results, bit for bit). */
int64_t vp_attention_fp8_workspace_bytes(const vp_attn_fp8_desc* d);
int vp_attention_fwd_fp8_ws(const vp_attn_fp8_desc* d, void* workspace, int64_t workspace_bytes, void* stream);

/* V [B, N, H*64] bf16 (row stride v_sn, batch stride v_sb, elements) -> V^T e4m3 [B, H, 64, npad] with the keys of
 * every 64-key tile in MFMA K-slot order, plus one E8M0 scale per (d, 32 keys) (MX rule of vp_mx_quantize_bf16).
 * Padded keys are zero.  vp_v_pack_fp8_bytes returns the V^T bytes and reports npad and the scale bytes. */
int64_t vp_v_pack_fp8_bytes(int32_t B, int32_t H, int32_t N, int64_t* npad, int64_t* scale_bytes);
int vp_v_pack_fp8(const void* V, int64_t v_sb, int64_t v_sn, int32_t B, int32_t N, int32_t H, void* vt, void* vs,
                  void* stream);
/* The same with a per-row length (ABI 24): lens int32 [B] (device; NULL: vp_v_pack_fp8).  Rows n >= lens[b] of batch
 * row b are packed as zeros and are not read (they may hold NaN bit patterns, and a zero P code times a NaN V byte is
 * NaN on the MFMA); a 64-key tile that lies wholly at or past lens[b] is not written at all — the attention with
 * k2_len = lens never reads it. */
int vp_v_pack_fp8_lens(const void* V, int64_t v_sb, int64_t v_sn, int32_t B, int32_t N, int32_t H, void* vt,
                       void* vs, const int32_t* lens, void* stream);


/* ---------------------------------------------------------------------------------------------------------------
 * AdaLN-Zero modulate — CogVideoXLayerNormZero.forward (DF/models/normalization.py:373-379):
 * y = rnd(rnd(rnd(LN(x)) * rnd(1 + scale)) + shift) over rows of x [B, Ntok, D] (contiguous).  mod is the bf16
 * output of the block's norm linear, [B, 6D] = shift | scale | gate | enc_shift | enc_scale | enc_gate at batch
 * stride mod_bstride; text rows (token < text_len) use the enc_* chunks.  LN affine (ln_w, ln_b), eps.  y rows at
 * stride ldy (>= D, % 8 == 0: e.g. the first D columns of an unfused-LoRA projection's K-augmented operand; ABI 15).
 * ------------------------------------------------------------------------------------------------------------- */
int vp_adaln_modulate_bf16(const void* x, void* y, int64_t ldy, int32_t B, int32_t Ntok, int32_t D, int32_t text_len,
                           const void* ln_w, const void* ln_b, float eps, const void* mod, int64_t mod_bstride,
                           void* stream);
/* the same, writing the modulated rows as MX-FP8 (q: e4m3 [B*Ntok][D], scales: MX layout with R = B*Ntok, K = D)
 * — the input of the fp8 FeedForward (BASELINE config 5).  D % 128 == 0. */
int vp_adaln_modulate_mx_fp8(const void* x, void* q, void* scales, int32_t B, int32_t Ntok, int32_t D,
                             int32_t text_len, const void* ln_w, const void* ln_b, float eps, const void* mod,
                             int64_t mod_bstride, void* stream);
/* both at once, from one read of x (ABI 32): y receives the bytes vp_adaln_modulate_bf16 writes (rows at stride ldy)
 * and q / scales the bytes vp_adaln_modulate_mx_fp8 writes, bit for bit — the MX quantiser reads the bf16-rounded row
 * in either kernel.  For the fp8 QKV projection under unfused LoRA: the MX rows are the base GEMM's operand, the bf16
 * rows the adapters' (T = x A^T, and in training dA = dT^T x).  D % 128 == 0. */
int vp_adaln_modulate_bf16_mx_fp8(const void* x, void* y, int64_t ldy, void* q, void* scales, int32_t B, int32_t Ntok,
                                  int32_t D, int32_t text_len, const void* ln_w, const void* ln_b, float eps,
                                  const void* mod, int64_t mod_bstride, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-head LayerNorm(64) + interleaved-pair RoPE — attn.norm_q / norm_k (attention_processor.py:2143-2146) and
 * apply_rotary_emb on tokens >= text_len (:2149-2154; DF/models/embeddings.py:655-701).
 * x_in/x_out: [B, Ntok, H*64] with row stride ld_* and batch stride bs_*; may alias.  cos/sin fp32 [Ntok-text_len,
 * 64] (NULL: no RoPE).  Optional pre-mask (resample processor, attention_processor.py:2251-2256): if tok_mask !=
 * NULL the input row is first replaced by rnd(rnd(x * tok_mask[b, n]) * pre_scale) — LN of a zeroed row gives the
 * LN bias (the "null key").
 * ------------------------------------------------------------------------------------------------------------- */
int vp_head_norm_rope_bf16(const void* x_in, int64_t ld_in, int64_t bs_in, void* x_out, int64_t ld_out,
                           int64_t bs_out, int32_t B, int32_t Ntok, int32_t H, int32_t text_len, const void* ln_w,
                           const void* ln_b, float eps, const float* cos, const float* sin, const uint8_t* tok_mask,
                           int64_t mask_bstride, float pre_scale, const int32_t* dst_rows, void* stream);

/* The same LN(64) + RoPE, output e4m3 (x_bf16 * out_mul, clamped to +-448, RNE) for the fp8 attention; ld_out /
 * bs_out in bytes. */
int vp_head_norm_rope_fp8(const void* x_in, int64_t ld_in, int64_t bs_in, void* q_out, int64_t ld_out,
                          int64_t bs_out, int32_t B, int32_t Ntok, int32_t H, int32_t text_len, const void* ln_w,
                          const void* ln_b, float eps, const float* cos, const float* sin, float out_mul,
                          void* stream);
/* The same with the pre-mask and the row permutation of vp_head_norm_rope_bf16 (ABI 24; the fp8 attention's second
 * key segment): the input row is first replaced by rnd(rnd(x * tok_mask[b, n]) * pre_scale) when tok_mask != NULL,
 * and output row n of batch b is written to row dst_rows[b * Ntok + n] when dst_rows != NULL (a negative entry:
 * neither read nor written).  Each byte is e4m3 of the bf16 value vp_head_norm_rope_bf16 writes, times out_mul. */
int vp_head_norm_rope_fp8_rows(const void* x_in, int64_t ld_in, int64_t bs_in, void* q_out, int64_t ld_out,
                               int64_t bs_out, int32_t B, int32_t Ntok, int32_t H, int32_t text_len,
                               const void* ln_w, const void* ln_b, float eps, const float* cos, const float* sin,
                               float out_mul, const uint8_t* tok_mask, int64_t mask_bstride, float pre_scale,
                               const int32_t* dst_rows, void* stream);

/* The send packer of the head-parallel (Ulysses) split's fp8 path (ABI 25; no reference counterpart): one launch that
 * reads a row shard's pre-norm fused projection qkv bf16 [B, n, 3 * H * 64] (row stride ld_in, batch stride bs_in,
 * elements; 16-byte aligned, multiples of 8) once and writes the first all-to-all's send buffer, uint8
 * [P, n, B, 4 * Dp] contiguous with Dp = (H / P) * 64 (H % P == 0): for head group j, row i, batch b
 *   bytes [0, Dp)       q of the group's heads as e4m3 — the bytes vp_head_norm_rope_fp8 writes for those columns with
 *                       q_ln_w / q_ln_b / q_eps and out_mul = q_mul (scale * log2 e * 2^q_exp),
 *   bytes [Dp, 2 Dp)    k likewise with k_ln_w / k_ln_b / k_eps and k_mul (2^k_exp),
 *   bytes [2 Dp, 4 Dp)  v of the group's heads, bf16, unchanged.
 * text_len (0 .. n) and cos / sin (fp32 [n - text_len, 64], zero rows for padding; NULL: no RoPE) are the shard's.
 * Chunk j is what rank j receives; the [n, B] order inside a chunk makes the received [P, n, B, 4 Dp] buffer the
 * attention's operands as it stands: q8 / k8 / v of every row of the head group are strided views of it (row stride
 * B * 4 Dp bytes, batch stride 4 Dp bytes) for vp_attention_fwd_fp8 and vp_v_pack_fp8. */
int vp_qkv_heads_pack_fp8(const void* qkv, int64_t ld_in, int64_t bs_in, void* send, int32_t B, int32_t n, int32_t H,
                          int32_t P, int32_t text_len, const void* q_ln_w, const void* q_ln_b, float q_eps,
                          const void* k_ln_w, const void* k_ln_b, float k_eps, const float* cos, const float* sin,
                          float q_mul, float k_mul, void* stream);

/* y[b, n, :] = rnd(rnd(x[b, n, :] * tok_mask[b, n]) * scale) — the masked value copy of the resample processor. */
/* (vp_head_norm_rope_bf16 and vp_mask_scale_rows_bf16 with dst_rows != NULL: output row n of batch b is written to
 * row dst_rows[b * Ntok + n] — the partition permutation of vp_partition_rows_index; a negative entry skips the row
 * (neither read nor written: the null rows when their keys are summed in closed form); the output must not alias the
 * input.) */

/* Stable partition of the resample processor's token mask (attention_processor.py:2244-2252): per batch row b,
 * counts[b] = #{n : mask[b, n] != 0}, dst_rows[b * N + n] = the rank of n among the set rows, or counts[b] + its
 * rank among the clear rows.  Written once per window (the mask is the same for every layer and step); the masked
 * keys / values then form the first counts[b] rows of the attention's second segment and the null keys (zero
 * values) the rest (vp_attn_desc.k2_full). */
int vp_partition_rows_index(const uint8_t* mask, int64_t mask_bstride, int32_t B, int32_t N, int32_t* dst_rows,
                            int32_t* counts, void* stream);

/* The resample processor's null keys in closed form (attention_processor.py:2244-2290 with mask 0: key LN(0) = the
 * norm_k bias beta, rotated by the position's RoPE on video rows; value 0).  With CogVideoX's separable 3D RoPE
 * (dims 0-15 by frame, 16-39 by row, 40-63 by column) a null key's score is S_t(t) + S_y(y) + S_x(x), so the
 * per-query sum of exp2(score) over all null keys factorises over the grid (DESIGN_LOG.md §3.0).
 * vp_mask_null_segments: the null pattern of the token mask [B, T + F*Hh*Ww] (text rows first), once per mask:
 *   segs (16-byte records, capacity B*F*Hh): per (b, t) the runs of equal consecutive rows that hold null keys —
 *   byte 0 = first row, 1 = end row, 2 = run count (<= 6, or 255: the row is scanned instead), bytes 4+2k / 5+2k =
 *   run k's [start, end) columns; meta int32 [B*F + B]: segments per (b, t), then the text rows with mask 0 per b.
 * vp_null_key_mass: out[b, h, n] = log2 of sum over the null keys of exp2(scale * log2 e * q[b, n, h] . k_null),
 *   -inf when there is none.  q: the normed + rotated queries [B, N, H*64] bf16 (strides in elements),
 *   N = T + F*Hh*Ww; beta bf16 [64]; the per-axis RoPE tables fp32: cos_t / sin_t [F][16], cos_y / sin_y [Hh][24],
 *   cos_x / sin_x [Ww][24].  segs / meta as vp_mask_null_segments wrote them (all B*F*Hh record slots are read,
 *   used or not).  F <= 16, Hh <= 64, Ww <= 255, vp_null_key_mass_lds_bytes <= 160 KiB. */
int vp_mask_null_segments(const uint8_t* mask, int64_t mask_bstride, int32_t B, int32_t T, int32_t F, int32_t Hh,
                          int32_t Ww, void* segs, int32_t* meta, void* stream);
int64_t vp_null_key_mass_lds_bytes(int32_t F, int32_t Hh, int32_t Ww);
int vp_null_key_mass(const void* q, int64_t q_sb, int64_t q_sn, int32_t B, int32_t H, int32_t N, int32_t T, int32_t F,
                     int32_t Hh, int32_t Ww, const void* beta, const float* cos_t, const float* sin_t,
                     const float* cos_y, const float* sin_y, const float* cos_x, const float* sin_x,
                     const uint8_t* mask, int64_t mask_bstride, const void* segs, const int32_t* meta, float scale,
                     float* out, void* stream);
int vp_mask_scale_rows_bf16(const void* x_in, int64_t ld_in, int64_t bs_in, void* y, int64_t ld_out, int64_t bs_out,
                            int32_t B, int32_t Ntok, int32_t D, const uint8_t* tok_mask, int64_t mask_bstride,
                            float scale, const int32_t* dst_rows, void* stream);

/* The training backward of the closed-form null keys (ABI 26).  A null key has value 0, so dP = 0 and its
 * dS = -P D; its share of the query gradient is
 *   dq[b, n, h] += -scale * delta[b, h, n] * G,   G = sum over the null keys j of exp2(c q.k_j - lse[b, h, n]) k_j
 * (c = scale * log2 e), summed over the grid like the mass: G's dims 0-15 = sum_t w_t(t) K_t(t), 16-39 =
 * sum_y w_y(y) K_y(y), 40-63 = sum_x w_x(x) K_x(x), where w_a(p) is the probability mass of the null cells with
 * coordinate p on axis a (two difference arrays over the segment records per query), plus
 * count * exp2(c q.beta - lse) beta for the null text rows.  The gradient towards the null keys themselves reaches
 * only the norm_k bias and is not built: the caller keeps that bias frozen.
 * q, beta, the tables, mask, segs, meta: exactly vp_null_key_mass's; lse / delta fp32 [B, H, N] (the forward's
 * vp_attn_desc.lse, which includes l_extra, and vp_attn_bwd_desc.delta); dq bf16 [B, N, H*64]-strided, read, added to
 * in fp32 and rounded once by the one thread that owns the (b, h, n) row; a batch row without a null key is left
 * untouched.  vp_null_key_mass_bwd_lds_bytes <= 160 KiB. */
int64_t vp_null_key_mass_bwd_lds_bytes(int32_t F, int32_t Hh, int32_t Ww);
int vp_null_key_mass_bwd(const void* q, int64_t q_sb, int64_t q_sn, int32_t B, int32_t H, int32_t N, int32_t T,
                         int32_t F, int32_t Hh, int32_t Ww, const void* beta, const float* cos_t, const float* sin_t,
                         const float* cos_y, const float* sin_y, const float* cos_x, const float* sin_x,
                         const uint8_t* mask, int64_t mask_bstride, const void* segs, const int32_t* meta, float scale,
                         const float* lse, const float* delta, void* dq, int64_t dq_sb, int64_t dq_sn, void* stream);

/* y[b, n, :] = rnd(y[b, n, :] + x[b, rows[b * Ntok + n], :]) for the rows n with tok_mask[b, n] != 0 and
 * 0 <= rows[b * Ntok + n] < x_rows; every other row of y is left as it is.  The gradient of a compact row copy
 * (vp_mask_scale_rows_bf16 / vp_head_norm_rope_bf16 with dst_rows) added back onto its source rows: one writer per
 * row, no atomics.  x must not overlap the rows of y that are written. */
int vp_gather_add_rows_bf16(const void* x, int64_t ld_x, int64_t bs_x, int32_t x_rows, void* y, int64_t ld_y,
                            int64_t bs_y, int32_t B, int32_t Ntok, int32_t D, const uint8_t* tok_mask,
                            int64_t mask_bstride, const int32_t* rows, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Output head norms — norm_final (cogvideox_transformer_3d.py:617-620) then AdaLayerNorm(chunk_dim=1)
 * (DF/models/normalization.py:73-85, shift|scale order): for video rows only,
 * y[b, v] = rnd(rnd(rnd(LN2(rnd(LN1(x[b, text_len + v])))) * rnd(1 + scale)) + shift);  mod bf16 [B, 2D].
 * ------------------------------------------------------------------------------------------------------------- */
int vp_final_norm_bf16(const void* x, void* y, int32_t B, int32_t Ntok, int32_t D, int32_t text_len,
                       const void* ln1_w, const void* ln1_b, const void* ln2_w, const void* ln2_b, float eps,
                       const void* mod, int64_t mod_bstride, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Small-M linear for the conditioning path: y[m, n] = act_out(Σ_k act_in(x[m, k]) W[n, k] + bias[n]), M <= 16.
 * act: 0 none, 1 SiLU (rounded to bf16 like the reference's bf16 nn.SiLU).  Replaces TimestepEmbedding
 * (DF/models/embeddings.py:729-774) and the AdaLN linears (normalization.py:64,370).
 * ------------------------------------------------------------------------------------------------------------- */
int vp_linear_small_bf16(const void* x, int64_t ldx, const void* W, const void* bias, void* y, int64_t ldy, int32_t M,
                         int32_t N, int32_t K, int32_t act_in, int32_t act_out, void* stream);

/* G such linears of one shape on ONE input, in one launch (ABI 23): the AdaLN modulation linears of every block of a
 * forward all read silu(temb), so a forward computes them together, right after the time embedding.  groups: a DEVICE
 * table of G (W, bias) pairs, W bf16 [N, K] 16-byte aligned, bias bf16 [N] or NULL; group g writes y + g * y_gs, rows
 * at stride ldy (elements).  Only the weight-streaming shapes (M <= 2, K <= 512, ldx % 8 == 0, x 16-byte aligned;
 * anything else: VP_ERR_UNSUPPORTED), with that kernel's reduction order per output element: bit-equal to G calls of
 * vp_linear_small_bf16. */
typedef struct vp_linear_group {
  const void* W;
  const void* bias;
} vp_linear_group;
int vp_linear_small_batched_bf16(const void* x, int64_t ldx, const vp_linear_group* groups, int32_t G, void* y,
                                 int64_t y_gs, int64_t ldy, int32_t M, int32_t N, int32_t K, int32_t act_in,
                                 int32_t act_out, void* stream);

/* sinusoidal timestep embedding, flip_sin_to_cos: out bf16 [B, dim] — get_timestep_embedding
 * (DF/models/embeddings.py:27-78); timesteps: device fp32 [B] (the reference casts to float). */
int vp_timestep_embedding_bf16(const float* timesteps, void* out, int32_t B, int32_t dim, float freq_shift,
                               void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Patch embedding data movement (DF/models/embeddings.py:413-430; branch concat branch_cogvideox.py:359):
 * im2col of src1 [B,F,C1,H,W] ⊕ src2 [B,F,C2,H,W] (channel concat) into rows (b, f, y, x) of out [B*F*(H/p)*(W/p),
 * Kpad], column c*p*p + dy*p + dx, zero-padded to Kpad.
 * ------------------------------------------------------------------------------------------------------------- */
int vp_patchify_bf16(const void* src1, int32_t C1, const void* src2, int32_t C2, void* out, int32_t Kpad, int32_t B,
                     int32_t F, int32_t H, int32_t W, int32_t p, void* stream);

/* token mask: out[b, v] = (Σ of mask[b, f, 0, patch(v)] > 0) — avg_pool2d(p) > 0 (embeddings.py:421-428).
 * mask_is_f32: 1 if mask is fp32, 0 if bf16. */
int vp_patch_mask(const void* mask, int32_t mask_is_f32, uint8_t* out, int32_t B, int32_t F, int32_t H, int32_t W,
                  int32_t p, void* stream);

/* Self-guidance after block i (cogvideox_transformer_3d.py:593-608): the unmasked video rows take the guidance
 * states, then the branch injection is added — per row r of batch b (tok_mask[b, r] from vp_patch_mask):
 *   tok_mask == 0:  x = guide                       (+ inject: rnd(guide + inject))
 *   tok_mask != 0:  x unchanged                     (+ inject when inject_all: rnd(x + inject))
 * x, guide, inject: bf16 [B, rows, D] at row stride ld_* and batch stride bs_*; inject NULL: none; inject_all: the
 * reference's unmasked injection (no branch_block_masks).  D % 8 == 0, strides % 8 == 0.  (ABI 18.) */
int vp_guide_rows_bf16(void* x, int64_t ld_x, int64_t bs_x, const void* guide, int64_t ld_g, int64_t bs_g,
                       const void* inject, int64_t ld_i, int64_t bs_i, int32_t inject_all, const uint8_t* tok_mask,
                       int64_t mask_bstride, int32_t B, int32_t rows, int32_t D, void* stream);

/* unpatchify (cogvideox_transformer_3d.py:630-632): out[b,f,c,y*p+py,x*p+px] = proj[b, (f,y,x), c*p*p+py*p+px] */
int vp_unpatchify_bf16(const void* proj, int64_t ld, void* out, int32_t B, int32_t F, int32_t C, int32_t H, int32_t W,
                       int32_t p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * One denoising-step glue, fused: CFG combine (anyl.py:995-997), CogVideoXDPMScheduler.step
 * (DF/schedulers/scheduling_dpm_cogvideox.py:330-439, v-prediction, incl. the 2nd-order branch) and the replace-gt
 * blend with add_noise (anyl.py:1017-1034; scheduler :442-466).  Scalars are precomputed on the host in the
 * reference's dtypes (bf16-rounded where the reference multiplies a bf16 tensor by a 0-dim fp64 tensor).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct vp_dpm_desc {
  int64_t n;
  const void* noise_pred; /* bf16 [2, n] when do_cfg (uncond, text), else [n]                               */
  int32_t do_cfg;
  float guidance;
  const float* model_output; /* fp32 [n]: used instead of noise_pred when non-NULL (scheduler.step API)     */
  const void* sample;     /* bf16 [n] */
  const float* old_pred;  /* fp32 [n] or NULL */
  float* pred_out;        /* fp32 [n] */
  const void* noise1;     /* bf16 [n] */
  const void* noise2;     /* bf16 [n] (second-order step only) */
  int32_t second_order, replace_gt;
  float sa, sb, m1, m2, mn, m3, m4; /* sqrt(a_t) (bf16-rounded), sqrt(1-a_t), mult1 (bf16), mult2, mult_noise
                                       (bf16), mult3, mult4 */
  int32_t gt_add_noise, mask_background;
  const void* gt;         /* bf16 [n] video latents */
  const void* gt_noise;   /* bf16 [n] */
  const void* mask;       /* bf16 [n] */
  float gsa, gsb;         /* add_noise scalars, bf16-rounded */
  void* latents_out;      /* bf16 [n] (cast + replace-gt) or NULL */
  float* prev_out;        /* fp32 [n] pre-cast prev_sample (scheduler.step API) or NULL */
} vp_dpm_desc;

int vp_dpm_step_bf16(const vp_dpm_desc* d, void* stream);

/* deterministic N(mean, std²) fill (splitmix64 + Box-Muller) for synthetic weights on the device */
int vp_fill_normal_bf16(void* out, int64_t n, uint64_t seed, float mean, float std, void* stream);

/* ---- CogVideoX 3D causal VAE (DF/models/autoencoders/autoencoder_kl_cogvideox.py) ----
 * Activations are channels-last bf16 [B, T, H, W, C] ("NDHWC"); a channel count that is not a power of two >= 8
 * (the 3 pixel channels, ...) is zero-padded to one.  Conv weights are re-laid-out once at load time as
 * [Cout, kt, kh, kw, Cin] (Cin padded like the activation) so every conv is an implicit GEMM whose K runs over
 * (tap, channel) with channels contiguous. */
#define VP_CONV_MAX_T 128
typedef struct vp_conv3d_desc {
  int32_t B, Cin, Cout;            /* Cin = the (padded, power of two >= 8) channel count of x / hist / weight rows */
  int32_t Tout, Hout, Wout;        /* output grid */
  int32_t Hin, Win;                /* physical input grid (before the nearest upsampling below) */
  int32_t kt, kh, kw;              /* kernel (each 1 or 3); temporal stride 1 */
  int32_t sh, sw;                  /* spatial stride (1 or 2) */
  int32_t ph, pw;                  /* top / left zero padding in the upsampled grid (bottom / right: the bounds) */
  int32_t uh, uw;                  /* nearest upsampling of the input grid (1 or 2), folded into the gather */
  int32_t x_frames, hist_frames;   /* frames per batch element of x / hist */
  int32_t ldy, ldr;                /* row (pixel) strides of y / resid in elements: multiples of 8, >= Cout */
  int32_t tmap[VP_CONV_MAX_T];     /* virtual input frame v = t + dt (t: output frame, dt: temporal tap) ->
                                      >= 0: frame of x, < 0: frame (-1 - value) of hist (the causal cache) */
  const void* x;                   /* bf16 [B, x_frames, Hin, Win, Cin] */
  const void* hist;                /* bf16 [B, hist_frames, Hin, Win, Cin] or NULL */
  const void* w;                   /* bf16 [Cout, kt, kh, kw, Cin] */
  const void* bias;                /* bf16 [Cout] or NULL */
  const void* resid;               /* bf16 [B, Tout, Hout, Wout] rows of stride ldr, added after the bias, or NULL */
  void* y;                         /* bf16 [B, Tout, Hout, Wout] rows of stride ldy; channels [Cout, ldy) get 0 */
} vp_conv3d_desc;

/* CogVideoXCausalConv3d.forward (:133-145; kt = 3, 1x1x1), the resnet conv_shortcut (:273), CogVideoXDownsample3D's
 * stride-2 conv2d (DF/models/downsampling.py:344-353) and CogVideoXUpsample3D's nearest-upsample + conv2d
 * (DF/models/upsampling.py:384-412) as one implicit-GEMM MFMA kernel. */
int vp_conv3d_bf16(const vp_conv3d_desc* d, void* stream);

/* nn.GroupNorm over [B, P, C] channels-last (groups of C / G consecutive channels), fp32 statistics (per-thread sums
 * shifted by the group's first element, combined in fp64): stats = float [B, G, 2] (mean, rstd); partials: float
 * workspace of vp_group_norm_workspace_floats(B, G) floats. */
int64_t vp_group_norm_workspace_floats(int32_t B, int32_t G);
int vp_group_norm_stats(const void* x, int32_t B, int64_t P, int32_t C, int32_t G, float eps, float* partials,
                        float* stats, void* stream);

/* y = act(GroupNorm(x) [* Ymod + Bmod]) over [B, T, H, W, C]: GroupNorm affine (gamma, beta bf16 [C]); with
 * mod != NULL the CogVideoXSpatialNorm3D modulation (:175-188): mod = bf16 [B, Tz, Hz, Wz, 2C] holding
 * conv_y(z) | conv_b(z) at the LATENT resolution (a 1x1x1 conv commutes with nearest resizing), gathered at the
 * nearest source position: frame tzmap[t] (host array of T entries), row floor(h * (Hz / H)), column
 * floor(w * (Wz / W)) (torch's nearest rule, float scale); act = SiLU if silu. */
int vp_group_norm_apply_bf16(const void* x, void* y, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C,
                             int32_t G, const float* stats, const void* gamma, const void* beta, const void* mod,
                             int32_t Tz, int32_t Hz, int32_t Wz, const int32_t* tzmap_host, int32_t silu,
                             void* stream);

/* CogVideoXDownsample3D's temporal compression (DF/models/downsampling.py:323-342): x [B, T, P, C] ->
 * [B, T', P, C] with frame 0 kept when T is odd and every following pair averaged. */
int vp_time_pool2_bf16(const void* x, void* y, int32_t B, int32_t T, int64_t P, int32_t C, void* stream);

/* layout: NCDHW (fp32 or bf16) [B, C, T, H, W] <-> channels-last bf16 [B, T, H, W, Cpad] (zero padding channels);
 * the reverse takes channels [c0, c0 + C) of rows of stride ldx and writes bf16 NCDHW */
int vp_ncdhw_to_ndhwc_bf16(const void* x, int32_t x_is_f32, void* y, int32_t B, int32_t C, int32_t T, int32_t H,
                           int32_t W, int32_t Cpad, void* stream);
int vp_ndhwc_to_ncdhw_bf16(const void* x, int32_t ldx, void* y, int32_t B, int32_t C, int32_t T, int32_t H,
                           int32_t W, int32_t c0, void* stream);

/* DiagonalGaussianDistribution (DF/models/autoencoders/vae.py:768-789) on the encoder output [B, T, H, W] rows of
 * stride ldp holding mean | logvar (2L channels): mean, logvar clamped to [-30, 20] as bf16 NCDHW [B, L, T, H, W];
 * with noise != NULL (bf16 NCDHW) sample = mean + exp(0.5 logvar) * noise is written to `sample`. */
int vp_latent_dist_bf16(const void* params, int32_t ldp, void* mean, void* logvar, const void* noise, void* sample,
                        int32_t B, int32_t L, int32_t T, int32_t H, int32_t W, void* stream);

/* AutoencoderKLCogVideoX.blend_v / blend_h (:1192-1206) on channels-last tiles, in place on b: with e = min(Ha, Hb,
 * extent) (axis 0) rows y < e of b become a[row Ha - e + y] * (1 - y / e) + b[row y] * (y / e); axis 1 the same over
 * columns (e = min(Wa, Wb, extent)).  a [B, T, Ha, Wa, C], b [B, T, Hb, Wb, C], both contiguous; axis 0 needs
 * Wa == Wb, axis 1 Ha == Hb. */
int vp_tile_blend_bf16(const void* a, void* b, int32_t B, int32_t T, int32_t Ha, int32_t Wa, int32_t Hb, int32_t Wb,
                       int32_t C, int32_t axis, int32_t extent, void* stream);


/* ---- T5 v1.1 encoder (transformers modeling_t5.py, pinned transformers==4.42.2) ----
 * The projections (q|k|v fused, o, wi_0 + GELU-tanh, wi_1, wo) run on vp_gemm_bf16 (no bias; the residual adds are
 * its VP_EPI_BIAS_ADDROWS epilogue).  T5Stack.embed_tokens: out[r] = table[ids[r]] (bf16 [vocab, D]). */
int vp_embedding_gather_bf16(const void* table, const int64_t* ids, void* out, int32_t rows, int32_t D, int32_t vocab,
                             void* stream);
/* T5LayerNorm: y = w * bf16(x * rsqrt(mean(x^2) + eps)) over rows of D (bf16 in / out, fp32 statistics) */
int vp_rms_norm_bf16(const void* x, const void* w, void* y, int32_t rows, int32_t D, float eps, void* stream);
/* T5DenseGatedActDense's product: y = bf16(a * b) elementwise (n % 8 == 0) */
int vp_mul_bf16(const void* a, const void* b, void* y, int64_t n, void* stream);
/* T5Attention (encoder, bidirectional): qkv [B, L, ld] bf16 holding q | k | v (inner = H * 64 columns each);
 * scores = bf16(q . k) + bias_table[buckets[q * L + k], h] (no 1/sqrt(d) scaling), masked keys (mask[b, k] == 0,
 * int64 [B, L], or mask NULL) get the bf16 minimum added, softmax in fp32, out [B, L] rows of stride ldo, head h at
 * column h * 64.  buckets: int32 [L, L] from T5Attention._relative_position_bucket (host-computed); L <= 512. */
int vp_t5_attention_bf16(const void* qkv, int64_t ld, int32_t inner, int32_t B, int32_t L, int32_t H,
                         const void* bias_table, const int32_t* buckets, const int64_t* mask, void* out, int64_t ldo,
                         void* stream);


/* ---- pixel-space glue of the any-length pipeline's VAE stage (…_anyl.py:339-484) ---- */
/* y = bf16(x * s) (the latents' scaling_factor and its inverse, :372 / :430 / :481) */
int vp_scale_bf16(const void* x, void* y, int64_t n, float s, void* stream);
/* out = video * (mask < 0.5) (keep_above: >= 0.5, mask_background) over [B, C, P] with mask [B, 1, P] fp32
 * (:890-893); video fp32 or bf16, out bf16 */
int vp_mask_video_bf16(const void* video, int32_t video_is_f32, const float* mask, int32_t keep_above, void* out,
                       int32_t B, int32_t C, int64_t P, void* stream);
/* F.interpolate(mode="nearest", size=(t, h, w)) of fp32 [BC, T, H, W] -> bf16 (:437-439) */
int vp_nearest_resize3d_bf16(const float* x, void* y, int32_t BC, int32_t T, int32_t H, int32_t W, int32_t t,
                             int32_t h, int32_t w, void* stream);
/* VaeImageProcessor.denormalize on bf16: (x / 2 + 0.5).clamp(0, 1) */
int vp_denormalize_bf16(const void* x, void* y, int64_t n, void* stream);


/* ---- backward (train/train_cogvideox_inpainting_i2v_video.py:1892 accelerator.backward) ---- */
/* Flash-attention backward of vp_attention_fwd_bf16 (no blend): with P = exp2(c q.k - lse), c = scale * log2 e, lse
 * from the forward's vp_attn_desc.lse: dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO with
 * dS = P (dO V^T - rowsum(dO O)).  delta: fp32 [B, H, Nq], written here (D = rowsum(dO O)) and left to the caller
 * (vp_null_key_mass_bwd reads it).  All tensors [B, N, H*64]-strided bf16.
 * The keys are one buffer of Nk rows; a forward over two segments is differentiated over their concatenation.
 * k_len (ABI 26): device int32 [B] or NULL — batch row b has min(k_len[b], Nk) keys (the resample processor's compact
 * second segment behind the N own keys, vp_attn_desc.k2_len; a negative entry counts as 0): K / V rows at or past the
 * length never affect a result (they may hold anything, NaN included; a batch row of length 0 has row 0 of its K and V
 * loaded and discarded, no other row at or past a length is read), and rows at or past it of dK / dV are written as
 * zeros.  lse may hold more mass than these keys give (the closed-form
 * null keys, vp_attn_desc.l_extra).  The default kernels only (VP_ATTN_BWD_VARIANT=0 with k_len: VP_ERR_UNSUPPORTED). */
typedef struct vp_attn_bwd_desc {
  int32_t B, H, Nq, Nk, head_dim, pad0;
  const void* Q;
  int64_t q_sb, q_sn;
  const void* K;
  int64_t k_sb, k_sn;
  const void* V;
  int64_t v_sb, v_sn;
  const void* O;
  int64_t o_sb, o_sn;
  const void* dO;
  int64_t do_sb, do_sn;
  const float* lse;
  float* delta;
  void* dQ;
  int64_t dq_sb, dq_sn;
  void* dK;
  int64_t dk_sb, dk_sn;
  void* dV;
  int64_t dv_sb, dv_sn;
  float scale;
  int32_t pad1;
  const int32_t* k_len;
} vp_attn_bwd_desc;
int vp_attention_bwd_bf16(const vp_attn_bwd_desc* d, void* stream);
/* The same with a workspace for the grid-tail split (ABI 19): the blocks of each kernel's last partial round run as
 * key- / query-range pieces at the end of its grid, their fp32 sums merged by a small pass.
 * vp_attention_bwd_workspace_bytes: bytes needed for this descriptor (0: no split; -1: invalid descriptor); a smaller
 * or NULL workspace runs unsplit.  VP_ATTN_NO_SPLIT disables the split (A/B). */
int64_t vp_attention_bwd_workspace_bytes(const vp_attn_bwd_desc* d);
int vp_attention_bwd_bf16_ws(const vp_attn_bwd_desc* d, void* workspace, int64_t workspace_bytes, void* stream);


/* The other backward passes (row / elementwise / column reductions; the backward's matrix products run on
 * vp_gemm_bf16 against transposed operands).  y[c][r] = x[r][c] for nbatch R x C bf16 matrices: */
int vp_transpose_bf16(const void* x, int64_t ldx, int64_t x_bs, void* y, int64_t ldy, int64_t y_bs, int32_t R,
                      int32_t Cc, int32_t nbatch, void* stream);
/* out[(batch * 2 + type) * cols + n] += sum over rows m of that (batch = m / Ntok, type = text (1) if m % Ntok <
 * text_len) of a[m, n] (* b[m, n] when b != NULL): bias / gate / shift / scale / LayerNorm-affine gradients (fp32
 * atomics; cols % 8 == 0) */
int vp_colsum_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t rows, int32_t cols, int32_t Ntok,
                   int32_t text_len, float* out, void* stream);
/* CogVideoXLayerNormZero backward (normalization.py:373-379): with n = bf16(LN(x) w + b) and the forward's
 * y = bf16(bf16(n s1) + shift), s1 = bf16(1 + scale) (scale / shift = chunks scale_v / shift_v of mod for video
 * rows, _t for text rows), dx += LN'(dy s1 w) (bf16 in place, one rounding of old + delta); optionally writes n,
 * dn = dy s1 and LN(x) without the affine (bf16 [rows, D]) for the parameter column sums.  x, dy, dx and the three
 * outputs are contiguous [B * Ntok, D]; D % 8 == 0, D <= 4096, mod_bstride % 8 == 0 (else VP_ERR_ARG). */
int vp_adaln_bwd_bf16(const void* x, const void* dy, void* dx, int32_t B, int32_t Ntok, int32_t D, int32_t text_len,
                      const void* ln_w, const void* ln_b, float eps, const void* mod, int64_t mod_bstride,
                      int32_t shift_v, int32_t scale_v, int32_t shift_t, int32_t scale_t, void* n_out, void* dn_out,
                      void* xhat_out, void* stream);
/* y = bf16(x * gate) with gate = chunk chunk_v (video rows) / chunk_t (text rows) of mod [B, *] (the gated
 * residual's gradient into its branch, cogvideox_transformer_3d.py:161-162, 179-180); D, ldx, ldy and mod_bstride
 * are multiples of 8 (else VP_ERR_ARG) */
int vp_rowscale_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t Ntok, int32_t D,
                     int32_t text_len, const void* mod, int64_t mod_bstride, int32_t chunk_v, int32_t chunk_t,
                     void* stream);
/* vp_rowscale_bf16 writing MX rows (ABI 28): q (e4m3 [rows][D], row stride ld_out bytes) and scales (the MX tile
 * layout above) are byte for byte vp_mx_quantize_bf16(vp_rowscale_bf16(x)) — the gated residual's branch gradient as
 * the operand of an MX dgrad GEMM.  D % 128 == 0, ldx and mod_bstride multiples of 8, ld_out >= D and a multiple of
 * 8, x and mod 16-byte aligned (else VP_ERR_ARG). */
int vp_rowscale_mx_fp8(const void* x, int64_t ldx, void* q, int64_t ld_out, void* scales, int32_t rows, int32_t Ntok,
                       int32_t D, int32_t text_len, const void* mod, int64_t mod_bstride, int32_t chunk_v,
                       int32_t chunk_t, void* stream);
/* GELU(tanh) forward h = gelu(z) and backward dz = dh * gelu'(z) (activations.py:65-90), elementwise bf16,
 * n % 8 == 0.  With u = sqrt(2 / pi) (z + 0.044715 z^3) and s = 1 / (1 + exp(-2 u)):  gelu = z s,
 * gelu' = s + z s (1 - s) 2 sqrt(2 / pi) (1 + 3 * 0.044715 z^2), each to the bf16 rounding of the exact value
 * (relative, also where the value is tiny: z << 0).  Domain: vp_gelu_bf16 takes every finite z (it saturates to z /
 * -0); vp_gelu_bwd_bf16 is defined for |z| <= 2^60 (gelu' is exactly 1 / 0 from |z| ~ 10 on); beyond that the
 * result is unspecified: once z^2 overflows fp32 (|z| >= 2^64) the polynomial factor is inf against a zero and the
 * result is NaN, as with torch's own fp32 formula.  A pre-activation of that size is not a trained network's. */
int vp_gelu_bf16(const void* z, void* h, int64_t n, void* stream);
int vp_gelu_bwd_bf16(const void* dh, const void* z, void* dz, int64_t n, void* stream);
/* y = bf16(a + alpha b) (gradient accumulation), n % 8 == 0 */
int vp_axpy_bf16(const void* a, const void* b, float alpha, void* y, int64_t n, void* stream);
/* y = silu(x) = x s and y = dy * silu'(x) = dy s (1 + x (1 - s)), s = 1 / (1 + exp(-x)) (the AdaLN / time-embedding
 * SiLU); every finite x: both saturate (silu to x / -0, silu' to 1 / 0) without forming inf * 0 */
int vp_silu_bf16(const void* x, void* y, int64_t n, void* stream);
int vp_silu_bwd_bf16(const void* dy, const void* x, void* y, int64_t n, void* stream);
/* backward of vp_head_norm_rope_bf16 (LayerNorm(64) + RoPE on rows >= text_len; no token mask): x_in = the
 * pre-norm q or k, dy = the gradient of the normed + rotated output, dx = the gradient of x_in (dx may be dy: each
 * head vector is read before it is written, by the same lanes); dln_w / dln_b: fp32 [64] accumulated (atomics) or
 * both NULL.  Every row and batch stride is a multiple of 4 elements (else VP_ERR_ARG). */
int vp_head_norm_rope_bwd_bf16(const void* x_in, int64_t ld_in, int64_t bs_in, const void* dy, int64_t ld_dy,
                               int64_t bs_dy, void* dx, int64_t ld_dx, int64_t bs_dx, int32_t B, int32_t Ntok,
                               int32_t H, int32_t text_len, const void* ln_w, const void* ln_b, float eps,
                               const float* cos, const float* sin, float* dln_w, float* dln_b, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training tail (ABI 21; csrc/optim.hip): the loss, the gradient norm / clip and the AdamW update of the reference's
 * training step (train/train_cogvideox_inpainting_i2v_video.py:1879-1902 under accelerate + DeepSpeed bf16: bf16
 * model weights, fp32 master weights and moments).  Multi-tensor kernels over a list of contiguous bf16 tensors of
 * any sizes, described by two DEVICE tables the caller builds and uploads (asynchronously on `stream`):
 *   tensors[t]: the gradient / parameter pointers, the element offset of the tensor's fp32 state in the flat state
 *               buffers, and its element count;
 *   chunks[c]:  one workgroup's work: elements [chunk * VP_MT_CHUNK, min(numel, (chunk + 1) * VP_MT_CHUNK)) of
 *               tensors[tensor] — a chunk never crosses a tensor, an empty tensor has no chunk.
 * 16-byte loads / stores in the body of a chunk, scalar head and tail (a chunk whose pointers do not share one
 * 16-byte phase runs scalar as a whole); 64-bit element offsets.  No float atomics: every reduction writes one fp32
 * partial per chunk into its own slot and a single-workgroup finaliser sums the slots in a fixed order, so results
 * are bit-identical run to run.  No entry point reads device memory on the host or synchronises. */
#define VP_MT_CHUNK 16384
typedef struct {
  void* grad;        /* bf16 [numel], contiguous */
  void* param;       /* bf16 [numel], contiguous (vp_mt_adamw_bf16 only; NULL otherwise) */
  int64_t state_off; /* element offset of this tensor in master / exp_avg / exp_avg_sq (vp_mt_adamw_bf16 only) */
  int64_t numel;
} vp_mt_tensor;
typedef struct {
  int32_t tensor; /* index into the tensor table */
  int32_t chunk;  /* chunk index inside that tensor */
} vp_mt_chunk;
/* the device "scalars" block of one optimizer / one norm call (written by vp_optim_finalize with ordinary vector
 * stores, read by the scale and update kernels) */
typedef struct {
  float grad_norm;   /* total L2 norm of the gradients (before any clip) */
  float clip_coef;   /* min(1, max_norm / (grad_norm + 1e-6)) (torch clip_grad_norm_); 1 when max_norm <= 0 */
  int32_t nonfinite; /* 1 when any gradient element is inf or NaN */
  int32_t step;      /* optimizer step counter (kept across calls; incremented by the finaliser) */
  float bias_c1;     /* 1 - beta1^step */
  float bias_c2;     /* 1 - beta2^step */
  int32_t skipped;   /* 1 when this step is skipped (nonfinite && skip_nonfinite): step not incremented */
  int32_t pad;
} vp_optim_scalars;
/* stage 1 of the gradient norm: partials[c] = sum of squares (fp32) of chunk c, flags[c] = 1 when the chunk holds an
 * inf / NaN (the bf16 bit pattern is tested: a finite value whose square overflows does not set it).
 * n_chunks = 0: no launch. */
int vp_mt_grad_sqnorm_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks, float* partials,
                           int32_t* flags, void* stream);
/* stage 2 (one workgroup): grad_norm = sqrt(sum of partials[0 .. n_chunks) in a fixed order), nonfinite, clip_coef
 * (max_norm <= 0: no clip, 1).  advance_step != 0: the optimizer's finaliser — skipped = nonfinite &&
 * skip_nonfinite; unless skipped, ++step and bias_c1 / bias_c2 = 1 - beta^step (evaluated in double).
 * advance_step == 0: step / bias_c* / skipped are left as they are.  n_chunks = 0 gives norm 0. */
int vp_optim_finalize(const float* partials, const int32_t* flags, int32_t n_chunks, float max_norm, double beta1,
                      double beta2, int32_t skip_nonfinite, int32_t advance_step, vp_optim_scalars* scalars,
                      void* stream);
/* grad = bf16(grad * scalars->clip_coef) in place over the tensor list (torch.nn.utils.clip_grad_norm_'s multiply);
 * nothing is written when the coefficient is exactly 1 */
int vp_mt_scale_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                     const vp_optim_scalars* scalars, void* stream);
/* torch.optim.AdamW (amsgrad = False, maximize = False) with fp32 master weights, over chunks [chunk_begin,
 * chunk_begin + n_chunks) of the table (one call per parameter group).  Per element, in fp32: g = grad (* clip_coef
 * when use_clip); p = master * (1 - lr * weight_decay); m += (1 - beta1) (g - m); v = beta2 v + (1 - beta2) g^2;
 * p -= (lr / bias_c1) * m / (sqrt(v) / sqrt(bias_c2) + eps); master, exp_avg, exp_avg_sq are stored and
 * param = bf16(p) (round to nearest even).  zero_grads: the gradient is zeroed in the same pass.  A skipped step
 * (scalars->skipped) writes no state and no parameter (it still zeroes the gradients when asked to). */
int vp_mt_adamw_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin, int32_t n_chunks,
                     float* master, float* exp_avg, float* exp_avg_sq, const vp_optim_scalars* scalars, double lr,
                     double beta1, double beta2, double eps, double weight_decay, int32_t use_clip,
                     int32_t zero_grads, void* stream);
/* y = bf16(x * *s) with the fp32 factor read on the device (the loss's backward: the incoming scalar gradient) */
int vp_scale_dev_bf16(const void* x, void* y, int64_t n, const float* s, void* stream);
/* The v-prediction training loss (:1879-1891), forward and gradient in one pass.  model_output, noisy, target:
 * bf16 [B, F, C, H*W] contiguous; mask [B, F, 1, H*W] bf16 or fp32, or NULL (no inpainting term then,
 * whatever lambda is).  Per sample b, in fp32, t = timesteps[b] (int64 on the device, clamped to [0, n_alphas)),
 * ac = alphas_cumprod[t]: sa = sqrt(ac), sb = sqrt(1 - ac), w = 1 / (1 - ac), d = sa noisy - sb model_output - target;
 *   *loss = mean_b mean(w d^2) + lambda mean_b mean(w (d mask)^2)
 *   dout  = bf16(-sb w 2 d (1 + lambda mask^2) / (B numel_per_sample))
 * partials: fp32 workspace of vp_v_loss_partials(...) slots (-1: invalid sizes); the sum runs through the same
 * two-stage reduction (bit-identical run to run). */
int64_t vp_v_loss_partials(int32_t B, int32_t F, int32_t C, int32_t HW);
int vp_v_loss_bf16(const void* model_output, const void* noisy, const void* target, const void* mask,
                   int32_t mask_is_f32, const int64_t* timesteps, const float* alphas_cumprod, int32_t n_alphas,
                   int32_t B, int32_t F, int32_t C, int32_t HW, float lambda, float* partials, float* loss,
                   void* dout, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Plain Adam and Prodigy (ABI 27; csrc/optim.hip, csrc/prodigy.hip): the other two choices of the reference's
 * get_optimizer (train/train_cogvideox_inpainting_i2v_video.py:1283-1361), on the tables, the flat fp32 state space,
 * the norm pass and the scalars block of the training tail above. */
/* torch.optim.Adam (amsgrad = False, maximize = False): vp_mt_adamw_bf16 with the weight decay as an L2 term on the
 * gradient, g = grad (* clip_coef) + weight_decay * master, instead of the factor on the master; everything else,
 * the skipped step included, as there. */
int vp_mt_adam_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin, int32_t n_chunks,
                    float* master, float* exp_avg, float* exp_avg_sq, const vp_optim_scalars* scalars, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int32_t use_clip, int32_t zero_grads,
                    void* stream);
/* Prodigy (prodigyopt 1.0's step() with slice_p = 1, no FSDP) with fp32 master weights.  State: master, exp_avg,
 * exp_avg_sq, s, p0 (the initial master), fp32 over the flat state space.  The distance estimate lives in a device
 * block of doubles (the reference keeps these in Python floats); only vp_prodigy_finalize writes it. */
typedef struct {
  double d;            /* the distance estimate (starts at d0) */
  double d_max;        /* the largest d_hat so far (starts at d0) */
  double d_hat;        /* d_coef * d_numerator / d_denom of the last step that made progress */
  double d_numerator;  /* beta3-decayed sum of (d / d0) dlr <g, p0 - p> */
  double d_denom;      /* sum |s| of the last step */
  double dlr;          /* d * lr * bias correction of the step, from the d BEFORE the step's update */
  int32_t no_progress; /* 1 when the last step found d_denom == 0: no parameter changed, the counter stood still */
  int32_t pad;
} vp_prodigy_scalars;
/* One step is, after the norm pass and vp_optim_finalize (advance_step = 1: clip_coef, skipped, the counter):
 *   vp_prodigy_finalize(phase 0)    dlr = d lr bc, bc = sqrt(1 - beta2^step) / (1 - beta1^step) with the advanced
 *                                   counter when use_bias_correction, else 1
 *   vp_mt_prodigy_moments_bf16      once per parameter group: the moments, s and the two partials of every chunk
 *   vp_prodigy_finalize(phase 1)    d_numerator = beta3 d_numerator + (d / d0) dlr sum(dot), d_denom = sum(|s|), both
 *                                   sums over partials[0 .. 2 n_chunks) in a fixed order in double; d_denom == 0:
 *                                   no_progress = 1, the counter goes back by one and the rest of the block stays;
 *                                   else, when lr > 0, d_hat = d_coef d_numerator / d_denom, d = max(d, d_hat) while
 *                                   d == d0, d_max = max(d_max, d_hat), d = min(d_max, d growth_rate)
 *   vp_mt_prodigy_update_bf16       once per parameter group: the update with the NEW d in d * eps
 * A skipped step (scalars->skipped) changes nothing in either phase.  One workgroup; n_chunks is used by phase 1 only
 * (partials may be NULL in phase 0).  VP_ERR_ARG for a phase other than 0 / 1, lr < 0, betas or beta3 outside [0, 1),
 * d0 <= 0, d_coef <= 0, growth_rate < 1, or any NaN. */
int vp_prodigy_finalize(int32_t phase, const float* partials, int32_t n_chunks, double lr, double beta1, double beta2,
                        double beta3, double d0, double d_coef, double growth_rate, int32_t use_bias_correction,
                        vp_optim_scalars* scalars, vp_prodigy_scalars* dstate, void* stream);
/* pass 1 over chunks [chunk_begin, chunk_begin + n_chunks).  Per element, in fp32, with d and dlr of the block:
 *   g = grad (* clip_coef when use_clip) (+ weight_decay * master: the coupled decay; pass 0 when decoupled)
 *   dot += g (p0 - master); exp_avg = beta1 exp_avg + d (1 - beta1) g; exp_avg_sq = beta2 exp_avg_sq +
 *   d^2 (1 - beta2) g^2; s = beta3 s + (d / d0) (safeguard_warmup ? d : dlr) g; den += |s|
 * partials[2 c] = dot and partials[2 c + 1] = den of chunk c (its index in the whole table).  22 bytes read and 12
 * written per element.  A skipped step writes nothing. */
int vp_mt_prodigy_moments_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                               int32_t n_chunks, const float* master, const float* p0, float* exp_avg,
                               float* exp_avg_sq, float* s, float* partials, const vp_optim_scalars* scalars,
                               const vp_prodigy_scalars* dstate, double beta1, double beta2, double beta3,
                               double weight_decay, double d0, int32_t safeguard_warmup, int32_t use_clip,
                               void* stream);
/* pass 2 over the same chunks.  Per element, in fp32: denom = sqrt(exp_avg_sq) + d eps (the new d);
 * p = master (+ master * (-weight_decay dlr): the decoupled decay; pass 0 when coupled); p -= dlr exp_avg / denom;
 * master = p, param = bf16(p).  12 bytes read and 6 written per element (8 with zero_grads).  A skipped or
 * no-progress step writes no state and no parameter (it still zeroes the gradients when asked to). */
int vp_mt_prodigy_update_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                              int32_t n_chunks, float* master, const float* exp_avg, const float* exp_avg_sq,
                              const vp_optim_scalars* scalars, const vp_prodigy_scalars* dstate, double eps,
                              double weight_decay, int32_t zero_grads, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Sharded training tail (ABI 22; csrc/zero.hip): the kernels of a data-parallel optimizer step with the fp32 state
 * sharded over the ranks (the reference trains under DeepSpeed ZeRO stage 2, accelerate_config_machine_single_ds.yaml).
 * The element space is the flat state space of the training tail above: tensor t at elements [state_off, state_off +
 * numel), state_off a multiple of 8, T elements in all.  per = ceil(T / world) rounded up to a multiple of 8; rank r
 * owns elements [r per, (r + 1) per) and keeps master / exp_avg / exp_avg_sq for them only (fp32 [per] each).  One
 * step is, with the three collectives left to the caller:
 *   vp_zero_pack_bf16        bf16 gradients -> fp32 flat [world per], scaled by 1 / world
 *   (reduce-scatter, sum)    -> this rank's fp32 gradient shard [per]: the average over the ranks
 *   vp_zero_shard_sqnorm     -> this rank's (sum of squares, non-finite flag) record
 *   (all-gather)             -> the records of all ranks, in rank order
 *   vp_zero_finalize         -> vp_optim_scalars, bit-identical on every rank
 *   vp_zero_shard_adamw      once per parameter group: the update of the shard, bf16(p) into a bf16 shard
 *   (all-gather)             -> bf16 flat [world per]
 *   vp_zero_unpack_bf16      bf16 flat -> the bf16 parameters
 * The shard kernels run over a DEVICE table of ranges: pieces of the shard of at most VP_MT_CHUNK elements, none of
 * which crosses a tensor (hence a parameter group) or the shard, and which cover only tensors that have a gradient
 * this step (no padding).  Range starts are multiples of 8 elements.  Same rules as the training tail: 16-byte body,
 * scalar head / tail, 64-bit offsets, no float atomics, fixed-order two-stage reductions, no host read.  A chunk or
 * range that does not fit the buffer length passed with it is left out (nothing is read or written for it). */
typedef struct {
  int64_t start; /* first element, relative to the start of this rank's shard */
  int32_t n;     /* 1 .. VP_MT_CHUNK elements; start + n <= per */
  int32_t pad;
} vp_zero_range;
typedef struct {
  float sqsum;       /* sum of squares of the averaged gradient over the rank's ranges */
  int32_t nonfinite; /* 1 when one of them is inf / NaN */
} vp_zero_record;
/* pack, over the tensor / chunk tables of ALL trainable tensors: flat[state_off + i] = (float)grad[i] * inv_world
 * (one fp32 product; inv_world in (0, 1]); a tensor whose grad pointer is NULL gets zeros.  zero_grads: the bf16
 * gradient is zeroed in the same pass (whether or not the step is skipped later).  Padding is never written. */
int vp_zero_pack_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks, float* flat,
                      int64_t flat_len, float inv_world, int32_t zero_grads, void* stream);
/* unpack, over the same tables: param[i] = flat[state_off + i] (bf16) for the tensors whose grad pointer is not
 * NULL; nothing at all in a skipped step (scalars->skipped) */
int vp_zero_unpack_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks, const void* flat,
                        int64_t flat_len, const vp_optim_scalars* scalars, void* stream);
/* shard norm: partials[c] / flags[c] = the fp32 sum of squares / non-finite flag of range c of grad_shard (fp32
 * [per]; the fp32 bit pattern is tested, so an average that overflowed counts), then one workgroup sums the slots in
 * a fixed order into *record.  n_ranges = 0 (a rank that owns only padding): record = (0, 0), still written. */
int vp_zero_shard_sqnorm(const vp_zero_range* ranges, int32_t n_ranges, const float* grad_shard, int64_t per,
                         float* partials, int32_t* flags, vp_zero_record* record, void* stream);
/* vp_optim_finalize (advance_step = 1; the same device code) over records[0 .. world) in rank order: every rank that
 * passes the same records and the same scalars block gets the same block, bit for bit */
int vp_zero_finalize(const vp_zero_record* records, int32_t world, float max_norm, double beta1, double beta2,
                     int32_t skip_nonfinite, vp_optim_scalars* scalars, void* stream);
/* vp_mt_adamw_bf16's update (the same per-element device function) over ranges [range_begin, range_begin + n_ranges)
 * of the shard: g = grad_shard (* clip_coef when use_clip), master / exp_avg / exp_avg_sq fp32 [per] updated in place,
 * param_shard[i] = bf16(p) (bf16 [per]).  A skipped step writes nothing. */
int vp_zero_shard_adamw(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges, const float* grad_shard,
                        float* master, float* exp_avg, float* exp_avg_sq, void* param_shard, int64_t per,
                        const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int32_t use_clip, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Sharded plain Adam and Prodigy (ABI 29; csrc/zero.hip): the other two optimizers on the sharded training tail
 * above — the same pack, reduce-scatter, shard norm, record all-gather and vp_zero_finalize, the same range table and
 * rules (one workgroup per range, 16-byte body, scalar head / tail, 64-bit offsets, no float atomics, fixed-order
 * two-stage reductions, no host read, a skipped step writes nothing, a range that does not fit `per` is left out),
 * the per-element arithmetic of vp_mt_adam_bf16 / vp_mt_prodigy_*_bf16 (the same device functions). */
/* vp_zero_shard_adamw with torch.optim.Adam's decay: g = grad_shard (* clip_coef) + weight_decay * master, no factor
 * on the master; everything else as there. */
int vp_zero_shard_adam(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges, const float* grad_shard,
                       float* master, float* exp_avg, float* exp_avg_sq, void* param_shard, int64_t per,
                       const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int32_t use_clip, void* stream);
/* Sharded Prodigy: rank r keeps master / exp_avg / exp_avg_sq / s / p0 (fp32 [per] each) and its own copy of the
 * vp_prodigy_scalars block.  The two sums of the d update are the only part that is not element-wise: every rank sums
 * its ranges' pairs into a record of two doubles, the records are all-gathered (16 bytes per rank) and every rank
 * runs the same finaliser over them in rank order.  After vp_zero_finalize, with the collectives left to the caller:
 *   vp_zero_prodigy_finalize(phase 0)   dlr from the old d (vp_prodigy_finalize's phase 0)
 *   vp_zero_shard_prodigy_moments       once per parameter group: pass 1 over the shard, one pair per range
 *   vp_zero_prodigy_record              -> this rank's (sum dot, sum |s|) record
 *   (all-gather)                        -> records [world][2], in rank order
 *   vp_zero_prodigy_finalize(phase 1)   the d update: the same block on every rank, bit for bit
 *   vp_zero_shard_prodigy_update        once per parameter group: pass 2, bf16(p) into the bf16 shard
 *   (all-gather), vp_zero_unpack_gated_bf16
 * pass 1 over ranges [range_begin, range_begin + n_ranges): vp_mt_prodigy_moments_bf16's arithmetic on g = grad_shard
 * (fp32); exp_avg / exp_avg_sq / s updated in place, master and p0 read only; partials[2 c] = dot and partials[2 c + 1]
 * = sum |s| of range c (its index in the whole table; (0, 0) for a range that does not fit).  24 bytes read and 12
 * written per element of the shard.  A skipped step writes nothing. */
int vp_zero_shard_prodigy_moments(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges,
                                  const float* grad_shard, const float* master, const float* p0, float* exp_avg,
                                  float* exp_avg_sq, float* s, int64_t per, float* partials,
                                  const vp_optim_scalars* scalars, const vp_prodigy_scalars* dstate, double beta1,
                                  double beta2, double beta3, double weight_decay, double d0,
                                  int32_t safeguard_warmup, int32_t use_clip, void* stream);
/* One workgroup: record[0] = sum of partials[2 c], record[1] = sum of partials[2 c + 1] over c in [0, n_ranges), as
 * vp_prodigy_finalize's phase 1 sums its chunks (thread t takes slots t, t + 256, ... in order, in double, then the
 * fixed block sum).  n_ranges = 0 (a rank that owns only padding) and a skipped step still write (0, 0). */
int vp_zero_prodigy_record(const float* partials, int32_t n_ranges, const vp_optim_scalars* scalars, double* record,
                           void* stream);
/* vp_prodigy_finalize over the ranks' records: phase 0 is its phase 0 (records and world are not used); phase 1 sums
 * records[0 .. world) (double [world][2], rank order) with the same strided double sum and runs the same d update
 * (d_numerator, d_denom, d_hat, d, d_max; all ranks' sum |s| == 0: no_progress = 1 and the counter goes back by one).
 * Every rank that passes the same records and blocks gets the same vp_prodigy_scalars, bit for bit.  VP_ERR_ARG as
 * vp_prodigy_finalize, and for world <= 0 or NULL records in phase 1. */
int vp_zero_prodigy_finalize(int32_t phase, const double* records, int32_t world, double lr, double beta1,
                             double beta2, double beta3, double d0, double d_coef, double growth_rate,
                             int32_t use_bias_correction, vp_optim_scalars* scalars, vp_prodigy_scalars* dstate,
                             void* stream);
/* pass 2 over the same ranges: vp_mt_prodigy_update_bf16's arithmetic; master updated in place, param_shard[i] =
 * bf16(p).  12 bytes read and 6 written per element of the shard.  A skipped or no-progress step writes nothing. */
int vp_zero_shard_prodigy_update(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges, float* master,
                                 const float* exp_avg, const float* exp_avg_sq, void* param_shard, int64_t per,
                                 const vp_optim_scalars* scalars, const vp_prodigy_scalars* dstate, double eps,
                                 double weight_decay, void* stream);
/* vp_zero_unpack_bf16 that also writes nothing in a no-progress step (dstate->no_progress): pass 2 left the bf16
 * shards as they were then, so the gathered staging buffer does not hold this step's parameters. */
int vp_zero_unpack_gated_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                              const void* flat, int64_t flat_len, const vp_optim_scalars* scalars,
                              const vp_prodigy_scalars* dstate, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Gradient accumulation in fp32 (ABI 30; csrc/optim.hip, csrc/prodigy.hip): the reference's
 * --gradient_accumulation_steps (train/train_cogvideox_inpainting_i2v_video.py:348, :1743, :1894).  The micro-batches'
 * bf16 gradients are folded into one fp32 accumulator over the flat state space (tensor t at elements [state_off,
 * state_off + numel)), and the norm and the update of the step read that accumulator instead of the bf16 gradients.
 * Same tables and rules as the training tail: 16-byte body, scalar head / tail, no float atomics, no host read. */
/* one fold, over the tensor / chunk tables: acc[state_off + i] = (first ? g : acc[state_off + i] + g) * scale with
 * g = (float)grad[i] — one rounding for the add, one for the product.  scale is 1 except in the last fold of a step,
 * where it is 1 / (number of micro-batches) (the sharded optimizers: 1 / (micro-batches x world), in place of
 * vp_zero_pack_bf16's inv_world); it must be positive and finite.  A tensor whose grad pointer is NULL gets zeros when
 * first and is left as it is otherwise.  zero_grads: the bf16 gradient is zeroed in the same pass.  A chunk that does
 * not fit acc_len writes nothing; padding is never written.  2 bytes read and 4 written per element when first,
 * 6 read and 4 written otherwise, 2 more written with zero_grads.  n_chunks = 0: no launch. */
int vp_mt_accumulate_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks, float* acc,
                          int64_t acc_len, int32_t first, float scale, int32_t zero_grads, void* stream);
/* vp_mt_grad_sqnorm_bf16 with the gradient of tensor t at acc + state_off (fp32; the fp32 bit pattern is tested for
 * inf / NaN): 4 bytes read per element.  The grad pointers of the table are not used. */
int vp_mt_grad_sqnorm_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks, const float* acc,
                          float* partials, int32_t* flags, void* stream);
/* vp_mt_adamw_bf16 / vp_mt_adam_bf16 with the gradient of tensor t at acc + state_off (fp32): the same per-element
 * device function, param = bf16(p) written directly.  16 bytes read and 14 written per element.  The accumulator is
 * left as it is; the bf16 gradients are not touched (the last fold zeroes them); a skipped step writes nothing. */
int vp_mt_adamw_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin, int32_t n_chunks,
                    const float* acc, float* master, float* exp_avg, float* exp_avg_sq,
                    const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int32_t use_clip, void* stream);
int vp_mt_adam_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin, int32_t n_chunks,
                   const float* acc, float* master, float* exp_avg, float* exp_avg_sq,
                   const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int32_t use_clip, void* stream);
/* vp_mt_prodigy_moments_bf16 with the gradient of tensor t at acc + state_off (fp32): 24 bytes read and 12 written
 * per element.  A chunk takes the scalar / vector path the bf16-gradient kernel takes for the table's grad pointer
 * (its phase only; it is not read), so the chunk's two sums are formed in the same order.  Pass 2 reads no gradient:
 * vp_mt_prodigy_update_bf16 as it is (zero_grads = 0 after a fold that zeroed them). */
int vp_mt_prodigy_moments_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                              int32_t n_chunks, const float* acc, const float* master, const float* p0,
                              float* exp_avg, float* exp_avg_sq, float* s, float* partials,
                              const vp_optim_scalars* scalars, const vp_prodigy_scalars* dstate, double beta1,
                              double beta2, double beta3, double weight_decay, double d0, int32_t safeguard_warmup,
                              int32_t use_clip, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The front of the training iteration (ABI 31; csrc/train_inputs.hip): everything between the three VAE encodes and
 * the models, train/train_cogvideox_inpainting_i2v_video.py:1774-1853 — the pixel-space first-frame noise, the three
 * posterior samples with the scaling factor and the [B, C, F, H, W] -> [B, F, C, H, W] permute, the zero-padded image
 * latents and their dropout, the mask's nearest resize as the 17th conditioning channel, scheduler.add_noise and the
 * 32-channel concatenation.  One launch, vector loads / stores, plain stores only, no host read of the device.
 *
 * Noise: a Philox4x32-10 counter generator.  Normal number e (a 64-bit element index) of (seed, stream) comes from
 * block e >> 2, lane e & 3: counter (lo32(block), hi32(block), lo32(stream), hi32(stream)), key (lo32(seed),
 * hi32(seed)), ten rounds with multipliers M0 = 0xD2511F53 (on c0) and M1 = 0xCD9E8D57 (on c2) and key increments
 * 0x9E3779B9 / 0xBB67AE85 between rounds; round output (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1,
 * lo(M0 c0)).  Output words (x0, x1) give lanes 0 and 1, (x2, x3) lanes 2 and 3, by Box-Muller in fp32:
 * u1 = ((xa >> 8) + 1) 2^-24 in (0, 1], u2 = (xb >> 8) 2^-24, r = sqrt(-2 ln u1), even lane r cos(2 pi u2), odd lane
 * r sin(2 pi u2) (logf, sincospif(2 u2): the accurate forms).  The fp32 value is the fp32 output; the bf16 output is
 * its one rounding.  The stream is a function of (seed, stream, e) alone: independent of launch shape and rank count,
 * and continued by continuing the offset. */
/* out[i] = normal number (offset + i) of (seed, stream), i < n; out fp32 (out_is_f32) or bf16.  Any offset and n:
 * whole blocks of four are one vector store where the address allows it, the head and tail scalar stores. */
int vp_philox_normal(void* out, int32_t out_is_f32, int64_t n, uint64_t seed, uint64_t stream, uint64_t offset,
                     void* hip_stream);
/* :1774-1779 on the first frame as the caller laid it out: x [B, n_per] fp32 (x_is_f32) or bf16, sigma [B] bf16 on
 * the device, noise in x's dtype or NULL (then normal number b n_per + i of (seed, stream), drawn in x's dtype as
 * vp_philox_normal draws it).  out bf16 [B, n_per], in torch's promoted arithmetic:
 *   fp32 x:  out = bf16(x + n * float(sigma_b))     the product and the sum each rounded in fp32
 *   bf16 x:  out = bf16(x + bf16(n * sigma_b)) */
int vp_noise_frame(const void* x, int32_t x_is_f32, const void* sigma, const void* noise, void* out, int32_t B,
                   int64_t n_per, uint64_t seed, uint64_t stream, void* hip_stream);
/* :1780-1853 in one launch.  rbf = round to bf16; every product below that is added to something has its own
 * rounding (it is not contracted into an fma).
 *   posterior parameters p_*: the VAE encoder's channels-last rows [B, T, h, w, ldp], mean = channels [0, L),
 *     logvar = [L, 2L); p_image has T = 1 (the noised first frame)
 *   sample(p, n):  lv = clamp(logvar, -30, 20);  std = rbf(expf(rbf(0.5 lv)));  x = rbf(mean + rbf(std n));
 *                  z = rbf(x * scaling_factor)                       (scaling_factor an fp32 value)
 *   noise_video / noise_cond / noise_image: the posterior noises [B, L, T, h, w] bf16 (T = 1 for the image);
 *     noise_diff: the diffusion noise eps [B, T, L, h, w] bf16.  NULL: normal number = the element's linear index in
 *     that layout of (seed, stream_*), rounded to bf16 — what vp_philox_normal(bf16, offset 0) writes into such a
 *     tensor.
 *   target               [B, T, L, h, w]      = z_video
 *   noisy                [B, T, L, h, w]      = rbf(rbf(sa_t z_video) + rbf(sb_t eps)),  (sa_t, sb_t) = sa_sb[t_b],
 *                                               t_b = timesteps[b] clamped to [0, n_alphas) as vp_v_loss_bf16 clamps
 *   noisy_model_input    [B, T, 2L, h, w]     channels [0, L) = noisy;  [L, 2L) = z_image in frame 0, zero in frames
 *                                               >= 1, zero everywhere when image_dropout
 *   masks_latent         [B, T, 1, h, w]      = bf16(mask[b, ft, 0, fy, fx]), F.interpolate(mode="nearest") per axis:
 *                                               src = min((int)floorf((float)dst * ((float)in / (float)out)), in - 1)
 *   conditioning_latents [B, T, L + 1, h, w]  channels [0, L) = z_cond, channel L = masks_latent
 * Every output element is written exactly once and nothing else is written.  16-byte loads and stores when h w is a
 * multiple of 8 and the noise / output pointers are 16-byte aligned, element-wise otherwise (same values).
 * VP_ERR_ARG (before any launch): a NULL required pointer, struct_bytes != sizeof, L != 16, ldp < 2L, B, T, h, w,
 * Fp, Hp, Wp or n_alphas <= 0, mask_dtype not 0..2.  (The image posterior has T = 1 by construction: image_T must
 * be 1.) */
typedef struct {
  int32_t struct_bytes; /* sizeof(vp_train_inputs_desc): the layout check of this descriptor */
  int32_t B, T, h, w, L, ldp;
  int32_t image_T;      /* frames of p_image: must be 1 */
  int32_t Fp, Hp, Wp;   /* the pixel mask [B, Fp, 1, Hp, Wp] */
  int32_t mask_dtype;   /* 0 fp32, 1 bf16, 2 uint8 */
  int32_t image_dropout;
  int32_t n_alphas;
  float scaling_factor;
  int32_t pad0;
  const void* p_video;
  const void* p_cond;
  const void* p_image;
  const void* noise_video;
  const void* noise_cond;
  const void* noise_image;
  const void* noise_diff;
  uint64_t seed, stream_video, stream_cond, stream_image, stream_diff;
  const int64_t* timesteps; /* [B] */
  const float* sa_sb;       /* [n_alphas, 2] */
  const void* mask;
  void* target;
  void* noisy;
  void* noisy_model_input;
  void* masks_latent;
  void* conditioning_latents;
} vp_train_inputs_desc;
int vp_train_inputs_bf16(const vp_train_inputs_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VP_HIP_H */
