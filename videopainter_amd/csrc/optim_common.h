// What the optimizer kernels of csrc/optim.hip (one GPU) and csrc/zero.hip (data-parallel, sharded state) share: the
// workgroup shape, the fixed-order workgroup sum, the chunk decoding of the multi-tensor tables, the per-element AdamW
// update and the finaliser of the gradient norm.  The two AdamW kernels call the SAME adam_element() with the same
// AdamArgs / AdamCoef, and every multiply-add in it is spelled out with contraction off, so they cannot drift apart by
// a fused multiply-add: a world-1 sharded step is bit-identical to the single-GPU step.
#pragma once
#include "vp_common.h"

namespace vp_optim {

constexpr int OT = 256;  // threads per workgroup; VP_MT_CHUNK = OT * 8 elements * 8 rounds
static_assert(VP_MT_CHUNK % (OT * 8) == 0, "a chunk is whole rounds of 8 elements per thread");

// fixed-order sum over the workgroup (xor butterfly inside a wave, then the waves in order); valid in thread 0
VP_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < OT / 64; ++w) s += red[w];
  }
  __syncthreads();
  return s;
}

VP_DEV bool bf16_nonfinite(bf16 x) { return (__builtin_bit_cast(uint16_t, x) & 0x7f80u) == 0x7f80u; }
VP_DEV bool f32_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// the element range of chunk c: tensor entry, first element, count
struct ChunkRange {
  vp_mt_tensor t;
  int64_t start;
  int n;
};
VP_DEV ChunkRange chunk_range(const vp_mt_tensor* __restrict__ tensors, const vp_mt_chunk* __restrict__ chunks,
                              int c) {
  const vp_mt_chunk ch = chunks[c];
  ChunkRange r;
  r.t = tensors[ch.tensor];
  r.start = (int64_t)ch.chunk * VP_MT_CHUNK;
  const int64_t left = r.t.numel - r.start;
  r.n = left < VP_MT_CHUNK ? (left > 0 ? (int)left : 0) : VP_MT_CHUNK;
  return r;
}

// scalar elements before p reaches a 16-byte boundary (all n when p is not even 2-byte aligned)
VP_DEV int head_of(const void* p, int n) {
  const uintptr_t a = (uintptr_t)p;
  if (a & 1) return n;
  const int h = (int)(((16 - (a & 15)) & 15) >> 1);
  return h < n ? h : n;
}

// ---- AdamW with fp32 master weights: the per-element update ----
struct AdamArgs {
  float lr, decay, omb1, beta2, omb2, eps;  // decay = 1 - lr * weight_decay, omb = 1 - beta
  int use_clip, zero_grads;
};

struct AdamCoef {
  float clip, step_size, bc2_sqrt;
};

// host: the fp32 constants of one launch from the double hyper-parameters (one rounding each)
inline AdamArgs adam_args(double lr, double beta1, double beta2, double eps, double weight_decay, int use_clip,
                          int zero_grads) {
  AdamArgs a;
  a.lr = (float)lr;
  a.decay = (float)(1.0 - lr * weight_decay);
  a.omb1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.use_clip = use_clip;
  a.zero_grads = zero_grads;
  return a;
}

inline bool adam_hyper_ok(double lr, double beta1, double beta2, double eps, double weight_decay) {
  return lr >= 0.0 && eps >= 0.0 && weight_decay >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0;
}

VP_DEV AdamCoef adam_coef(const AdamArgs& a, const vp_optim_scalars* __restrict__ sc) {
  AdamCoef k;
  k.clip = a.use_clip ? sc->clip_coef : 1.f;
  k.step_size = a.lr / sc->bias_c1;
  k.bc2_sqrt = sqrtf(sc->bias_c2);
  return k;
}

VP_DEV void adam_element(float g, float& p, float& m, float& v, const AdamArgs& a, const AdamCoef& k) {
  // torch.optim.adamw._single_tensor_adamw, one rounded operation per torch op (no contraction across them)
#pragma clang fp contract(off)
  g *= k.clip;
  p *= a.decay;                               // param.mul_(1 - lr * weight_decay)
  m = __builtin_fmaf(a.omb1, g - m, m);       // exp_avg.lerp_(grad, 1 - beta1)
  v = v * a.beta2 + a.omb2 * g * g;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / k.bc2_sqrt + a.eps;
  p = p - k.step_size * (m / denom);          // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// ---- second stage of every reduction here (one workgroup): the fixed-order sum of n slots and the OR of their flags.
// Thread t takes slots t, t + OT, ... in order, then the fixed block sum; slot i is partials[i * stride] /
// flags[i * stride].  The sum is valid in thread 0, *bad_any in every thread after the call. ----
VP_DEV float sum_slots(const float* __restrict__ partials, const int* __restrict__ flags, int stride, int n,
                       float* red, int* bad_any) {
#pragma clang fp contract(off)
  if (threadIdx.x == 0) *bad_any = 0;
  float acc = 0.f;
  bool bad = false;
  for (int i = threadIdx.x; i < n; i += OT) {
    acc += partials[(int64_t)i * stride];
    bad |= flags[(int64_t)i * stride] != 0;
  }
  __syncthreads();
  if (bad) *bad_any = 1;
  return block_sum(acc, red);
}

// ---- the finaliser of the gradient norm: sum_slots, then the scalars block (stride 1: the per-chunk workspace of one
// GPU; stride 2: the (sum, flag) records of the ranks, in rank order) ----
VP_DEV void optim_finalize_body(const float* __restrict__ partials, const int* __restrict__ flags, int stride, int n,
                                float max_norm, double beta1, double beta2, int skip_nonfinite, int advance_step,
                                vp_optim_scalars* __restrict__ sc, float* red, int* bad_any) {
#pragma clang fp contract(off)
  const float s = sum_slots(partials, flags, stride, n, red, bad_any);
  if (threadIdx.x != 0) return;
  const float norm = sqrtf(s);
  const int nonfinite = *bad_any;
  sc->grad_norm = norm;
  sc->nonfinite = nonfinite;
  float coef = 1.f;
  if (max_norm > 0.f) {
    coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;  // (a NaN coefficient stays NaN, as torch.clamp keeps it)
  }
  sc->clip_coef = coef;
  if (!advance_step) return;
  const int skipped = (nonfinite && skip_nonfinite) ? 1 : 0;
  sc->skipped = skipped;
  if (skipped) return;
  const int step = sc->step + 1;
  sc->step = step;
  sc->bias_c1 = (float)(1.0 - pow(beta1, (double)step));
  sc->bias_c2 = (float)(1.0 - pow(beta2, (double)step));
}

}  // namespace vp_optim
