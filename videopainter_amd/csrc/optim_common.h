// What the optimizer kernels of csrc/optim.hip (one GPU) and csrc/zero.hip (data-parallel, sharded state) share —
// everything but the decoding of their tables and the choice of each piece's scalar head: the workgroup shape and its
// fixed-order sum, stream_piece (scalar head / 16-byte body / scalar tail of one piece), the zero fill, the gradient
// norm's first stage (sqnorm_piece) and finaliser, one fold of a gradient accumulation (accumulate_piece), the AdamW
// update of one piece (adam_piece), the two passes of
// Prodigy over one piece (prodigy_moments_piece, prodigy_update_piece), Prodigy's one-workgroup finaliser (the strided
// double sum, dlr, the d update: over the chunks' pairs in csrc/prodigy.hip, over the ranks' records in csrc/zero.hip)
// and the host-side argument checks.  Both AdamW kernels are adam_piece around the SAME adam_element(), and every
// multiply-add in it is spelled out with contraction off, so they cannot drift apart by a fused multiply-add: a
// world-1 sharded step is bit-identical to the single-GPU step.
#pragma once
#include <type_traits>

#include "vp_common.h"

namespace vp_optim {

constexpr int OT = 256;  // threads per workgroup; VP_MT_CHUNK = OT * 8 elements * 8 rounds
static_assert(VP_MT_CHUNK % (OT * 8) == 0, "a chunk is whole rounds of 8 elements per thread");

// fixed-order sum over the workgroup (xor butterfly inside a wave, then the waves in order); valid in thread 0
VP_DEV float block_sum(float v) {
  __shared__ float red[OT / 64];
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

// the two element types of a gradient (bf16 from the backward, fp32 after the reduce-scatter) and their 16-byte vector
VP_DEV bool nonfinite(bf16 x) { return (__builtin_bit_cast(uint16_t, x) & 0x7f80u) == 0x7f80u; }
VP_DEV bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
VP_DEV float to_f32(bf16 x) { return bf2f(x); }
VP_DEV float to_f32(float x) { return x; }
template <class T>
using vec16_t = std::conditional_t<sizeof(T) == 2, bf16x8, f32x4>;

// 8 consecutive elements as fp32 (16-byte accesses: p is 16-byte aligned)
VP_DEV void load8(const bf16* p, float (&x)[8]) {
  const bf16x8 v = *(const bf16x8*)p;
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = bf2f(v[e]);
}
VP_DEV void load8(const float* p, float (&x)[8]) {
  const f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = lo[e], x[4 + e] = hi[e];
}
VP_DEV void store8(bf16* p, const float (&x)[8]) {
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = f2bf(x[e]);
  *(bf16x8*)p = v;
}
VP_DEV void store8(float* p, const float (&x)[8]) {
  *(f32x4*)p = f32x4{x[0], x[1], x[2], x[3]};
  *(f32x4*)(p + 4) = f32x4{x[4], x[5], x[6], x[7]};
}

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

// ---- one piece (n <= VP_MT_CHUNK elements) over the workgroup: scalar(i) for the first `head` elements, vec(o) for
// every whole W-element vector after them (o: its first element), scalar(i) for the tail.  head == n: all scalar. ----
template <int W, class S, class V>
VP_DEV void stream_piece(int head, int n, S&& scalar, V&& vec) {
  const int nvec = (n - head) / W;
  for (int i = threadIdx.x; i < head; i += OT) scalar(i);
  for (int i = threadIdx.x; i < nvec; i += OT) vec(head + i * W);
  for (int i = head + nvec * W + threadIdx.x; i < n; i += OT) scalar(i);
}

// x[0, n) = 0 (x + head on a 16-byte boundary, or head == n)
template <class T>
VP_DEV void zero_piece(T* __restrict__ x, int head, int n) {
  stream_piece<16 / sizeof(T)>(
      head, n, [&](int i) { x[i] = T(0.f); }, [&](int o) { *(vec16_t<T>*)(x + o) = vec16_t<T>{}; });
}

// ---- stage 1 of a gradient norm over one piece: the fp32 sum of squares (thread t folds its elements in index
// order, one fma each, then the fixed block sum) and the non-finite flag of g[0, n) into slot blockIdx.x ----
template <class T>
VP_DEV void sqnorm_piece(const T* __restrict__ g, int head, int n, float* __restrict__ partials,
                         int* __restrict__ flags) {
#pragma clang fp contract(off)
  constexpr int W = 16 / sizeof(T);
  __shared__ int bad_any;
  float acc = 0.f;
  bool bad = false;
  if (threadIdx.x == 0) bad_any = 0;
  auto one = [&](T x) {
    bad |= nonfinite(x);
    acc = __builtin_fmaf(to_f32(x), to_f32(x), acc);
  };
  stream_piece<W>(
      head, n, [&](int i) { one(g[i]); },
      [&](int o) {
        const vec16_t<T> v = *(const vec16_t<T>*)(g + o);
#pragma unroll
        for (int e = 0; e < W; ++e) one(v[e]);
      });
  __syncthreads();
  if (bad) bad_any = 1;  // (every writer stores the same value)
  const float s = block_sum(acc);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s;
    flags[blockIdx.x] = bad_any;
  }
}

// ---- one fold of a gradient accumulation over one piece: acc[i] = (FIRST ? g : acc[i] + g) * scale with
// g = float(grad[i]) — one rounding for the add, one for the product; the bf16 gradient zeroed in the same pass when
// asked to (acc + head and g + head on a 16-byte boundary, or head == n) ----
template <bool FIRST>
VP_DEV void accumulate_piece(bf16* __restrict__ g, float* __restrict__ acc, int head, int n, float scale,
                             int zero_grads) {
#pragma clang fp contract(off)
  const bf16 zero = f2bf(0.f);
  stream_piece<8>(
      head, n,
      [&](int i) {
        const float x = bf2f(g[i]);
        acc[i] = (FIRST ? x : acc[i] + x) * scale;
        if (zero_grads) g[i] = zero;
      },
      [&](int o) {
        float x[8];
        load8(g + o, x);
        if constexpr (!FIRST) {
          float a[8];
          load8(acc + o, a);
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = a[e] + x[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] *= scale;
        store8(acc + o, x);
        if (zero_grads) *(bf16x8*)(g + o) = bf16x8{};
      });
}

// ---- AdamW with fp32 master weights: the per-element update ----
struct AdamArgs {
  float lr, decay, omb1, beta2, omb2, eps;  // decay = 1 - lr * weight_decay, omb = 1 - beta
  int use_clip, zero_grads;
  float wd;  // weight_decay itself: the L2 term of plain Adam (adam_element<true>)
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
  a.wd = (float)weight_decay;
  return a;
}

// host: the argument checks of the entry points
inline bool betas_ok(double beta1, double beta2) { return beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0; }
inline bool adam_hyper_ok(double lr, double beta1, double beta2, double eps, double weight_decay) {
  return lr >= 0.0 && eps >= 0.0 && weight_decay >= 0.0 && betas_ok(beta1, beta2);
}
inline bool finalize_args_ok(float max_norm, double beta1, double beta2, int advance_step) {
  return max_norm == max_norm && (!advance_step || betas_ok(beta1, beta2));
}

VP_DEV AdamCoef adam_coef(const AdamArgs& a, const vp_optim_scalars* __restrict__ sc) {
  AdamCoef k;
  k.clip = a.use_clip ? sc->clip_coef : 1.f;
  k.step_size = a.lr / sc->bias_c1;
  k.bc2_sqrt = sqrtf(sc->bias_c2);
  return k;
}

// L2 = false: AdamW, the decay as a factor on the parameter.  L2 = true: torch.optim.Adam, the decay as an L2 term on
// the gradient (and no factor on the parameter); the lines below the first two are the same code for both.
template <bool L2 = false>
VP_DEV void adam_element(float g, float& p, float& m, float& v, const AdamArgs& a, const AdamCoef& k) {
  // torch.optim.adamw._single_tensor_adamw, one rounded operation per torch op (no contraction across them)
#pragma clang fp contract(off)
  g *= k.clip;
  if constexpr (L2)
    g = __builtin_fmaf(a.wd, p, g);           // grad.add(param, alpha=weight_decay)
  else
    p *= a.decay;                             // param.mul_(1 - lr * weight_decay)
  m = __builtin_fmaf(a.omb1, g - m, m);       // exp_avg.lerp_(grad, 1 - beta1)
  v = v * a.beta2 + a.omb2 * g * g;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / k.bc2_sqrt + a.eps;
  p = p - k.step_size * (m / denom);          // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// ---- the update of one piece: gradient g[0, n) (bf16, or fp32 from the reduce-scatter), master and moments in and
// out, bf16(master) into w.  The caller picks `head` (every stream 16-byte aligned at `head`, or head == n); that
// decides which path an element takes, not its value.  Only a bf16 gradient can be zeroed in the same pass. ----
template <bool L2 = false, class G>
VP_DEV void adam_piece(G* __restrict__ g, float* __restrict__ pm, float* __restrict__ mm, float* __restrict__ vm,
                       bf16* __restrict__ w, int head, int n, const AdamArgs& a, const AdamCoef& k) {
  constexpr bool can_zero = std::is_same_v<G, bf16>;
  stream_piece<8>(
      head, n,
      [&](int i) {
        float p = pm[i], m = mm[i], v = vm[i];
        adam_element<L2>(to_f32(g[i]), p, m, v, a, k);
        pm[i] = p;
        mm[i] = m;
        vm[i] = v;
        w[i] = f2bf(p);
        if constexpr (can_zero)
          if (a.zero_grads) g[i] = f2bf(0.f);
      },
      [&](int o) {
        float g8[8], p[8], m[8], v[8];
        load8(g + o, g8);
        load8(pm + o, p);
        load8(mm + o, m);
        load8(vm + o, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) adam_element<L2>(g8[e], p[e], m[e], v[e], a, k);
        store8(pm + o, p);
        store8(mm + o, m);
        store8(vm + o, v);
        store8(w + o, p);
        if constexpr (can_zero)
          if (a.zero_grads) *(bf16x8*)(g + o) = bf16x8{};
      });
}

// ---- Prodigy with fp32 master weights (prodigyopt 1.0's step(), slice_p = 1): the per-element work of its two
// passes.  The distance estimate is a block of doubles on the device; each pass rounds the products it needs to fp32
// once per thread (the reference forms them in Python floats and torch rounds them to the tensors' fp32). ----
struct ProdigyMomentArgs {
  float beta1, beta2, beta3, wd;  // wd: the coupled decay (0 when decoupled)
  double omb1, omb2, d0;          // omb = 1 - beta
  int safeguard, use_clip;
};

struct ProdigyMomentCoef {
  float clip, c1, c2, c3;  // d (1 - beta1), d^2 (1 - beta2), (d / d0) (safeguard ? d : dlr)
};

inline ProdigyMomentArgs prodigy_moment_args(double beta1, double beta2, double beta3, double weight_decay, double d0,
                                             int safeguard, int use_clip) {
  ProdigyMomentArgs a;
  a.beta1 = (float)beta1;
  a.beta2 = (float)beta2;
  a.beta3 = (float)beta3;
  a.wd = (float)weight_decay;
  a.omb1 = 1.0 - beta1;
  a.omb2 = 1.0 - beta2;
  a.d0 = d0;
  a.safeguard = safeguard;
  a.use_clip = use_clip;
  return a;
}

inline bool prodigy_hyper_ok(double beta1, double beta2, double beta3, double d0) {
  return betas_ok(beta1, beta2) && beta3 >= 0.0 && beta3 < 1.0 && d0 > 0.0;
}

VP_DEV ProdigyMomentCoef prodigy_moment_coef(const ProdigyMomentArgs& a, const vp_optim_scalars* __restrict__ sc,
                                             const vp_prodigy_scalars* __restrict__ ds) {
#pragma clang fp contract(off)
  const double d = ds->d, dlr = ds->dlr;
  ProdigyMomentCoef k;
  k.clip = a.use_clip ? sc->clip_coef : 1.f;
  k.c1 = (float)(d * a.omb1);
  k.c2 = (float)(d * d * a.omb2);
  k.c3 = (float)((d / a.d0) * (a.safeguard ? d : dlr));
  return k;
}

VP_DEV void prodigy_moment_element(float g, float p, float p0, float& m, float& v, float& s, float& dot, float& den,
                                   const ProdigyMomentArgs& a, const ProdigyMomentCoef& k) {
  // one rounded operation per torch op of the reference's first loop (no contraction across them)
#pragma clang fp contract(off)
  g *= k.clip;
  if (a.wd != 0.f) g = __builtin_fmaf(a.wd, p, g);  // grad.add_(p, alpha=decay)
  dot = __builtin_fmaf(g, p0 - p, dot);             // torch.dot(grad, p0 - p)
  m = m * a.beta1 + k.c1 * g;                       // exp_avg.mul_(beta1).add_(grad, alpha=d * (1 - beta1))
  v = v * a.beta2 + k.c2 * g * g;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=d d (1 - b2))
  s = s * a.beta3 + k.c3 * g;                       // s.mul_(beta3).add_(grad, alpha=(d / d0) * dlr)
  den += fabsf(s);                                  // s.abs().sum()
}

// pass 1 of one piece: moments and s in and out, master and p0 read only, the piece's (dot, sum |s|) into
// partials[0], partials[1] (thread t folds its elements in index order, then the fixed block sum)
template <class G>
VP_DEV void prodigy_moments_piece(const G* __restrict__ g, const float* __restrict__ pm, const float* __restrict__ p0m,
                                  float* __restrict__ mm, float* __restrict__ vm, float* __restrict__ sm, int head,
                                  int n, float* __restrict__ partials, const ProdigyMomentArgs& a,
                                  const ProdigyMomentCoef& k) {
  float dot = 0.f, den = 0.f;
  stream_piece<8>(
      head, n,
      [&](int i) {
        float m = mm[i], v = vm[i], s = sm[i];
        prodigy_moment_element(to_f32(g[i]), pm[i], p0m[i], m, v, s, dot, den, a, k);
        mm[i] = m;
        vm[i] = v;
        sm[i] = s;
      },
      [&](int o) {
        float g8[8], p[8], p0[8], m[8], v[8], s[8];
        load8(g + o, g8);
        load8(pm + o, p);
        load8(p0m + o, p0);
        load8(mm + o, m);
        load8(vm + o, v);
        load8(sm + o, s);
#pragma unroll
        for (int e = 0; e < 8; ++e) prodigy_moment_element(g8[e], p[e], p0[e], m[e], v[e], s[e], dot, den, a, k);
        store8(mm + o, m);
        store8(vm + o, v);
        store8(sm + o, s);
      });
  const float sd = block_sum(dot);
  const float sn = block_sum(den);
  if (threadIdx.x == 0) {
    partials[0] = sd;
    partials[1] = sn;
  }
}

struct ProdigyUpdateCoef {
  float deps, wdl, dlr;  // d eps with the NEW d, -weight_decay dlr (0: no decoupled decay), dlr
};

VP_DEV ProdigyUpdateCoef prodigy_update_coef(double eps, double weight_decay,
                                             const vp_prodigy_scalars* __restrict__ ds) {
#pragma clang fp contract(off)
  ProdigyUpdateCoef k;
  k.deps = (float)(ds->d * eps);
  k.wdl = (float)(-weight_decay * ds->dlr);
  k.dlr = (float)ds->dlr;
  return k;
}

VP_DEV void prodigy_update_element(float& p, float m, float v, const ProdigyUpdateCoef& k) {
  // the reference's second loop, one rounded operation per torch op
#pragma clang fp contract(off)
  const float denom = sqrtf(v) + k.deps;              // exp_avg_sq.sqrt().add_(d * eps)
  if (k.wdl != 0.f) p = __builtin_fmaf(p, k.wdl, p);  // p.add_(p, alpha=-decay * dlr)
  p = p - k.dlr * (m / denom);                        // p.addcdiv_(exp_avg, denom, value=-dlr)
}

// pass 2 of one piece: master in and out, moments read only, bf16(master) into w
VP_DEV void prodigy_update_piece(float* __restrict__ pm, const float* __restrict__ mm, const float* __restrict__ vm,
                                 bf16* __restrict__ w, int head, int n, const ProdigyUpdateCoef& k) {
  stream_piece<8>(
      head, n,
      [&](int i) {
        float p = pm[i];
        prodigy_update_element(p, mm[i], vm[i], k);
        pm[i] = p;
        w[i] = f2bf(p);
      },
      [&](int o) {
        float p[8], m[8], v[8];
        load8(pm + o, p);
        load8(mm + o, m);
        load8(vm + o, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) prodigy_update_element(p[e], m[e], v[e], k);
        store8(pm + o, p);
        store8(w + o, p);
      });
}

// ---- second stage of every reduction here (one workgroup): the fixed-order sum of n slots and the OR of their flags.
// Thread t takes slots t, t + OT, ... in order, then the fixed block sum; slot i is partials[i * stride] /
// flags[i * stride].  The sum is valid in thread 0, *any_bad in every thread after the call. ----
VP_DEV float sum_slots(const float* __restrict__ partials, const int* __restrict__ flags, int stride, int n,
                       int* any_bad) {
#pragma clang fp contract(off)
  __shared__ int bad_any;
  if (threadIdx.x == 0) bad_any = 0;
  float acc = 0.f;
  bool bad = false;
  for (int i = threadIdx.x; i < n; i += OT) {
    acc += partials[(int64_t)i * stride];
    bad |= flags[(int64_t)i * stride] != 0;
  }
  __syncthreads();
  if (bad) bad_any = 1;
  const float s = block_sum(acc);
  *any_bad = bad_any;
  return s;
}

// ---- the finaliser of the gradient norm: sum_slots, then the scalars block (stride 1: the per-chunk workspace of one
// GPU; stride 2: the (sum, flag) records of the ranks, in rank order) ----
VP_DEV void optim_finalize_body(const float* __restrict__ partials, const int* __restrict__ flags, int stride, int n,
                                float max_norm, double beta1, double beta2, int skip_nonfinite, int advance_step,
                                vp_optim_scalars* __restrict__ sc) {
#pragma clang fp contract(off)
  int nonfinite;
  const float s = sum_slots(partials, flags, stride, n, &nonfinite);
  if (threadIdx.x != 0) return;
  const float norm = sqrtf(s);
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

// ---- Prodigy's finaliser (one workgroup), shared by csrc/prodigy.hip (the sums run over the chunks' pairs) and
// csrc/zero.hip (over the ranks' records): the fixed-order double sum, dlr of the step, and the d update ----

// fixed-order sum of doubles over the workgroup, as block_sum; valid in thread 0
VP_DEV double block_sum_f64(double v) {
  __shared__ double red64[OT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red64[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < OT / 64; ++w) s += red64[w];
  }
  __syncthreads();
  return s;
}

// (sum of x[0], x[2], ...; sum of x[1], x[3], ...) over n pairs of fp32 or double: thread t takes pairs t, t + OT, ...
// in order, in double, then the fixed block sum; valid in thread 0
template <class T>
VP_DEV void sum_pairs_f64(const T* __restrict__ x, int n, double& a, double& b) {
#pragma clang fp contract(off)
  double sa = 0.0, sb = 0.0;
  for (int i = threadIdx.x; i < n; i += OT) {
    sa += (double)x[2 * (int64_t)i];
    sb += (double)x[2 * (int64_t)i + 1];
  }
  a = block_sum_f64(sa);
  b = block_sum_f64(sb);
}

struct ProdigyFinalizeArgs {
  double lr, beta1, beta2, beta3, d0, d_coef, growth_rate;
  int use_bias_correction;
};

inline bool finite_nonneg(double x) { return x >= 0.0 && x <= 1.79769313486231570e308; }
inline bool prodigy_finalize_args_ok(double lr, double beta1, double beta2, double beta3, double d0, double d_coef,
                                     double growth_rate) {
  return finite_nonneg(lr) && prodigy_hyper_ok(beta1, beta2, beta3, d0) && finite_nonneg(d0) && d_coef > 0.0 &&
         finite_nonneg(d_coef) && growth_rate >= 1.0;  // (growth_rate may be +inf: no limit)
}

// phase 0 (every thread may call; thread 0 writes): dlr of the step from the OLD d and the counter the norm's finaliser
// has advanced already
VP_DEV void prodigy_dlr_body(const ProdigyFinalizeArgs& a, const vp_optim_scalars* __restrict__ sc,
                             vp_prodigy_scalars* __restrict__ ds) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || sc->skipped) return;
  double bc = 1.0;
  if (a.use_bias_correction) {
    const double step = (double)sc->step;  // k + 1
    bc = sqrt(1.0 - pow(a.beta2, step)) / (1.0 - pow(a.beta1, step));
  }
  ds->dlr = ds->d * a.lr * bc;
}

// phase 1 after the sums (thread 0 only): the d update from dot = sum <g, p0 - p> and den = sum |s|
VP_DEV void prodigy_d_update(double dot, double den, const ProdigyFinalizeArgs& a, vp_optim_scalars* __restrict__ sc,
                             vp_prodigy_scalars* __restrict__ ds) {
#pragma clang fp contract(off)
  if (den == 0.0) {  // no progress: pass 2 writes nothing, the counter goes back, d and its numerator stay
    ds->d_denom = 0.0;
    ds->no_progress = 1;
    sc->step = sc->step - 1;
    return;
  }
  double d = ds->d, d_max = ds->d_max;
  const double num = ds->d_numerator * a.beta3 + (d / a.d0) * ds->dlr * dot;
  ds->d_numerator = num;
  ds->d_denom = den;
  ds->no_progress = 0;
  if (a.lr > 0.0) {
    const double d_hat = a.d_coef * num / den;
    if (d == a.d0) d = d > d_hat ? d : d_hat;
    d_max = d_max > d_hat ? d_max : d_hat;
    const double grown = d * a.growth_rate;
    d = d_max < grown ? d_max : grown;
    ds->d_hat = d_hat;
    ds->d_max = d_max;
    ds->d = d;
  }
}

}  // namespace vp_optim
