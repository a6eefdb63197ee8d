// The tail of the training step (gfx950): the fused v-prediction loss + its gradient, the multi-tensor gradient norm /
// clip, and AdamW / plain Adam with fp32 master weights behind the bf16 parameters (include/vp_hip.h "Training tail").
// All of it is memory-bound streaming: one workgroup per VP_MT_CHUNK elements of one tensor, 16-byte loads / stores in
// the body, scalar head / tail.  Reductions are two-stage (a partial per chunk in its own slot, then one workgroup that
// sums the slots in a fixed order): no float atomics, bit-identical run to run.
#include "optim_common.h"  // shared with csrc/zero.hip: stream_piece, sqnorm_piece, adam_piece, the finaliser

namespace {

using namespace vp_optim;

// ---- a. squared gradient norm, stage 1 ----
__global__ __launch_bounds__(OT) void mt_sqnorm_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                       const vp_mt_chunk* __restrict__ chunks,
                                                       float* __restrict__ partials, int* __restrict__ flags) {
  const ChunkRange r = chunk_range(tensors, chunks, blockIdx.x);
  const bf16* g = (const bf16*)r.t.grad + r.start;
  sqnorm_piece(g, head_of(g, r.n), r.n, partials, flags);
}

// ---- a. stage 2: one workgroup; thread t sums slots t, t + OT, ... in order, then the fixed block sum ----
__global__ __launch_bounds__(OT) void optim_finalize_kernel(const float* __restrict__ partials,
                                                            const int* __restrict__ flags, int n, float max_norm,
                                                            double beta1, double beta2, int skip_nonfinite,
                                                            int advance_step, vp_optim_scalars* __restrict__ sc) {
  optim_finalize_body(partials, flags, 1, n, max_norm, beta1, beta2, skip_nonfinite, advance_step, sc);
}

// ---- b. in-place scale by the device clip coefficient ----
__global__ __launch_bounds__(OT) void mt_scale_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                      const vp_mt_chunk* __restrict__ chunks,
                                                      const vp_optim_scalars* __restrict__ sc) {
  const float coef = sc->clip_coef;
  if (coef == 1.f) return;
  const ChunkRange r = chunk_range(tensors, chunks, blockIdx.x);
  bf16* g = (bf16*)r.t.grad + r.start;
  stream_piece<8>(
      head_of(g, r.n), r.n, [&](int i) { g[i] = f2bf(bf2f(g[i]) * coef); },
      [&](int o) {
        float x[8];
        load8(g + o, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] *= coef;
        store8(g + o, x);
      });
}

// ---- c. AdamW (L2 = false) and plain Adam (L2 = true: the decay as an L2 term on the gradient) with fp32 master
// weights (adam_piece: optim_common.h) ----
template <bool L2>
__global__ __launch_bounds__(OT) void mt_adamw_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                      const vp_mt_chunk* __restrict__ chunks, int chunk_begin,
                                                      float* __restrict__ master, float* __restrict__ exp_avg,
                                                      float* __restrict__ exp_avg_sq,
                                                      const vp_optim_scalars* __restrict__ sc, const AdamArgs a) {
  const ChunkRange r = chunk_range(tensors, chunks, chunk_begin + blockIdx.x);
  bf16* g = (bf16*)r.t.grad + r.start;
  bf16* w = (bf16*)r.t.param + r.start;
  const int64_t so = r.t.state_off + r.start;
  float* pm = master + so;
  float* mm = exp_avg + so;
  float* vm = exp_avg_sq + so;
  // one 16-byte phase for every stream of the chunk, else the whole chunk runs scalar
  int head = head_of(g, r.n);
  if (head_of(w, r.n) != head || (((uintptr_t)(pm + head) | (uintptr_t)(mm + head) | (uintptr_t)(vm + head)) & 15))
    head = r.n;
  if (sc->skipped) {  // a skipped step writes no state and no parameter
    if (a.zero_grads) zero_piece(g, head, r.n);
    return;
  }
  adam_piece<L2>(g, pm, mm, vm, w, head, r.n, a, adam_coef(a, sc));
}

// ---- e. gradient accumulation: one fold of the bf16 gradients into the fp32 flat accumulator (accumulate_piece), and
// the norm and the update with the accumulator as the gradient: tensor t's is acc + state_off, so every fp32 stream of
// a chunk starts at the same flat offset ----
template <bool FIRST>
__global__ __launch_bounds__(OT) void mt_accumulate_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                           const vp_mt_chunk* __restrict__ chunks,
                                                           float* __restrict__ acc, int64_t acc_len, float scale,
                                                           int zero_grads) {
  const ChunkRange r = chunk_range(tensors, chunks, blockIdx.x);
  const int64_t o = r.t.state_off + r.start;
  if (r.t.state_off < 0 || o + r.n > acc_len) return;  // (a table that does not fit the buffer writes nothing)
  float* out = acc + o;
  bf16* g = (bf16*)r.t.grad;
  if (g == nullptr) {  // a tensor without a gradient: zeros in the first fold, as it is afterwards
    if (FIRST) zero_piece(out, ((uintptr_t)out & 15) ? r.n : 0, r.n);
    return;
  }
  g += r.start;
  int head = head_of(g, r.n);
  if ((uintptr_t)(out + head) & 15) head = r.n;
  accumulate_piece<FIRST>(g, out, head, r.n, scale, zero_grads);
}

__global__ __launch_bounds__(OT) void mt_sqnorm_f32_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                           const vp_mt_chunk* __restrict__ chunks,
                                                           const float* __restrict__ acc,
                                                           float* __restrict__ partials, int* __restrict__ flags) {
  const ChunkRange r = chunk_range(tensors, chunks, blockIdx.x);
  const float* g = acc + r.t.state_off + r.start;
  sqnorm_piece(g, ((uintptr_t)g & 15) ? r.n : 0, r.n, partials, flags);
}

template <bool L2>
__global__ __launch_bounds__(OT) void mt_adamw_f32_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                          const vp_mt_chunk* __restrict__ chunks, int chunk_begin,
                                                          const float* __restrict__ acc, float* __restrict__ master,
                                                          float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                          const vp_optim_scalars* __restrict__ sc, const AdamArgs a) {
  if (sc->skipped) return;  // a skipped step writes no state and no parameter (the last fold zeroed the gradients)
  const ChunkRange r = chunk_range(tensors, chunks, chunk_begin + blockIdx.x);
  bf16* w = (bf16*)r.t.param + r.start;
  const int64_t so = r.t.state_off + r.start;
  const float* g = acc + so;
  float* pm = master + so;
  float* mm = exp_avg + so;
  float* vm = exp_avg_sq + so;
  int head = head_of(w, r.n);
  if (((uintptr_t)(g + head) | (uintptr_t)(pm + head) | (uintptr_t)(mm + head) | (uintptr_t)(vm + head)) & 15)
    head = r.n;
  adam_piece<L2>(g, pm, mm, vm, w, head, r.n, a, adam_coef(a, sc));
}

// ---- y = bf16(x * *s) ----
__global__ __launch_bounds__(OT) void scale_dev_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int64_t n,
                                                       const float* __restrict__ s) {
  const float c = *s;
  const bool vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  const int64_t nvec = vec ? n / 8 : 0;
  const int64_t stride = (int64_t)gridDim.x * OT;
  const int64_t tid = (int64_t)blockIdx.x * OT + threadIdx.x;
  for (int64_t i = tid; i < nvec; i += stride) {
    bf16x8 v = ((const bf16x8*)x)[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = f2bf(bf2f(v[e]) * c);
    ((bf16x8*)y)[i] = v;
  }
  for (int64_t i = nvec * 8 + tid; i < n; i += stride) y[i] = f2bf(bf2f(x[i]) * c);
}

// ---- d. the v-prediction loss and its gradient ----
struct LossArgs {
  const bf16* out;
  const bf16* noisy;
  const bf16* target;
  const void* mask;
  int mask_is_f32;
  const int64_t* timesteps;
  const float* ac;
  int n_alphas, F, C, HW;
  int64_t n_sample;  // F * C * HW < 2^31
  int chunks_per_sample;
  float lambda, inv_total;  // 1 / (B * n_sample)
  float* partials;
  bf16* dout;
};

VP_DEV float loss_element(float o, float x, float t, float mk, float sa, float sb, float lambda, float gc, float& q,
                          float& qm) {
#pragma clang fp contract(off)
  const float d = (sa * x - sb * o) - t;
  const float dm = d * mk;
  q += d * d;
  qm += dm * dm;
  return gc * d * (1.f + lambda * (mk * mk));
}

__global__ __launch_bounds__(OT) void v_loss_kernel(const LossArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  int64_t t = a.timesteps[b];
  t = t < 0 ? 0 : (t >= a.n_alphas ? a.n_alphas - 1 : t);
  const float ac = a.ac[t];
  const float sa = sqrtf(ac), sb = sqrtf(1.f - ac), w = 1.f / (1.f - ac);
  const float gc = -2.f * sb * w * a.inv_total;
  const bool masked = a.mask != nullptr;
  const float lambda = masked ? a.lambda : 0.f;
  const int start = blockIdx.x * VP_MT_CHUNK;  // inside the sample (n_sample < 2^31)
  const int64_t left = a.n_sample - start;
  const int n = left < VP_MT_CHUNK ? (int)left : VP_MT_CHUNK;
  const int64_t base = (int64_t)b * a.n_sample + start;
  const bf16* po = a.out + base;
  const bf16* px = a.noisy + base;
  const bf16* pt = a.target + base;
  bf16* pd = a.dout + base;
  int head = head_of(po, n);
  if (head_of(px, n) != head || head_of(pt, n) != head || head_of(pd, n) != head) head = n;
  const int CHW = a.C * a.HW;
  const int64_t mbase = (int64_t)b * a.F * a.HW;
  auto mask_at = [&](int i) -> float {  // i: element inside the sample
    if (!masked) return 0.f;
    const int64_t mi = mbase + (int64_t)(i / CHW) * a.HW + (i % a.HW);
    return a.mask_is_f32 ? ((const float*)a.mask)[mi] : bf2f(((const bf16*)a.mask)[mi]);
  };
  float q = 0.f, qm = 0.f;
  stream_piece<8>(
      head, n,
      [&](int i) {
        pd[i] = f2bf(loss_element(bf2f(po[i]), bf2f(px[i]), bf2f(pt[i]), mask_at(start + i), sa, sb, lambda, gc, q,
                                  qm));
      },
      [&](int o) {
        float o8[8], x8[8], t8[8], d8[8];
        load8(po + o, o8);
        load8(px + o, x8);
        load8(pt + o, t8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          d8[e] = loss_element(o8[e], x8[e], t8[e], mask_at(start + o + e), sa, sb, lambda, gc, q, qm);
        store8(pd + o, d8);
      });
  const float s = block_sum(w * (q + lambda * qm));
  if (threadIdx.x == 0) a.partials[(int64_t)b * a.chunks_per_sample + blockIdx.x] = s;
}

__global__ __launch_bounds__(OT) void sum_partials_kernel(const float* __restrict__ partials, int64_t n, float scale,
                                                          float* __restrict__ out) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += OT) acc += partials[i];
  const float s = block_sum(acc);
  if (threadIdx.x == 0) out[0] = s * scale;
}

}  // namespace

extern "C" int vp_mt_grad_sqnorm_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                                      float* partials, int32_t* flags, void* stream) {
  if (n_chunks < 0) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks || !partials || !flags) return VP_ERR_ARG;
  hipLaunchKernelGGL(mt_sqnorm_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks, partials,
                     flags);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_optim_finalize(const float* partials, const int32_t* flags, int32_t n_chunks, float max_norm,
                                 double beta1, double beta2, int32_t skip_nonfinite, int32_t advance_step,
                                 vp_optim_scalars* scalars, void* stream) {
  if (!scalars || n_chunks < 0 || (n_chunks > 0 && (!partials || !flags))) return VP_ERR_ARG;
  if (!finalize_args_ok(max_norm, beta1, beta2, advance_step)) return VP_ERR_ARG;
  hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, partials, flags, n_chunks,
                     max_norm, beta1, beta2, skip_nonfinite, advance_step, scalars);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_mt_scale_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                                const vp_optim_scalars* scalars, void* stream) {
  if (n_chunks < 0 || !scalars) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks) return VP_ERR_ARG;
  hipLaunchKernelGGL(mt_scale_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks, scalars);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

template <bool L2>
static int mt_adam_launch(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                          int32_t n_chunks, float* master, float* exp_avg, float* exp_avg_sq,
                          const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                          double weight_decay, int32_t use_clip, int32_t zero_grads, void* stream) {
  if (n_chunks < 0 || chunk_begin < 0 || !scalars || !master || !exp_avg || !exp_avg_sq) return VP_ERR_ARG;
  if (!adam_hyper_ok(lr, beta1, beta2, eps, weight_decay)) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks) return VP_ERR_ARG;
  const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, use_clip, zero_grads);
  hipLaunchKernelGGL(mt_adamw_kernel<L2>, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                     chunk_begin, master, exp_avg, exp_avg_sq, scalars, a);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_mt_adamw_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                                int32_t n_chunks, float* master, float* exp_avg, float* exp_avg_sq,
                                const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int32_t use_clip, int32_t zero_grads, void* stream) {
  return mt_adam_launch<false>(tensors, chunks, chunk_begin, n_chunks, master, exp_avg, exp_avg_sq, scalars, lr, beta1,
                               beta2, eps, weight_decay, use_clip, zero_grads, stream);
}

extern "C" int vp_mt_adam_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                               int32_t n_chunks, float* master, float* exp_avg, float* exp_avg_sq,
                               const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int32_t use_clip, int32_t zero_grads, void* stream) {
  return mt_adam_launch<true>(tensors, chunks, chunk_begin, n_chunks, master, exp_avg, exp_avg_sq, scalars, lr, beta1,
                              beta2, eps, weight_decay, use_clip, zero_grads, stream);
}

extern "C" int vp_mt_accumulate_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                                    float* acc, int64_t acc_len, int32_t first, float scale, int32_t zero_grads,
                                    void* stream) {
  if (n_chunks < 0 || acc_len < 0 || !(scale > 0.f && scale <= 3.402823466e38f)) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks || !acc) return VP_ERR_ARG;
  if (first)
    hipLaunchKernelGGL(mt_accumulate_kernel<true>, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                       acc, acc_len, scale, zero_grads);
  else
    hipLaunchKernelGGL(mt_accumulate_kernel<false>, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                       acc, acc_len, scale, zero_grads);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_mt_grad_sqnorm_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                                     const float* acc, float* partials, int32_t* flags, void* stream) {
  if (n_chunks < 0) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks || !acc || !partials || !flags) return VP_ERR_ARG;
  hipLaunchKernelGGL(mt_sqnorm_f32_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks, acc,
                     partials, flags);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

template <bool L2>
static int mt_adam_f32_launch(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                              int32_t n_chunks, const float* acc, float* master, float* exp_avg, float* exp_avg_sq,
                              const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                              double weight_decay, int32_t use_clip, void* stream) {
  if (n_chunks < 0 || chunk_begin < 0 || !scalars || !acc || !master || !exp_avg || !exp_avg_sq) return VP_ERR_ARG;
  if (!adam_hyper_ok(lr, beta1, beta2, eps, weight_decay)) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks) return VP_ERR_ARG;
  const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, use_clip, 0);
  hipLaunchKernelGGL(mt_adamw_f32_kernel<L2>, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                     chunk_begin, acc, master, exp_avg, exp_avg_sq, scalars, a);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_mt_adamw_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                               int32_t n_chunks, const float* acc, float* master, float* exp_avg, float* exp_avg_sq,
                               const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int32_t use_clip, void* stream) {
  return mt_adam_f32_launch<false>(tensors, chunks, chunk_begin, n_chunks, acc, master, exp_avg, exp_avg_sq, scalars,
                                   lr, beta1, beta2, eps, weight_decay, use_clip, stream);
}

extern "C" int vp_mt_adam_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                              int32_t n_chunks, const float* acc, float* master, float* exp_avg, float* exp_avg_sq,
                              const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                              double weight_decay, int32_t use_clip, void* stream) {
  return mt_adam_f32_launch<true>(tensors, chunks, chunk_begin, n_chunks, acc, master, exp_avg, exp_avg_sq, scalars,
                                  lr, beta1, beta2, eps, weight_decay, use_clip, stream);
}

extern "C" int vp_scale_dev_bf16(const void* x, void* y, int64_t n, const float* s, void* stream) {
  if (!x || !y || !s || n <= 0) return VP_ERR_ARG;
  const int64_t want = (n / 8 + OT - 1) / OT + 1;
  hipLaunchKernelGGL(scale_dev_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(OT), 0, (hipStream_t)stream,
                     (const bf16*)x, (bf16*)y, n, s);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int64_t vp_v_loss_partials(int32_t B, int32_t F, int32_t C, int32_t HW) {
  if (B <= 0 || F <= 0 || C <= 0 || HW <= 0 || B > 65535) return -1;
  const int64_t n = (int64_t)F * C * HW;
  if (n > 0x7fffffffll - VP_MT_CHUNK) return -1;
  return (int64_t)B * ((n + VP_MT_CHUNK - 1) / VP_MT_CHUNK);
}

extern "C" int vp_v_loss_bf16(const void* model_output, const void* noisy, const void* target, const void* mask,
                              int32_t mask_is_f32, const int64_t* timesteps, const float* alphas_cumprod,
                              int32_t n_alphas, int32_t B, int32_t F, int32_t C, int32_t HW, float lambda,
                              float* partials, float* loss, void* dout, void* stream) {
  const int64_t slots = vp_v_loss_partials(B, F, C, HW);
  if (slots < 0 || !model_output || !noisy || !target || !timesteps || !alphas_cumprod || n_alphas <= 0 ||
      !partials || !loss || !dout || lambda != lambda)
    return VP_ERR_ARG;
  LossArgs a;
  a.out = (const bf16*)model_output;
  a.noisy = (const bf16*)noisy;
  a.target = (const bf16*)target;
  a.mask = mask;
  a.mask_is_f32 = mask_is_f32;
  a.timesteps = timesteps;
  a.ac = alphas_cumprod;
  a.n_alphas = n_alphas;
  a.F = F;
  a.C = C;
  a.HW = HW;
  a.n_sample = (int64_t)F * C * HW;
  a.chunks_per_sample = (int)(slots / B);
  a.lambda = lambda;
  a.inv_total = (float)(1.0 / ((double)B * (double)a.n_sample));
  a.partials = partials;
  a.dout = (bf16*)dout;
  hipLaunchKernelGGL(v_loss_kernel, dim3(a.chunks_per_sample, B), dim3(OT), 0, (hipStream_t)stream, a);
  VP_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, (const float*)partials, slots,
                     a.inv_total, loss);
  VP_CHECK_LAUNCH();
  return VP_OK;
}
