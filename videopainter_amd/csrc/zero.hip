// Data-parallel training tail (gfx950): the kernels around the collectives of a sharded optimizer step
// (include/vp_hip.h "Sharded training tail"; videopainter_amd/zero.py).  The element space is the flat fp32 state
// space of csrc/optim.hip (every tensor at its state_off, 8-element aligned), cut into `world` shards of `per`
// elements.  pack / unpack move between the bf16 tensors and the flat staging buffers over the multi-tensor tables;
// the norm and the update — AdamW, plain Adam, or Prodigy's two passes around the cross-rank reduction of its two
// sums — run over this rank's shard, described by a table of ranges (pieces of at most VP_MT_CHUNK elements that cross
// no tensor and leave out padding and tensors without a gradient).  All of it is memory-bound streaming: one workgroup
// per chunk / range, 16-byte loads and stores in the body, scalar head / tail (the whole piece scalar when its streams
// do not share one 16-byte phase), 64-bit offsets, no float atomics, two-stage reductions with a fixed-order
// one-workgroup second stage.
#include "optim_common.h"

namespace {

using namespace vp_optim;

// ---- 1. pack: flat[state_off + i] = float(grad[i]) * inv_world (zeros for a tensor without a gradient) ----
__global__ __launch_bounds__(OT) void zero_pack_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                       const vp_mt_chunk* __restrict__ chunks,
                                                       float* __restrict__ flat, int64_t flat_len, float inv_world,
                                                       int zero_grads) {
#pragma clang fp contract(off)
  const ChunkRange r = chunk_range(tensors, chunks, blockIdx.x);
  const int64_t o = r.t.state_off + r.start;
  if (r.t.state_off < 0 || o + r.n > flat_len) return;  // (a table that does not fit the buffer writes nothing)
  float* out = flat + o;
  bf16* g = (bf16*)r.t.grad;
  if (g == nullptr) {
    zero_piece(out, ((uintptr_t)out & 15) ? r.n : 0, r.n);
    return;
  }
  g += r.start;
  int head = head_of(g, r.n);
  if ((uintptr_t)(out + head) & 15) head = r.n;
  const bf16 zero = f2bf(0.f);
  stream_piece<8>(
      head, r.n,
      [&](int i) {
        out[i] = bf2f(g[i]) * inv_world;
        if (zero_grads) g[i] = zero;
      },
      [&](int e0) {
        float x[8];
        load8(g + e0, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] *= inv_world;
        store8(out + e0, x);
        if (zero_grads) *(bf16x8*)(g + e0) = bf16x8{};
      });
}

// ---- 4. unpack: param[i] = flat[state_off + i] for the tensors that had a gradient (nothing in a skipped step, nor,
// with a d block (ds != NULL: Prodigy), in a no-progress step) ----
__global__ __launch_bounds__(OT) void zero_unpack_kernel(const vp_mt_tensor* __restrict__ tensors,
                                                         const vp_mt_chunk* __restrict__ chunks,
                                                         const bf16* __restrict__ flat, int64_t flat_len,
                                                         const vp_optim_scalars* __restrict__ sc,
                                                         const vp_prodigy_scalars* __restrict__ ds) {
  if (sc->skipped || (ds != nullptr && ds->no_progress)) return;
  const ChunkRange r = chunk_range(tensors, chunks, blockIdx.x);
  if (r.t.grad == nullptr || r.t.param == nullptr) return;
  const int64_t o = r.t.state_off + r.start;
  if (r.t.state_off < 0 || o + r.n > flat_len) return;
  const bf16* in = flat + o;
  bf16* w = (bf16*)r.t.param + r.start;
  int head = head_of(w, r.n);
  if (head_of(in, r.n) != head) head = r.n;
  stream_piece<8>(
      head, r.n, [&](int i) { w[i] = in[i]; }, [&](int e0) { *(bf16x8*)(w + e0) = *(const bf16x8*)(in + e0); });
}

// the piece of the shard range c describes (n = 0 when it does not fit the shard: nothing is read or written)
struct ShardRange {
  int64_t start;
  int n;
};
VP_DEV ShardRange shard_range(const vp_zero_range* __restrict__ ranges, int c, int64_t per) {
  const vp_zero_range rr = ranges[c];
  ShardRange r;
  r.start = rr.start;
  r.n = (rr.start < 0 || rr.n < 0 || rr.n > VP_MT_CHUNK || rr.start + rr.n > per) ? 0 : rr.n;
  return r;
}

// ---- 2. shard norm, stage 1: one fp32 sum of squares and one non-finite flag per range ----
__global__ __launch_bounds__(OT) void zero_sqnorm_kernel(const vp_zero_range* __restrict__ ranges,
                                                         const float* __restrict__ grad, int64_t per,
                                                         float* __restrict__ partials, int* __restrict__ flags) {
  const ShardRange r = shard_range(ranges, blockIdx.x, per);
  const float* g = grad + r.start;
  sqnorm_piece(g, ((uintptr_t)g & 15) ? r.n : 0, r.n, partials, flags);
}

// ---- 2. stage 2 (one workgroup): this rank's (sum, flag) record from its per-range slots, in a fixed order ----
__global__ __launch_bounds__(OT) void zero_record_kernel(const float* __restrict__ partials,
                                                         const int* __restrict__ flags, int n,
                                                         vp_zero_record* __restrict__ rec) {
  int bad_any;
  const float s = sum_slots(partials, flags, 1, n, &bad_any);  // (optim_common.h: the finaliser's own sum)
  if (threadIdx.x != 0) return;
  rec->sqsum = s;
  rec->nonfinite = bad_any;
}

// ---- 2. the finaliser over the ranks' records in rank order: optim.hip's, reading slots of stride 2 ----
__global__ __launch_bounds__(OT) void zero_finalize_kernel(const vp_zero_record* __restrict__ records, int world,
                                                           float max_norm, double beta1, double beta2,
                                                           int skip_nonfinite, vp_optim_scalars* __restrict__ sc) {
  static_assert(sizeof(vp_zero_record) == 8, "a record is one (fp32 sum, int32 flag) pair");
  optim_finalize_body((const float*)records, (const int*)records + 1, 2, world, max_norm, beta1, beta2,
                      skip_nonfinite, 1, sc);
}

// ---- 3. AdamW (L2 = false) or plain Adam (L2 = true: the decay as an L2 term on the gradient) on this rank's shard:
// fp32 gradient, master and moments in, bf16(p) out ----
template <bool L2>
__global__ __launch_bounds__(OT) void zero_adam_kernel(const vp_zero_range* __restrict__ ranges, int range_begin,
                                                        const float* __restrict__ grad, float* __restrict__ master,
                                                        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                        bf16* __restrict__ param, int64_t per,
                                                        const vp_optim_scalars* __restrict__ sc, const AdamArgs a) {
  if (sc->skipped) return;  // a skipped step writes no state and no parameter
  const ShardRange r = shard_range(ranges, range_begin + blockIdx.x, per);
  const float* g = grad + r.start;
  float* pm = master + r.start;
  float* mm = exp_avg + r.start;
  float* vm = exp_avg_sq + r.start;
  bf16* w = param + r.start;
  // (range starts are multiples of 8 elements: with 16-byte aligned buffers every stream is in phase)
  const bool vec = ((((uintptr_t)g | (uintptr_t)pm | (uintptr_t)mm | (uintptr_t)vm | (uintptr_t)w) & 15) == 0);
  adam_piece<L2>(g, pm, mm, vm, w, vec ? 0 : r.n, r.n, a, adam_coef(a, sc));
}

// ---- 3p. Prodigy on this rank's shard.  Pass 1: moments and s in and out, the fp32 gradient, master and p0 read
// only, the range's (dot, sum |s|) pair into partials[2 c] (c: the range's index in the whole table) ----
__global__ __launch_bounds__(OT) void zero_prodigy_moments_kernel(
    const vp_zero_range* __restrict__ ranges, int range_begin, const float* __restrict__ grad,
    const float* __restrict__ master, const float* __restrict__ p0, float* __restrict__ exp_avg,
    float* __restrict__ exp_avg_sq, float* __restrict__ s, int64_t per, float* __restrict__ partials,
    const vp_optim_scalars* __restrict__ sc, const vp_prodigy_scalars* __restrict__ ds, const ProdigyMomentArgs a) {
  if (sc->skipped) return;  // a skipped step writes no state (the record kernel does not read the pairs then)
  const int c = range_begin + blockIdx.x;
  const ShardRange r = shard_range(ranges, c, per);  // (n = 0: nothing is touched, the pair is (0, 0))
  const float* g = grad + r.start;
  const float* pm = master + r.start;
  const float* p0m = p0 + r.start;
  float* mm = exp_avg + r.start;
  float* vm = exp_avg_sq + r.start;
  float* sm = s + r.start;
  const bool vec = ((((uintptr_t)g | (uintptr_t)pm | (uintptr_t)p0m | (uintptr_t)mm | (uintptr_t)vm | (uintptr_t)sm) &
                     15) == 0);
  prodigy_moments_piece(g, pm, p0m, mm, vm, sm, vec ? 0 : r.n, r.n, partials + 2 * (int64_t)c, a,
                        prodigy_moment_coef(a, sc, ds));
}

// ---- this rank's Prodigy record (one workgroup): (sum of dot, sum of sum |s|) over its n range pairs as two doubles,
// summed as prodigy.hip's finaliser sums its chunks.  A skipped step publishes (0, 0): the pairs are stale then. ----
__global__ __launch_bounds__(OT) void zero_prodigy_record_kernel(const float* __restrict__ partials, int n,
                                                                 const vp_optim_scalars* __restrict__ sc,
                                                                 double* __restrict__ rec) {
  double dot, den;
  sum_pairs_f64(partials, sc->skipped ? 0 : n, dot, den);
  if (threadIdx.x != 0) return;
  rec[0] = dot;
  rec[1] = den;
}

// ---- Prodigy's finaliser over the ranks' records in rank order: phase 0 is prodigy.hip's, phase 1 its d update after
// the same strided double sum, so every rank that holds the same records and blocks writes the same d block ----
__global__ __launch_bounds__(OT) void zero_prodigy_begin_kernel(const ProdigyFinalizeArgs a,
                                                                const vp_optim_scalars* __restrict__ sc,
                                                                vp_prodigy_scalars* __restrict__ ds) {
  prodigy_dlr_body(a, sc, ds);
}

__global__ __launch_bounds__(OT) void zero_prodigy_end_kernel(const double* __restrict__ records, int world,
                                                              const ProdigyFinalizeArgs a,
                                                              vp_optim_scalars* __restrict__ sc,
                                                              vp_prodigy_scalars* __restrict__ ds) {
  if (sc->skipped) return;  // (uniform: every thread reads the same word)
  double dot, den;
  sum_pairs_f64(records, world, dot, den);
  if (threadIdx.x != 0) return;
  prodigy_d_update(dot, den, a, sc, ds);
}

// ---- 3p. pass 2: master in and out, moments read only, bf16(p) into the bf16 parameter shard ----
__global__ __launch_bounds__(OT) void zero_prodigy_update_kernel(
    const vp_zero_range* __restrict__ ranges, int range_begin, float* __restrict__ master,
    const float* __restrict__ exp_avg, const float* __restrict__ exp_avg_sq, bf16* __restrict__ param, int64_t per,
    const vp_optim_scalars* __restrict__ sc, const vp_prodigy_scalars* __restrict__ ds, double eps,
    double weight_decay) {
  if (sc->skipped || ds->no_progress) return;  // no state and no parameter is written
  const ShardRange r = shard_range(ranges, range_begin + blockIdx.x, per);
  float* pm = master + r.start;
  const float* mm = exp_avg + r.start;
  const float* vm = exp_avg_sq + r.start;
  bf16* w = param + r.start;
  const bool vec = ((((uintptr_t)pm | (uintptr_t)mm | (uintptr_t)vm | (uintptr_t)w) & 15) == 0);
  prodigy_update_piece(pm, mm, vm, w, vec ? 0 : r.n, r.n, prodigy_update_coef(eps, weight_decay, ds));
}

int launch_unpack(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks, const void* flat,
                  int64_t flat_len, const vp_optim_scalars* scalars, const vp_prodigy_scalars* dstate, void* stream) {
  if (n_chunks < 0 || flat_len < 0 || !scalars) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks || !flat) return VP_ERR_ARG;
  hipLaunchKernelGGL(zero_unpack_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                     (const bf16*)flat, flat_len, scalars, dstate);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

template <bool L2>
int launch_shard_adam(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges, const float* grad_shard,
                      float* master, float* exp_avg, float* exp_avg_sq, void* param_shard, int64_t per,
                      const vp_optim_scalars* scalars, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int32_t use_clip, void* stream) {
  if (n_ranges < 0 || range_begin < 0 || per < 0 || !scalars || !grad_shard || !master || !exp_avg || !exp_avg_sq ||
      !param_shard)
    return VP_ERR_ARG;
  if (!adam_hyper_ok(lr, beta1, beta2, eps, weight_decay)) return VP_ERR_ARG;
  if (n_ranges == 0) return VP_OK;
  if (!ranges) return VP_ERR_ARG;
  const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, use_clip, 0);
  hipLaunchKernelGGL(zero_adam_kernel<L2>, dim3(n_ranges), dim3(OT), 0, (hipStream_t)stream, ranges, range_begin,
                     grad_shard, master, exp_avg, exp_avg_sq, (bf16*)param_shard, per, scalars, a);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

}  // namespace

extern "C" int vp_zero_pack_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                                 float* flat, int64_t flat_len, float inv_world, int32_t zero_grads, void* stream) {
  if (n_chunks < 0 || flat_len < 0 || !(inv_world > 0.f && inv_world <= 1.f)) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks || !flat) return VP_ERR_ARG;
  hipLaunchKernelGGL(zero_pack_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks, flat,
                     flat_len, inv_world, zero_grads);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_zero_unpack_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                                   const void* flat, int64_t flat_len, const vp_optim_scalars* scalars,
                                   void* stream) {
  return launch_unpack(tensors, chunks, n_chunks, flat, flat_len, scalars, nullptr, stream);
}

extern "C" int vp_zero_unpack_gated_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t n_chunks,
                                         const void* flat, int64_t flat_len, const vp_optim_scalars* scalars,
                                         const vp_prodigy_scalars* dstate, void* stream) {
  if (!dstate) return VP_ERR_ARG;
  return launch_unpack(tensors, chunks, n_chunks, flat, flat_len, scalars, dstate, stream);
}

extern "C" int vp_zero_shard_sqnorm(const vp_zero_range* ranges, int32_t n_ranges, const float* grad_shard,
                                    int64_t per, float* partials, int32_t* flags, vp_zero_record* record,
                                    void* stream) {
  if (n_ranges < 0 || per < 0 || !record) return VP_ERR_ARG;
  if (n_ranges > 0) {
    if (!ranges || !grad_shard || !partials || !flags) return VP_ERR_ARG;
    hipLaunchKernelGGL(zero_sqnorm_kernel, dim3(n_ranges), dim3(OT), 0, (hipStream_t)stream, ranges, grad_shard, per,
                       partials, flags);
    VP_CHECK_LAUNCH();
  }
  // (a rank that owns only padding or idle tensors still publishes its record: sum 0, flag 0)
  hipLaunchKernelGGL(zero_record_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, (const float*)partials,
                     (const int*)flags, n_ranges, record);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_zero_finalize(const vp_zero_record* records, int32_t world, float max_norm, double beta1,
                                double beta2, int32_t skip_nonfinite, vp_optim_scalars* scalars, void* stream) {
  if (!records || !scalars || world <= 0) return VP_ERR_ARG;
  if (!finalize_args_ok(max_norm, beta1, beta2, 1)) return VP_ERR_ARG;
  hipLaunchKernelGGL(zero_finalize_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, records, world, max_norm, beta1,
                     beta2, skip_nonfinite, scalars);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_zero_shard_adamw(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges,
                                   const float* grad_shard, float* master, float* exp_avg, float* exp_avg_sq,
                                   void* param_shard, int64_t per, const vp_optim_scalars* scalars, double lr,
                                   double beta1, double beta2, double eps, double weight_decay, int32_t use_clip,
                                   void* stream) {
  return launch_shard_adam<false>(ranges, range_begin, n_ranges, grad_shard, master, exp_avg, exp_avg_sq, param_shard,
                                  per, scalars, lr, beta1, beta2, eps, weight_decay, use_clip, stream);
}

extern "C" int vp_zero_shard_adam(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges,
                                  const float* grad_shard, float* master, float* exp_avg, float* exp_avg_sq,
                                  void* param_shard, int64_t per, const vp_optim_scalars* scalars, double lr,
                                  double beta1, double beta2, double eps, double weight_decay, int32_t use_clip,
                                  void* stream) {
  return launch_shard_adam<true>(ranges, range_begin, n_ranges, grad_shard, master, exp_avg, exp_avg_sq, param_shard,
                                 per, scalars, lr, beta1, beta2, eps, weight_decay, use_clip, stream);
}

extern "C" int vp_zero_shard_prodigy_moments(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges,
                                             const float* grad_shard, const float* master, const float* p0,
                                             float* exp_avg, float* exp_avg_sq, float* s, int64_t per,
                                             float* partials, const vp_optim_scalars* scalars,
                                             const vp_prodigy_scalars* dstate, double beta1, double beta2,
                                             double beta3, double weight_decay, double d0, int32_t safeguard_warmup,
                                             int32_t use_clip, void* stream) {
  if (n_ranges < 0 || range_begin < 0 || per < 0 || !scalars || !dstate || !grad_shard || !master || !p0 ||
      !exp_avg || !exp_avg_sq || !s)
    return VP_ERR_ARG;
  if (!prodigy_hyper_ok(beta1, beta2, beta3, d0) || !finite_nonneg(d0) || !finite_nonneg(weight_decay))
    return VP_ERR_ARG;
  if (n_ranges == 0) return VP_OK;
  if (!ranges || !partials) return VP_ERR_ARG;
  const ProdigyMomentArgs a = prodigy_moment_args(beta1, beta2, beta3, weight_decay, d0, safeguard_warmup, use_clip);
  hipLaunchKernelGGL(zero_prodigy_moments_kernel, dim3(n_ranges), dim3(OT), 0, (hipStream_t)stream, ranges,
                     range_begin, grad_shard, master, p0, exp_avg, exp_avg_sq, s, per, partials, scalars, dstate, a);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_zero_prodigy_record(const float* partials, int32_t n_ranges, const vp_optim_scalars* scalars,
                                      double* record, void* stream) {
  if (n_ranges < 0 || !scalars || !record || (n_ranges > 0 && !partials)) return VP_ERR_ARG;
  // (a rank that owns only padding or idle tensors still publishes its record: (0, 0))
  hipLaunchKernelGGL(zero_prodigy_record_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, partials, n_ranges,
                     scalars, record);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_zero_prodigy_finalize(int32_t phase, const double* records, int32_t world, double lr, double beta1,
                                        double beta2, double beta3, double d0, double d_coef, double growth_rate,
                                        int32_t use_bias_correction, vp_optim_scalars* scalars,
                                        vp_prodigy_scalars* dstate, void* stream) {
  if (!scalars || !dstate || (phase != 0 && phase != 1)) return VP_ERR_ARG;
  if (!prodigy_finalize_args_ok(lr, beta1, beta2, beta3, d0, d_coef, growth_rate)) return VP_ERR_ARG;
  if (phase == 1 && (world <= 0 || !records)) return VP_ERR_ARG;
  const ProdigyFinalizeArgs a{lr, beta1, beta2, beta3, d0, d_coef, growth_rate, use_bias_correction};
  if (phase == 0)
    hipLaunchKernelGGL(zero_prodigy_begin_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, a, scalars, dstate);
  else
    hipLaunchKernelGGL(zero_prodigy_end_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, records, world, a, scalars,
                       dstate);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_zero_shard_prodigy_update(const vp_zero_range* ranges, int32_t range_begin, int32_t n_ranges,
                                            float* master, const float* exp_avg, const float* exp_avg_sq,
                                            void* param_shard, int64_t per, const vp_optim_scalars* scalars,
                                            const vp_prodigy_scalars* dstate, double eps, double weight_decay,
                                            void* stream) {
  if (n_ranges < 0 || range_begin < 0 || per < 0 || !scalars || !dstate || !master || !exp_avg || !exp_avg_sq ||
      !param_shard)
    return VP_ERR_ARG;
  if (!finite_nonneg(eps) || !finite_nonneg(weight_decay)) return VP_ERR_ARG;
  if (n_ranges == 0) return VP_OK;
  if (!ranges) return VP_ERR_ARG;
  hipLaunchKernelGGL(zero_prodigy_update_kernel, dim3(n_ranges), dim3(OT), 0, (hipStream_t)stream, ranges, range_begin,
                     master, exp_avg, exp_avg_sq, (bf16*)param_shard, per, scalars, dstate, eps, weight_decay);
  VP_CHECK_LAUNCH();
  return VP_OK;
}
