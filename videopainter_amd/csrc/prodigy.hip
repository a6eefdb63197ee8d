// Prodigy with fp32 master weights behind the bf16 parameters (gfx950; include/vp_hip.h "Plain Adam and Prodigy"):
// two streaming passes over the chunk tables of csrc/optim.hip with a one-workgroup finaliser before and between
// them.  The new d enters the update through d * eps, so the update cannot be folded into the pass that measures d.
// The passes are the piece functions of optim_common.h; the distance estimate is a block of doubles that only the
// finaliser writes, with ordinary stores from one thread.  No float atomics: one (dot, sum |s|) pair per chunk, summed
// in a fixed order in double, so a step is bit-identical run to run.
#include "optim_common.h"

namespace {

using namespace vp_optim;

// ---- phase 0: dlr of the step from the OLD d and the counter vp_optim_finalize has advanced already ----
__global__ __launch_bounds__(OT) void prodigy_begin_kernel(const ProdigyFinalizeArgs a,
                                                           const vp_optim_scalars* __restrict__ sc,
                                                           vp_prodigy_scalars* __restrict__ ds) {
  prodigy_dlr_body(a, sc, ds);
}

// ---- phase 1: the two sums (thread t takes chunks t, t + OT, ... in order, then the fixed block sum) and the d
// update (optim_common.h: the sharded finaliser runs the same body over the ranks' records) ----
__global__ __launch_bounds__(OT) void prodigy_end_kernel(const float* __restrict__ partials, int n,
                                                         const ProdigyFinalizeArgs a,
                                                         vp_optim_scalars* __restrict__ sc,
                                                         vp_prodigy_scalars* __restrict__ ds) {
  if (sc->skipped) return;  // (uniform: every thread reads the same word)
  double dot, den;
  sum_pairs_f64(partials, n, dot, den);
  if (threadIdx.x != 0) return;
  prodigy_d_update(dot, den, a, sc, ds);
}

// ---- pass 1 ----
__global__ __launch_bounds__(OT) void mt_prodigy_moments_kernel(
    const vp_mt_tensor* __restrict__ tensors, const vp_mt_chunk* __restrict__ chunks, int chunk_begin,
    const float* __restrict__ master, const float* __restrict__ p0, float* __restrict__ exp_avg,
    float* __restrict__ exp_avg_sq, float* __restrict__ s, float* __restrict__ partials,
    const vp_optim_scalars* __restrict__ sc, const vp_prodigy_scalars* __restrict__ ds, const ProdigyMomentArgs a) {
  if (sc->skipped) return;  // a skipped step writes no state (the finaliser does not read the partials then)
  const int c = chunk_begin + blockIdx.x;
  const ChunkRange r = chunk_range(tensors, chunks, c);
  const bf16* g = (const bf16*)r.t.grad + r.start;
  const int64_t so = r.t.state_off + r.start;
  const float* pm = master + so;
  const float* p0m = p0 + so;
  float* mm = exp_avg + so;
  float* vm = exp_avg_sq + so;
  float* sm = s + so;
  // one 16-byte phase for every stream of the chunk, else the whole chunk runs scalar
  int head = head_of(g, r.n);
  if (((uintptr_t)(pm + head) | (uintptr_t)(p0m + head) | (uintptr_t)(mm + head) | (uintptr_t)(vm + head) |
       (uintptr_t)(sm + head)) & 15)
    head = r.n;
  prodigy_moments_piece(g, pm, p0m, mm, vm, sm, head, r.n, partials + 2 * (int64_t)c, a,
                        prodigy_moment_coef(a, sc, ds));
}

// ---- pass 1 on an accumulated gradient: the fp32 accumulator is the gradient, tensor t's at acc + state_off ----
__global__ __launch_bounds__(OT) void mt_prodigy_moments_f32_kernel(
    const vp_mt_tensor* __restrict__ tensors, const vp_mt_chunk* __restrict__ chunks, int chunk_begin,
    const float* __restrict__ acc, const float* __restrict__ master, const float* __restrict__ p0,
    float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, float* __restrict__ s, float* __restrict__ partials,
    const vp_optim_scalars* __restrict__ sc, const vp_prodigy_scalars* __restrict__ ds, const ProdigyMomentArgs a) {
  if (sc->skipped) return;
  const int c = chunk_begin + blockIdx.x;
  const ChunkRange r = chunk_range(tensors, chunks, c);
  const int64_t so = r.t.state_off + r.start;
  const float* g = acc + so;
  const float* pm = master + so;
  const float* p0m = p0 + so;
  float* mm = exp_avg + so;
  float* vm = exp_avg_sq + so;
  float* sm = s + so;
  // the head is the one the bf16-gradient kernel picks from the phase of the last folded gradient (the pointer is not
  // dereferenced): an element's path decides the order of the chunk's two sums, so a step on an accumulated gradient
  // sums as a step on that gradient itself would
  int head = head_of((const bf16*)r.t.grad + r.start, r.n);
  if (((uintptr_t)(g + head) | (uintptr_t)(pm + head) | (uintptr_t)(p0m + head) | (uintptr_t)(mm + head) |
       (uintptr_t)(vm + head) | (uintptr_t)(sm + head)) & 15)
    head = r.n;
  prodigy_moments_piece(g, pm, p0m, mm, vm, sm, head, r.n, partials + 2 * (int64_t)c, a,
                        prodigy_moment_coef(a, sc, ds));
}

// ---- pass 2 ----
__global__ __launch_bounds__(OT) void mt_prodigy_update_kernel(
    const vp_mt_tensor* __restrict__ tensors, const vp_mt_chunk* __restrict__ chunks, int chunk_begin,
    float* __restrict__ master, const float* __restrict__ exp_avg, const float* __restrict__ exp_avg_sq,
    const vp_optim_scalars* __restrict__ sc, const vp_prodigy_scalars* __restrict__ ds, double eps,
    double weight_decay, int zero_grads) {
  const ChunkRange r = chunk_range(tensors, chunks, chunk_begin + blockIdx.x);
  bf16* g = (bf16*)r.t.grad + r.start;
  if (zero_grads) zero_piece(g, head_of(g, r.n), r.n);  // (the gradient is not read here: a phase of its own)
  if (sc->skipped || ds->no_progress) return;           // no state and no parameter is written
  bf16* w = (bf16*)r.t.param + r.start;
  const int64_t so = r.t.state_off + r.start;
  float* pm = master + so;
  const float* mm = exp_avg + so;
  const float* vm = exp_avg_sq + so;
  int head = head_of(w, r.n);
  if (((uintptr_t)(pm + head) | (uintptr_t)(mm + head) | (uintptr_t)(vm + head)) & 15) head = r.n;
  prodigy_update_piece(pm, mm, vm, w, head, r.n, prodigy_update_coef(eps, weight_decay, ds));
}

}  // namespace

extern "C" int vp_prodigy_finalize(int32_t phase, const float* partials, int32_t n_chunks, double lr, double beta1,
                                   double beta2, double beta3, double d0, double d_coef, double growth_rate,
                                   int32_t use_bias_correction, vp_optim_scalars* scalars, vp_prodigy_scalars* dstate,
                                   void* stream) {
  if (!scalars || !dstate || (phase != 0 && phase != 1)) return VP_ERR_ARG;
  if (!prodigy_finalize_args_ok(lr, beta1, beta2, beta3, d0, d_coef, growth_rate)) return VP_ERR_ARG;
  if (phase == 1 && (n_chunks < 0 || (n_chunks > 0 && !partials))) return VP_ERR_ARG;
  const ProdigyFinalizeArgs a{lr, beta1, beta2, beta3, d0, d_coef, growth_rate, use_bias_correction};
  if (phase == 0)
    hipLaunchKernelGGL(prodigy_begin_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, a, scalars, dstate);
  else
    hipLaunchKernelGGL(prodigy_end_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, partials, n_chunks, a, scalars,
                       dstate);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_mt_prodigy_moments_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                                          int32_t n_chunks, const float* master, const float* p0, float* exp_avg,
                                          float* exp_avg_sq, float* s, float* partials,
                                          const vp_optim_scalars* scalars, const vp_prodigy_scalars* dstate,
                                          double beta1, double beta2, double beta3, double weight_decay, double d0,
                                          int32_t safeguard_warmup, int32_t use_clip, void* stream) {
  if (n_chunks < 0 || chunk_begin < 0 || !scalars || !dstate || !master || !p0 || !exp_avg || !exp_avg_sq || !s)
    return VP_ERR_ARG;
  if (!prodigy_hyper_ok(beta1, beta2, beta3, d0) || !finite_nonneg(d0) || !finite_nonneg(weight_decay))
    return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks || !partials) return VP_ERR_ARG;
  const ProdigyMomentArgs a = prodigy_moment_args(beta1, beta2, beta3, weight_decay, d0, safeguard_warmup, use_clip);
  hipLaunchKernelGGL(mt_prodigy_moments_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                     chunk_begin, master, p0, exp_avg, exp_avg_sq, s, partials, scalars, dstate, a);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_mt_prodigy_moments_f32(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                                         int32_t n_chunks, const float* acc, const float* master, const float* p0,
                                         float* exp_avg, float* exp_avg_sq, float* s, float* partials,
                                         const vp_optim_scalars* scalars, const vp_prodigy_scalars* dstate,
                                         double beta1, double beta2, double beta3, double weight_decay, double d0,
                                         int32_t safeguard_warmup, int32_t use_clip, void* stream) {
  if (n_chunks < 0 || chunk_begin < 0 || !scalars || !dstate || !acc || !master || !p0 || !exp_avg || !exp_avg_sq ||
      !s)
    return VP_ERR_ARG;
  if (!prodigy_hyper_ok(beta1, beta2, beta3, d0) || !finite_nonneg(d0) || !finite_nonneg(weight_decay))
    return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks || !partials) return VP_ERR_ARG;
  const ProdigyMomentArgs a = prodigy_moment_args(beta1, beta2, beta3, weight_decay, d0, safeguard_warmup, use_clip);
  hipLaunchKernelGGL(mt_prodigy_moments_f32_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                     chunk_begin, acc, master, p0, exp_avg, exp_avg_sq, s, partials, scalars, dstate, a);
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_mt_prodigy_update_bf16(const vp_mt_tensor* tensors, const vp_mt_chunk* chunks, int32_t chunk_begin,
                                         int32_t n_chunks, float* master, const float* exp_avg,
                                         const float* exp_avg_sq, const vp_optim_scalars* scalars,
                                         const vp_prodigy_scalars* dstate, double eps, double weight_decay,
                                         int32_t zero_grads, void* stream) {
  if (n_chunks < 0 || chunk_begin < 0 || !scalars || !dstate || !master || !exp_avg || !exp_avg_sq) return VP_ERR_ARG;
  if (!finite_nonneg(eps) || !finite_nonneg(weight_decay)) return VP_ERR_ARG;
  if (n_chunks == 0) return VP_OK;
  if (!tensors || !chunks) return VP_ERR_ARG;
  hipLaunchKernelGGL(mt_prodigy_update_kernel, dim3(n_chunks), dim3(OT), 0, (hipStream_t)stream, tensors, chunks,
                     chunk_begin, master, exp_avg, exp_avg_sq, scalars, dstate, eps, weight_decay, zero_grads);
  VP_CHECK_LAUNCH();
  return VP_OK;
}
