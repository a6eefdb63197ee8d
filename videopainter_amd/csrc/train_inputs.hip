// The front of the training iteration for gfx950 (MI355X): train/train_cogvideox_inpainting_i2v_video.py:1774-1853,
// everything between the three VAE encodes and the models.  The ABI and the rounding chains are include/vp_hip.h
// (ABI 31): a Philox4x32-10 normal generator (one device function under the fill entry, the frame noise and the
// fused kernel, so a given noise tensor and a generated one agree bit for bit), vp_noise_frame and
// vp_train_inputs_bf16.  All three are bandwidth- and launch-bound: vector loads and stores, plain stores only, no
// host read of the device.
#include "vp_common.h"

namespace {

// ---- Philox4x32-10 (Salmon et al., SC'11) ----
constexpr uint32_t PH_M0 = 0xD2511F53u, PH_M1 = 0xCD9E8D57u, PH_W0 = 0x9E3779B9u, PH_W1 = 0xBB67AE85u;

VP_DEV u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)PH_M0 * c[0], p1 = (uint64_t)PH_M1 * c[2];
    c = (u32x4){(uint32_t)(p1 >> 32) ^ c[1] ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c[3] ^ k1, (uint32_t)p0};
    k0 += PH_W0;
    k1 += PH_W1;
  }
  return c;
}

// one Box-Muller pair in fp32 from two output words: u1 in (0, 1], u2 in [0, 1), both exact in fp32
VP_DEV void box_muller(uint32_t xa, uint32_t xb, float& z_even, float& z_odd) {
#pragma clang fp contract(off)
  const float u1 = (float)((xa >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(xb >> 8) * 5.9604644775390625e-8f;
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
  sincospif(2.f * u2, &s, &c);
  z_even = r * c;
  z_odd = r * s;
}

// the four fp32 normal numbers of block blk (elements 4 blk .. 4 blk + 3) of (seed, stream)
VP_DEV f32x4 philox_normal4(uint64_t seed, uint64_t stream, uint64_t blk) {
  const u32x4 ctr = {(uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
  const u32x4 x = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
  f32x4 z;
  float a, b;
  box_muller(x[0], x[1], a, b);
  z[0] = a;
  z[1] = b;
  box_muller(x[2], x[3], a, b);
  z[2] = a;
  z[3] = b;
  return z;
}

VP_DEV float pick4(const f32x4& z, int lane) {
  return lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
}

// z[j] = fp32 normal number e0 + j, j < 8 (any e0: the 8 elements span two or three blocks)
VP_DEV void philox_normal8(uint64_t seed, uint64_t stream, uint64_t e0, float (&z)[8]) {
  if ((e0 & 3) == 0) {
    const f32x4 a = philox_normal4(seed, stream, e0 >> 2), b = philox_normal4(seed, stream, (e0 >> 2) + 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      z[j] = a[j];
      z[4 + j] = b[j];
    }
    return;
  }
  uint64_t cur = e0 >> 2;
  f32x4 v = philox_normal4(seed, stream, cur);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint64_t e = e0 + (uint64_t)j;
    if ((e >> 2) != cur) {
      cur = e >> 2;
      v = philox_normal4(seed, stream, cur);
    }
    z[j] = pick4(v, (int)(e & 3));
  }
}

// one thread per block of four: the blocks that cover [offset, offset + n).  A whole block is one vector store when
// `vec` (the host checked the address of the first whole block); the partial first / last blocks are scalar stores.
template <typename T>
__global__ __launch_bounds__(256) void philox_fill_kernel(T* __restrict__ out, int64_t n, uint64_t seed,
                                                          uint64_t stream, uint64_t offset, int64_t nblk, int vec) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nblk; k += (int64_t)gridDim.x * 256) {
    const uint64_t blk = (offset >> 2) + (uint64_t)k;
    const f32x4 z = philox_normal4(seed, stream, blk);
    // index of the block's lane 0 in out (negative inside the head block); offset & 3 < 4 so no overflow
    const int64_t i0 = 4 * k - (int64_t)(offset & 3);
    if (vec && i0 >= 0 && i0 + 4 <= n) {
      if constexpr (sizeof(T) == 4) {
        *(f32x4*)(out + i0) = z;
      } else {
        *(bf16x4*)(out + i0) = (bf16x4){f2bf(z[0]), f2bf(z[1]), f2bf(z[2]), f2bf(z[3])};
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j;
        if (i >= 0 && i < n) out[i] = (T)z[j];
      }
    }
  }
}

// ---- first-frame noise in pixel space ----
// 8 elements of one batch row per thread; a vector load / store when the chunk is whole and `vec`
template <typename T>
__global__ __launch_bounds__(256) void noise_frame_kernel(const T* __restrict__ x, const bf16* __restrict__ sigma,
                                                          const T* __restrict__ noise, bf16* __restrict__ out, int B,
                                                          int64_t n_per, int64_t chunks, uint64_t seed,
                                                          uint64_t stream, int vec) {
#pragma clang fp contract(off)
  const int64_t total = (int64_t)B * chunks;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
    const int b = (int)(it / chunks);
    const int64_t i0 = (it % chunks) * 8;
    const int64_t base = (int64_t)b * n_per + i0;
    const int cnt = (int)(n_per - i0 < 8 ? n_per - i0 : 8);
    const float sg = bf2f(sigma[b]);
    const bool whole = vec && cnt == 8;
    float xv[8], nv[8];
    if (whole) {
      if constexpr (sizeof(T) == 4) {
        const f32x4 a = *(const f32x4*)(x + base), c = *(const f32x4*)(x + base + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xv[j] = a[j];
          xv[4 + j] = c[j];
        }
      } else {
        const bf16x8 a = *(const bf16x8*)(x + base);
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = bf2f(a[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) xv[j] = j < cnt ? (float)x[base + j] : 0.f;
    }
    if (noise != nullptr) {
      if (whole) {
        if constexpr (sizeof(T) == 4) {
          const f32x4 a = *(const f32x4*)(noise + base), c = *(const f32x4*)(noise + base + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            nv[j] = a[j];
            nv[4 + j] = c[j];
          }
        } else {
          const bf16x8 a = *(const bf16x8*)(noise + base);
#pragma unroll
          for (int j = 0; j < 8; ++j) nv[j] = bf2f(a[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) nv[j] = j < cnt ? (float)noise[base + j] : 0.f;
      }
    } else {
      philox_normal8(seed, stream, (uint64_t)base, nv);
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) nv[j] = rbf_prod(nv[j]);  // drawn in bf16
      }
    }
    bf16 y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (sizeof(T) == 4) {
        const float p = nv[j] * sg;  // fp32 product, fp32 sum, then the one bf16 rounding
        y[j] = f2bf(xv[j] + p);
      } else {
        y[j] = f2bf(xv[j] + rbf_prod(nv[j] * sg));
      }
    }
    if (whole) {
      *(bf16x8*)(out + base) = (bf16x8){y[0], y[1], y[2], y[3], y[4], y[5], y[6], y[7]};
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) out[base + j] = y[j];
    }
  }
}

// ---- the fused front ----
constexpr int TI_L = 16;     // latent channels (vp_train_inputs_bf16 takes no other)
constexpr int TI_ROLES = 7;  // video channels 0-7 / 8-15, conditioning 0-7 / 8-15, image 0-7 / 8-15, mask

// 8 bf16 at p (vector when VEC, else the first cnt element-wise; the rest zero)
template <bool VEC>
VP_DEV void load8(const bf16* __restrict__ p, int cnt, float (&v)[8]) {
  if constexpr (VEC) {
    const bf16x8 a = *(const bf16x8*)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(a[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < cnt ? bf2f(p[j]) : 0.f;
  }
}

template <bool VEC>
VP_DEV void store8(bf16* __restrict__ p, int cnt, const float (&v)[8]) {
  if constexpr (VEC) {
    *(bf16x8*)p =
        (bf16x8){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3]), f2bf(v[4]), f2bf(v[5]), f2bf(v[6]), f2bf(v[7])};
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < cnt) p[j] = f2bf(v[j]);
  }
}

// noise elements [e0, e0 + 8) of a bf16 tensor, or of (seed, stream) rounded to bf16 when the tensor is NULL
template <bool VEC>
VP_DEV void noise8(const bf16* __restrict__ noise, uint64_t seed, uint64_t stream, int64_t e0, int cnt,
                   float (&v)[8]) {
  if (noise != nullptr) {
    load8<VEC>(noise + e0, cnt, v);
  } else {
    philox_normal8(seed, stream, (uint64_t)e0, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rbf_prod(v[j]);
  }
}

// the reference's DiagonalGaussianDistribution.sample() * scaling_factor in bf16 (rounding chain: include/vp_hip.h)
VP_DEV float sample_scaled(float mean, float logvar, float n, float sf) {
#pragma clang fp contract(off)
  const float lv = fminf(fmaxf(logvar, -30.f), 20.f);
  const float sd = rbf_prod(expf(rbf_prod(0.5f * lv)));
  const float x = rbf_prod(mean + rbf_prod(sd * n));
  return rbf_prod(x * sf);
}

VP_DEV int nearest_src(int dst, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out;
  const int s = (int)floorf((float)dst * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

// the 8 means and 8 logvars (channels c0 .. c0 + 7) of pixels p0 .. p0 + cnt - 1 of frame (b, t) of a posterior with Tn
// frames: one 16-byte load each per pixel when ROWVEC (ldp a multiple of 8, 16-byte aligned base: the host checked)
template <bool ROWVEC>
VP_DEV void load_rows(const bf16* __restrict__ prm, int ldp, int Tn, int b, int t, int c0, int p0, int cnt, int hw,
                      bf16x8 (&mu)[8], bf16x8 (&lv)[8]) {
  const bf16* rows = prm + (((int64_t)b * Tn + t) * hw + p0) * ldp + c0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bf16* r = rows + (int64_t)(j < cnt ? j : 0) * ldp;  // (a pixel past the row's end repeats pixel 0: unused)
    if constexpr (ROWVEC) {
      mu[j] = *(const bf16x8*)r;
      lv[j] = *(const bf16x8*)(r + TI_L);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        mu[j][c] = r[c];
        lv[j][c] = r[TI_L + c];
      }
    }
  }
}

// z[j] = the scaled sample of channel c0 + c at pixels p0 + j, with the posterior noise [B, L, Tn, h, w]
template <bool VEC, int c>
VP_DEV void sample_channel(const vp_train_inputs_desc& d, const bf16* __restrict__ noise, uint64_t stream, int Tn,
                           int b, int t, int c0, int p0, int cnt, int hw, const bf16x8 (&mu)[8],
                           const bf16x8 (&lv)[8], float (&z)[8]) {
  float nz[8];
  noise8<VEC>(noise, d.seed, stream, (((int64_t)b * TI_L + c0 + c) * Tn + t) * hw + p0, cnt, nz);
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = sample_scaled(bf2f(mu[j][c]), bf2f(lv[j][c]), nz[j], d.scaling_factor);
}

template <int c>
struct ChannelTag {
  static constexpr int value = c;
};

// f(ChannelTag<0>) ... f(ChannelTag<7>): the channel index as a constant, so the vector element picks stay static
template <typename F>
VP_DEV void for_channels(F&& f) {
  f(ChannelTag<0>{});
  f(ChannelTag<1>{});
  f(ChannelTag<2>{});
  f(ChannelTag<3>{});
  f(ChannelTag<4>{});
  f(ChannelTag<5>{});
  f(ChannelTag<6>{});
  f(ChannelTag<7>{});
}

template <bool VEC, bool ROWVEC>
__global__ __launch_bounds__(256) void train_inputs_kernel(const vp_train_inputs_desc d, int chunks, int64_t per_role) {
#pragma clang fp contract(off)
  const int hw = d.h * d.w, L = TI_L;
  const int64_t total = per_role * TI_ROLES;
  bf16* const target = (bf16*)d.target;
  bf16* const noisy = (bf16*)d.noisy;
  bf16* const nmi = (bf16*)d.noisy_model_input;
  bf16* const cond = (bf16*)d.conditioning_latents;
  bf16* const mlat = (bf16*)d.masks_latent;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
    const int role = (int)(it / per_role);  // role-major: a wave has one role except at the six seams
    int64_t r = it % per_role;
    const int p0 = (int)(r % chunks) * 8;
    r /= chunks;
    const int t = (int)(r % d.T), b = (int)(r / d.T);
    const int cnt = hw - p0 < 8 ? hw - p0 : 8;
    const int64_t bt = (int64_t)b * d.T + t;
    const int c0 = (role & 1) * 8;
    bf16x8 mu[8], lv[8];
    if (role < 2) {  // video sample -> target, noisy latents (twice)
      load_rows<ROWVEC>((const bf16*)d.p_video, d.ldp, d.T, b, t, c0, p0, cnt, hw, mu, lv);
      int64_t ts = d.timesteps[b];
      ts = ts < 0 ? 0 : (ts >= d.n_alphas ? d.n_alphas - 1 : ts);
      const float sa = d.sa_sb[2 * ts], sb = d.sa_sb[2 * ts + 1];
      for_channels([&](auto tag) {
        constexpr int c = decltype(tag)::value;
        float z[8], eps[8], ny[8];
        sample_channel<VEC, c>(d, (const bf16*)d.noise_video, d.stream_video, d.T, b, t, c0, p0, cnt, hw, mu, lv, z);
        const int64_t e = (bt * L + c0 + c) * hw + p0;  // [B, T, L, h, w]
        noise8<VEC>((const bf16*)d.noise_diff, d.seed, d.stream_diff, e, cnt, eps);
#pragma unroll
        for (int j = 0; j < 8; ++j) ny[j] = rbf_prod(sa * z[j]) + rbf_prod(sb * eps[j]);
        store8<VEC>(target + e, cnt, z);
        store8<VEC>(noisy + e, cnt, ny);
        store8<VEC>(nmi + (bt * 2 * L + c0 + c) * hw + p0, cnt, ny);
      });
    } else if (role < 4) {  // conditioning sample
      load_rows<ROWVEC>((const bf16*)d.p_cond, d.ldp, d.T, b, t, c0, p0, cnt, hw, mu, lv);
      for_channels([&](auto tag) {
        constexpr int c = decltype(tag)::value;
        float z[8];
        sample_channel<VEC, c>(d, (const bf16*)d.noise_cond, d.stream_cond, d.T, b, t, c0, p0, cnt, hw, mu, lv, z);
        store8<VEC>(cond + (bt * (L + 1) + c0 + c) * hw + p0, cnt, z);
      });
    } else if (role < 6) {  // image channels of the model input: the sample in frame 0, else zeros
      const bool live = t == 0 && !d.image_dropout;
      if (live) load_rows<ROWVEC>((const bf16*)d.p_image, d.ldp, 1, b, 0, c0, p0, cnt, hw, mu, lv);
      for_channels([&](auto tag) {
        constexpr int c = decltype(tag)::value;
        float z[8];
        if (live) {
          sample_channel<VEC, c>(d, (const bf16*)d.noise_image, d.stream_image, 1, b, 0, c0, p0, cnt, hw, mu, lv, z);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) z[j] = 0.f;
        }
        store8<VEC>(nmi + (bt * 2 * L + L + c0 + c) * hw + p0, cnt, z);
      });
    } else {  // the mask on the latent grid: its own tensor and the last conditioning channel
      const int ft = nearest_src(t, d.Fp, d.T);
      float m[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        m[j] = 0.f;
        if (j < cnt) {
          const int p = p0 + j;
          const int fy = nearest_src(p / d.w, d.Hp, d.h), fx = nearest_src(p % d.w, d.Wp, d.w);
          const int64_t src = (((int64_t)b * d.Fp + ft) * d.Hp + fy) * d.Wp + fx;
          m[j] = d.mask_dtype == 0 ? ((const float*)d.mask)[src]
                                   : (d.mask_dtype == 1 ? bf2f(((const bf16*)d.mask)[src])
                                                        : (float)((const uint8_t*)d.mask)[src]);
        }
      }
      store8<VEC>(mlat + bt * hw + p0, cnt, m);
      store8<VEC>(cond + (bt * (L + 1) + L) * hw + p0, cnt, m);
    }
  }
}

inline unsigned ti_grid(int64_t work) {
  const int64_t g = (work + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));  // memory-bound: cap the grid, stride the rest
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int vp_philox_normal(void* out, int32_t out_is_f32, int64_t n, uint64_t seed, uint64_t stream,
                                uint64_t offset, void* hip_stream) {
  if (out == nullptr || n <= 0 || offset + (uint64_t)n < offset) return VP_ERR_ARG;
  const int64_t esz = out_is_f32 ? 4 : 2;
  const int64_t head = (int64_t)((4 - (offset & 3)) & 3);  // elements before the first whole block
  const int vec = (((uintptr_t)out + (uintptr_t)(head * esz)) % (uintptr_t)(4 * esz)) == 0;
  const int64_t nblk = (int64_t)(((offset + (uint64_t)n - 1) >> 2) - (offset >> 2)) + 1;
  if (out_is_f32) {
    hipLaunchKernelGGL(philox_fill_kernel<float>, dim3(ti_grid(nblk)), dim3(256), 0, (hipStream_t)hip_stream,
                       (float*)out, n, seed, stream, offset, nblk, vec);
  } else {
    hipLaunchKernelGGL(philox_fill_kernel<bf16>, dim3(ti_grid(nblk)), dim3(256), 0, (hipStream_t)hip_stream,
                       (bf16*)out, n, seed, stream, offset, nblk, vec);
  }
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_noise_frame(const void* x, int32_t x_is_f32, const void* sigma, const void* noise, void* out,
                              int32_t B, int64_t n_per, uint64_t seed, uint64_t stream, void* hip_stream) {
  if (x == nullptr || sigma == nullptr || out == nullptr || B <= 0 || n_per <= 0) return VP_ERR_ARG;
  const int64_t chunks = (n_per + 7) / 8;
  // whole chunks start at b n_per + 8 k: 16-byte (bf16) / 32-byte (fp32: two 16-byte halves) steps from the bases
  const int vec = (n_per % 8) == 0 && al16(x) && al16(out) && (noise == nullptr || al16(noise));
  if (x_is_f32) {
    hipLaunchKernelGGL(noise_frame_kernel<float>, dim3(ti_grid(B * chunks)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const float*)x, (const bf16*)sigma, (const float*)noise, (bf16*)out, B, n_per, chunks, seed,
                       stream, vec);
  } else {
    hipLaunchKernelGGL(noise_frame_kernel<bf16>, dim3(ti_grid(B * chunks)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const bf16*)x, (const bf16*)sigma, (const bf16*)noise, (bf16*)out, B, n_per, chunks, seed,
                       stream, vec);
  }
  VP_CHECK_LAUNCH();
  return VP_OK;
}

extern "C" int vp_train_inputs_bf16(const vp_train_inputs_desc* d, void* stream) {
  if (d == nullptr || d->struct_bytes != (int32_t)sizeof(vp_train_inputs_desc)) return VP_ERR_ARG;
  if (d->L != TI_L || d->ldp < 2 * d->L || (d->ldp & 1) || d->image_T != 1) return VP_ERR_ARG;
  if (d->B <= 0 || d->T <= 0 || d->h <= 0 || d->w <= 0 || d->Fp <= 0 || d->Hp <= 0 || d->Wp <= 0 || d->n_alphas <= 0)
    return VP_ERR_ARG;
  if (d->mask_dtype < 0 || d->mask_dtype > 2) return VP_ERR_ARG;
  if (!d->p_video || !d->p_cond || !d->p_image || !d->timesteps || !d->sa_sb || !d->mask || !d->target || !d->noisy ||
      !d->noisy_model_input || !d->masks_latent || !d->conditioning_latents)
    return VP_ERR_ARG;
  if ((int64_t)d->h * d->w > (int64_t)1 << 30) return VP_ERR_ARG;
  const int hw = d->h * d->w;
  const int chunks = (hw + 7) / 8;
  const int64_t per_role = (int64_t)d->B * d->T * chunks;
  const bool vec = (hw % 8) == 0 && al16(d->target) && al16(d->noisy) && al16(d->noisy_model_input) &&
                   al16(d->masks_latent) && al16(d->conditioning_latents) &&
                   (!d->noise_video || al16(d->noise_video)) && (!d->noise_cond || al16(d->noise_cond)) &&
                   (!d->noise_image || al16(d->noise_image)) && (!d->noise_diff || al16(d->noise_diff));
  const bool rowvec = (d->ldp % 8) == 0 && al16(d->p_video) && al16(d->p_cond) && al16(d->p_image);
  const dim3 grid(ti_grid(per_role * TI_ROLES)), block(256);
  if (vec && rowvec)
    hipLaunchKernelGGL((train_inputs_kernel<true, true>), grid, block, 0, (hipStream_t)stream, *d, chunks, per_role);
  else if (vec)
    hipLaunchKernelGGL((train_inputs_kernel<true, false>), grid, block, 0, (hipStream_t)stream, *d, chunks, per_role);
  else if (rowvec)
    hipLaunchKernelGGL((train_inputs_kernel<false, true>), grid, block, 0, (hipStream_t)stream, *d, chunks, per_role);
  else
    hipLaunchKernelGGL((train_inputs_kernel<false, false>), grid, block, 0, (hipStream_t)stream, *d, chunks, per_role);
  VP_CHECK_LAUNCH();
  return VP_OK;
}
