// The SDXL flow around the UNet: the sigma-parameterised step epilogue (CFG + Euler / Euler-ancestral update + frozen-mask
// blend + history row + next scaled model input, one launch per step), its DPM-Solver++ multistep sibling (tg_step_epilogue_dpm:
// one extra fp32 state tensor, the previous data prediction) and the T2I-Adapter's data-movement / pointwise pieces
// (pixel-unshuffle into token-major, ReLU, 2 x 2 ceil-mode average pool, scale-and-repeat of the conditioning features).
// Everything here is HBM-bound and runs once per step or once per image; no hot GEMM / conv epilogue is touched.
#include "tg_common.h"

namespace {

inline int blocks_for(long n) {
  long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

struct SigmaStepParams {
  const float* noise_pred;
  float* latents;
  int n_img, chw, hw;
  int has_cfg;
  float g;
  const float* coef;          // [n_steps][4]: eps weight, sigma_up, scale of the next model input, sigma_i
  int* step_idx;
  const void* noise;          // [n_steps][n_img * chw] storage dtype, or null (sigma_up ignored)
  int noise_dtype;
  const float* frozen;
  const float* frozen_mask;
  int mask_per_img;
  int frozen_steps;
  float* history;
  void* model_in;
  int model_in_dtype;
};

__device__ __forceinline__ float load_any(const void* p, int dt, long i) {
  if (dt == TG_BF16) return (float)reinterpret_cast<const bf16_t*>(p)[i];
  if (dt == TG_F16) return (float)reinterpret_cast<const f16_t*>(p)[i];
  return reinterpret_cast<const float*>(p)[i];
}

__global__ __launch_bounds__(256) void step_epilogue_sigma_kernel(SigmaStepParams p) {
  const int step = *p.step_idx;
  const float ce = p.coef[step * 4], su = p.coef[step * 4 + 1], cnext = p.coef[step * 4 + 2];
  const long total = (long)p.n_img * p.chw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const float u = p.noise_pred[i];
    float eps = u;
    if (p.has_cfg) { const float c = p.noise_pred[total + i]; eps = u + p.g * (c - u); }
    float nx = p.latents[i] + eps * ce;
    if (p.noise) nx += su * load_any(p.noise, p.noise_dtype, (long)step * total + i);
    if (p.frozen && step < p.frozen_steps) {
      const long img = i / p.chw;
      const long pix = (i - img * p.chw) % p.hw;
      const float m = p.frozen_mask[(p.mask_per_img ? img * p.hw : 0) + pix];
      const float f = p.frozen[(long)(step + 1) * total + i];
      nx = f * m + nx * (1.f - m);
    }
    p.latents[i] = nx;
    if (p.history) p.history[(long)(step + 1) * total + i] = nx;
    if (p.model_in) {
      // next UNet input = scale_model_input(cat([latents] * 2), t_next) = x / sqrt(sigma_next^2 + 1), in the model dtype; PyTorch divides a
      // tensor by a scalar as a multiply by the fp32 reciprocal, which the table holds
      const float s = nx * cnext;
      if (p.model_in_dtype == TG_BF16) {
        reinterpret_cast<bf16_t*>(p.model_in)[i] = (bf16_t)s;
        reinterpret_cast<bf16_t*>(p.model_in)[total + i] = (bf16_t)s;
      } else if (p.model_in_dtype == TG_F16) {
        reinterpret_cast<f16_t*>(p.model_in)[i] = (f16_t)s;
        reinterpret_cast<f16_t*>(p.model_in)[total + i] = (f16_t)s;
      } else {
        reinterpret_cast<float*>(p.model_in)[i] = s;
        reinterpret_cast<float*>(p.model_in)[total + i] = s;
      }
    }
  }
}

__global__ void sigma_step_advance_kernel(int* step_idx) { *step_idx += 1; }

struct DpmStepParams {
  const float* noise_pred;
  float* latents;
  float* x0_prev;             // [n_img * chw] fp32: the previous step's data prediction, replaced by this step's
  int n_img, chw, hw;
  int has_cfg;
  float g;
  const float* coef;          // [n_steps][8]: cx, ce, A, B, C, 0, 0, 0
  int* step_idx;
  const float* frozen;
  const float* frozen_mask;
  int mask_per_img;
  int frozen_steps;
  float* history;
  void* model_in;
  int model_in_dtype;
};

// DPM-Solver++ multistep (data prediction, midpoint 2M): x0 = cx x + ce m, x' = A x + B x0 + C x0_prev with the row of this
// step.  C == 0 marks a first-order row: the state is then NOT read (0 * NaN of a never-written buffer would be NaN); the row is
// the same for every thread, so the branch is wave-uniform.  Each element of x0_prev is read and rewritten by one thread only.
__global__ __launch_bounds__(256) void step_epilogue_dpm_kernel(DpmStepParams p) {
  const int step = *p.step_idx;
  const float* row = p.coef + (long)step * 8;
  const float cx = row[0], ce = row[1], ca = row[2], cb = row[3], cc = row[4];
  const bool second = cc != 0.f;
  const long total = (long)p.n_img * p.chw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const float u = p.noise_pred[i];
    float m = u;
    if (p.has_cfg) { const float c = p.noise_pred[total + i]; m = u + p.g * (c - u); }
    const float x = p.latents[i];
    const float x0 = cx * x + ce * m;
    float nx = ca * x + cb * x0;
    if (second) nx += cc * p.x0_prev[i];
    p.x0_prev[i] = x0;                     // the model's prediction, not the blended latents (host loop: scheduler.step, then the blend)
    if (p.frozen && step < p.frozen_steps) {
      const long img = i / p.chw;
      const long pix = (i - img * p.chw) % p.hw;
      const float mk = p.frozen_mask[(p.mask_per_img ? img * p.hw : 0) + pix];
      const float f = p.frozen[(long)(step + 1) * total + i];
      nx = f * mk + nx * (1.f - mk);
    }
    p.latents[i] = nx;
    if (p.history) p.history[(long)(step + 1) * total + i] = nx;
    if (p.model_in) {
      // next UNet input = cat([latents] * 2) in the model dtype (scale_model_input is the identity: init_noise_sigma = 1)
      if (p.model_in_dtype == TG_BF16) {
        reinterpret_cast<bf16_t*>(p.model_in)[i] = (bf16_t)nx;
        reinterpret_cast<bf16_t*>(p.model_in)[total + i] = (bf16_t)nx;
      } else if (p.model_in_dtype == TG_F16) {
        reinterpret_cast<f16_t*>(p.model_in)[i] = (f16_t)nx;
        reinterpret_cast<f16_t*>(p.model_in)[total + i] = (f16_t)nx;
      } else {
        reinterpret_cast<float*>(p.model_in)[i] = nx;
        reinterpret_cast<float*>(p.model_in)[total + i] = nx;
      }
    }
  }
}

// out[((b * oh + y) * ow + x) * (C r^2) + c r^2 + i r + j] = in[b, c, r y + i, r x + j]   (F.pixel_unshuffle, token-major)
template <typename T>
__global__ __launch_bounds__(256) void pixel_unshuffle_kernel(const T* in, int batch, int ch, int h, int w, int r, T* out) {
  const int oh = h / r, ow = w / r, cr = ch * r * r;
  const long total = (long)batch * oh * ow * cr;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
    const int k = (int)(o % cr);
    const long pix = o / cr;
    const int x = (int)(pix % ow);
    const long by = pix / ow;
    const int y = (int)(by % oh);
    const long b = by / oh;
    const int c = k / (r * r), ij = k - c * r * r, i = ij / r, j = ij - i * r;
    out[o] = in[((b * ch + c) * h + (long)(r * y + i)) * w + (r * x + j)];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void relu_kernel(const T* x, long n, T* out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float f = to_f32<T>(x[i]);
    out[i] = from_f32<T>(f > 0.f ? f : 0.f);
  }
}

// AvgPool2d(2, 2, ceil_mode=True) on token-major [batch * h * w, C]: a window cut by the bottom / right edge averages the
// pixels it covers (padding 0: PyTorch's divisor is the in-bounds window size)
template <typename T>
__global__ __launch_bounds__(256) void avgpool2x2_kernel(const T* x, int batch, int h, int w, int ch, T* out) {
  const int oh = (h + 1) / 2, ow = (w + 1) / 2;
  const long total = (long)batch * oh * ow * ch;
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
    const int c = (int)(o % ch);
    const long pix = o / ch;
    const int ox = (int)(pix % ow);
    const long by = pix / ow;
    const int oy = (int)(by % oh);
    const long b = by / oh;
    const int y0 = 2 * oy, x0 = 2 * ox, y1 = min(y0 + 2, h), x1 = min(x0 + 2, w);
    float s = 0.f;
    for (int y = y0; y < y1; ++y)
      for (int xx = x0; xx < x1; ++xx) s += to_f32<T>(x[((b * h + y) * w + xx) * ch + c]);
    out[o] = from_f32<T>(s / (float)((y1 - y0) * (x1 - x0)));
  }
}

// out[r * n + i] = x[i] * scale for r < copies (the adapter's `state * conditioning_scale` then `cat([state] * 2)`)
template <typename T>
__global__ __launch_bounds__(256) void scale_repeat_kernel(const T* x, long n, float scale, int copies, T* out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const T v = from_f32<T>(to_f32<T>(x[i]) * scale);
    for (int r = 0; r < copies; ++r) out[(long)r * n + i] = v;
  }
}

}  // namespace

extern "C" int tg_step_epilogue_sigma(const float* noise_pred, float* latents, int32_t n_img, int32_t chw, int32_t hw,
                                      int32_t has_cfg, float guidance_scale, const float* coef, int32_t* step_idx, int32_t advance,
                                      const void* noise, int32_t noise_dtype, const float* frozen, const float* frozen_mask,
                                      int32_t mask_per_img, int32_t frozen_steps, float* history, void* model_in,
                                      int32_t model_in_dtype, void* stream) {
  TG_CHECK(noise_pred && latents && coef && step_idx && n_img > 0 && chw > 0 && hw > 0 && chw % hw == 0, TG_ERR_ARG,
           "tg_step_epilogue_sigma: bad args");
  TG_CHECK(!noise || noise_dtype == TG_BF16 || noise_dtype == TG_F16 || noise_dtype == 2, TG_ERR_ARG,
           "tg_step_epilogue_sigma: noise dtype must be TG_BF16, TG_F16 or 2 (fp32)");
  TG_CHECK(!model_in || model_in_dtype == TG_BF16 || model_in_dtype == TG_F16 || model_in_dtype == 2, TG_ERR_ARG,
           "tg_step_epilogue_sigma: model_in dtype must be TG_BF16, TG_F16 or 2 (fp32)");
  TG_CHECK(!frozen || frozen_mask, TG_ERR_ARG, "tg_step_epilogue_sigma: frozen latents need a mask");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SigmaStepParams p{noise_pred, latents, n_img, chw, hw, has_cfg, guidance_scale, coef, step_idx, noise, noise_dtype, frozen,
                    frozen_mask, mask_per_img, frozen_steps, history, model_in, model_in_dtype};
  hipLaunchKernelGGL(step_epilogue_sigma_kernel, dim3(blocks_for((long)n_img * chw)), dim3(256), 0, st, p);
  TG_LAUNCH_CHECK();
  if (advance) {
    hipLaunchKernelGGL(sigma_step_advance_kernel, dim3(1), dim3(1), 0, st, step_idx);
    TG_LAUNCH_CHECK();
  }
  return TG_OK;
}

extern "C" int tg_step_epilogue_dpm(const float* noise_pred, float* latents, float* x0_prev, int32_t n_img, int32_t chw, int32_t hw,
                                    int32_t has_cfg, float guidance_scale, const float* coef, int32_t* step_idx, int32_t advance,
                                    const float* frozen, const float* frozen_mask, int32_t mask_per_img, int32_t frozen_steps,
                                    float* history, void* model_in, int32_t model_in_dtype, void* stream) {
  TG_CHECK(noise_pred && latents && x0_prev && coef && step_idx && n_img > 0 && chw > 0 && hw > 0 && chw % hw == 0, TG_ERR_ARG,
           "tg_step_epilogue_dpm: bad args");
  TG_CHECK(x0_prev != latents && (const float*)x0_prev != noise_pred, TG_ERR_ARG,
           "tg_step_epilogue_dpm: x0_prev must be a buffer of its own");
  TG_CHECK(!model_in || model_in_dtype == TG_BF16 || model_in_dtype == TG_F16 || model_in_dtype == 2, TG_ERR_ARG,
           "tg_step_epilogue_dpm: model_in dtype must be TG_BF16, TG_F16 or 2 (fp32)");
  TG_CHECK(!frozen || frozen_mask, TG_ERR_ARG, "tg_step_epilogue_dpm: frozen latents need a mask");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  DpmStepParams p{noise_pred, latents, x0_prev, n_img, chw, hw, has_cfg, guidance_scale, coef, step_idx, frozen,
                  frozen_mask, mask_per_img, frozen_steps, history, model_in, model_in_dtype};
  hipLaunchKernelGGL(step_epilogue_dpm_kernel, dim3(blocks_for((long)n_img * chw)), dim3(256), 0, st, p);
  TG_LAUNCH_CHECK();
  if (advance) {
    // a launch of its own, ordered after the epilogue on the stream: no thread of the epilogue can read a moved counter
    hipLaunchKernelGGL(sigma_step_advance_kernel, dim3(1), dim3(1), 0, st, step_idx);
    TG_LAUNCH_CHECK();
  }
  return TG_OK;
}

extern "C" int tg_pixel_unshuffle(int32_t dtype, const void* in, int32_t batch, int32_t channels, int32_t h, int32_t w,
                                  int32_t factor, void* out, void* stream) {
  TG_CHECK((dtype == TG_BF16 || dtype == TG_F16) && in && out && in != out && batch > 0 && channels > 0 && factor > 0 &&
               h > 0 && w > 0 && h % factor == 0 && w % factor == 0, TG_ERR_ARG,
           "tg_pixel_unshuffle: bad args (h and w must be multiples of the factor)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(blocks_for((long)batch * channels * h * w));
  if (dtype == TG_BF16)
    hipLaunchKernelGGL(pixel_unshuffle_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)in, batch, channels, h, w, factor, (bf16_t*)out);
  else
    hipLaunchKernelGGL(pixel_unshuffle_kernel<f16_t>, grid, dim3(256), 0, st, (const f16_t*)in, batch, channels, h, w, factor, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_relu(int32_t dtype, const void* x, int64_t n, void* out, void* stream) {
  TG_CHECK((dtype == TG_BF16 || dtype == TG_F16) && x && out && n > 0, TG_ERR_ARG, "tg_relu: bad args");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16) hipLaunchKernelGGL(relu_kernel<bf16_t>, dim3(blocks_for(n)), dim3(256), 0, st, (const bf16_t*)x, (long)n, (bf16_t*)out);
  else hipLaunchKernelGGL(relu_kernel<f16_t>, dim3(blocks_for(n)), dim3(256), 0, st, (const f16_t*)x, (long)n, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_avgpool2x2(int32_t dtype, const void* x, int32_t batch, int32_t h, int32_t w, int32_t channels, void* out, void* stream) {
  TG_CHECK((dtype == TG_BF16 || dtype == TG_F16) && x && out && x != out && batch > 0 && h > 0 && w > 0 && channels > 0, TG_ERR_ARG,
           "tg_avgpool2x2: bad args");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(blocks_for((long)batch * ((h + 1) / 2) * ((w + 1) / 2) * channels));
  if (dtype == TG_BF16)
    hipLaunchKernelGGL(avgpool2x2_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, batch, h, w, channels, (bf16_t*)out);
  else
    hipLaunchKernelGGL(avgpool2x2_kernel<f16_t>, grid, dim3(256), 0, st, (const f16_t*)x, batch, h, w, channels, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_scale_repeat(int32_t dtype, const void* x, int64_t n, float scale, int32_t copies, void* out, void* stream) {
  TG_CHECK((dtype == TG_BF16 || dtype == TG_F16) && x && out && x != out && n > 0 && copies > 0, TG_ERR_ARG, "tg_scale_repeat: bad args");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16)
    hipLaunchKernelGGL(scale_repeat_kernel<bf16_t>, dim3(blocks_for(n)), dim3(256), 0, st, (const bf16_t*)x, (long)n, scale, copies, (bf16_t*)out);
  else
    hipLaunchKernelGGL(scale_repeat_kernel<f16_t>, dim3(blocks_for(n)), dim3(256), 0, st, (const f16_t*)x, (long)n, scale, copies, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
