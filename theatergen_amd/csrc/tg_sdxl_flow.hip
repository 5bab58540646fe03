// The SDXL flow around the UNet, without its step: the T2I-Adapter's data-movement / pointwise pieces (pixel-unshuffle into token-major, ReLU,
// 2 x 2 ceil-mode average pool, scale-and-repeat of the conditioning features).  The sigma-parameterised (Euler / Euler ancestral) and DPM-Solver++
// step epilogues that used to live here are update policies of the one step-epilogue body in tg_step.hip.
// Everything here is HBM-bound and runs once per image; no hot GEMM / conv epilogue is touched.
#include "tg_common.h"

namespace {

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

extern "C" int tg_pixel_unshuffle(int32_t dtype, const void* in, int32_t batch, int32_t channels, int32_t h, int32_t w,
                                  int32_t factor, void* out, void* stream) {
  TG_CHECK((dtype == TG_BF16 || dtype == TG_F16) && in && out && in != out && batch > 0 && channels > 0 && factor > 0 &&
               h > 0 && w > 0 && h % factor == 0 && w % factor == 0, TG_ERR_ARG,
           "tg_pixel_unshuffle: bad args (h and w must be multiples of the factor)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(tg_blocks_1d((long)batch * channels * h * w));
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
  if (dtype == TG_BF16) hipLaunchKernelGGL(relu_kernel<bf16_t>, dim3(tg_blocks_1d(n)), dim3(256), 0, st, (const bf16_t*)x, (long)n, (bf16_t*)out);
  else hipLaunchKernelGGL(relu_kernel<f16_t>, dim3(tg_blocks_1d(n)), dim3(256), 0, st, (const f16_t*)x, (long)n, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_avgpool2x2(int32_t dtype, const void* x, int32_t batch, int32_t h, int32_t w, int32_t channels, void* out, void* stream) {
  TG_CHECK((dtype == TG_BF16 || dtype == TG_F16) && x && out && x != out && batch > 0 && h > 0 && w > 0 && channels > 0, TG_ERR_ARG,
           "tg_avgpool2x2: bad args");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(tg_blocks_1d((long)batch * ((h + 1) / 2) * ((w + 1) / 2) * channels));
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
    hipLaunchKernelGGL(scale_repeat_kernel<bf16_t>, dim3(tg_blocks_1d(n)), dim3(256), 0, st, (const bf16_t*)x, (long)n, scale, copies, (bf16_t*)out);
  else
    hipLaunchKernelGGL(scale_repeat_kernel<f16_t>, dim3(tg_blocks_1d(n)), dim3(256), 0, st, (const f16_t*)x, (long)n, scale, copies, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
