// The image boundary of the pipelines: uint8 RGB HWC on the host side of the device, NCHW floats on the model side.
//   tg_image_from_u8: [batch, h, w, 3] uint8 -> `copies` x [batch, 3, h, w] in bf16 / fp16 / fp32, u / 255 (control image) or 2 (u / 255) - 1 (VAE input)
//   tg_image_to_u8  : [batch, 3, h, w] bf16 / fp16 / fp32 -> [batch, h, w, 3] uint8, round(clamp(x / 2 + 0.5, 0, 1) * 255), ties to even
// Both are HBM-bound glue, once per image.  PX = 4: a thread owns four consecutive pixels of one image — 12 interleaved bytes as three dwords on the
// uint8 side, one 16-byte (fp32) or 8-byte (bf16 / fp16) unit per channel plane on the float side; the 3-byte interleave happens in registers.  That
// needs h * w % 4 == 0 (every image and plane base then keeps the alignment of its tensor) and aligned tensor bases; anything else — odd sizes, a
// sliced tensor — takes PX = 1, one pixel per thread with element-wide accesses.  No LDS, no scratch.
#include "tg_common.h"

namespace {

template <typename T> __device__ __forceinline__ T image_round(float v) { return from_f32<T>(v); }
template <> __device__ __forceinline__ float image_round<float>(float v) { return v; }
template <typename T> __device__ __forceinline__ float image_widen(T v) { return to_f32<T>(v); }
template <> __device__ __forceinline__ float image_widen<float>(float v) { return v; }

// float(u) / 255.0f is an IEEE division (correctly rounded: the compiler's default for HIP); u * (1.0f / 255.0f) differs from it for 126 byte values.
// 2 v is exact, so 2 v - 1 rounds once whether or not the compiler contracts it into an fma.
__device__ __forceinline__ float image_value(unsigned u, int range_mode) {
  const float v = (float)u / 255.0f;
  return range_mode ? 2.0f * v - 1.0f : v;
}

// x / 2 is exact (or below the rounding of + 0.5), so x * 0.5 + 0.5 rounds once, contracted or not; the product with 255 is rounded to fp32 BEFORE rintf
// (a separate operation: nothing to contract with); fmaxf / fminf drop a NaN, which lands on 0.
__device__ __forceinline__ unsigned image_byte(float x) {
  const float y = fminf(fmaxf(x * 0.5f + 0.5f, 0.0f), 1.0f);
  return (unsigned)(int)rintf(y * 255.0f);
}

template <typename T, int PX>
__global__ __launch_bounds__(256) void image_from_u8_kernel(const uint8_t* __restrict__ src, int batch, long hw, int range_mode, int copies,
                                                            T* __restrict__ dst) {
  const long per_img = hw / PX;
  for (long b = blockIdx.y; b < batch; b += gridDim.y)
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < per_img; t += (long)gridDim.x * blockDim.x) {
    const long p = t * PX;
    const uint8_t* s = src + (b * hw + p) * 3;
    T vals[3][PX];
    if constexpr (PX == 4) {
      unsigned w[3];
      __builtin_memcpy(w, __builtin_assume_aligned(s, 4), 12);
#pragma unroll
      for (int k = 0; k < 12; ++k) vals[k % 3][k / 3] = image_round<T>(image_value((w[k >> 2] >> (8 * (k & 3))) & 0xffu, range_mode));
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) vals[c][0] = image_round<T>(image_value(s[c], range_mode));
    }
    for (int r = 0; r < copies; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        T* d = dst + (((long)r * batch + b) * 3 + c) * hw + p;
        if constexpr (PX == 4) __builtin_memcpy(__builtin_assume_aligned(d, 4 * sizeof(T)), vals[c], 4 * sizeof(T));
        else d[0] = vals[c][0];
      }
    }
  }
}

template <typename T, int PX>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const T* __restrict__ src, int batch, long hw, uint8_t* __restrict__ dst) {
  const long per_img = hw / PX;
  for (long b = blockIdx.y; b < batch; b += gridDim.y)
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < per_img; t += (long)gridDim.x * blockDim.x) {
    const long p = t * PX;
    T vals[3][PX];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T* s = src + (b * 3 + c) * hw + p;
      if constexpr (PX == 4) __builtin_memcpy(vals[c], __builtin_assume_aligned(s, 4 * sizeof(T)), 4 * sizeof(T));
      else vals[c][0] = s[0];
    }
    uint8_t* d = dst + (b * hw + p) * 3;
    if constexpr (PX == 4) {
      unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 12; ++k) w[k >> 2] |= image_byte(image_widen<T>(vals[k % 3][k / 3])) << (8 * (k & 3));
      __builtin_memcpy(__builtin_assume_aligned(d, 4), w, 12);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c] = (uint8_t)image_byte(image_widen<T>(vals[c][0]));
    }
  }
}

// x: 256-thread blocks over one image's pixel groups (grid-stride past 2048 blocks); y: the images (strided past the grid limit) — no division per thread
inline dim3 image_grid(int batch, long per_img) { return dim3(tg_blocks_1d(per_img), batch < 65535 ? batch : 65535); }
inline bool image_aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

template <typename T>
void launch_from_u8(const void* src, int batch, long hw, int range_mode, int copies, void* dst, hipStream_t st) {
  if (hw % 4 == 0 && image_aligned(src, 4) && image_aligned(dst, 4 * sizeof(T)))
    hipLaunchKernelGGL((image_from_u8_kernel<T, 4>), image_grid(batch, hw / 4), dim3(256), 0, st, (const uint8_t*)src, batch, hw, range_mode,
                       copies, (T*)dst);
  else
    hipLaunchKernelGGL((image_from_u8_kernel<T, 1>), image_grid(batch, hw), dim3(256), 0, st, (const uint8_t*)src, batch, hw, range_mode, copies,
                       (T*)dst);
}

template <typename T>
void launch_to_u8(const void* src, int batch, long hw, void* dst, hipStream_t st) {
  if (hw % 4 == 0 && image_aligned(dst, 4) && image_aligned(src, 4 * sizeof(T)))
    hipLaunchKernelGGL((image_to_u8_kernel<T, 4>), image_grid(batch, hw / 4), dim3(256), 0, st, (const T*)src, batch, hw, (uint8_t*)dst);
  else
    hipLaunchKernelGGL((image_to_u8_kernel<T, 1>), image_grid(batch, hw), dim3(256), 0, st, (const T*)src, batch, hw, (uint8_t*)dst);
}

}  // namespace

extern "C" int tg_image_from_u8(const void* src, int32_t batch, int32_t h, int32_t w, int32_t range_mode, int32_t copies, void* dst,
                                int32_t dst_dtype, void* stream) {
  TG_CHECK(src && dst && src != dst && batch > 0 && h > 0 && w > 0 && copies >= 1 && (range_mode == 0 || range_mode == 1) &&
               (dst_dtype == TG_BF16 || dst_dtype == TG_F16 || dst_dtype == 2),
           TG_ERR_ARG, "tg_image_from_u8: bad args (copies >= 1, range_mode 0 / 1, dst_dtype TG_BF16 / TG_F16 / 2 = fp32, non-null pointers)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long hw = (long)h * w;
  if (dst_dtype == TG_BF16) launch_from_u8<bf16_t>(src, batch, hw, range_mode, copies, dst, st);
  else if (dst_dtype == TG_F16) launch_from_u8<f16_t>(src, batch, hw, range_mode, copies, dst, st);
  else launch_from_u8<float>(src, batch, hw, range_mode, copies, dst, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_image_to_u8(const void* src, int32_t src_dtype, int32_t batch, int32_t h, int32_t w, void* dst, void* stream) {
  TG_CHECK(src && dst && src != dst && batch > 0 && h > 0 && w > 0 && (src_dtype == TG_BF16 || src_dtype == TG_F16 || src_dtype == 2), TG_ERR_ARG,
           "tg_image_to_u8: bad args (src_dtype TG_BF16 / TG_F16 / 2 = fp32, non-null pointers)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long hw = (long)h * w;
  if (src_dtype == TG_BF16) launch_to_u8<bf16_t>(src, batch, hw, dst, st);
  else if (src_dtype == TG_F16) launch_to_u8<f16_t>(src, batch, hw, dst, st);
  else launch_to_u8<float>(src, batch, hw, dst, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
