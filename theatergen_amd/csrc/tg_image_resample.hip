// Image preprocessing on the device: Pillow's 8-bit two-pass resampling, the processor's rescale + normalise as a table lookup, zero padding.
//   tg_image_resample_u8: uint8 RGB [batch, hs, ws, 3] -> NCHW [batch, 3, hp, wp] in bf16 / fp16 / fp32 (and, optionally, the resized bytes themselves)
// The arithmetic is integer: per axis the host plan (theatergen_amd/preprocess.py, resample_plan) brings int32 coefficients k[out][ksize] at 22 fractional bits
// with first[out] / count[out]; a pass computes (2^21 + sum p * k) >> 22 (arithmetic shift) clipped to 0 .. 255.  The HORIZONTAL pass runs first and rounds to
// uint8, then the vertical pass — Pillow's order, so the bytes are Pillow's.  value = lut[c][byte], rounded once to the destination dtype; every destination
// element outside the window is +0.  One lane writes each element; no atomics; a batch item never reads another's data.
//
// Fused route: a 256-thread workgroup owns TILE_H x TILE_W window pixels of one image.  It runs the horizontal pass over the source rows its vertical taps
// reach (first_v of its first row .. first_v + count_v of its last row: both tables grow with the row) into LDS as uint8 [rows][TILE_W * 3], then the
// vertical pass out of LDS: the [hs, ow] intermediate never exists in memory.  LDS budget TG_RESAMPLE_LDS_BYTES = 160 KiB / 8: eight workgroups (the CU's 32 wave
// slots) stay resident.  `stage_rows`, from the host plan, is the largest row count any tile needs; the kernel never stages more (a wrong value costs wrong
// bytes, never an access outside LDS).  LDS reads in the vertical pass: lane j reads bytes 3 j .. 3 j + 2 of a row, 64 lanes span 192 B = 48 banks, lanes
// sharing a dword read the same address (a broadcast), so the pass is conflict-free; the horizontal pass's byte stores are 3 B apart in the same way.
// Two-launch route (a tile's rows do not fit: strong vertical downscales): the horizontal pass writes uint8 [batch, hs, ow, 3] to `tmp`, the vertical pass
// reads it back.  Both routes call the same two pass functions, so they give the same bytes.
// Every table index is clamped to its table and every pixel index to its image: tables that do not describe the sizes give wrong bytes, not a fault.
#include "tg_common.h"

namespace {

constexpr int TILE_H = TG_RESAMPLE_TILE_H;
constexpr int TILE_W = TG_RESAMPLE_TILE_W;
constexpr int STAGE_BYTES = TG_RESAMPLE_LDS_BYTES;
constexpr int ROW_BYTES = TILE_W * 3;
constexpr int MAX_STAGE_ROWS = STAGE_BYTES / ROW_BYTES;
constexpr int PRECISION_BITS = 22;

template <typename T> __device__ __forceinline__ T resample_round(float v) { return from_f32<T>(v); }
template <> __device__ __forceinline__ float resample_round<float>(float v) { return v; }

__device__ __forceinline__ int clip_u8(int acc) {
  const int v = acc >> PRECISION_BITS;                      // arithmetic: a negative sum lands below 0 and clips to 0, as Pillow's lookup does
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct Axis {
  const int32_t* k;       // [out][ksize]
  const int32_t* first;   // [out]
  const int32_t* count;   // [out]
  int ksize, in, out;
};

// taps of output index o, clamped to the table and to the source axis
__device__ __forceinline__ void axis_taps(const Axis& a, int o, int& first, int& count) {
  int c = a.count[o], f = a.first[o];
  c = c < 0 ? 0 : (c > a.ksize ? a.ksize : c);
  c = c > a.in ? a.in : c;
  f = f < 0 ? 0 : (f > a.in - c ? a.in - c : f);
  first = f;
  count = c;
}

// one pixel of the horizontal pass: three channels of source row `row` (interleaved RGB) at resized column x
__device__ __forceinline__ void pass_h(const uint8_t* __restrict__ row, const Axis& ax, int x, int out[3]) {
  int first, count;
  axis_taps(ax, x, first, count);
  const int32_t* k = ax.k + (long)x * ax.ksize;
  const uint8_t* p = row + (long)first * 3;
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < count; ++t) {
    const int kk = k[t];
    a0 += (int)p[3 * t] * kk;
    a1 += (int)p[3 * t + 1] * kk;
    a2 += (int)p[3 * t + 2] * kk;
  }
  out[0] = clip_u8(a0);
  out[1] = clip_u8(a1);
  out[2] = clip_u8(a2);
}

// value of one byte in the destination dtype
template <typename T>
__device__ __forceinline__ void store_pixel(const int px[3], bool inside, const float* __restrict__ lut, T* __restrict__ dst, long plane, long at) {
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c * plane + at] = inside ? resample_round<T>(lut[c * 256 + px[c]]) : resample_round<T>(0.0f);
}

template <typename T>
__global__ __launch_bounds__(256) void image_resample_fused_kernel(const uint8_t* __restrict__ src, int batch, Axis av, Axis ah, int oy, int ox, int oh, int ow,
                                                                   const float* __restrict__ lut, T* __restrict__ dst, int hp, int wp,
                                                                   uint8_t* __restrict__ u8_out, int stage_rows) {
  __shared__ uint8_t stage[STAGE_BYTES];
  const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
  const int tw = min(TILE_W, ow - tx0), th = min(TILE_H, oh - ty0);              // the window's share of the tile (<= 0: padding only)
  const bool live = tw > 0 && th > 0;
  int rmin = 0, nrows = 0;
  if (live) {
    int f0, c0, f1, c1;
    axis_taps(av, oy + ty0, f0, c0);
    axis_taps(av, oy + ty0 + th - 1, f1, c1);
    rmin = f0;
    nrows = f1 + c1 - f0;
    const int cap = min(stage_rows, MAX_STAGE_ROWS);
    nrows = nrows < 0 ? 0 : (nrows > cap ? cap : nrows);
  }
  const long plane = (long)hp * wp;
  for (int b = blockIdx.z; b < batch; b += gridDim.z) {
    const uint8_t* img = src + (long)b * av.in * ah.in * 3;
    // horizontal pass into LDS: item = (staged row, tile column); a thread keeps its column while it walks the rows
    for (int i = threadIdx.x; i < nrows * TILE_W; i += 256) {
      const int j = i % TILE_W, r = i / TILE_W;
      if (j < tw) {
        int px[3];
        pass_h(img + (long)(rmin + r) * ah.in * 3, ah, ox + tx0 + j, px);
        uint8_t* s = stage + r * ROW_BYTES + j * 3;
        s[0] = (uint8_t)px[0];
        s[1] = (uint8_t)px[1];
        s[2] = (uint8_t)px[2];
      }
    }
    __syncthreads();
    // vertical pass out of LDS, lookup, store: item = (tile row, tile column) of the padded destination
    for (int i = threadIdx.x; i < TILE_H * TILE_W; i += 256) {
      const int j = i % TILE_W, r = i / TILE_W;
      const int y = ty0 + r, x = tx0 + j;
      if (y >= hp || x >= wp) continue;
      const bool inside = y < oh && x < ow;
      int px[3] = {0, 0, 0};
      if (inside) {
        int first, count;
        axis_taps(av, oy + y, first, count);
        const int32_t* k = av.k + (long)(oy + y) * av.ksize;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < count; ++t) {
          int rr = first - rmin + t;
          rr = rr < 0 ? 0 : (rr >= nrows ? max(nrows - 1, 0) : rr);
          const uint8_t* s = stage + rr * ROW_BYTES + j * 3;
          const int kk = k[t];
          a0 += (int)s[0] * kk;
          a1 += (int)s[1] * kk;
          a2 += (int)s[2] * kk;
        }
        px[0] = clip_u8(a0);
        px[1] = clip_u8(a1);
        px[2] = clip_u8(a2);
        if (u8_out) {
          uint8_t* u = u8_out + (((long)b * oh + y) * ow + x) * 3;
          u[0] = (uint8_t)px[0];
          u[1] = (uint8_t)px[1];
          u[2] = (uint8_t)px[2];
        }
      }
      store_pixel<T>(px, inside, lut, dst + (long)b * 3 * plane, plane, (long)y * wp + x);
    }
    __syncthreads();                                                              // the next image's horizontal pass overwrites the stage
  }
}

// two-launch route, first launch: tmp uint8 [batch, hs, ow, 3] = horizontal pass of the window's columns over every source row
__global__ __launch_bounds__(256) void image_resample_h_kernel(const uint8_t* __restrict__ src, int batch, int hs, Axis ah, int ox, int ow,
                                                               uint8_t* __restrict__ tmp) {
  const long per_img = (long)hs * ow;
  for (long b = blockIdx.y; b < batch; b += gridDim.y)
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < per_img; t += (long)gridDim.x * blockDim.x) {
    const int r = (int)(t / ow), x = (int)(t % ow);
    int px[3];
    pass_h(src + ((long)b * hs + r) * ah.in * 3, ah, ox + x, px);
    uint8_t* d = tmp + (b * per_img + t) * 3;
    d[0] = (uint8_t)px[0];
    d[1] = (uint8_t)px[1];
    d[2] = (uint8_t)px[2];
  }
}

// second launch: the vertical pass over tmp, lookup, padding
template <typename T>
__global__ __launch_bounds__(256) void image_resample_v_kernel(const uint8_t* __restrict__ tmp, int batch, Axis av, int oy, int oh, int ow,
                                                               const float* __restrict__ lut, T* __restrict__ dst, int hp, int wp, uint8_t* __restrict__ u8_out) {
  const long plane = (long)hp * wp;
  for (long b = blockIdx.y; b < batch; b += gridDim.y)
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < plane; t += (long)gridDim.x * blockDim.x) {
    const int y = (int)(t / wp), x = (int)(t % wp);
    const bool inside = y < oh && x < ow;
    int px[3] = {0, 0, 0};
    if (inside) {
      int first, count;
      axis_taps(av, oy + y, first, count);
      const int32_t* k = av.k + (long)(oy + y) * av.ksize;
      const uint8_t* s = tmp + ((b * av.in + first) * ow + x) * 3;
      int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
      for (int tt = 0; tt < count; ++tt) {
        const int kk = k[tt];
        a0 += (int)s[0] * kk;
        a1 += (int)s[1] * kk;
        a2 += (int)s[2] * kk;
        s += (long)ow * 3;
      }
      px[0] = clip_u8(a0);
      px[1] = clip_u8(a1);
      px[2] = clip_u8(a2);
      if (u8_out) {
        uint8_t* u = u8_out + ((b * oh + y) * ow + x) * 3;
        u[0] = (uint8_t)px[0];
        u[1] = (uint8_t)px[1];
        u[2] = (uint8_t)px[2];
      }
    }
    store_pixel<T>(px, inside, lut, dst + b * 3 * plane, plane, t);
  }
}

template <typename T>
void launch_resample(const void* src, int batch, const Axis& av, const Axis& ah, int oy, int ox, int oh, int ow, const float* lut, void* dst, int hp, int wp,
                     void* u8_out, int stage_rows, void* tmp, hipStream_t st) {
  const int by = batch < 65535 ? batch : 65535;
  if (tmp) {
    hipLaunchKernelGGL(image_resample_h_kernel, dim3(tg_blocks_1d((long)av.in * ow), by), dim3(256), 0, st, (const uint8_t*)src, batch, av.in, ah, ox, ow,
                       (uint8_t*)tmp);
    hipLaunchKernelGGL((image_resample_v_kernel<T>), dim3(tg_blocks_1d((long)hp * wp), by), dim3(256), 0, st, (const uint8_t*)tmp, batch, av, oy, oh, ow, lut,
                       (T*)dst, hp, wp, (uint8_t*)u8_out);
  } else {
    const dim3 grid((wp + TILE_W - 1) / TILE_W, (hp + TILE_H - 1) / TILE_H, by);
    hipLaunchKernelGGL((image_resample_fused_kernel<T>), grid, dim3(256), 0, st, (const uint8_t*)src, batch, av, ah, oy, ox, oh, ow, lut, (T*)dst, hp, wp,
                       (uint8_t*)u8_out, stage_rows);
  }
}

inline bool size_ok(int v) { return v >= 1 && v <= TG_RESAMPLE_MAX_SIZE; }

}  // namespace

extern "C" int tg_image_resample_u8(const void* src, int32_t batch, int32_t hs, int32_t ws, const int32_t* kv, const int32_t* first_v, const int32_t* count_v,
                                    int32_t ksize_v, int32_t rh, const int32_t* kh, const int32_t* first_h, const int32_t* count_h, int32_t ksize_h, int32_t rw,
                                    int32_t oy, int32_t ox, int32_t oh, int32_t ow, const float* lut, void* dst, int32_t dst_dtype, int32_t hp, int32_t wp,
                                    void* u8_out, int32_t stage_rows, void* tmp, void* stream) {
  TG_CHECK(src && dst && kv && first_v && count_v && kh && first_h && count_h && lut, TG_ERR_ARG,
           "tg_image_resample_u8: null pointer (src, dst, lut and the six tables are required)");
  TG_CHECK(src != dst && (const void*)u8_out != src && (const void*)u8_out != dst && (const void*)tmp != src && (const void*)tmp != dst &&
               !(tmp && tmp == u8_out),
           TG_ERR_ARG, "tg_image_resample_u8: src, dst, u8_out and tmp must be different buffers");
  TG_CHECK(size_ok(batch) && size_ok(hs) && size_ok(ws) && size_ok(rh) && size_ok(rw) && size_ok(oh) && size_ok(ow) && size_ok(hp) && size_ok(wp), TG_ERR_ARG,
           "tg_image_resample_u8: batch and every size must be in 1 .. %d", TG_RESAMPLE_MAX_SIZE);
  TG_CHECK(ksize_v >= 1 && ksize_h >= 1, TG_ERR_ARG, "tg_image_resample_u8: ksize_v = %d, ksize_h = %d (>= 1)", ksize_v, ksize_h);
  TG_CHECK(oy >= 0 && ox >= 0 && oy <= rh - oh && ox <= rw - ow, TG_ERR_ARG,
           "tg_image_resample_u8: window (%d, %d) + (%d, %d) leaves the resized image (%d, %d)", oy, ox, oh, ow, rh, rw);
  TG_CHECK(hp >= oh && wp >= ow, TG_ERR_ARG, "tg_image_resample_u8: destination (%d, %d) smaller than the window (%d, %d)", hp, wp, oh, ow);
  TG_CHECK(dst_dtype == TG_BF16 || dst_dtype == TG_F16 || dst_dtype == 2, TG_ERR_ARG, "tg_image_resample_u8: dst_dtype %d (TG_BF16 / TG_F16 / 2 = fp32)", dst_dtype);
  TG_CHECK(tmp || (stage_rows >= 1 && stage_rows <= MAX_STAGE_ROWS), TG_ERR_ARG,
           "tg_image_resample_u8: stage_rows %d does not fit the fused route's LDS (1 .. %d rows); pass tmp for the two-launch route", stage_rows, MAX_STAGE_ROWS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Axis av{kv, first_v, count_v, ksize_v, hs, rh}, ah{kh, first_h, count_h, ksize_h, ws, rw};
  if (dst_dtype == TG_BF16) launch_resample<bf16_t>(src, batch, av, ah, oy, ox, oh, ow, lut, dst, hp, wp, u8_out, stage_rows, tmp, st);
  else if (dst_dtype == TG_F16) launch_resample<f16_t>(src, batch, av, ah, oy, ox, oh, ow, lut, dst, hp, wp, u8_out, stage_rows, tmp, st);
  else launch_resample<float>(src, batch, av, ah, oy, ox, oh, ow, lut, dst, hp, wp, u8_out, stage_rows, tmp, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
