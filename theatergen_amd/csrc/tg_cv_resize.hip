// The two resizes around the lineart annotator's network (controlnet_aux LineartDetector.__call__), in the arithmetic of OpenCV's portable C++ path as
// include/theatergen_hip.h restates it (written from resize.cpp; not run against a cv2 build):
//   tg_cv_area_u8  : cv2.resize(..., INTER_AREA) of uint8 RGB [batch, hs, ws, 3], shrinking or equal on both axes, then byte / 255 as the network's NCHW
//                    input in bf16 / fp16 / fp32 (and, optionally, the resized bytes themselves)
//   tg_cv_linear_u8: cv2.resize(..., INTER_LINEAR) of the network's byte map (three equal channels: one is computed, three are stored), in either
//                    direction, optionally around the annotator's 255 - x, as uint8 RGB and / or the [0, 1] control image NCHW
// Both are byte-bound glue, once per image.  One lane writes each element; no atomics; a batch item never reads another's data.
//
// AREA, general route: a 256-thread workgroup owns AT_H x AT_W destination pixels.  It runs the horizontal pass over the source rows its vertical entries
// reach into LDS as fp32 [rows][AT_W * 3] (OpenCV's `buf`, never rounded), then the vertical pass out of LDS.  Every product and every sum is a separate
// fp32 operation (cv_mul / cv_add: contraction off), in entry order.  Lane j reads and writes floats 3 j .. 3 j + 2 of a row: a stride of three dwords,
// which is coprime to the bank count, so both passes are conflict-free.  `stage_rows`, from the host plan, is the largest row count any tile needs.
// AREA, integer scales on both axes: OpenCV's fast path, a block sum per pixel: no tables, no LDS.
// LINEAR: a workgroup owns LT_H x LT_W destination pixels and stages the horizontal pass (int32 S[s0] a0 + S[s1] a1) of the source rows its vertical taps
// reach in LDS; a thread then owns four consecutive pixels of one row: two 16-byte LDS reads, 12 interleaved bytes as three dwords and one 4-element
// unit per channel plane (wd % 4 == 0 and aligned bases; otherwise element-wide stores).  A tile whose rows do not fit the stage (vertical downscales
// beyond about LT_STAGE_ROWS / LT_H) computes the same horizontal values straight from memory: the same function, the same bytes.
// Every table index is clamped to its table and every pixel index to its image: tables that do not describe the sizes give wrong bytes, not a fault.
#include <cfloat>
#include <cmath>

#include "tg_common.h"

namespace {

constexpr int AT_H = 4, AT_W = 64;
constexpr int AT_STAGE_ROWS = TG_CV_AREA_STAGE_ROWS;
constexpr int AT_MAX_TAPS = TG_CV_AREA_MAX_TAPS;
constexpr int LT_H = 16, LT_W = 64;
constexpr int LT_STAGE_ROWS = 64;

template <typename T> __device__ __forceinline__ T cv_round(float v) { return from_f32<T>(v); }
template <> __device__ __forceinline__ float cv_round<float>(float v) { return v; }

// one fp32 rounding each: the compiler must not contract a product into the sum that follows it
__device__ __forceinline__ float cv_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float cv_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// saturate_cast<uchar>(float): round half to even, then 0 .. 255
__device__ __forceinline__ int cv_byte(float v) {
  const int r = (int)rintf(v);
  return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// tg_image_from_u8's range_mode 0: an IEEE division, one rounding to T
template <typename T> __device__ __forceinline__ T cv_unit(int byte) { return cv_round<T>((float)byte / 255.0f); }

struct AreaAxis {
  const int32_t* first;   // [out]
  const int32_t* count;   // [out]
  const float* alpha;     // [out][ksize]
  int ksize, in, out;
};

__device__ __forceinline__ void area_taps(const AreaAxis& a, int o, int& first, int& count) {
  int c = a.count[o], f = a.first[o];
  c = c < 0 ? 0 : (c > a.ksize ? a.ksize : c);
  c = c > a.in ? a.in : c;
  f = f < 0 ? 0 : (f > a.in - c ? a.in - c : f);
  first = f;
  count = c;
}

template <typename T>
__device__ __forceinline__ void area_store(const int px[3], int b, int y, int x, int hd, int wd, T* __restrict__ dst, uint8_t* __restrict__ u8_out) {
  const long plane = (long)hd * wd, at = (long)y * wd + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[((long)b * 3 + c) * plane + at] = cv_unit<T>(px[c]);
  if (u8_out) {
    uint8_t* u = u8_out + ((long)b * plane + at) * 3;
    u[0] = (uint8_t)px[0];
    u[1] = (uint8_t)px[1];
    u[2] = (uint8_t)px[2];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cv_area_kernel(const uint8_t* __restrict__ src, int batch, AreaAxis av, AreaAxis ah, T* __restrict__ dst,
                                                      uint8_t* __restrict__ u8_out, int stage_rows) {
  __shared__ float stage[AT_STAGE_ROWS * AT_W * 3];
  const int hd = av.out, wd = ah.out;
  const int tx0 = blockIdx.x * AT_W, ty0 = blockIdx.y * AT_H;
  const int tw = min(AT_W, wd - tx0), th = min(AT_H, hd - ty0);
  int f0, c0, f1, c1;
  area_taps(av, ty0, f0, c0);
  area_taps(av, ty0 + th - 1, f1, c1);
  const int rmin = f0, cap = min(stage_rows, AT_STAGE_ROWS);
  int nrows = f1 + c1 - f0;
  nrows = nrows < 0 ? 0 : (nrows > cap ? cap : nrows);
  for (int b = blockIdx.z; b < batch; b += gridDim.z) {
    const uint8_t* img = src + (long)b * av.in * ah.in * 3;
    // horizontal pass into LDS: item = (staged row, tile column); a thread keeps its column (and its entries) while it walks the rows
    for (int i = threadIdx.x; i < nrows * AT_W; i += 256) {
      const int j = i % AT_W, r = i / AT_W;
      if (j < tw) {
        int first, count;
        area_taps(ah, tx0 + j, first, count);
        const float* alpha = ah.alpha + (long)(tx0 + j) * ah.ksize;
        const uint8_t* p = img + ((long)(rmin + r) * ah.in + first) * 3;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int t = 0; t < count; ++t) {
          const float a = alpha[t];
          s0 = cv_add(s0, cv_mul((float)p[3 * t], a));
          s1 = cv_add(s1, cv_mul((float)p[3 * t + 1], a));
          s2 = cv_add(s2, cv_mul((float)p[3 * t + 2], a));
        }
        float* s = stage + (r * AT_W + j) * 3;
        s[0] = s0;
        s[1] = s1;
        s[2] = s2;
      }
    }
    __syncthreads();
    // vertical pass out of LDS: one destination pixel per thread, a wave per tile row
    {
      const int j = threadIdx.x % AT_W, r = threadIdx.x / AT_W;
      if (r < th && j < tw) {
        int first, count;
        area_taps(av, ty0 + r, first, count);
        const float* beta = av.alpha + (long)(ty0 + r) * av.ksize;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int t = 0; t < count; ++t) {
          int rr = first - rmin + t;
          rr = rr < 0 ? 0 : (rr >= nrows ? max(nrows - 1, 0) : rr);
          const float* s = stage + (rr * AT_W + j) * 3;
          const float bt = beta[t];
          if (t == 0) {
            s0 = cv_mul(bt, s[0]);
            s1 = cv_mul(bt, s[1]);
            s2 = cv_mul(bt, s[2]);
          } else {
            s0 = cv_add(s0, cv_mul(bt, s[0]));
            s1 = cv_add(s1, cv_mul(bt, s[1]));
            s2 = cv_add(s2, cv_mul(bt, s[2]));
          }
        }
        const int px[3] = {cv_byte(s0), cv_byte(s1), cv_byte(s2)};
        area_store<T>(px, b, ty0 + r, tx0 + j, hd, wd, dst, u8_out);
      }
    }
    __syncthreads();                                                              // the next image's horizontal pass overwrites the stage
  }
}

// integer scales on both axes (1 x 1 is the copy): the int32 sum of the sy x sx block; 2 x 2 rounds as (sum + 2) >> 2, everything else as
// rint(float(sum) * inv), inv = float32(1 / (sx sy))
template <typename T>
__global__ __launch_bounds__(256) void cv_area_int_kernel(const uint8_t* __restrict__ src, int batch, int hs, int ws, int hd, int wd, int sy, int sx,
                                                          float inv, T* __restrict__ dst, uint8_t* __restrict__ u8_out) {
  const long plane = (long)hd * wd;
  const bool two = sy == 2 && sx == 2;
  for (int b = blockIdx.y; b < batch; b += gridDim.y)
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < plane; t += (long)gridDim.x * blockDim.x) {
    const int y = (int)(t / wd), x = (int)(t % wd);
    const uint8_t* p = src + (((long)b * hs + (long)y * sy) * ws + (long)x * sx) * 3;
    int a0 = 0, a1 = 0, a2 = 0;
    for (int i = 0; i < sy; ++i) {
      for (int k = 0; k < sx; ++k) {
        a0 += p[3 * k];
        a1 += p[3 * k + 1];
        a2 += p[3 * k + 2];
      }
      p += (long)ws * 3;
    }
    int px[3];
    if (two) {
      px[0] = (a0 + 2) >> 2;
      px[1] = (a1 + 2) >> 2;
      px[2] = (a2 + 2) >> 2;
    } else {
      px[0] = cv_byte(cv_mul((float)a0, inv));
      px[1] = cv_byte(cv_mul((float)a1, inv));
      px[2] = cv_byte(cv_mul((float)a2, inv));
    }
    area_store<T>(px, b, y, x, hd, wd, dst, u8_out);
  }
}

// ---- INTER_LINEAR ---------------------------------------------------------------------------------------------------------------------------------

// one table entry per destination index: (s0, s1, c0, c1), the two taps clamped to the source axis
__device__ __forceinline__ int4 linear_tap(const int4* __restrict__ tab, int o, int in) {
  int4 e = tab[o];
  e.x = e.x < 0 ? 0 : (e.x > in - 1 ? in - 1 : e.x);
  e.y = e.y < 0 ? 0 : (e.y > in - 1 ? in - 1 : e.y);
  return e;
}

// the horizontal pass of channel 0 of one source row at one destination column (invert: the taps are 255 - byte)
__device__ __forceinline__ int linear_h(const uint8_t* __restrict__ row, const int4& e, int invert) {
  int p0 = row[(long)e.x * 3], p1 = row[(long)e.y * 3];
  if (invert) {
    p0 = 255 - p0;
    p1 = 255 - p1;
  }
  return p0 * e.z + p1 * e.w;
}

template <typename T>
__global__ __launch_bounds__(256) void cv_linear_kernel(const uint8_t* __restrict__ src, int batch, int hs, int ws, int hd, int wd,
                                                        const int4* __restrict__ tv, const int4* __restrict__ th, int invert, uint8_t* __restrict__ u8_out,
                                                        T* __restrict__ dst, int vec) {
  __shared__ __attribute__((aligned(16))) int stage[LT_STAGE_ROWS * LT_W];
  const int tx0 = blockIdx.x * LT_W, ty0 = blockIdx.y * LT_H;
  const int tw = min(LT_W, wd - tx0), tht = min(LT_H, hd - ty0);
  const int rmin = linear_tap(tv, ty0, hs).x;
  int nrows = linear_tap(tv, ty0 + tht - 1, hs).y - rmin + 1;
  nrows = nrows < 1 ? 1 : nrows;
  const bool staged = nrows <= LT_STAGE_ROWS;                                     // uniform over the workgroup
  const long plane = (long)hd * wd;
  const int j0 = (threadIdx.x % (LT_W / 4)) * 4, r = threadIdx.x / (LT_W / 4);
  const int y = ty0 + r, x0 = tx0 + j0;
  for (int b = blockIdx.z; b < batch; b += gridDim.z) {
    const uint8_t* img = src + (long)b * hs * ws * 3;
    if (staged) {
      for (int i = threadIdx.x; i < nrows * LT_W; i += 256) {
        const int j = i % LT_W, rr = i / LT_W;
        if (j < tw) stage[rr * LT_W + j] = linear_h(img + (long)min(rmin + rr, hs - 1) * ws * 3, linear_tap(th, tx0 + j, ws), invert);
      }
      __syncthreads();
    }
    if (y < hd && x0 < wd) {
      const int4 ev = linear_tap(tv, y, hs);
      int px[4] = {0, 0, 0, 0};
      if (staged) {
        int ra = ev.x - rmin, rb = ev.y - rmin;
        ra = ra < 0 ? 0 : (ra >= nrows ? nrows - 1 : ra);
        rb = rb < 0 ? 0 : (rb >= nrows ? nrows - 1 : rb);
        int h0[4], h1[4];
        __builtin_memcpy(h0, __builtin_assume_aligned(stage + ra * LT_W + j0, 16), 16);
        __builtin_memcpy(h1, __builtin_assume_aligned(stage + rb * LT_W + j0, 16), 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = (((ev.z * (h0[k] >> 4)) >> 16) + ((ev.w * (h1[k] >> 4)) >> 16) + 2) >> 2;
      } else {
        const uint8_t* ra = img + (long)ev.x * ws * 3;
        const uint8_t* rb = img + (long)ev.y * ws * 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (x0 + k < wd) {
            const int4 eh = linear_tap(th, x0 + k, ws);
            px[k] = (((ev.z * (linear_h(ra, eh, invert) >> 4)) >> 16) + ((ev.w * (linear_h(rb, eh, invert) >> 4)) >> 16) + 2) >> 2;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        px[k] = px[k] < 0 ? 0 : (px[k] > 255 ? 255 : px[k]);
        if (invert) px[k] = 255 - px[k];
      }
      const long at = (long)y * wd + x0;
      if (vec) {                                                                  // wd % 4 == 0: all four pixels are inside the image
        if (u8_out) {
          const unsigned p0 = px[0], p1 = px[1], p2 = px[2], p3 = px[3];
          const unsigned w[3] = {p0 | (p0 << 8) | (p0 << 16) | (p1 << 24), p1 | (p1 << 8) | (p2 << 16) | (p2 << 24), p2 | (p3 << 8) | (p3 << 16) | (p3 << 24)};
          __builtin_memcpy(__builtin_assume_aligned(u8_out + ((long)b * plane + at) * 3, 4), w, 12);
        }
        if (dst) {
          T v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = cv_unit<T>(px[k]);
#pragma unroll
          for (int c = 0; c < 3; ++c) __builtin_memcpy(__builtin_assume_aligned(dst + ((long)b * 3 + c) * plane + at, 4 * sizeof(T)), v, 4 * sizeof(T));
        }
      } else {
        for (int k = 0; k < 4 && x0 + k < wd; ++k) {
          if (u8_out) {
            uint8_t* u = u8_out + ((long)b * plane + at + k) * 3;
            u[0] = u[1] = u[2] = (uint8_t)px[k];
          }
          if (dst) {
            const T v = cv_unit<T>(px[k]);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[((long)b * 3 + c) * plane + at + k] = v;
          }
        }
      }
    }
    if (staged) __syncthreads();                                                  // the next image's horizontal pass overwrites the stage
  }
}

inline bool cv_size_ok(int v) { return v >= 1 && v <= TG_CV_RESIZE_MAX_SIZE; }
inline bool cv_aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
inline bool cv_dtype_ok(int d) { return d == TG_BF16 || d == TG_F16 || d == 2; }
inline int cv_grid_z(int batch) { return batch < 65535 ? batch : 65535; }

// OpenCV's test for the fast path on one axis: |scale - int(scale)| < DBL_EPSILON in double
inline bool cv_integer_scale(int in, int out, int& iscale) {
  const double scale = (double)in / (double)out;
  iscale = (int)scale;
  return std::fabs(scale - (double)iscale) < DBL_EPSILON;
}

template <typename T>
void launch_area(const void* src, int batch, const AreaAxis& av, const AreaAxis& ah, bool fast, int sy, int sx, void* dst, void* u8_out, int stage_rows,
                 hipStream_t st) {
  if (fast) {
    const float inv = (float)(1.0 / ((double)sx * (double)sy));
    hipLaunchKernelGGL((cv_area_int_kernel<T>), dim3(tg_blocks_1d((long)av.out * ah.out), cv_grid_z(batch)), dim3(256), 0, st, (const uint8_t*)src, batch,
                       av.in, ah.in, av.out, ah.out, sy, sx, inv, (T*)dst, (uint8_t*)u8_out);
  } else {
    const dim3 grid((ah.out + AT_W - 1) / AT_W, (av.out + AT_H - 1) / AT_H, cv_grid_z(batch));
    hipLaunchKernelGGL((cv_area_kernel<T>), grid, dim3(256), 0, st, (const uint8_t*)src, batch, av, ah, (T*)dst, (uint8_t*)u8_out, stage_rows);
  }
}

template <typename T>
void launch_linear(const void* src, int batch, int hs, int ws, int hd, int wd, const void* tv, const void* th, int invert, void* u8_out, void* dst,
                   hipStream_t st) {
  const int vec = wd % 4 == 0 && (!u8_out || cv_aligned(u8_out, 4)) && (!dst || cv_aligned(dst, 4 * sizeof(T)));
  const dim3 grid((wd + LT_W - 1) / LT_W, (hd + LT_H - 1) / LT_H, cv_grid_z(batch));
  hipLaunchKernelGGL((cv_linear_kernel<T>), grid, dim3(256), 0, st, (const uint8_t*)src, batch, hs, ws, hd, wd, (const int4*)tv, (const int4*)th, invert,
                     (uint8_t*)u8_out, (T*)dst, vec);
}

}  // namespace

extern "C" int tg_cv_area_u8(const void* src, int32_t batch, int32_t hs, int32_t ws, int32_t hd, int32_t wd, const int32_t* first_v,
                             const int32_t* count_v, const float* alpha_v, int32_t ksize_v, const int32_t* first_h, const int32_t* count_h,
                             const float* alpha_h, int32_t ksize_h, int32_t stage_rows, void* dst, int32_t dst_dtype, void* u8_out, void* stream) {
  TG_CHECK(src && dst, TG_ERR_ARG, "tg_cv_area_u8: null pointer (src and dst are required)");
  TG_CHECK(src != dst && (const void*)u8_out != src && u8_out != dst, TG_ERR_ARG, "tg_cv_area_u8: src, dst and u8_out must be different buffers");
  TG_CHECK(cv_size_ok(batch) && cv_size_ok(hs) && cv_size_ok(ws) && cv_size_ok(hd) && cv_size_ok(wd), TG_ERR_ARG,
           "tg_cv_area_u8: batch and every size must be in 1 .. %d", TG_CV_RESIZE_MAX_SIZE);
  TG_CHECK(hd <= hs && wd <= ws, TG_ERR_ARG, "tg_cv_area_u8: (%d, %d) -> (%d, %d) grows an axis; INTER_AREA is built for shrinking or equal axes only", hs, ws,
           hd, wd);
  TG_CHECK(cv_dtype_ok(dst_dtype), TG_ERR_ARG, "tg_cv_area_u8: dst_dtype %d (TG_BF16 / TG_F16 / 2 = fp32)", dst_dtype);
  int sy = 1, sx = 1;
  const bool fast_v = cv_integer_scale(hs, hd, sy), fast_h = cv_integer_scale(ws, wd, sx);
  const bool fast = fast_v && fast_h;
  if (!fast) {
    TG_CHECK(first_v && count_v && alpha_v && first_h && count_h && alpha_h, TG_ERR_ARG,
             "tg_cv_area_u8: (%d, %d) -> (%d, %d) is not an integer scale on both axes: the six entry tables are required", hs, ws, hd, wd);
    TG_CHECK(ksize_v >= 1 && ksize_v <= AT_MAX_TAPS && ksize_h >= 1 && ksize_h <= AT_MAX_TAPS, TG_ERR_ARG,
             "tg_cv_area_u8: ksize_v = %d, ksize_h = %d (1 .. %d entries per destination index)", ksize_v, ksize_h, AT_MAX_TAPS);
    TG_CHECK(stage_rows >= 1 && stage_rows <= AT_STAGE_ROWS, TG_ERR_ARG, "tg_cv_area_u8: stage_rows %d does not fit the tile's LDS (1 .. %d rows)", stage_rows,
             AT_STAGE_ROWS);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const AreaAxis av{first_v, count_v, alpha_v, ksize_v, hs, hd}, ah{first_h, count_h, alpha_h, ksize_h, ws, wd};
  if (dst_dtype == TG_BF16) launch_area<bf16_t>(src, batch, av, ah, fast, sy, sx, dst, u8_out, stage_rows, st);
  else if (dst_dtype == TG_F16) launch_area<f16_t>(src, batch, av, ah, fast, sy, sx, dst, u8_out, stage_rows, st);
  else launch_area<float>(src, batch, av, ah, fast, sy, sx, dst, u8_out, stage_rows, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_cv_linear_u8(const void* src, int32_t batch, int32_t hs, int32_t ws, int32_t hd, int32_t wd, const int32_t* tab_v, const int32_t* tab_h,
                               int32_t invert, void* u8_out, void* dst, int32_t dst_dtype, void* stream) {
  TG_CHECK(src && tab_v && tab_h, TG_ERR_ARG, "tg_cv_linear_u8: null pointer (src and the two tables are required)");
  TG_CHECK(u8_out || dst, TG_ERR_ARG, "tg_cv_linear_u8: no output (u8_out, dst or both)");
  TG_CHECK((const void*)u8_out != src && (const void*)dst != src && !(dst && dst == u8_out), TG_ERR_ARG,
           "tg_cv_linear_u8: src, u8_out and dst must be different buffers");
  TG_CHECK(cv_size_ok(batch) && cv_size_ok(hs) && cv_size_ok(ws) && cv_size_ok(hd) && cv_size_ok(wd), TG_ERR_ARG,
           "tg_cv_linear_u8: batch and every size must be in 1 .. %d", TG_CV_RESIZE_MAX_SIZE);
  TG_CHECK(invert == 0 || invert == 1, TG_ERR_ARG, "tg_cv_linear_u8: invert %d (0 / 1)", invert);
  TG_CHECK(!dst || cv_dtype_ok(dst_dtype), TG_ERR_ARG, "tg_cv_linear_u8: dst_dtype %d (TG_BF16 / TG_F16 / 2 = fp32)", dst_dtype);
  TG_CHECK(cv_aligned(tab_v, 16) && cv_aligned(tab_h, 16), TG_ERR_ARG, "tg_cv_linear_u8: the tables must be 16-byte aligned (one int32 x 4 entry per index)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dst && dst_dtype == TG_F16) launch_linear<f16_t>(src, batch, hs, ws, hd, wd, tab_v, tab_h, invert, u8_out, dst, st);
  else if (dst && dst_dtype == 2) launch_linear<float>(src, batch, hs, ws, hd, wd, tab_v, tab_h, invert, u8_out, dst, st);
  else launch_linear<bf16_t>(src, batch, hs, ws, hd, wd, tab_v, tab_h, invert, u8_out, dst, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
