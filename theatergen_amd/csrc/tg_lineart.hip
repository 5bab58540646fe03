// The lineart annotator's own layers (controlnet_aux's Generator(3, 1, 3): stage 2's ControlNet control image).  Activations are token-major NHWC in the
// storage dtype; the 3x3 convs between these layers are tg_gemm mode 1 / tg_conv_up2.
//   tg_lineart_instnorm : InstanceNorm2d (no affine, biased variance, per (image, channel)) + optional ReLU + optional residual add, three launches:
//                         per-slab (count, mean, M2) -> one fixed-order combine per (image, channel) -> apply.  The apply pass can write a REFLECT-1
//                         bordered image [h + 2, w + 2]: ReflectionPad2d(1) is then the zero-padded 3x3 conv on that buffer, interior of the result.
//   tg_lineart_conv7_in : ReflectionPad2d(3) + Conv2d(3, 64, 7) from the NCHW image, fp32 FMAs, reflected halo tile in LDS
//   tg_lineart_conv7_out: ReflectionPad2d(3) + Conv2d(64, 1, 7) + sigmoid + 255 - trunc(255 s) -> uint8 RGB (the map three times), halo tile in LDS
// Determinism: no atomics, no arrival counters; every sum has one order fixed by the geometry.  Statistics: a thread sums (x - x_first) and its square over
// at most 64 pixels (the shift is a sample, so |mean| >> std costs nothing), then (count, mean, M2) triples are merged pairwise in a fixed sequence (Chan
// et al.), rows of the block first, slabs of the image second.
#include "tg_common.h"

namespace {

constexpr int IN_THREADS = 256;
constexpr int IN_PX_PER_THREAD = 64;          // a slab is (256 / (c / 8)) pixel rows of threads x 64 pixels

// input layouts of the InstanceNorm passes
constexpr int LAY_DENSE = 0;                  // [b, h * w, c]
constexpr int LAY_BORDER = 1;                 // interior of [b, (h + 2) * (w + 2), c]
constexpr int LAY_PARITY = 2;                 // [b, (h / 2) * (w / 2), 4 c]: pixel (2 i + py, 2 j + px) is channel block 2 py + px of low-resolution pixel (i, j)

__device__ __forceinline__ long in_offset(int layout, int y, int x, int h, int w, int c) {
  if (layout == LAY_DENSE) return ((long)y * w + x) * c;
  if (layout == LAY_BORDER) return ((long)(y + 1) * (w + 2) + x + 1) * c;
  return (((long)(y >> 1) * (w >> 1) + (x >> 1)) * 4 + ((y & 1) * 2 + (x & 1))) * c;
}
__device__ __forceinline__ long in_image_elems(int layout, int h, int w, int c) {
  return layout == LAY_BORDER ? (long)(h + 2) * (w + 2) * c : (long)h * w * c;
}

// index -i -> i, n - 1 + i -> n - 1 - i (one reflection: pad < n), then clamped so that tile positions past the image still read inside it
__device__ __forceinline__ int reflect_idx(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

template <typename T> __device__ __forceinline__ void load8(const T* p, float (&v)[8]) {
  typename Vec<T>::v8 r = *reinterpret_cast<const typename Vec<T>::v8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = to_f32<T>(r[j]);
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&v)[8]) {
  typename Vec<T>::v8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = from_f32<T>(v[j]);
  *reinterpret_cast<typename Vec<T>::v8*>(p) = r;
}

// (n, mean, M2) <- merge with (nb, mb, M2b); nb > 0
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
  const float nn = n + nb, delta = mb - mean;
  mean += delta * (nb / nn);
  m2 += m2b + delta * delta * (n * nb / nn);
  n = nn;
}

// grid (slabs, batch); thread (r, g): pixel row r of the slab, channels [8 g, 8 g + 8)
template <typename T>
__global__ __launch_bounds__(IN_THREADS) void lineart_in_stats_kernel(const T* __restrict__ x, int layout, int h, int w, int c, float4* __restrict__ part) {
  __shared__ float2 sm[IN_THREADS * 8];       // [row][channel] (mean, M2)
  __shared__ float sn[IN_THREADS];            // [row] count
  const int G = c >> 3, R = IN_THREADS / G, tid = threadIdx.x;
  const int g = tid % G, r = tid / G;
  const long hw = (long)h * w, slab_px = (long)R * IN_PX_PER_THREAD;
  const long p0 = (long)blockIdx.x * slab_px, p1 = min(hw, p0 + slab_px);
  const T* xb = x + (long)blockIdx.y * in_image_elems(layout, h, w, c) + 8 * g;
  float shift[8], s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) shift[j] = s[j] = q[j] = 0.f;
  int cnt = 0;
  for (long p = p0 + r; p < p1; p += R) {
    float v[8];
    load8<T>(xb + in_offset(layout, (int)(p / w), (int)(p % w), h, w, c), v);
    if (cnt == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) shift[j] = v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = v[j] - shift[j];
      s[j] += d;
      q[j] = __builtin_fmaf(d, d, q[j]);
    }
    ++cnt;
  }
  const float fn = (float)cnt, inv = cnt > 0 ? 1.0f / fn : 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) sm[r * c + 8 * g + j] = make_float2(shift[j] + s[j] * inv, fmaxf(q[j] - s[j] * s[j] * inv, 0.f));
  if (g == 0) sn[r] = fn;
  __syncthreads();
  if (tid < c) {
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int rr = 0; rr < R; ++rr) {
      const float nb = sn[rr];
      if (nb > 0.f) {
        const float2 t = sm[rr * c + tid];
        chan_merge(n, mean, m2, nb, t.x, t.y);
      }
    }
    part[((long)blockIdx.y * gridDim.x + blockIdx.x) * c + tid] = make_float4(n, mean, m2, 0.f);
  }
}

// grid (batch), block c threads: the slabs of one (image, channel) in slab order -> (mean, 1 / sqrt(var + eps))
__global__ void lineart_in_finalize_kernel(const float4* __restrict__ part, int nslab, int c, float eps, float2* __restrict__ coef) {
  const int ch = threadIdx.x;
  if (ch >= c) return;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int sl = 0; sl < nslab; ++sl) {
    const float4 t = part[((long)blockIdx.x * nslab + sl) * c + ch];
    if (t.x > 0.f) chan_merge(n, mean, m2, t.x, t.y, t.z);
  }
  coef[(long)blockIdx.x * c + ch] = make_float2(mean, 1.0f / sqrtf(m2 / n + eps));
}

// grid (blocks, batch); one thread = 8 channels of one OUTPUT position (border positions included: they recompute their reflected source pixel)
template <typename T>
__global__ __launch_bounds__(256) void lineart_in_apply_kernel(const T* __restrict__ x, int layout, int h, int w, int c, const float2* __restrict__ coef,
                                                               int relu, const T* __restrict__ res, int res_layout, T* __restrict__ out, int ob) {
  const int G = c >> 3, oh = h + 2 * ob, ow = w + 2 * ob;
  const long total = (long)oh * ow * G;
  const long b = blockIdx.y;
  const T* xb = x + b * in_image_elems(layout, h, w, c);
  const T* rb = res ? res + b * in_image_elems(res_layout, h, w, c) : nullptr;
  T* outb = out + b * (long)oh * ow * c;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int g = (int)(t % G);
    const long pos = t / G;
    const int y = reflect_idx((int)(pos / ow) - ob, h), xx = reflect_idx((int)(pos % ow) - ob, w);
    float v[8];
    load8<T>(xb + in_offset(layout, y, xx, h, w, c) + 8 * g, v);
    const float4* cf = reinterpret_cast<const float4*>(coef + b * c + 8 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 m = cf[j];
      v[2 * j] = (v[2 * j] - m.x) * m.y;
      v[2 * j + 1] = (v[2 * j + 1] - m.z) * m.w;
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    if (rb) {
      float rv[8];
      load8<T>(rb + in_offset(res_layout, y, xx, h, w, c) + 8 * g, rv);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += rv[j];
    }
    store8<T>(outb + pos * c + 8 * g, v);
  }
}

// ---- 7x7, 3 -> 64 ------------------------------------------------------------------------------------------------------------------------------------
// block = 16 x 16 output pixels x 64 channels; wave = 16 channels (its weights are wave-uniform: scalar loads), lane = 4 pixels of one row.
constexpr int C7_TILE = 16, C7_HALO = C7_TILE + 6, C7_PITCH = 24;

template <typename T>
__global__ __launch_bounds__(256) void lineart_conv7_in_kernel(const T* __restrict__ x, int h, int w, const float* __restrict__ wt,
                                                               const float* __restrict__ bias, T* __restrict__ out) {
  __shared__ float tile[3][C7_HALO][C7_PITCH];
  const int tid = threadIdx.x, b = blockIdx.z, ty0 = blockIdx.y * C7_TILE, tx0 = blockIdx.x * C7_TILE;
  for (int i = tid; i < 3 * C7_HALO * C7_HALO; i += 256) {
    const int ch = i / (C7_HALO * C7_HALO), rem = i % (C7_HALO * C7_HALO), yy = rem / C7_HALO, xx = rem % C7_HALO;
    const int gy = reflect_idx(ty0 + yy - 3, h), gx = reflect_idx(tx0 + xx - 3, w);
    tile[ch][yy][xx] = to_f32<T>(x[(((long)b * 3 + ch) * h + gy) * w + gx]);
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int py = lane >> 2, px = (lane & 3) * 4;
  float acc[4][16];
#pragma unroll
  for (int n = 0; n < 16; ++n) {
    const float bv = bias[wave * 16 + n];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p][n] = bv;
  }
#pragma unroll 1
  for (int ck = 0; ck < 21; ++ck) {                       // (channel, ky)
    const int ch = ck / 7, ky = ck % 7;
    float in[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) in[j] = tile[ch][py + ky][px + j];
    const float* wp = wt + (long)ck * 7 * 64 + wave * 16;
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
#pragma unroll
      for (int n = 0; n < 16; ++n) {
        const float wv = wp[kx * 64 + n];
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[p][n] = __builtin_fmaf(in[kx + p], wv, acc[p][n]);
      }
    }
  }
  const int y = ty0 + py;
  if (y < h) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int xo = tx0 + px + p;
      if (xo < w) {
        T* o = out + (((long)b * h + y) * w + xo) * 64 + wave * 16;
        float lo[8], hi[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) { lo[n] = acc[p][n]; hi[n] = acc[p][8 + n]; }
        store8<T>(o, lo);
        store8<T>(o + 8, hi);
      }
    }
  }
}

// ---- 7x7, 64 -> 1, sigmoid, byte map -------------------------------------------------------------------------------------------------------------------
// block = 16 x 8 output pixels; thread = one pixel x 32 channels (waves 0, 1: channels 0 .. 31, waves 2, 3: 32 .. 63; weights wave-uniform).  The halo tile
// keeps the storage dtype, one pixel = 128 bytes at a 144-byte pitch: the 16 pixels of a row read their 16-byte units from 16 different slots.
constexpr int C7O_TW = 16, C7O_TH = 8, C7O_HW = C7O_TW + 6, C7O_HH = C7O_TH + 6, C7O_PITCH = 144;

template <typename T>
__global__ __launch_bounds__(256) void lineart_conv7_out_kernel(const T* __restrict__ x, int h, int w, const float* __restrict__ wt, float bias,
                                                                uint8_t* __restrict__ out, float* __restrict__ sig) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[C7O_HW * C7O_HH * C7O_PITCH];
  __shared__ float red[128];
  const int tid = threadIdx.x, b = blockIdx.z, ty0 = blockIdx.y * C7O_TH, tx0 = blockIdx.x * C7O_TW;
  for (int i = tid; i < C7O_HW * C7O_HH * 8; i += 256) {
    const int pos = i >> 3, unit = i & 7;
    const int gy = reflect_idx(ty0 + pos / C7O_HW - 3, h), gx = reflect_idx(tx0 + pos % C7O_HW - 3, w);
    *reinterpret_cast<u32x4*>(tile + pos * C7O_PITCH + unit * 16) =
        *reinterpret_cast<const u32x4*>(x + (((long)b * h + gy) * w + gx) * 64 + unit * 8);
  }
  __syncthreads();
  const int half = __builtin_amdgcn_readfirstlane(tid >> 7), pix = tid & 127;
  const int py = pix >> 4, px = pix & 15;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const unsigned char* src = tile + ((py + ky) * C7O_HW + px + kx) * C7O_PITCH + half * 64;
      const float* wp = wt + (ky * 7 + kx) * 64 + half * 32;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v[8];
        load8<T>(reinterpret_cast<const T*>(src + 16 * u), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j & 3] = __builtin_fmaf(v[j], wp[8 * u + j], acc[j & 3]);
      }
    }
  }
  const float part = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (half == 1) red[pix] = part;
  __syncthreads();
  const int y = ty0 + py, xo = tx0 + px;
  if (half == 0 && y < h && xo < w) {
    const float v = (part + red[pix]) + bias;
    const float s = 1.0f / (1.0f + expf(-v));
    const int q = min(max((int)(s * 255.0f), 0), 255);                  // (line * 255).clip(0, 255).astype(uint8): truncation
    const uint8_t m = (uint8_t)(255 - q);
    const long p = ((long)b * h + y) * w + xo;
    out[3 * p] = m; out[3 * p + 1] = m; out[3 * p + 2] = m;
    if (sig) sig[p] = s;
  }
}

inline int in_slab_px(int c) { return IN_THREADS / (c / 8) * IN_PX_PER_THREAD; }
inline long in_nslab(int h, int w, int c) { return ((long)h * w + in_slab_px(c) - 1) / in_slab_px(c); }

template <typename T>
int launch_instnorm(const void* x, int layout, int batch, int h, int w, int c, float eps, int relu, const void* res, int res_layout, void* out, int ob,
                    void* scratch, hipStream_t st) {
  const int nslab = (int)in_nslab(h, w, c);
  float4* part = reinterpret_cast<float4*>(scratch);
  float2* coef = reinterpret_cast<float2*>(part + (long)batch * nslab * c);
  hipLaunchKernelGGL((lineart_in_stats_kernel<T>), dim3(nslab, batch), dim3(IN_THREADS), 0, st, (const T*)x, layout, h, w, c, part);
  hipLaunchKernelGGL(lineart_in_finalize_kernel, dim3(batch), dim3(c), 0, st, (const float4*)part, nslab, c, eps, coef);
  const long total = (long)(h + 2 * ob) * (w + 2 * ob) * (c / 8);
  hipLaunchKernelGGL((lineart_in_apply_kernel<T>), dim3(tg_blocks_1d(total), batch), dim3(256), 0, st, (const T*)x, layout, h, w, c,
                     (const float2*)coef, relu, (const T*)res, res_layout, (T*)out, ob);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int64_t tg_lineart_instnorm_scratch_bytes(int32_t batch, int32_t h, int32_t w, int32_t c) {
  if (batch <= 0 || h <= 0 || w <= 0 || !(c == 64 || c == 128 || c == 256)) return -1;
  return (int64_t)batch * c * (in_nslab(h, w, c) * 16 + 8);
}

extern "C" int tg_lineart_instnorm(int32_t dtype, const void* x, int32_t x_layout, int32_t batch, int32_t h, int32_t w, int32_t c, float eps,
                                   int32_t relu, const void* res, int32_t res_layout, void* out, int32_t out_border, void* scratch, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_lineart_instnorm: bad dtype %d", dtype);
  TG_CHECK(x && out && scratch && x != out && res != out, TG_ERR_ARG, "tg_lineart_instnorm: null x / out / scratch, or out aliases an input");
  TG_CHECK(batch > 0 && batch <= 65535 && h > 0 && w > 0 && (long)h * w < (1L << 31) && (c == 64 || c == 128 || c == 256), TG_ERR_ARG,
           "tg_lineart_instnorm: batch 1 .. 65535, c 64 / 128 / 256 (got batch %d, %d x %d x %d)", batch, h, w, c);
  TG_CHECK(x_layout >= 0 && x_layout <= 2 && (res == nullptr || res_layout == 0 || res_layout == 1) && (out_border == 0 || out_border == 1), TG_ERR_ARG,
           "tg_lineart_instnorm: x_layout 0 / 1 / 2, res_layout 0 / 1, out_border 0 / 1");
  TG_CHECK(x_layout != 2 || (h % 2 == 0 && w % 2 == 0), TG_ERR_ARG, "tg_lineart_instnorm: the parity-class layout needs even h, w (%d x %d)", h, w);
  TG_CHECK(out_border == 0 || (h >= 2 && w >= 2), TG_ERR_ARG, "tg_lineart_instnorm: a reflect-1 border needs h, w >= 2 (%d x %d)", h, w);
  TG_CHECK(aligned16(x) && aligned16(out) && aligned16(res) && aligned16(scratch), TG_ERR_ARG, "tg_lineart_instnorm: x / res / out / scratch must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16) return launch_instnorm<bf16_t>(x, x_layout, batch, h, w, c, eps, relu, res, res_layout, out, out_border, scratch, st);
  return launch_instnorm<f16_t>(x, x_layout, batch, h, w, c, eps, relu, res, res_layout, out, out_border, scratch, st);
}

extern "C" int tg_lineart_conv7_in(int32_t dtype, const void* x, int32_t batch, int32_t h, int32_t w, const void* wt, const void* bias, void* out,
                                   void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_lineart_conv7_in: bad dtype %d", dtype);
  TG_CHECK(x && wt && bias && out && x != out, TG_ERR_ARG, "tg_lineart_conv7_in: null pointer");
  TG_CHECK(batch > 0 && batch <= 65535 && h >= 4 && w >= 4 && (long)h * w < (1L << 31), TG_ERR_ARG,
           "tg_lineart_conv7_in: batch 1 .. 65535 and h, w >= 4 (reflection by 3) required, got %d x %d x %d", batch, h, w);
  TG_CHECK(aligned16(out) && (reinterpret_cast<uintptr_t>(wt) & 3) == 0 && (reinterpret_cast<uintptr_t>(bias) & 3) == 0, TG_ERR_ARG,
           "tg_lineart_conv7_in: out must be 16-byte aligned, wt / bias fp32");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((w + C7_TILE - 1) / C7_TILE, (h + C7_TILE - 1) / C7_TILE, batch);
  TG_CHECK(grid.y <= 65535, TG_ERR_UNSUPPORTED, "tg_lineart_conv7_in: image too tall (%d)", h);
  if (dtype == TG_BF16)
    hipLaunchKernelGGL((lineart_conv7_in_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, h, w, (const float*)wt, (const float*)bias, (bf16_t*)out);
  else
    hipLaunchKernelGGL((lineart_conv7_in_kernel<f16_t>), grid, dim3(256), 0, st, (const f16_t*)x, h, w, (const float*)wt, (const float*)bias, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_lineart_conv7_out(int32_t dtype, const void* x, int32_t batch, int32_t h, int32_t w, const void* wt, float bias, void* out_u8,
                                    void* out_sigmoid, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_lineart_conv7_out: bad dtype %d", dtype);
  TG_CHECK(x && wt && out_u8 && x != out_u8, TG_ERR_ARG, "tg_lineart_conv7_out: null pointer");
  TG_CHECK(batch > 0 && batch <= 65535 && h >= 4 && w >= 4 && (long)h * w < (1L << 31), TG_ERR_ARG,
           "tg_lineart_conv7_out: batch 1 .. 65535 and h, w >= 4 (reflection by 3) required, got %d x %d x %d", batch, h, w);
  TG_CHECK(aligned16(x) && (reinterpret_cast<uintptr_t>(wt) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_sigmoid) & 3) == 0, TG_ERR_ARG,
           "tg_lineart_conv7_out: x must be 16-byte aligned, wt / out_sigmoid fp32");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((w + C7O_TW - 1) / C7O_TW, (h + C7O_TH - 1) / C7O_TH, batch);
  TG_CHECK(grid.y <= 65535, TG_ERR_UNSUPPORTED, "tg_lineart_conv7_out: image too tall (%d)", h);
  if (dtype == TG_BF16)
    hipLaunchKernelGGL((lineart_conv7_out_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, h, w, (const float*)wt, bias, (uint8_t*)out_u8,
                       (float*)out_sigmoid);
  else
    hipLaunchKernelGGL((lineart_conv7_out_kernel<f16_t>), grid, dim3(256), 0, st, (const f16_t*)x, h, w, (const float*)wt, bias, (uint8_t*)out_u8,
                       (float*)out_sigmoid);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
