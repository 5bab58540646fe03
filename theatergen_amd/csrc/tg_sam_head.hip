// SAM's prompt / mask head around the two-way transformer (include/theatergen_hip.h: tg_sam_posenc, tg_sam_mask_head, tg_sam_mask_post).
//
//   tg_sam_posenc     random-Fourier positional encoding [sin(2 pi t) | cos(2 pi t)], t = (2 c - 1) G, in fp32 with the argument reduced in TURNS
//                     (t - rint(t) is exact) before the sine / cosine: |t| reaches a few hundred, where the raw radian argument has lost its low bits.
//   tg_sam_mask_head  upscale_conv1 (ConvTranspose2d 256 -> 64, k = s = 2) -> channel LayerNorm -> GELU -> upscale_conv2 (64 -> 32, k = s = 2) -> GELU ->
//                     dot with hyper_in, one launch.  A ConvTranspose with kernel = stride is row-local: token (i, j) alone makes the 4 x 4 output pixels
//                     (4 i + 2 a + a', 4 j + 2 b + b').  One wave = 32 tokens x one (a, b): transposed products (lane & 31 = the token), so the 64
//                     channels of a pixel sit in the two lanes (hi = 0 / 1) of its token and the LayerNorm is 32 registers + one cross-half add.  The
//                     second GEMM reads its B operand straight from those registers: its K order is the accumulator order of the first
//                     (weights_pack.pack_sam_upscale writes the A fragments in that order), no LDS, no shuffle.  The [P, 32, (4 g)^2] tensor is never written.
//   tg_sam_mask_post  post_process_masks (bilinear L -> S, crop, bilinear -> original, > threshold) + the caller's F.interpolate(mask.float(), target,
//                     'bilinear').bool(), which is an OR over the taps of non-zero weight.  Every output pixel evaluates its own taps from the logits; no
//                     S x S tensor.  Source indices and weights follow ATen's fp32 CPU sequence: fma(scale, dst + 0.5, -0.5), ONE rounding (its vectorised
//                     builds contract the expression), clamped at 0 — whether a tap's weight is exactly 0 depends on that last bit.
#include "tg_common.h"

namespace {

// ---- positional encoding ------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T pe_cast(float v) { return from_f32<T>(v); }
template <> __device__ __forceinline__ float pe_cast<float>(float v) { return v; }

// one thread per (row, f): out[row, f] = sin, out[row, F + f] = cos.  labels / table (fp32 [5, 2F]: point_embed[0..3], not_a_point_embed):
// label >= 0 adds row min(label, 3), label < 0 REPLACES the encoding by row 4.
template <typename T>
__global__ __launch_bounds__(256) void sam_posenc_kernel(const float* __restrict__ coords, long n, const float* __restrict__ gm, int F,
                                                         const int* __restrict__ labels, const float* __restrict__ table, T* __restrict__ out) {
  const long total = n * F;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / F;
    const int f = (int)(i - row * F);
    const float x = 2.0f * coords[2 * row] - 1.0f, y = 2.0f * coords[2 * row + 1] - 1.0f;
    const float t = x * gm[f] + y * gm[F + f];
    const float r = t - __builtin_rintf(t);                       // exact: |r| <= 0.5
    const float a = 6.283185307179586f * r;
    float s = sinf(a), c = cosf(a);
    if (labels != nullptr) {
      const int lb = labels[row];
      const float* tr = table + (long)(lb < 0 ? 4 : (lb > 3 ? 3 : lb)) * 2 * F;
      if (lb < 0) {
        s = tr[f];
        c = tr[F + f];
      } else {
        s += tr[f];
        c += tr[F + f];
      }
    }
    out[row * 2 * F + f] = pe_cast<T>(s);
    out[row * 2 * F + F + f] = pe_cast<T>(c);
  }
}

// ---- mask head --------------------------------------------------------------------------------------------------------------------------
struct HeadParams {
  const void* x;          // [P g^2, 256]
  const void* w1;         // fragments [ab 4][ct 2][ks 16][lane 64][8]
  const void* w2;         // fragments [a'b' 4][ks 4][lane 64][8], K in accumulator order
  const float* vec;       // fp32 [64 b1 | 64 gamma | 64 beta | 32 b2]
  const void* hyper;      // [P, M, 32]
  float* out;             // [P, M, 4g, 4g]
  int g, M;
  float eps;
};

template <typename T>
__global__ __launch_bounds__(256) void sam_mask_head_kernel(HeadParams p) {
  typedef typename Vec<T>::v8 V8;
  typedef typename Vec<T>::v4 V4;
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int ab = __builtin_amdgcn_readfirstlane(tid >> 6);            // wave = output offset (a, b) of upscale_conv1
  const int g = p.g, gg = g * g;
  const long tok = (long)blockIdx.x * 32 + l31;                       // g % 8 == 0: a 32-token tile never straddles two images
  const int img = (int)(((long)blockIdx.x * 32) / gg);
  const int t_in = (int)(tok - (long)img * gg);
  const int ti = t_in / g, tj = t_in - ti * g;

  // ---- GEMM 1: D[64 channels, 32 tokens] = W1_ab [64, 256] X^T
  f32x16 acc[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  const T* xp = reinterpret_cast<const T*>(p.x) + tok * 256 + hi * 8;
  const T* w1p = reinterpret_cast<const T*>(p.w1) + (long)ab * (2 * 16 * 512) + lane * 8;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const V8 b = *reinterpret_cast<const V8*>(xp + ks * 16);
    const V8 a0 = *reinterpret_cast<const V8*>(w1p + ks * 512);
    const V8 a1 = *reinterpret_cast<const V8*>(w1p + (16 + ks) * 512);
    acc[0] = mfma32(a0, b, acc[0]);
    acc[1] = mfma32(a1, b, acc[1]);
  }
  // register (ct, r) of lane (token, hi) = channel 32 ct + 8 (r >> 2) + 4 hi + (r & 3): four consecutive channels per register quad
  float sum = 0.f;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(p.vec + 32 * ct + 8 * q + 4 * hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[ct][4 * q + j] += bv[j];
        sum += acc[ct][4 * q + j];
      }
    }
  sum += __shfl_xor(sum, 32, 64);
  const float mean = sum * (1.0f / 64.0f);
  float sq = 0.f;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = acc[ct][r] - mean;
      sq = __builtin_fmaf(d, d, sq);
    }
  sq += __shfl_xor(sq, 32, 64);
  const float rstd = 1.0f / __builtin_sqrtf(sq * (1.0f / 64.0f) + p.eps);

  // LayerNorm + GELU, rounded once to the storage dtype: the B operand of GEMM 2, k-step ks = registers 8 (ks & 1) .. + 7 of tile ks >> 1
  V8 yb[4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(p.vec + 64 + 32 * ct + 8 * q + 4 * hi);
      const f32x4 ev = *reinterpret_cast<const f32x4*>(p.vec + 128 + 32 * ct + 8 * q + 4 * hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = __builtin_fmaf((acc[ct][4 * q + j] - mean) * rstd, gv[j], ev[j]);
        yb[2 * ct + (q >> 1)][4 * (q & 1) + j] = from_f32<T>(gelu_erf_f(v));
      }
    }

  // ---- GEMM 2 per (a', b'): D[32 channels, 32 tokens] = W2_{a'b'} [32, 64] Y, then GELU and the hypernetwork product
  const T* w2p = reinterpret_cast<const T*>(p.w2) + lane * 8;
  const T* hp = reinterpret_cast<const T*>(p.hyper) + (long)img * p.M * 32 + 4 * hi;
  const int L4 = 4 * g;
  const int a = ab >> 1, bq = ab & 1;
#pragma unroll
  for (int a2 = 0; a2 < 2; ++a2) {
    float res[2][4];                                                   // [b'][m]
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2) {
      f32x16 d;
#pragma unroll
      for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) d = mfma32(*reinterpret_cast<const V8*>(w2p + ((2 * a2 + b2) * 4 + ks) * 512), yb[ks], d);
      // register r of lane (token, hi) = channel 8 (r >> 2) + 4 hi + (r & 3)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(p.vec + 192 + 8 * q + 4 * hi);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[4 * q + j] = gelu_erf_f(d[4 * q + j] + bv[j]);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float s = 0.f;
        if (m < p.M) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const V4 hv = *reinterpret_cast<const V4*>(hp + m * 32 + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = __builtin_fmaf(d[4 * q + j], to_f32<T>(hv[j]), s);
          }
          s += __shfl_xor(s, 32, 64);
        }
        res[b2][m] = s;
      }
    }
    // both halves hold the sums: half hi stores masks m = hi, hi + 2 (pixels b' = 0, 1 are neighbours: one 8-byte store)
    const long y = 4 * ti + 2 * a + a2, x0 = 4 * tj + 2 * bq;
#pragma unroll
    for (int mm = 0; mm < 2; ++mm) {
      const int m = hi + 2 * mm;
      if (m < p.M) {
        float2 v;
        v.x = hi ? res[0][2 * mm + 1] : res[0][2 * mm];
        v.y = hi ? res[1][2 * mm + 1] : res[1][2 * mm];
        *reinterpret_cast<float2*>(p.out + (((long)img * p.M + m) * L4 + y) * L4 + x0) = v;
      }
    }
  }
}

// ---- mask post-processing ---------------------------------------------------------------------------------------------------------------
struct PostParams {
  const float* logits;    // [PM, L, L]
  unsigned char* mask;    // [PM, ht, wt]
  int* areas;             // [PM]
  int L, hr, wr, h0, w0, ht, wt;
  float sc1, sc2y, sc2x, sc3y, sc3x, thr;
};

// ATen's area_pixel_compute_source_index in fp32 as its CPU kernels evaluate it: one fused multiply-add, clamped at 0
__device__ __forceinline__ void src_index(float scale, int dst, int in_size, int& i0, int& i1, float& l1) {
  float s = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
  s = s < 0.f ? 0.f : s;
  int k = (int)s;
  k = k > in_size - 1 ? in_size - 1 : k;
  i0 = k;
  i1 = k + (k < in_size - 1 ? 1 : 0);
  l1 = s - (float)k;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
}

// the L -> S bilinear value at padded-image pixel (ys, xs)
__device__ __forceinline__ float up1(const float* __restrict__ lg, int L, float sc1, int ys, int xs) {
  int y0, y1, x0, x1;
  float ly, lx;
  src_index(sc1, ys, L, y0, y1, ly);
  src_index(sc1, xs, L, x0, x1, lx);
  const float v00 = lg[(long)y0 * L + x0], v01 = lg[(long)y0 * L + x1], v10 = lg[(long)y1 * L + x0], v11 = lg[(long)y1 * L + x1];
  return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

// the thresholded mask at original-size pixel (yo, xo)
__device__ __forceinline__ bool mask_at(const PostParams& p, const float* __restrict__ lg, int yo, int xo) {
  int y0, y1, x0, x1;
  float ly, lx;
  src_index(p.sc2y, yo, p.hr, y0, y1, ly);
  src_index(p.sc2x, xo, p.wr, x0, x1, lx);
  const float v00 = up1(lg, p.L, p.sc1, y0, x0), v01 = up1(lg, p.L, p.sc1, y0, x1);
  const float v10 = up1(lg, p.L, p.sc1, y1, x0), v11 = up1(lg, p.L, p.sc1, y1, x1);
  const float v = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  return v > p.thr;
}

__global__ __launch_bounds__(256) void sam_mask_post_kernel(PostParams p) {
  const int pm = blockIdx.y;
  const float* lg = p.logits + (long)pm * p.L * p.L;
  unsigned char* mo = p.mask + (long)pm * p.ht * p.wt;
  const int npix = p.ht * p.wt;
  int count = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    const int yt = i / p.wt, xt = i - yt * p.wt;
    int y0, y1, x0, x1;
    float ly, lx;
    src_index(p.sc3y, yt, p.h0, y0, y1, ly);
    src_index(p.sc3x, xt, p.w0, x0, x1, lx);
    // 1 - l is never 0 in fp32 (l < 1), so tap 0 always counts; tap 1 counts when its weight l is non-zero (and it is another pixel)
    const bool ty = ly > 0.f && y1 != y0, tx = lx > 0.f && x1 != x0;
    bool on = mask_at(p, lg, y0, x0);
    if (!on && tx) on = mask_at(p, lg, y0, x1);
    if (!on && ty) on = mask_at(p, lg, y1, x0);
    if (!on && ty && tx) on = mask_at(p, lg, y1, x1);
    mo[i] = on ? 1 : 0;
    count += on ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(p.areas + pm, count);
}

}  // namespace

extern "C" int tg_sam_posenc(int32_t out_dtype, const float* coords, int64_t n, const float* gauss, int32_t F, const int32_t* labels,
                             const float* table, void* out, void* stream) {
  TG_CHECK(out_dtype == TG_BF16 || out_dtype == TG_F16 || out_dtype == 2, TG_ERR_ARG, "tg_sam_posenc: bad output dtype %d (0 bf16, 1 f16, 2 f32)", out_dtype);
  TG_CHECK(n > 0 && F > 0, TG_ERR_ARG, "tg_sam_posenc: empty problem (n = %lld, F = %d)", (long long)n, F);
  TG_CHECK(n * (int64_t)F < ((int64_t)1 << 40), TG_ERR_ARG, "tg_sam_posenc: n * F too large");
  TG_CHECK(coords && gauss && out, TG_ERR_ARG, "tg_sam_posenc: null coords / gauss / out");
  TG_CHECK((labels == nullptr) == (table == nullptr), TG_ERR_ARG, "tg_sam_posenc: labels and table come together");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)tg_blocks_1d(n * F));
  if (out_dtype == 2) hipLaunchKernelGGL((sam_posenc_kernel<float>), grid, dim3(256), 0, st, coords, (long)n, gauss, F, labels, table, reinterpret_cast<float*>(out));
  else if (out_dtype == TG_BF16)
    hipLaunchKernelGGL((sam_posenc_kernel<bf16_t>), grid, dim3(256), 0, st, coords, (long)n, gauss, F, labels, table, reinterpret_cast<bf16_t*>(out));
  else hipLaunchKernelGGL((sam_posenc_kernel<f16_t>), grid, dim3(256), 0, st, coords, (long)n, gauss, F, labels, table, reinterpret_cast<f16_t*>(out));
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_sam_mask_head(int32_t dtype, const void* x, int32_t images, int32_t g, const void* w1, const void* w2, const float* vec,
                                const void* hyper_in, int32_t M, float eps, float* out, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_sam_mask_head: bad dtype");
  TG_CHECK(images > 0 && g > 0 && M > 0, TG_ERR_ARG, "tg_sam_mask_head: empty problem (images = %d, g = %d, M = %d)", images, g, M);
  TG_CHECK(g % 8 == 0 && g <= 64, TG_ERR_UNSUPPORTED, "tg_sam_mask_head: g = %d unsupported (a multiple of 8 up to 64)", g);
  TG_CHECK(M <= 4, TG_ERR_UNSUPPORTED, "tg_sam_mask_head: M = %d unsupported (at most 4 masks)", M);
  TG_CHECK((int64_t)images * g * g / 32 <= 0x7fffffffLL, TG_ERR_ARG, "tg_sam_mask_head: too many tokens");
  TG_CHECK(x && w1 && w2 && vec && hyper_in && out, TG_ERR_ARG, "tg_sam_mask_head: null x / w1 / w2 / vec / hyper_in / out");
  TG_CHECK(eps > 0.f, TG_ERR_ARG, "tg_sam_mask_head: eps must be > 0");
  TG_CHECK((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(vec)) % 16 == 0 &&
               (reinterpret_cast<uintptr_t>(hyper_in) | reinterpret_cast<uintptr_t>(out)) % 8 == 0,
           TG_ERR_ARG, "tg_sam_mask_head: x, w1, w2, vec must be 16-byte aligned, hyper_in and out 8-byte");
  HeadParams p{};
  p.x = x; p.w1 = w1; p.w2 = w2; p.vec = vec; p.hyper = hyper_in; p.out = out; p.g = g; p.M = M; p.eps = eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)((int64_t)images * g * g / 32));
  if (dtype == TG_BF16) hipLaunchKernelGGL((sam_mask_head_kernel<bf16_t>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((sam_mask_head_kernel<f16_t>), grid, dim3(256), 0, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_sam_mask_post(const float* logits, int32_t planes, int32_t L, int32_t S, int32_t hr, int32_t wr, int32_t h0, int32_t w0,
                                float threshold, int32_t ht, int32_t wt, uint8_t* mask, int32_t* areas, void* stream) {
  TG_CHECK(planes > 0 && L > 0 && S > 0 && hr > 0 && wr > 0 && h0 > 0 && w0 > 0 && ht > 0 && wt > 0, TG_ERR_ARG,
           "tg_sam_mask_post: empty size (planes %d, L %d, S %d, reshaped %d x %d, original %d x %d, target %d x %d)", planes, L, S, hr, wr, h0, w0, ht, wt);
  TG_CHECK(planes <= 65535, TG_ERR_ARG, "tg_sam_mask_post: more than 65535 planes");
  TG_CHECK(hr <= S && wr <= S, TG_ERR_ARG, "tg_sam_mask_post: reshaped size %d x %d exceeds the padded size %d", hr, wr, S);
  TG_CHECK(L <= 32768 && S <= 32768 && h0 <= 32768 && w0 <= 32768 && ht <= 32768 && wt <= 32768, TG_ERR_ARG, "tg_sam_mask_post: a side exceeds 32768");
  TG_CHECK(logits && mask && areas, TG_ERR_ARG, "tg_sam_mask_post: null logits / mask / areas");
  PostParams p{};
  p.logits = logits; p.mask = mask; p.areas = areas;
  p.L = L; p.hr = hr; p.wr = wr; p.h0 = h0; p.w0 = w0; p.ht = ht; p.wt = wt;
  p.sc1 = (float)L / (float)S;
  p.sc2y = (float)hr / (float)h0; p.sc2x = (float)wr / (float)w0;
  p.sc3y = (float)h0 / (float)ht; p.sc3x = (float)w0 / (float)wt;
  p.thr = threshold;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(areas, 0, sizeof(int32_t) * (size_t)planes, st) != hipSuccess) {
    tg_set_error("tg_sam_mask_post: clearing the areas failed");
    return TG_ERR_LAUNCH;
  }
  const long npix = (long)ht * wt;
  long bx = (npix + 1023) / 1024;                                       // four pixels per thread: a quarter of the atomics
  bx = bx < 1 ? 1 : (bx > 4096 ? 4096 : bx);
  hipLaunchKernelGGL(sam_mask_post_kernel, dim3((unsigned)bx, (unsigned)planes), dim3(256), 0, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
