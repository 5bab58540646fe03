// Multi-scale deformable attention from the projected operands on (include/theatergen_hip.h: tg_msdeform_attn).
//
//   out[b, q, h*32 + c] = sum_{l < L, p < 4} softmax(logits[b, q, h, :])[l*4 + p] * bilinear(value_l[b, :, :, h*32 + c], x_lp, y_lp)
//
// the contract of transformers' GroundingDinoMultiscaleDeformableAttention between its projections: where that module runs L grid_sample calls, a
// stack, a multiply and a sum over a [B heads, 32, Nq, L*4] fp32 tensor, this is a GATHER: 4 L 4 taps of 64 contiguous bytes per (query, head).
//
// A GROUP OF 4 LANES = ONE (batch item, query, head), head fastest; a lane owns 8 of the 32 channels, so a tap is one 16-byte load per lane and the
// four lanes of a group read one 64-byte piece of a value row.  The lanes of a group compute the same softmax and positions redundantly (their
// 8-byte logit and 16-byte offset loads hit the same lines): no LDS, no cross-lane traffic, 8 fp32 accumulators per lane.  The kernel is latency- and
// gather-bound: every tap's address is clamped into the map and loaded UNCONDITIONALLY (the 16 loads of a level are independent and stay in flight
// together), and a tap outside the map or on a masked token is replaced by zeros after the load, so that whatever the clamped row holds (NaN
// included) contributes exactly 0.  Positions are clamped to [-2, W + 1] in fp32 before the float -> int conversion: NaN / huge offsets sample nothing.
// Block order: attn_xcd_block(), neighbouring queries (neighbouring rows of every level) share one XCD's L2.
#include "tg_attn_fwd.h"

namespace {

constexpr int MS_MAXL = 4, MS_P = 4, MS_D = 32;

struct MsdParams {
  int batch, heads, n_q, L;
  int H[MS_MAXL], W[MS_MAXL], start[MS_MAXL];
  long ngroups;                                                   // batch * n_q * heads
  const void* value; long v_ld, v_bs;
  const void* offsets; long off_ld;
  const void* logits; long log_ld;
  const float* ref;
  const unsigned char* vmask; long nv;
  void* out; long out_ld, out_bs;
};

template <typename T, int R, bool MASK>
__global__ __launch_bounds__(256) void msdeform_attn_kernel(MsdParams p) {
  typedef typename Vec<T>::v8 V8;
  typedef typename Vec<T>::v4 V4;
  constexpr float LOG2E = 1.4426950408889634f;
  const int sub = threadIdx.x & 3;
  const long g = (long)attn_xcd_block() * 64 + (threadIdx.x >> 2);
  if (g >= p.ngroups) return;                                     // no barrier below
  const int h = (int)(g % p.heads);
  const long bq = g / p.heads;                                    // b * n_q + q
  const int b = (int)(bq / p.n_q), q = (int)(bq % p.n_q);

  // ---- softmax over the L * 4 logits of this (query, head), fp32 from the stored values
  float w[MS_MAXL][MS_P];
  {
    const T* lp = reinterpret_cast<const T*>(p.logits) + bq * p.log_ld + (long)h * p.L * MS_P;
    float mx = -INFINITY;
#pragma unroll
    for (int l = 0; l < MS_MAXL; ++l) {
      if (l < p.L) {
        const V4 v = *reinterpret_cast<const V4*>(lp + l * MS_P);
#pragma unroll
        for (int j = 0; j < MS_P; ++j) { w[l][j] = to_f32<T>(v[j]); mx = fmaxf(mx, w[l][j]); }
      } else {
#pragma unroll
        for (int j = 0; j < MS_P; ++j) w[l][j] = -INFINITY;
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int l = 0; l < MS_MAXL; ++l)
#pragma unroll
      for (int j = 0; j < MS_P; ++j) { w[l][j] = __builtin_amdgcn_exp2f((w[l][j] - mx) * LOG2E); sum += w[l][j]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int l = 0; l < MS_MAXL; ++l)
#pragma unroll
      for (int j = 0; j < MS_P; ++j) w[l][j] *= inv;
  }

  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;

  const T* vbase = reinterpret_cast<const T*>(p.value) + (long)b * p.v_bs + h * MS_D + sub * 8;
  const unsigned char* mbase = MASK ? p.vmask + (long)b * p.nv : nullptr;
  const T* op = reinterpret_cast<const T*>(p.offsets) + bq * p.off_ld + (long)h * p.L * (MS_P * 2);
  const float* rp = p.ref + bq * p.L * R;

#pragma unroll
  for (int l = 0; l < MS_MAXL; ++l) {
    if (l >= p.L) break;
    const int Hl = p.H[l], Wl = p.W[l];
    const float fH = (float)Hl, fW = (float)Wl;
    const V8 ov = *reinterpret_cast<const V8*>(op + l * (MS_P * 2));
    float rx, ry, rw = 0.f, rh = 0.f;
    if constexpr (R == 2) {
      const float2 r2 = *reinterpret_cast<const float2*>(rp + l * 2);
      rx = r2.x; ry = r2.y;
    } else {
      const float4 r4 = *reinterpret_cast<const float4*>(rp + l * 4);
      rx = r4.x; ry = r4.y; rw = r4.z; rh = r4.w;
    }
    const T* vl = vbase + (long)p.start[l] * p.v_ld;
    const unsigned char* ml = MASK ? mbase + p.start[l] : nullptr;

    V8 tap[MS_P][4];
    float tw[MS_P][4];
#pragma unroll
    for (int s = 0; s < MS_P; ++s) {
      const float ox = to_f32<T>(ov[2 * s]), oy = to_f32<T>(ov[2 * s + 1]);
      float x, y;
      if constexpr (R == 2) {
        x = rx * fW + ox - 0.5f;
        y = ry * fH + oy - 0.5f;
      } else {
        x = (rx + ox / (float)MS_P * rw * 0.5f) * fW - 0.5f;
        y = (ry + oy / (float)MS_P * rh * 0.5f) * fH - 0.5f;
      }
      x = fminf(fmaxf(x, -2.f), fW + 1.f);                         // NaN -> -2: every tap outside
      y = fminf(fmaxf(y, -2.f), fH + 1.f);
      const float x0f = floorf(x), y0f = floorf(y);
      const float fx = x - x0f, fy = y - y0f;
      const int x0 = (int)x0f, y0 = (int)y0f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
        const bool in = xx >= 0 && xx < Wl && yy >= 0 && yy < Hl;
        const int tok = in ? yy * Wl + xx : 0;                     // clamped: the load below is always inside the level
        bool ok = in;
        if constexpr (MASK) ok = ok && ml[tok] == 0;
        tap[s][t] = *reinterpret_cast<const V8*>(vl + (long)tok * p.v_ld);
        const float bw = ((t & 1) ? fx : 1.f - fx) * ((t >> 1) ? fy : 1.f - fy);
        tw[s][t] = ok ? w[l][s] * bw : 0.f;
        if (!ok) {
#pragma unroll
          for (int j = 0; j < 8; ++j) tap[s][t][j] = from_f32<T>(0.f);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < MS_P; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(tw[s][t], to_f32<T>(tap[s][t][j]), acc[j]);
  }

  V8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = from_f32<T>(acc[j]);
  *reinterpret_cast<V8*>(reinterpret_cast<T*>(p.out) + (long)b * p.out_bs + (long)q * p.out_ld + h * MS_D + sub * 8) = o;
}

template <typename T>
void launch_msd(const MsdParams& p, int R, bool mask, hipStream_t st) {
  dim3 grid((unsigned)((p.ngroups + 63) / 64));
  if (R == 2) {
    if (mask) hipLaunchKernelGGL((msdeform_attn_kernel<T, 2, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((msdeform_attn_kernel<T, 2, false>), grid, dim3(256), 0, st, p);
  } else {
    if (mask) hipLaunchKernelGGL((msdeform_attn_kernel<T, 4, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((msdeform_attn_kernel<T, 4, false>), grid, dim3(256), 0, st, p);
  }
}

}  // namespace

extern "C" int tg_msdeform_attn(int32_t dtype, int32_t batch, int32_t heads, int32_t head_dim, int32_t n_levels, int32_t n_points, int32_t n_q,
                                int32_t ref_dim, const int32_t* shapes, const void* value, int64_t v_ld, int64_t v_bs, const void* offsets,
                                int64_t off_ld, const void* logits, int64_t log_ld, const float* ref, const uint8_t* value_mask, void* out,
                                int64_t out_ld, int64_t out_bs, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_msdeform_attn: bad dtype");
  TG_CHECK(batch > 0 && heads > 0 && n_q > 0, TG_ERR_ARG, "tg_msdeform_attn: empty problem");
  TG_CHECK(shapes && value && offsets && logits && ref && out, TG_ERR_ARG, "tg_msdeform_attn: null shapes / value / offsets / logits / ref / out");
  TG_CHECK(head_dim == MS_D, TG_ERR_UNSUPPORTED, "tg_msdeform_attn: head_dim %d unsupported (32)", head_dim);
  TG_CHECK(n_points == MS_P, TG_ERR_UNSUPPORTED, "tg_msdeform_attn: n_points %d unsupported (4)", n_points);
  TG_CHECK(n_levels >= 1 && n_levels <= MS_MAXL, TG_ERR_UNSUPPORTED, "tg_msdeform_attn: n_levels %d unsupported (1 .. 4)", n_levels);
  TG_CHECK(ref_dim == 2 || ref_dim == 4, TG_ERR_UNSUPPORTED, "tg_msdeform_attn: ref_dim %d unsupported (2 or 4)", ref_dim);
  MsdParams p{};
  long nv = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int H = shapes[2 * l], W = shapes[2 * l + 1];
    TG_CHECK(H > 0 && W > 0 && H <= 32768 && W <= 32768, TG_ERR_ARG, "tg_msdeform_attn: level %d is %d x %d (sides 1 .. 32768)", l, H, W);
    p.H[l] = H; p.W[l] = W; p.start[l] = (int)nv;
    nv += (long)H * W;
    TG_CHECK(nv <= 0x7fffffffL, TG_ERR_ARG, "tg_msdeform_attn: more than 2^31 - 1 value tokens");
  }
  const int64_t need = (int64_t)heads * MS_D;
  TG_CHECK(v_ld % 8 == 0 && out_ld % 8 == 0 && v_ld >= need && out_ld >= need, TG_ERR_ARG,
           "tg_msdeform_attn: v_ld and out_ld must be multiples of 8 and cover heads * 32");
  TG_CHECK(off_ld % 8 == 0 && off_ld >= (int64_t)heads * n_levels * 8 && log_ld % 4 == 0 && log_ld >= (int64_t)heads * n_levels * 4, TG_ERR_ARG,
           "tg_msdeform_attn: off_ld must be a multiple of 8 and cover heads * L * 8, log_ld a multiple of 4 and cover heads * L * 4");
  TG_CHECK(batch == 1 || (v_bs % 8 == 0 && out_bs % 8 == 0 && v_bs >= 0 && out_bs >= ((int64_t)n_q - 1) * out_ld + need), TG_ERR_ARG,
           "tg_msdeform_attn: with batch > 1 v_bs and out_bs must be multiples of 8, v_bs >= 0 and out_bs (%lld) must clear one item's n_q rows of "
           "out_ld (%lld): every output element belongs to one lane", (long long)out_bs, (long long)out_ld);
  TG_CHECK((reinterpret_cast<uintptr_t>(value) | reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(ref) |
            reinterpret_cast<uintptr_t>(out)) % 16 == 0 && reinterpret_cast<uintptr_t>(logits) % 8 == 0,
           TG_ERR_ARG, "tg_msdeform_attn: value, offsets, ref and out must be 16-byte aligned, logits 8-byte");
  p.batch = batch; p.heads = heads; p.n_q = n_q; p.L = n_levels;
  p.ngroups = (long)batch * n_q * heads;
  TG_CHECK((p.ngroups + 63) / 64 <= 0x7fffffffL, TG_ERR_ARG, "tg_msdeform_attn: too many (query, head) pairs for one launch");
  p.value = value; p.v_ld = v_ld; p.v_bs = v_bs;
  p.offsets = offsets; p.off_ld = off_ld; p.logits = logits; p.log_ld = log_ld;
  p.ref = ref; p.vmask = value_mask; p.nv = nv;
  p.out = out; p.out_ld = out_ld; p.out_bs = out_bs;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16) launch_msd<bf16_t>(p, ref_dim, value_mask != nullptr, st);
  else launch_msd<f16_t>(p, ref_dim, value_mask != nullptr, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
