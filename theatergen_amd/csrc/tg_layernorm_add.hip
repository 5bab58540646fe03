// LayerNorm of a SUM, out = LN(x + r) (include/theatergen_hip.h: tg_layernorm_add): the post-norm residual blocks of GroundingDINO's encoder
// (hidden = LN(hidden + sublayer(hidden))).  A GEMM with a residual epilogue followed by tg_layernorm rounds the sum to the storage dtype before the
// statistics are taken; here both operands are read in the storage dtype, added in fp32 and normalised from that sum, so the only rounding is the
// output's.  The layout is layernorm_kernel's (tg_norm.hip): LPR lanes share one token row, each lane owns the 16-byte chunks l, l + LPR, ... of it;
// two-pass statistics in registers, xor-shuffle reductions inside the lane group.
#include "tg_common.h"

namespace {

template <typename T, int LPR, int MAXC>
__global__ __launch_bounds__(256) void layernorm_add_kernel(const T* x, long ldx, const T* r, long ldr, long rows, int C, float eps, const T* gamma,
                                                            const T* beta, T* out, long ldo) {
  typedef typename Vec<T>::v8 V8;
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int l = lane % LPR;
  const long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
  const bool row_ok = row < rows;
  const int cpr = C / 8;
  float v[MAXC][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = l + LPR * i;
    if (row_ok && c < cpr) {
      const V8 a = *reinterpret_cast<const V8*>(x + row * ldx + c * 8);
      const V8 b = *reinterpret_cast<const V8*>(r + row * ldr + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[i][j] = to_f32<T>(a[j]) + to_f32<T>(b[j]); s += v[i][j]; }
    }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = l + LPR * i;
    if (row_ok && c < cpr) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float dlt = v[i][j] - mean; q += dlt * dlt; }
    }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q / (float)C + eps);
  if (!row_ok) return;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = l + LPR * i;
    if (c < cpr) {
      const V8 g8 = *reinterpret_cast<const V8*>(gamma + c * 8);
      const V8 b8 = *reinterpret_cast<const V8*>(beta + c * 8);
      V8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = from_f32<T>((v[i][j] - mean) * rstd * to_f32<T>(g8[j]) + to_f32<T>(b8[j]));
      *reinterpret_cast<V8*>(out + row * ldo + c * 8) = o;
    }
  }
}

template <typename T>
int launch_ln_add(const void* x, long ldx, const void* r, long ldr, long rows, int C, float eps, const void* gamma, const void* beta, void* out, long ldo,
                  hipStream_t st) {
  const int cpr = C / 8;
#define LNA_CASE(LPR, MAXC)                                                                                                   \
  hipLaunchKernelGGL((layernorm_add_kernel<T, LPR, MAXC>), dim3((unsigned)((rows + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)))), \
                     dim3(256), 0, st, (const T*)x, ldx, (const T*)r, ldr, rows, C, eps, (const T*)gamma, (const T*)beta, (T*)out, ldo)
  if (cpr <= 8) LNA_CASE(8, 1);
  else if (cpr <= 40) LNA_CASE(8, 5);          // C <= 320
  else if (cpr <= 80) LNA_CASE(16, 5);         // C <= 640
  else LNA_CASE(32, 5);                        // C <= 1280
#undef LNA_CASE
  TG_LAUNCH_CHECK();
  return TG_OK;
}

}  // namespace

extern "C" int tg_layernorm_add(int32_t dtype, const void* x, int64_t ldx, const void* res, int64_t ldres, int64_t rows, int32_t C, float eps,
                                const void* gamma, const void* beta, void* out, int64_t ldo, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_layernorm_add: bad dtype");
  TG_CHECK(x && res && gamma && beta && out, TG_ERR_ARG, "tg_layernorm_add: null x / res / gamma / beta / out");
  TG_CHECK(rows > 0 && rows <= 0x7fffffffL && C > 0 && C % 8 == 0, TG_ERR_ARG, "tg_layernorm_add: bad args rows=%lld C=%d", (long long)rows, C);
  TG_CHECK(C <= 1280, TG_ERR_UNSUPPORTED, "tg_layernorm_add: C %d unsupported (multiples of 8 up to 1280)", C);
  TG_CHECK(ldx % 8 == 0 && ldres % 8 == 0 && ldo % 8 == 0 && ldx >= C && ldres >= C && ldo >= C, TG_ERR_ARG,
           "tg_layernorm_add: row pitches must be multiples of 8 and cover C");
  TG_CHECK((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) |
            reinterpret_cast<uintptr_t>(out)) % 16 == 0, TG_ERR_ARG, "tg_layernorm_add: x, res, gamma, beta and out must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16) return launch_ln_add<bf16_t>(x, ldx, res, ldres, rows, C, eps, gamma, beta, out, ldo, st);
  return launch_ln_add<f16_t>(x, ldx, res, ldres, rows, C, eps, gamma, beta, out, ldo, st);
}
