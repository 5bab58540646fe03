// Swin shifted-window attention on image-ordered tokens (include/theatergen_hip.h: tg_attention_swin).
//
//   O[b, src(i), h, :] = softmax_j( s q_i.k_j + table[(ri - rj + 6) * 13 + (ci - cj + 6), h] + m_ij ) V          i, j = the 49 tokens of one 7 x 7 window
//
// q / k / v / out are token-major in IMAGE order; the pad to a multiple of 7, the roll by -shift, the window partition and their inverses are the
// address arithmetic of `token_row` below, so nothing but q, k, v is read and nothing but out is written.  A window token whose source lies past the
// H x W grid is a padded token: its q / k / v are the pad vectors (the projection biases), it is a real key, and its output is not stored.
//
// ONE WAVE = ONE (batch item, window, head), four per block, head fastest (the waves of a block read neighbouring 64-byte slices of the same rows).
// 49 tokens padded to 64: scores S^T = K Q^T are four 32 x 32 MFMA tiles over d = 32 (two k-steps), transposed as in tg_attn_fwd.h so that lane & 31 is
// the query, the whole softmax row sits in the lane's registers plus those of lane ^ 32 and P^T feeds the PV MFMA from the score registers.  Q and K
// fragments are 16-byte loads straight from global memory (a lane's fragment is 8 consecutive channels of ONE token: no LDS needed); K rows use the key
// permutation of attn_perm_row.  V has to be transposed: each lane writes its 8 channels of a key into the wave's [32 d][64 keys] LDS image (XOR
// swizzle on the 16-byte slot: 2-way on the writes, conflict-free ds_read_b128 fragments).  The bias table of the wave's head sits beside it as 169
// floats in exp2 units; a score's entry is (query's row base) - (key's offset), the key's offset being one of two compile-time constants picked by
// the lane half.  The shift mask is a 64-bit word per lane: bit j = region(i) != region(j), built from two constant masks (keys of window rows 4-6,
// keys of window columns 4-6) and the window's position; windows off the last row and column skip it.
// The two query blocks run one after the other on the same K registers and V^T image.  No scratch (build.py gate).
#include "tg_attn_fwd.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int WIN = 7, NTOK = 49, TBL = 169;
constexpr int VT_ELEMS = 32 * 64;                                  // the V^T image of one wave
constexpr int WAVE_LDS = VT_ELEMS * 2 + 176 * 4;                   // + the head's table as floats (169, padded to 176)

struct SwinParams {
  int batch, heads, H, W, Hp, Wp, nwx, nwin, shift;
  long npairs;
  const void* q; long q_ld, q_bs;
  const void* k; long k_ld, k_bs;
  const void* v; long v_ld, v_bs;
  const void* pad_q; const void* pad_k; const void* pad_v;
  const void* table;
  float scale_log2;
  void* out; long out_ld, out_bs;
};

constexpr unsigned long long swin_rows_hi() {                      // keys of window rows 4 .. 6
  unsigned long long m = 0;
  for (int j = 0; j < NTOK; ++j) m |= (unsigned long long)(j / WIN >= 4) << j;
  return m;
}
constexpr unsigned long long swin_cols_hi() {                      // keys of window columns 4 .. 6
  unsigned long long m = 0;
  for (int j = 0; j < NTOK; ++j) m |= (unsigned long long)(j % WIN >= 4) << j;
  return m;
}
// table offset of key j: rj * 13 + cj (keys >= 49 are masked: any valid offset)
constexpr int swin_key_ofs(int j) { return j < NTOK ? (j / WIN) * 13 + (j % WIN) : 0; }

template <typename T>
__global__ __launch_bounds__(256) void attention_swin_kernel(SwinParams p) {
  typedef typename Vec<T>::v8 V8;
  __shared__ __attribute__((aligned(16))) char smem[4 * WAVE_LDS];

  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  T* sV = reinterpret_cast<T*>(smem + wave * WAVE_LDS);
  float* sTab = reinterpret_cast<float*>(smem + wave * WAVE_LDS + VT_ELEMS * 2);

  // XCD-aware block order (speed only): neighbouring blocks share token rows (a block of four pairs straddles windows unless heads % 4 == 0, and the
  // rows of a window continue in the next window's 128-byte lines), so they go to ONE XCD's L2
  long pair = (long)attn_xcd_block() * 4 + wave;
  const bool live = pair < p.npairs;                               // a wave past the end recomputes the last pair and stores nothing
  if (!live) pair = p.npairs - 1;
  const int h = (int)(pair % p.heads);
  const int win = (int)((pair / p.heads) % p.nwin);
  const int b = (int)(pair / ((long)p.heads * p.nwin));
  const int wy = win / p.nwx, wx = win % p.nwx;

  // window token t (row-major in the window) -> row of its source in the image-ordered tensors; -1 = padded token, -2 = t >= 49
  auto token_row = [&](int t) -> long {
    if (t >= NTOK) return -2;
    int r = wy * WIN + t / WIN + p.shift, c = wx * WIN + t % WIN + p.shift;
    if (r >= p.Hp) r -= p.Hp;
    if (c >= p.Wp) c -= p.Wp;
    return (r < p.H && c < p.W) ? (long)r * p.W + c : -1;
  };
  auto zero8 = [] {
    V8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = from_f32<T>(0.f);
    return z;
  };
  // 8 channels from channel ch of the head's slice of token t
  auto load8 = [&](const void* base, long ld, long bs, const void* pad, int t, int ch) -> V8 {
    const long row = token_row(t);
    if (row == -2) return zero8();
    const T* src = row >= 0 ? reinterpret_cast<const T*>(base) + (long)b * bs + row * ld + h * 32 + ch
                            : reinterpret_cast<const T*>(pad) + h * 32 + ch;
    return *reinterpret_cast<const V8*>(src);
  };

  // ---- V^T image: lane handles key 16 i + (lane >> 2), channels 8 (lane & 3) .. + 7
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = 16 * i + (lane >> 2), dc = (lane & 3) * 8;
    const V8 vv = load8(p.v, p.v_ld, p.v_bs, p.pad_v, key, dc);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = dc + j;
      sV[d * 64 + ((((key >> 3) ^ ((d >> 1) & 7) ^ (d >> 4))) << 3) + (key & 7)] = vv[j];
    }
  }
  // ---- the head's table, exp2 units
  {
    const T* tb = reinterpret_cast<const T*>(p.table);
    for (int i = lane; i < TBL; i += 64) sTab[i] = to_f32<T>(tb[(long)i * p.heads + h]) * LOG2E;
  }
  // ---- K fragments (A operand): MFMA row l31 of key block kb is key 32 kb + perm(l31)
  V8 kf[2][2];
  {
    const int prow = attn_perm_row(l31);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[kb][ks] = load8(p.k, p.k_ld, p.k_bs, p.pad_k, kb * 32 + prow, ks * 16 + hi * 8);
  }
  int vofs[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) vofs[c] = attn_frag_ofs(l31, ((l31 >> 1) & 7) ^ (l31 >> 4), c, hi);

  // ---- shift mask: keys whose region differs from the query's, per query block below
  const bool last_r = p.shift > 0 && wy == (p.Hp / WIN) - 1, last_c = p.shift > 0 && wx == p.nwx - 1;
  const bool masked = last_r || last_c;                            // wave-uniform

  __syncthreads();

#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qi = qb * 32 + l31;
    const int qc = qi < NTOK ? qi : NTOK - 1;                      // queries 49 .. 63: finite values, never stored
    const int ri = qc / WIN, ci = qc % WIN;
    V8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = load8(p.q, p.q_ld, p.q_bs, p.pad_q, qi, ks * 16 + hi * 8);

    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s[kb] = mfma32(kf[kb][ks], qf[ks], s[kb]);
    }

    unsigned long long dm = 0;
    if (masked) {
      if (last_r) dm |= ri >= 4 ? ~swin_rows_hi() : swin_rows_hi();
      if (last_c) dm |= ci >= 4 ? ~swin_cols_hi() : swin_cols_hi();
      dm >>= 8 * hi;
    }
    const float* trow = sTab + (ri * 13 + ci + 84);
    // register r of block kb holds key 32 kb + 16 (r >> 3) + 8 hi + (r & 7)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k0_ = kb * 32 + 16 * (r >> 3) + (r & 7), k1_ = k0_ + 8;        // the key for hi = 0 / 1
        if (k0_ >= NTOK) {
          s[kb][r] = -INFINITY;
          continue;
        }
        const int o0 = swin_key_ofs(k0_), o1 = swin_key_ofs(k1_);
        const float bias = trow[-(hi ? o1 : o0)];
        float x = __builtin_fmaf(s[kb][r], p.scale_log2, bias);
        if (masked && ((dm >> k0_) & 1)) x -= 100.f * LOG2E;
        if (k1_ >= NTOK && hi) x = -INFINITY;
        s[kb][r] = x;
      }

    const float m = attn_tile_max<2>(s);
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[kb][r] - m);
        s[kb][r] = e;
        l += e;
      }
    l += __shfl_xor(l, 32, 64);

    f32x16 o[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) o[0][r] = 0.f;
    attn_pv<T, VT_ELEMS, 2, 1>(o, s, sV, vofs);
    attn_scale_acc(o, 1.f / l);

    const long orow = token_row(qi);
    if (live && orow >= 0) attn_store(o, reinterpret_cast<T*>(p.out) + (long)b * p.out_bs + orow * p.out_ld + h * 32, hi, 32);
  }
}

}  // namespace

extern "C" int tg_attention_swin(int32_t dtype, int32_t batch, int32_t heads, int32_t head_dim, int32_t window, int32_t H, int32_t W, int32_t shift,
                                 float scale, const void* q, int64_t q_ld, int64_t q_bs, const void* k, int64_t k_ld, int64_t k_bs, const void* v,
                                 int64_t v_ld, int64_t v_bs, const void* pad_q, const void* pad_k, const void* pad_v, const void* table, void* out,
                                 int64_t out_ld, int64_t out_bs, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_attention_swin: bad dtype");
  TG_CHECK(batch > 0 && heads > 0, TG_ERR_ARG, "tg_attention_swin: empty problem");
  TG_CHECK(q && k && v && pad_q && pad_k && pad_v && table && out, TG_ERR_ARG, "tg_attention_swin: null q / k / v / pad_q / pad_k / pad_v / table / out");
  TG_CHECK(head_dim == 32, TG_ERR_UNSUPPORTED, "tg_attention_swin: head_dim %d unsupported (32)", head_dim);
  TG_CHECK(window == 7, TG_ERR_UNSUPPORTED, "tg_attention_swin: window %d unsupported (7)", window);
  TG_CHECK(H >= 7 && W >= 7, TG_ERR_ARG, "tg_attention_swin: grid %d x %d is smaller than the window: not supported (transformers' backbone would pad it to one window)", H, W);
  TG_CHECK(H <= 32768 && W <= 32768, TG_ERR_ARG, "tg_attention_swin: grid %d x %d: a side above 32768", H, W);
  TG_CHECK(shift == 0 || shift == 3, TG_ERR_ARG, "tg_attention_swin: shift %d (0 or 3)", shift);
  TG_CHECK(scale > 0.f, TG_ERR_ARG, "tg_attention_swin: scale must be > 0");
  const int64_t need = (int64_t)heads * 32;
  TG_CHECK(q_ld % 8 == 0 && k_ld % 8 == 0 && v_ld % 8 == 0 && out_ld % 4 == 0 && q_ld >= need && k_ld >= need && v_ld >= need && out_ld >= need,
           TG_ERR_ARG, "tg_attention_swin: pitches must cover heads * 32 and keep the load width (q_ld, k_ld, v_ld multiples of 8, out_ld of 4)");
  TG_CHECK(batch == 1 || (q_bs % 8 == 0 && k_bs % 8 == 0 && v_bs % 8 == 0 && out_bs % 4 == 0), TG_ERR_ARG,
           "tg_attention_swin: batch strides must keep the load width (q_bs, k_bs, v_bs multiples of 8, out_bs of 4)");
  TG_CHECK(batch == 1 || (q_bs >= 0 && k_bs >= 0 && v_bs >= 0 && out_bs >= ((int64_t)H * W - 1) * out_ld + need), TG_ERR_ARG,
           "tg_attention_swin: with batch > 1 the input batch pitches must be >= 0 and out_bs (%lld) must clear one item's H * W rows of out_ld (%lld): "
           "every output element belongs to one lane", (long long)out_bs, (long long)out_ld);
  TG_CHECK((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(pad_q) |
            reinterpret_cast<uintptr_t>(pad_k) | reinterpret_cast<uintptr_t>(pad_v)) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(out) % 8 == 0 && reinterpret_cast<uintptr_t>(table) % 2 == 0,
           TG_ERR_ARG, "tg_attention_swin: q, k, v and the pad vectors must be 16-byte aligned, out 8-byte, table 2-byte");
  SwinParams p{};
  p.batch = batch; p.heads = heads; p.H = H; p.W = W; p.shift = shift;
  p.Hp = (H + 6) / 7 * 7; p.Wp = (W + 6) / 7 * 7;
  p.nwx = p.Wp / 7; p.nwin = (p.Hp / 7) * p.nwx;
  p.npairs = (long)batch * p.nwin * heads;
  TG_CHECK((p.npairs + 3) / 4 <= 0x7fffffffL, TG_ERR_ARG, "tg_attention_swin: too many (window, head) pairs for one launch");
  p.q = q; p.q_ld = q_ld; p.q_bs = q_bs; p.k = k; p.k_ld = k_ld; p.k_bs = k_bs; p.v = v; p.v_ld = v_ld; p.v_bs = v_bs;
  p.pad_q = pad_q; p.pad_k = pad_k; p.pad_v = pad_v; p.table = table;
  p.scale_log2 = scale * LOG2E;
  p.out = out; p.out_ld = out_ld; p.out_bs = out_bs;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)((p.npairs + 3) / 4));
  if (dtype == TG_BF16) hipLaunchKernelGGL(attention_swin_kernel<bf16_t>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(attention_swin_kernel<f16_t>, grid, dim3(256), 0, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
