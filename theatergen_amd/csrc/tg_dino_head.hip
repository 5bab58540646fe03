// GroundingDINO's decoder head pieces that are not GEMMs, attention or LayerNorm (include/theatergen_hip.h: tg_dino_contrastive, tg_dino_box_update).
//
//   tg_dino_contrastive  transformers' GroundingDinoContrastiveEmbedding without its tensor: logits[b, q, t] = q_bq . text_bt over the real tokens, -inf
//                        elsewhere, and / or the row maximum alone (the two-stage query selection needs nothing else of the [B, Nv, max_text_len] tensor).
//                        ONE WAVE = 32 QUERIES x every text tile: transposed products, the 32 x 32 x 16 MFMA's A operand is a tile of 32 text rows and its B
//                        operand the wave's 32 query rows, so lane & 31 is the QUERY and a lane's 16 accumulators are 16 tokens of that query: the row
//                        maximum is 16 fmaxf per tile and ONE cross-half exchange at the end; the query fragments (d / 16 registers of 8 elements) are
//                        loaded once and stay in registers over the tiles.  Four consecutive accumulators are four consecutive tokens: 16-byte stores
//                        where max_text_len and the base allow them.  Tiles at or past Lt run no MFMA and read nothing, and without logits they are not visited.
//   tg_dino_box_update   the tail of every box step: ref = sigmoid(h . w3^T + b3 + prior) with prior a logit or a box whose logit(eps = 1e-5) is taken here,
//                        the per-level boxes ref * valid_ratios (tg_msdeform_attn's ref operand, ref_dim 4) and the sinusoidal embedding of the level-0 box
//                        (the input of reference_points_head), all fp32 from the one dot product on.  ONE WAVE = ONE ROW: d / 64 products per lane and
//                        four butterfly sums (every lane ends with the four sums in the same order: the result does not depend on the lane that writes
//                        it), then lane c < 4 writes ref[c], lane i < 4 L writes ref_levels[i] and every lane writes d / 64 (sin, cos) pairs.
#include "tg_common.h"

namespace {

// ---- contrastive embedding ------------------------------------------------------------------------------------------------------------
struct CtrParams {
  const void* q; long q_ld, q_bs;
  const void* text; long t_ld, t_bs;
  const unsigned char* mask;
  float* logits;
  float* row_max;
  int n, Lt, mtl, qblocks, vec4;
};

template <typename T, int KS>
__global__ __launch_bounds__(64) void dino_contrastive_kernel(CtrParams p) {
  typedef typename Vec<T>::v8 V8;
  const int lane = threadIdx.x;
  const int col = lane & 31, hi = lane >> 5;
  const int b = (int)(blockIdx.x / (unsigned)p.qblocks);
  const int qrow = (int)(blockIdx.x % (unsigned)p.qblocks) * 32 + col;
  const bool live = qrow < p.n;
  const int qload = live ? qrow : p.n - 1;                          // clamped: the load is always inside the item's rows, the row is never stored

  V8 qf[KS];
  {
    const T* qp = reinterpret_cast<const T*>(p.q) + (long)b * p.q_bs + (long)qload * p.q_ld + hi * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const V8*>(qp + ks * 16);
  }
  const T* tb = reinterpret_cast<const T*>(p.text) + (long)b * p.t_bs + hi * 8;
  const unsigned char* mb = p.mask + (long)b * p.Lt;
  float* lrow = p.logits != nullptr ? p.logits + ((long)b * p.n + qrow) * p.mtl : nullptr;
  float mx = -INFINITY;

  const int t_end = p.logits != nullptr ? p.mtl : p.Lt;             // row maximum alone: tiles at or past Lt hold -inf only, nothing to store
  for (int t0 = 0; t0 < t_end; t0 += 32) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (t0 < p.Lt) {                                                // wave-uniform
      const int trow = t0 + col < p.Lt ? t0 + col : p.Lt - 1;       // rows past Lt are never read; the clamped row's products are discarded below
      const T* tp = tb + (long)trow * p.t_ld;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = mfma32(*reinterpret_cast<const V8*>(tp + ks * 16), qf[ks], acc);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int tok = t0 + 8 * g + 4 * hi;                          // accumulators 4 g .. 4 g + 3 = tokens tok .. tok + 3 of query `col`
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int tk = tok + j;
        const bool real = tk < p.Lt && mb[tk < p.Lt ? tk : p.Lt - 1] != 0;
        v[j] = real ? acc[4 * g + j] : -INFINITY;
        mx = fmaxf(mx, v[j]);
      }
      if (live && lrow != nullptr) {
        if (p.vec4) {
          if (tok < p.mtl) *reinterpret_cast<float4*>(lrow + tok) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (tok + j < p.mtl) lrow[tok + j] = v[j];
        }
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if (live && hi == 0 && p.row_max != nullptr) p.row_max[(long)b * p.n + qrow] = mx;
}

template <typename T>
void launch_ctr(const CtrParams& p, int d, long blocks, hipStream_t st) {
  if (d == 128) hipLaunchKernelGGL((dino_contrastive_kernel<T, 8>), dim3((unsigned)blocks), dim3(64), 0, st, p);
  else hipLaunchKernelGGL((dino_contrastive_kernel<T, 16>), dim3((unsigned)blocks), dim3(64), 0, st, p);
}

// ---- box update -----------------------------------------------------------------------------------------------------------------------
constexpr int BOX_MAXL = 4;

struct BoxParams {
  const void* h; long h_ld;
  const void* w3;
  const float* b3;
  const float* prior;
  const float* vr;
  float* ref;
  float* ref_levels;
  void* pos_in; long pos_ld;
  long rows;
  int rows_per_batch, L, prior_is_box;
};

template <typename T, int D>
__global__ __launch_bounds__(256) void dino_box_update_kernel(BoxParams p) {
  constexpr int E = D / 64;                                         // elements of h, and (sin, cos) pairs of pos_in, per lane
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;                                        // wave-uniform, no barrier below

  float z[4];
  {
    const T* hp = reinterpret_cast<const T*>(p.h) + row * p.h_ld + lane * E;
    const T* wp = reinterpret_cast<const T*>(p.w3) + lane * E;
    float hv[E];
#pragma unroll
    for (int e = 0; e < E; ++e) hv[e] = to_f32<T>(hp[e]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) s = __builtin_fmaf(hv[e], to_f32<T>(wp[c * D + e]), s);
      z[c] = wave_sum(s);
    }
  }
  float r[4];
  {
    const float4 pr = *reinterpret_cast<const float4*>(p.prior + row * 4);
    float pv[4] = {pr.x, pr.y, pr.z, pr.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float lg = pv[c];
      if (p.prior_is_box) {                                         // torch.special.logit(x, eps = 1e-5) in fp32
        const float x = fminf(fmaxf(lg, 1e-5f), 1.0f - 1e-5f);
        lg = logf(x / (1.0f - x));
      }
      const float t = (z[c] + p.b3[c]) + lg;
      r[c] = 1.0f / (1.0f + expf(-t));                              // t = +inf: exp(-inf) = 0, exactly 1
    }
  }
  if (lane < 4) p.ref[row * 4 + lane] = lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : r[3];
  if (p.ref_levels == nullptr && p.pos_in == nullptr) return;

  const float* vr = p.vr + (row / p.rows_per_batch) * (long)p.L * 2;
  if (p.ref_levels != nullptr && lane < 4 * p.L) {
    const int c = lane & 3;
    const float rc = c == 0 ? r[0] : c == 1 ? r[1] : c == 2 ? r[2] : r[3];
    p.ref_levels[row * (long)p.L * 4 + lane] = rc * vr[(lane >> 2) * 2 + (c & 1)];
  }
  if (p.pos_in != nullptr) {
    // block cb of d / 2 channels = one coordinate, (y, x, w, h): x and y swapped as encode_sinusoidal_position_embedding does; a lane's pairs share it
    const int cb = lane >> 4;
    const float coord = cb == 0 ? r[1] * vr[1] : cb == 1 ? r[0] * vr[0] : cb == 2 ? r[2] * vr[0] : r[3] * vr[1];
    T* op = reinterpret_cast<T*>(p.pos_in) + row * p.pos_ld + lane * (2 * E);
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int jm = (lane & 15) * E + i;                           // pair index inside the coordinate's block: channels 2 jm (sin), 2 jm + 1 (cos)
      const float dim_t = powf(10000.0f, (float)(4 * jm) / (float)D);   // 10000^(2 floor(j / 2) / (d / 2))
      const float t = coord / dim_t;                                // turns
      const float a = 6.283185307179586f * (t - __builtin_rintf(t));
      op[2 * i] = from_f32<T>(sinf(a));
      op[2 * i + 1] = from_f32<T>(cosf(a));
    }
  }
}

template <typename T>
void launch_box(const BoxParams& p, int d, hipStream_t st) {
  dim3 grid((unsigned)((p.rows + 3) / 4));
  if (d == 128) hipLaunchKernelGGL((dino_box_update_kernel<T, 128>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((dino_box_update_kernel<T, 256>), grid, dim3(256), 0, st, p);
}

}  // namespace

extern "C" int tg_dino_contrastive(int32_t dtype, int32_t batch, int32_t n, int32_t d, int32_t text_len, int32_t max_text_len, const void* q,
                                   int64_t q_ld, int64_t q_bs, const void* text, int64_t t_ld, int64_t t_bs, const uint8_t* token_mask, float* logits,
                                   float* row_max, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_dino_contrastive: bad dtype");
  TG_CHECK(batch > 0 && n > 0, TG_ERR_ARG, "tg_dino_contrastive: empty problem (batch = %d, n = %d)", batch, n);
  TG_CHECK(d == 128 || d == 256, TG_ERR_UNSUPPORTED, "tg_dino_contrastive: d = %d unsupported (128 or 256)", d);
  TG_CHECK(text_len >= 1 && text_len <= max_text_len && max_text_len <= 256, TG_ERR_UNSUPPORTED,
           "tg_dino_contrastive: text_len %d / max_text_len %d unsupported (1 <= text_len <= max_text_len <= 256)", text_len, max_text_len);
  TG_CHECK(q && text && token_mask, TG_ERR_ARG, "tg_dino_contrastive: null q / text / token_mask");
  TG_CHECK(logits || row_max, TG_ERR_ARG, "tg_dino_contrastive: neither logits nor row_max given");
  TG_CHECK(q_ld % 8 == 0 && t_ld % 8 == 0 && q_ld >= d && t_ld >= d, TG_ERR_ARG, "tg_dino_contrastive: q_ld and t_ld must be multiples of 8 and cover d");
  TG_CHECK(batch == 1 || (q_bs % 8 == 0 && t_bs % 8 == 0 && q_bs >= 0 && t_bs >= 0), TG_ERR_ARG,
           "tg_dino_contrastive: with batch > 1 q_bs and t_bs must be non-negative multiples of 8");
  TG_CHECK((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(text)) % 16 == 0 &&
               (reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(row_max)) % 4 == 0,
           TG_ERR_ARG, "tg_dino_contrastive: q and text must be 16-byte aligned, logits and row_max 4-byte");
  const long qblocks = ((long)n + 31) / 32;
  TG_CHECK(qblocks * batch <= 0x7fffffffL, TG_ERR_ARG, "tg_dino_contrastive: too many query rows for one launch");
  CtrParams p{};
  p.q = q; p.q_ld = q_ld; p.q_bs = q_bs; p.text = text; p.t_ld = t_ld; p.t_bs = t_bs; p.mask = token_mask;
  p.logits = logits; p.row_max = row_max; p.n = n; p.Lt = text_len; p.mtl = max_text_len; p.qblocks = (int)qblocks;
  p.vec4 = logits != nullptr && max_text_len % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16) launch_ctr<bf16_t>(p, d, qblocks * batch, st);
  else launch_ctr<f16_t>(p, d, qblocks * batch, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_dino_box_update(int32_t dtype, int64_t rows, int32_t rows_per_batch, int32_t d, const void* h, int64_t h_ld, const void* w3,
                                  const float* b3, const float* prior, int32_t prior_is_box, const float* valid_ratios, int32_t n_levels, float* ref,
                                  float* ref_levels, void* pos_in, int64_t pos_ld, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_dino_box_update: bad dtype");
  TG_CHECK(rows > 0 && rows <= 0x7fffffffL && rows_per_batch > 0 && rows % rows_per_batch == 0, TG_ERR_ARG,
           "tg_dino_box_update: rows = %lld must be a positive multiple of rows_per_batch = %d", (long long)rows, rows_per_batch);
  TG_CHECK(d == 128 || d == 256, TG_ERR_UNSUPPORTED, "tg_dino_box_update: d = %d unsupported (128 or 256)", d);
  TG_CHECK(prior_is_box == 0 || prior_is_box == 1, TG_ERR_ARG, "tg_dino_box_update: prior_is_box must be 0 (logits) or 1 (boxes)");
  TG_CHECK(h && w3 && b3 && prior && ref, TG_ERR_ARG, "tg_dino_box_update: null h / w3 / b3 / prior / ref");
  TG_CHECK(h_ld >= d, TG_ERR_ARG, "tg_dino_box_update: h_ld must cover d");
  TG_CHECK((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(w3)) % 2 == 0 && reinterpret_cast<uintptr_t>(prior) % 16 == 0 &&
               (reinterpret_cast<uintptr_t>(b3) | reinterpret_cast<uintptr_t>(ref) | reinterpret_cast<uintptr_t>(ref_levels) |
                reinterpret_cast<uintptr_t>(valid_ratios)) % 4 == 0 && reinterpret_cast<uintptr_t>(pos_in) % 2 == 0,
           TG_ERR_ARG, "tg_dino_box_update: prior must be 16-byte aligned, the other fp32 operands 4-byte, h / w3 / pos_in 2-byte");
  if (ref_levels != nullptr || pos_in != nullptr) {
    TG_CHECK(valid_ratios != nullptr, TG_ERR_ARG, "tg_dino_box_update: ref_levels / pos_in need valid_ratios");
    TG_CHECK(n_levels >= 1 && n_levels <= BOX_MAXL, TG_ERR_UNSUPPORTED, "tg_dino_box_update: n_levels %d unsupported (1 .. 4)", n_levels);
  }
  TG_CHECK(pos_in == nullptr || pos_ld >= 2 * (int64_t)d, TG_ERR_ARG, "tg_dino_box_update: pos_ld must cover 2 d");
  BoxParams p{};
  p.h = h; p.h_ld = h_ld; p.w3 = w3; p.b3 = b3; p.prior = prior; p.vr = valid_ratios; p.ref = ref; p.ref_levels = ref_levels;
  p.pos_in = pos_in; p.pos_ld = pos_ld; p.rows = rows; p.rows_per_batch = rows_per_batch; p.L = n_levels; p.prior_is_box = prior_is_box;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16) launch_box<bf16_t>(p, d, st);
  else launch_box<f16_t>(p, d, st);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
