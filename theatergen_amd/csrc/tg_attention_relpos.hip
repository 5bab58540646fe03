// Flash attention with SAM's decomposed relative-position bias (include/theatergen_hip.h: tg_relpos_tables, tg_attention_relpos).
//
//   O[b,h,i,:] = softmax_j( s q_i.k_j + Bh[b,h,i, j / G] + Bw[b,h,i, j % G] ) V          n_q = len0 = G * G, G = 64 (image) or 14 (window)
//
// The bias is separable: two fp32 tables [N, G] per (batch item, head) instead of an [N, N] tensor (ViT-H global layer: 33.5 MB per image
// against 1 GiB).  tg_relpos_tables builds them from the stored, unscaled q and the layer's rel_pos_h / rel_pos_w; the attention kernel adds
// them to the fp32 scores tile by tile, in registers.
//
// The attention kernel is tg_attention.hip's generic (non-FOLD) instance with the bias in place of the materialised mask: same block (4 waves x 32
// queries), same LDS-DMA K / V^T tiles with the XOR swizzle, same transposed products (lane & 31 = the query), same lazy running max.  Those pieces
// are tg_attn_fwd.h's (read its header first); this file keeps the bias registers and the unrolled G = 14 tiles.
// Scores are kept in exp2 units from the bias add on:  x = fma(q.k, s log2 e, bias log2 e);  p = exp2(x - m).
//   G = 64: a 64-key tile is one grid row kh = t, so Bh is ONE value per query per tile (loaded one tile ahead of its use, before the next tile's
//           DMA is issued) and the lane's 32 Bw values are the same for every tile: 32 registers, loaded once.
//   G = 14: 196 keys = 4 tiles, the last ragged (4 keys).  The query's 14 + 14 table entries sit in registers and the tile loop is fully unrolled,
//           so the (kh, kw) of a score register are two compile-time pairs selected by the lane half.  Keys of the window that are PADDING are real
//           keys here (they carry the projection bias and their table entries): only keys >= 196 are masked.
// Occupancy: d = 64 keeps the parent's three waves per SIMD (164 VGPRs with the 32 bias registers), d = 80 its two (192 / 206 VGPRs); the attribute
// below only sets the floor of two.  No scratch in any instance (build.py gate).
#include "tg_attn_fwd.h"

namespace {

constexpr int KV = 64;        // keys per tile
constexpr float LOG2E = 1.4426950408889634f;

struct RelposParams {
  int heads, n_q, n_qblk;
  const void* q; long q_ld, q_bs;
  const void* k0; long k0_ld, k0_bs;
  const void* vt0; long vt0_ld, vt0_bs;
  float scale_log2;
  void* out; long out_ld, out_bs;
  const float* bh;
  const float* bw;
};

// <T, DPAD, DV, ONES, G>: head dim 64 = <64, 64, false>, head dim 80 = <80, 96, true> (V^T row 95 is fed 1.0: the PV MFMA accumulates the softmax
// denominator)
template <typename T, int DPAD, int DV, bool ONES, int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attention_relpos_kernel(RelposParams p) {
  typedef typename Vec<T>::v8 V8;
  constexpr int HD = ONES ? DV - 16 : DV;       // 80 or 64
  constexpr int LEN = G * G;
  constexpr int NT = (LEN + KV - 1) / KV;
  constexpr int NP = (DPAD + 63) / 64;          // K panels
  constexpr int NKS = DPAD / 16;
  constexpr int DT = DV / 32;
  constexpr int K_ELEMS = NP * 64 * 64;
  constexpr int STAGE = K_ELEMS + DV * 64;
  static_assert(HD == 64 || HD == 80, "head dim 64 or 80");
  static_assert(G == 64 || G == 14, "grid 64 or 14");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sbase = reinterpret_cast<T*>(smem);         // [2][ K: NP x 64 x 64 | V^T: DV x 64 ]

  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lbid = attn_xcd_block();             // over (batch, head, q-block), q-block fastest
  const int qblk = lbid % p.n_qblk;
  const int h = (lbid / p.n_qblk) % p.heads, b = lbid / (p.n_qblk * p.heads);
  const long qrow = (long)qblk * 128 + wave * 32 + l31;
  const bool q_ok = qrow < LEN;

  V8 qf[NKS];
  {
    const T* qp = reinterpret_cast<const T*>(p.q) + (long)b * p.q_bs + qrow * p.q_ld + (long)h * HD;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int d = ks * 16 + hi * 8;
      qf[ks] = attn_q_frag(qp + d, q_ok && d < HD);
    }
  }

  // ---- this query's bias rows (rows >= n_q of the last block read row 0: finite values, their output is never stored)
  const long brow = ((long)b * p.heads + h) * LEN + (q_ok ? qrow : 0);
  const float* bhp = p.bh + brow * G;
  const float* bwp = p.bw + brow * G;
  constexpr int NB = G == 64 ? 32 : 14;
  float bwr[NB];                                 // G = 64: Bw of the lane's 32 keys of every tile; G = 14: the Bw row.  exp2 units
  float bhr[G == 64 ? 1 : 14];                   // G = 14: the Bh row
  if constexpr (G == 64) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {                // chunk c: keys 16 c + 8 hi + 0..7 of the tile = registers 8 (c & 1) .. + 7 of s[c >> 1]
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(bwp + 16 * c + 8 * hi);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(bwp + 16 * c + 8 * hi + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bwr[8 * c + j] = v0[j] * LOG2E;
        bwr[8 * c + 4 + j] = v1[j] * LOG2E;
      }
    }
    bhr[0] = 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < 14; ++j) {
      bwr[j] = bwp[j] * LOG2E;
      bhr[j] = bhp[j] * LOG2E;
    }
  }

  f32x16 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;          // m_run: exp2 units

  const T* kb0 = reinterpret_cast<const T*>(p.k0) + (long)b * p.k0_bs + (long)h * HD;
  const T* vb0 = reinterpret_cast<const T*>(p.vt0) + (long)b * p.vt0_bs + (long)h * HD * p.vt0_ld;
  // ---- LDS-DMA tile loader
  const int lrow = lane >> 3, slot = lane & 7;
  auto issue = [&](int kv0, int stage) {
    T* sK = sbase + stage * STAGE;
    attn_issue_tile<T, NP, DV, ONES>(sK, sK + K_ELEMS, kb0, p.k0_ld, vb0, p.vt0_ld, LEN, kv0, HD, wave, lrow, slot);
  };

  const int prow = attn_perm_row(l31);
  int kofs[4], vofs[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) kofs[c] = attn_frag_ofs(prow, (prow >> 1) & 7, c, hi);
#pragma unroll
  for (int c = 0; c < 4; ++c) vofs[c] = attn_frag_ofs(l31, (l31 >> 1) & 7, c, hi);

  float bh_nxt = 0.f;
  if constexpr (G == 64) bh_nxt = bhp[0];
  issue(0, 0);

  auto tile = [&](const int t) __attribute__((always_inline)) {
    const int st = t & 1, kv0 = t * KV;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kv0 + KV > LEN && ((LEN - kv0) & 7)) {           // the chunk that straddles key 196 brought 4 columns past the window along
      if (tid < HD) attn_zero_vt_tail(sbase + st * STAGE + K_ELEMS, tid, LEN - kv0);
      __syncthreads();
    }
    float bh_t = 0.f;
    if constexpr (G == 64) {
      bh_t = bh_nxt * LOG2E;
      if (t + 1 < NT) bh_nxt = bhp[t + 1];             // before the DMA of tile t + 1: consumed after the wait at the top of the next tile
    }
    if (t + 1 < NT) issue(kv0 + KV, st ^ 1);
    const T* sK = sbase + st * STAGE;
    f32x16 s[2];
    attn_qk<T>(s, sK, qf, kofs);
    // x = s * (scale log2 e) + bias log2 e, fp32
#pragma unroll
    for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float bias;
        if constexpr (G == 64) {
          bias = bwr[kvt * 16 + r] + bh_t;
        } else {
          const int k0_ = kv0 + kvt * 32 + 16 * (r >> 3) + (r & 7), k1_ = k0_ + 8;      // the key of register r for hi = 0 / 1
          const int c0 = k0_ < LEN ? k0_ : LEN - 1, c1 = k1_ < LEN ? k1_ : LEN - 1;
          // values first, then the select: `hi ? a[i] : a[j]` is an lvalue conditional, i.e. a selected ADDRESS and a run-time indexed array
          const float h0 = bhr[c0 / G], h1 = bhr[c1 / G], w0 = bwr[c0 % G], w1 = bwr[c1 % G];
          bias = (hi ? h1 : h0) + (hi ? w1 : w0);
        }
        s[kvt][r] = __builtin_fmaf(s[kvt][r], p.scale_log2, bias);
      }
    if (kv0 + KV > LEN) {
#pragma unroll
      for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + kvt * 32 + 16 * (r >> 3) + 8 * hi + (r & 7);
          if (kv >= LEN) s[kvt][r] = -INFINITY;
        }
    }
    attn_lazy_max<ONES>(o, m_run, l_run, attn_tile_max(s), 1.f);
    float ps = 0.f;
#pragma unroll
    for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[kvt][r] - m_run);
        s[kvt][r] = e;
        if (!ONES) ps += e;
      }
    if (!ONES) l_run += ps;
    attn_pv<T, 32 * 64>(o, s, sK + K_ELEMS, vofs);
  };

  if constexpr (G == 14) {
    // four explicit calls, not `#pragma unroll`: the body is past the unroller's size threshold, and a tile index that is not a constant would turn
    // the bias rows into run-time indexed arrays (scratch)
    static_assert(NT == 4, "196 keys = 4 tiles");
    tile(0);
    tile(1);
    tile(2);
    tile(3);
  } else {
#pragma unroll 1
    for (int t = 0; t < NT; ++t) tile(t);
  }

  attn_scale_acc(o, 1.f / attn_row_sum<ONES>(o, l_run, hi));
  if (q_ok) attn_store(o, reinterpret_cast<T*>(p.out) + (long)b * p.out_bs + qrow * p.out_ld + (long)h * HD, hi, HD);
}

template <typename T, int DPAD, int DV, bool ONES, int G>
int launch_relpos(const tg_attn_desc* d, const RelposParams& p, hipStream_t st) {
  constexpr int NP = (DPAD + 63) / 64;
  const size_t lds = (size_t)2 * (NP * 64 * 64 + DV * 64) * sizeof(T);
  RelposParams pp = p;
  pp.n_qblk = (d->n_q + 127) / 128;
  dim3 grid((unsigned)(pp.n_qblk * d->heads * d->batch));
  auto k = attention_relpos_kernel<T, DPAD, DV, ONES, G>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)attr;
  hipLaunchKernelGGL(k, grid, dim3(256), lds, st, pp);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

template <typename T>
int dispatch_relpos(const tg_attn_desc* d, const RelposParams& p, int G, hipStream_t st) {
  if (d->head_dim == 64) return G == 64 ? launch_relpos<T, 64, 64, false, 64>(d, p, st) : launch_relpos<T, 64, 64, false, 14>(d, p, st);
  return G == 64 ? launch_relpos<T, 80, 96, true, 64>(d, p, st) : launch_relpos<T, 80, 96, true, 14>(d, p, st);
}

// ---- the tables ------------------------------------------------------------------------------------------------------------------------
// One block per (batch item, head, grid row qh): its G queries against the G relative offsets of each axis.  Lane = the key coordinate k (the
// output's contiguous index: 256-byte stores at G = 64), a thread walks QPT queries of the row.  rel_pos_h / rel_pos_w ([2G - 1, D]) and the row's
// queries are staged in LDS in the storage dtype with rows padded by 16 bytes: neighbouring lanes read neighbouring table rows, and with a pitch of
// D + 8 elements (36 / 44 dwords) the 16 lanes of a ds_read_b128 group fall on 16 different 16-byte slots.  Products are exact in fp32 (8- or
// 11-bit significands) and are summed in fp32 by one fma chain over c ascending.
template <typename T, int D, int G>
__global__ __launch_bounds__(256) void relpos_tables_kernel(int heads, const T* __restrict__ q, long q_ld, long q_bs, const T* __restrict__ rph,
                                                            const T* __restrict__ rpw, float* __restrict__ bh, float* __restrict__ bw) {
  typedef typename Vec<T>::v8 V8;
  constexpr int R = 2 * G - 1, PITCH = D + 8, CH = D / 8;
  constexpr int QG = G == 64 ? 4 : 14;            // query groups: 256 / G (G = 64), or one thread per (query, k) pair (G = 14: 196 threads)
  constexpr int QPT = G / QG;
  __shared__ __attribute__((aligned(16))) T sm[(2 * R + G) * PITCH];
  T* sH = sm;
  T* sW = sm + R * PITCH;
  T* sQ = sm + 2 * R * PITCH;
  const int tid = threadIdx.x;
  const int qh = blockIdx.x % G, h = (blockIdx.x / G) % heads, b = blockIdx.x / (G * heads);
  for (int i = tid; i < R * CH; i += 256) {
    const int r = i / CH, c = (i % CH) * 8;
    *reinterpret_cast<V8*>(sH + r * PITCH + c) = *reinterpret_cast<const V8*>(rph + (long)r * D + c);
    *reinterpret_cast<V8*>(sW + r * PITCH + c) = *reinterpret_cast<const V8*>(rpw + (long)r * D + c);
  }
  const T* qp = q + (long)b * q_bs + (long)qh * G * q_ld + (long)h * D;
  for (int i = tid; i < G * CH; i += 256) {
    const int r = i / CH, c = (i % CH) * 8;
    *reinterpret_cast<V8*>(sQ + r * PITCH + c) = *reinterpret_cast<const V8*>(qp + (long)r * q_ld + c);
  }
  __syncthreads();
  if (tid >= G * QG) return;
  const int k = tid % G, g = tid / G;
  const T* hrow = sH + (qh - k + G - 1) * PITCH;
  const long obase = (((long)b * heads + h) * G + qh) * (long)G * G;        // row (b, h, qh * G + qw) of [.., N, G]
#pragma unroll 2
  for (int qq = 0; qq < QPT; ++qq) {
    const int qw = g + qq * QG;
    const T* wrow = sW + (qw - k + G - 1) * PITCH;
    const T* qrow = sQ + qw * PITCH;
    float ah = 0.f, aw = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const V8 qv = *reinterpret_cast<const V8*>(qrow + 8 * c);
      const V8 hv = *reinterpret_cast<const V8*>(hrow + 8 * c);
      const V8 wv = *reinterpret_cast<const V8*>(wrow + 8 * c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float qf = to_f32<T>(qv[j]);
        ah = __builtin_fmaf(qf, to_f32<T>(hv[j]), ah);
        aw = __builtin_fmaf(qf, to_f32<T>(wv[j]), aw);
      }
    }
    bh[obase + (long)qw * G + k] = ah;
    bw[obase + (long)qw * G + k] = aw;
  }
}

template <typename T>
int launch_tables(int batch, int heads, int head_dim, int grid, const void* q, long q_ld, long q_bs, const void* rph, const void* rpw, float* bh,
                  float* bw, hipStream_t st) {
  dim3 g((unsigned)(batch * heads * grid));
  const T* q_ = reinterpret_cast<const T*>(q);
  const T* h_ = reinterpret_cast<const T*>(rph);
  const T* w_ = reinterpret_cast<const T*>(rpw);
  if (head_dim == 64 && grid == 64) hipLaunchKernelGGL((relpos_tables_kernel<T, 64, 64>), g, dim3(256), 0, st, heads, q_, q_ld, q_bs, h_, w_, bh, bw);
  else if (head_dim == 64) hipLaunchKernelGGL((relpos_tables_kernel<T, 64, 14>), g, dim3(256), 0, st, heads, q_, q_ld, q_bs, h_, w_, bh, bw);
  else if (grid == 64) hipLaunchKernelGGL((relpos_tables_kernel<T, 80, 64>), g, dim3(256), 0, st, heads, q_, q_ld, q_bs, h_, w_, bh, bw);
  else hipLaunchKernelGGL((relpos_tables_kernel<T, 80, 14>), g, dim3(256), 0, st, heads, q_, q_ld, q_bs, h_, w_, bh, bw);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

}  // namespace

extern "C" int tg_relpos_tables(int32_t dtype, int32_t batch, int32_t heads, int32_t head_dim, int32_t grid, const void* q, int64_t q_ld,
                                int64_t q_bs, const void* rel_pos_h, const void* rel_pos_w, float* bh, float* bw, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_relpos_tables: bad dtype");
  TG_CHECK(batch > 0 && heads > 0, TG_ERR_ARG, "tg_relpos_tables: empty problem");
  TG_CHECK(q && rel_pos_h && rel_pos_w && bh && bw, TG_ERR_ARG, "tg_relpos_tables: null q / rel_pos_h / rel_pos_w / bh / bw");
  TG_CHECK(head_dim == 64 || head_dim == 80, TG_ERR_UNSUPPORTED, "tg_relpos_tables: head_dim %d unsupported (64, 80)", head_dim);
  TG_CHECK(grid == 64 || grid == 14, TG_ERR_UNSUPPORTED, "tg_relpos_tables: grid %d unsupported (64, 14)", grid);
  TG_CHECK(q_ld % 8 == 0 && (batch == 1 || q_bs % 8 == 0), TG_ERR_ARG, "tg_relpos_tables: q_ld / q_bs must keep 16-byte alignment");
  TG_CHECK((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(rel_pos_h) | reinterpret_cast<uintptr_t>(rel_pos_w)) % 16 == 0, TG_ERR_ARG,
           "tg_relpos_tables: q, rel_pos_h and rel_pos_w must be 16-byte aligned");
  TG_CHECK((reinterpret_cast<uintptr_t>(bh) | reinterpret_cast<uintptr_t>(bw)) % 16 == 0, TG_ERR_ARG, "tg_relpos_tables: bh and bw must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == TG_BF16) return launch_tables<bf16_t>(batch, heads, head_dim, grid, q, q_ld, q_bs, rel_pos_h, rel_pos_w, bh, bw, st);
  return launch_tables<f16_t>(batch, heads, head_dim, grid, q, q_ld, q_bs, rel_pos_h, rel_pos_w, bh, bw, st);
}

extern "C" int tg_attention_relpos(const tg_attn_desc* d, const float* bh, const float* bw, int32_t grid, void* stream) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_attention_relpos: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_attention_relpos: bad dtype");
  TG_CHECK(d->batch > 0 && d->heads > 0 && d->n_q > 0 && d->len0 > 0, TG_ERR_ARG, "tg_attention_relpos: empty problem");
  TG_CHECK(d->q && d->k0 && d->vt0 && d->out, TG_ERR_ARG, "tg_attention_relpos: null q/k0/vt0/out");
  TG_CHECK(bh && bw, TG_ERR_ARG, "tg_attention_relpos: null bias tables");
  TG_CHECK(d->head_dim == 64 || d->head_dim == 80, TG_ERR_UNSUPPORTED, "tg_attention_relpos: head_dim %d unsupported (64, 80)", d->head_dim);
  TG_CHECK(grid == 64 || grid == 14, TG_ERR_UNSUPPORTED, "tg_attention_relpos: grid %d unsupported (64, 14)", grid);
  TG_CHECK(d->len1 == 0 && d->causal == 0 && d->mask == nullptr && d->w1_dev == nullptr, TG_ERR_UNSUPPORTED,
           "tg_attention_relpos: one unmasked softmax segment only (len1 = %d, causal = %d, mask %s, w1_dev %s)", d->len1, d->causal,
           d->mask ? "set" : "null", d->w1_dev ? "set" : "null");
  TG_CHECK(d->n_q == grid * grid && d->len0 == grid * grid, TG_ERR_ARG, "tg_attention_relpos: n_q (%d) and len0 (%d) must both be grid^2 = %d", d->n_q,
           d->len0, grid * grid);
  TG_CHECK(d->scale > 0.f, TG_ERR_ARG, "tg_attention_relpos: scale must be > 0");
  TG_CHECK(d->q_ld % 8 == 0 && d->k0_ld % 8 == 0 && d->vt0_ld % 8 == 0 && d->out_ld % 4 == 0, TG_ERR_ARG,
           "tg_attention_relpos: pitches must keep 16-byte alignment (q_ld, k0_ld, vt0_ld multiples of 8, out_ld of 4)");
  TG_CHECK(d->vt0_ld >= (d->len0 + 7) / 8 * 8, TG_ERR_ARG, "tg_attention_relpos: vt0_ld (%lld) must cover len0 rounded up to 8", (long long)d->vt0_ld);
  TG_CHECK(d->batch == 1 || (d->q_bs % 8 == 0 && d->k0_bs % 8 == 0 && d->vt0_bs % 8 == 0 && d->out_bs % 4 == 0), TG_ERR_ARG,
           "tg_attention_relpos: batch strides must keep 16-byte alignment");
  TG_CHECK((reinterpret_cast<uintptr_t>(d->q) | reinterpret_cast<uintptr_t>(d->k0) | reinterpret_cast<uintptr_t>(d->vt0)) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(d->out) % 8 == 0 && (reinterpret_cast<uintptr_t>(bh) | reinterpret_cast<uintptr_t>(bw)) % 16 == 0,
           TG_ERR_ARG, "tg_attention_relpos: q, k0, vt0, bh, bw must be 16-byte aligned, out 8-byte");
  RelposParams p{};
  p.heads = d->heads; p.n_q = d->n_q;
  p.q = d->q; p.q_ld = d->q_ld; p.q_bs = d->q_bs;
  p.k0 = d->k0; p.k0_ld = d->k0_ld; p.k0_bs = d->k0_bs; p.vt0 = d->vt0; p.vt0_ld = d->vt0_ld; p.vt0_bs = d->vt0_bs;
  p.scale_log2 = d->scale * LOG2E;
  p.out = d->out; p.out_ld = d->out_ld; p.out_bs = d->out_bs;
  p.bh = bh; p.bw = bw;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return dispatch_relpos<bf16_t>(d, p, grid, st);
  return dispatch_relpos<f16_t>(d, p, grid, st);
}
