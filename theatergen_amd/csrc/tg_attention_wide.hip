// Flash attention for WIDE heads on MFMA for gfx950 (include/theatergen_hip.h: tg_attention_wide): head_dim 256 / 512, one softmax segment
//
//   O = softmax(s Q K^T) V
//
// The VAE mid block's single-head d = C = 512 attention (theatergen_amd/vae.py) is the user: 4096 tokens at 512 x 512, 16384 at 1024 x 1024.  Nothing
// [n_q, len] exists in memory; scores are fp32 from the stored Q and K, the softmax is online (running max / sum in fp32), P is rounded to the storage dtype
// where it enters the PV product (as tg_attention does) and O is accumulated in fp32 and rounded once.
//
// The formulation and its shared pieces are tg_attn_fwd.h's (read its header first), with KVT = 1: tiles of 32 keys.  This file keeps the column
// parts, the V^T image of d pairs, the key split and the combine.
//
// What differs is the budget.  One wave per SIMD (the unified 512-register file): a wave's Q fragment is D / 4 registers (128 at d = 512) and its
// O^T accumulator DO / 2 (256 for all 512 columns) — with the score tile, fragments and addresses the full-width d = 512 accumulator leaves the
// compiler nothing, so at d = 512 a block owns DO = 256 output columns: two blocks per (batch, head, query block) each recompute S over the full head dim
// (1.5 x the MFMAs, half the accumulator, 0 scratch); d = 256 is the same template with DO = D.  Tiles are 32 keys: K [32][D] + V^T [DO][32] =
// 48 KiB a stage at d = 512 (96 KiB of the 160 KiB LDS for both stages), 32 KiB at d = 256.
//
// LDS images (128-byte rows, 16-byte slots XOR-swizzled with ((row >> 1) & 7) on the DMA's source address and again on the fragment read):
//   K    D / 64 panels of [32 keys][64 d]
//   V^T  [DO / 2 rows]: row R holds d = 2R (slots 0-3 = keys 0-31) and d = 2R + 1 (slots 4-7)
// both conflict-free for the 4 x 16 lane groups of ds_read_b128.
// len is a multiple of 8, so a 16-byte V^T chunk never straddles it: chunks and K rows at or past len are DMA'd from a page of zeros, and the scores of
// those keys are set to -inf, so a masked key contributes exactly 0 to the max, the sum and PV.
//
// KEY SPLIT (tg_attention_wide_split; the SPLIT = true instances + attention_wide_combine_kernel).  The grid above is ceil(n_q / 128) x heads x batch x
// (D / DO) blocks: 64 at the VAE's 512 x 512 decode (N = 4096, d = 512) on 256 CUs at one block per CU, every block walking all 128 key tiles in
// turn.  With S splits, S blocks share one (batch, head, query block, column part); split s runs the SAME loop over the key tiles
// [s nt / S, (s + 1) nt / S), nt = ceil(len / 32) (S <= nt: no split is empty, and a tile holds >= 8 valid keys, so every split's max is finite), and
// instead of normalising stores its fp32 accumulators, relative to its own running reference m, plus (m, l) per query row:
//   workspace = o [S][batch][heads][R][D] fp32 | ml [S][batch][heads][R][2] fp32,   R = n_qblk * 128   (S batch heads R (D + 2) * 4 bytes)
// Rows [n_q, R) of a (split, batch, head) are written (zero queries) and never read.  A SECOND LAUNCH on the same stream combines:
//   M = max_s m_s,  w_s = exp2((m_s - M) scale log2 e),  out = sum_s w_s o_s / sum_s w_s l_s      fp32, s ascending, one rounding
// The hand-off is the kernel boundary: per-XCD L2s are not coherent inside a launch, and in-launch device-scope hand-offs measured -4 / -7 % here
// (README, round 5), so there is no arrival counter, no atomic and no "last block combines".  Block order: column part fastest, then query block,
// then split, head, batch, so the blocks that read one (batch, head, split)'s K / V^T range are contiguous and fall into one XCD chunk.
#include "tg_attn_fwd.h"

#include <cstdlib>

namespace {

constexpr int WKV = 32;        // keys per tile

struct WideParams {
  int heads, n_q, n_qblk;
  const void* q; long q_ld, q_bs;
  const void* k; long k_ld, k_bs;
  const void* vt; long vt_ld, vt_bs;
  int len;
  float scale_log2;
  void* out; long out_ld, out_bs;
  // key split only (appended: the unsplit instances read nothing past out_bs)
  int batch, splits;
  float* ws;
  // key-padding mask only (KMASK instances): uint8 [batch][len], 1 = masked, batch pitch kmask_bs
  const unsigned char* kmask; long kmask_bs;
};

struct CombineParams {
  int batch, heads, n_q, rows, splits;           // rows = n_qblk * 128
  long total;                                    // batch * heads * n_q
  const float* ws;
  float scale_log2;
  void* out; long out_ld, out_bs;
};

// the body of attention_wide_kernel (KMASK = false: the kernel as it always was) and attention_wide_kmask_kernel (KMASK = true)
template <typename T, int D, int DO, bool SPLIT, bool KMASK>
__device__ __forceinline__ void attention_wide_body(WideParams p) {
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  typedef typename Vec<T>::v8 V8;
  constexpr int NP = D / 64;                    // K panels
  constexpr int NKS = D / 16;
  constexpr int DT = DO / 32;
  constexpr int NSPLIT = D / DO;                // blocks that share one (batch, head, query block)
  constexpr int KJ = NP;                        // K DMA instructions per wave per tile (8 rows x 8 slots each)
  constexpr int VJ = DO / 64;                   // V^T DMA instructions per wave per tile
  constexpr int K_ELEMS = NP * 32 * 64;
  constexpr int STAGE = K_ELEMS + DO * 32;
  static_assert(D % 64 == 0 && DO % 64 == 0 && D % DO == 0, "tile shape");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sbase = reinterpret_cast<T*>(smem);         // [2][ K: NP x 32 x 64 | V^T: DO / 2 x 64 ]

  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lbid = attn_xcd_block();             // over (batch, head, [split,] q-block, column part), column part fastest
  const int dbase = (lbid % NSPLIT) * DO;        // first output column of this block
  const int lq = lbid / NSPLIT;
  const int qblk = lq % p.n_qblk;
  int ks = 0, h, b;                              // ks: this block's key split
  if constexpr (SPLIT) {
    const int lh = lq / p.n_qblk;
    ks = lh % p.splits;
    h = (lh / p.splits) % p.heads;
    b = lh / (p.splits * p.heads);
  } else {
    h = (lq / p.n_qblk) % p.heads;
    b = lq / (p.n_qblk * p.heads);
  }
  const long qrow = (long)qblk * 128 + wave * 32 + l31;
  const bool q_ok = qrow < p.n_q;

  // Q fragments (B operand): this lane's query row, d = ks*16 + hi*8 .. +8; rows >= n_q are not read
  V8 qf[NKS];
  {
    const T* qp = reinterpret_cast<const T*>(p.q) + (long)b * p.q_bs + qrow * p.q_ld + (long)h * D;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = attn_q_frag(qp + ks * 16 + hi * 8, q_ok);
  }

  f32x16 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // ---- LDS-DMA tile loader
  const int lrow = lane >> 3, slot = lane & 7;
  const T* zero = reinterpret_cast<const T*>(attn_zero_page);
  const T* kb = reinterpret_cast<const T*>(p.k) + (long)b * p.k_bs + (long)h * D;
  const T* vb = reinterpret_cast<const T*>(p.vt) + (long)b * p.vt_bs + ((long)h * D + dbase) * p.vt_ld;
  auto issue = [&](int kv0, int stage) {
    T* sK = sbase + stage * STAGE;
    T* sV = sK + K_ELEMS;
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int q = j * 4 + wave;                       // rows [8q, 8q+8) of the panel stack
      const int prow = 8 * q + lrow;
      const int r = prow & 31, panel = prow >> 5;
      const int d0 = panel * 64 + ((slot ^ ((r >> 1) & 7)) << 3);
      const T* src = kv0 + r < p.len ? kb + (long)(kv0 + r) * p.k_ld + d0 : zero;
      attn_dma16(src, sK + q * 512);
    }
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
      const int q = j * 4 + wave;
      const int R = 8 * q + lrow;                       // LDS row = the d pair 2R, 2R + 1
      const int ls = slot ^ ((R >> 1) & 7);
      const int d = 2 * R + (ls >> 2);
      const int c0 = kv0 + ((ls & 3) << 3);
      const T* src = c0 < p.len ? vb + (long)d * p.vt_ld + c0 : zero;
      attn_dma16(src, sV + q * 512);
    }
  };

  // per-lane LDS element offsets of the fragment reads; V^T: LDS row l31 >> 1 holds d = l31 in slots 4 (l31 & 1) .. + 3
  const int prow = attn_perm_row(l31);
  int kofs[4], vofs[2];
#pragma unroll
  for (int c = 0; c < 4; ++c) kofs[c] = attn_frag_ofs(prow, (prow >> 1) & 7, c, hi);
#pragma unroll
  for (int c = 0; c < 2; ++c) vofs[c] = (l31 >> 1) * 64 + (((((l31 & 1) << 2) + 2 * c + hi) ^ ((l31 >> 2) & 7)) << 3);

  const int nt_all = (p.len + WKV - 1) / WKV;
  // tiles [t0, nt) of this block: all of them, or split ks of p.splits (long product: nt_all * splits stays far below 2^31 anyway)
  const int t0 = SPLIT ? (int)((long)ks * nt_all / p.splits) : 0;
  const int nt = SPLIT ? (int)((long)(ks + 1) * nt_all / p.splits) : nt_all;
  issue(t0 * WKV, 0);
  for (int t = t0; t < nt; ++t) {
    const int st = (t - t0) & 1, kv0 = t * WKV;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 < nt) issue(kv0 + WKV, st ^ 1);
    const T* sK = sbase + st * STAGE;
    const T* sV = sK + K_ELEMS;

    // RAW scores of the 32-key tile for this lane's query: register r holds key kv0 + 16 (r >> 3) + 8 hi + (r & 7)
    f32x16 s[1];
    attn_qk<T>(s, sK, qf, kofs);
    if (kv0 + WKV > p.len) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kv0 + 16 * (r >> 3) + 8 * hi + (r & 7) >= p.len) s[0][r] = -INFINITY;
    }
    if constexpr (KMASK) {
      // the lane's 16 keys are two runs of 8: one 8-byte load of mask bytes each (len % 8 == 0: a run is inside len or wholly past it, where the
      // block above has already set -inf and nothing is read)
      const unsigned char* mp = p.kmask + (long)b * p.kmask_bs + kv0 + 8 * hi;
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        if (kv0 + 16 * cc + 8 * hi < p.len) {
          const unsigned long long mw = *reinterpret_cast<const unsigned long long*>(mp + 16 * cc);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if ((mw >> (8 * j)) & 0xff) s[0][8 * cc + j] = -INFINITY;
        }
      }
    }
    // m_run in RAW score units, exp2 arguments fma(s, c, -m c) with c = scale * log2(e) > 0.  The rescale of O is DO / 2 accumulator registers,
    // through v_accvgpr moves
    attn_lazy_max<false>(o, m_run, l_run, attn_tile_max(s), p.scale_log2);
    // KMASK: while every key so far was masked m_run is still -inf and fma(-inf, c, +inf) would be NaN; against the reference 0 such a tile's
    // probabilities are exp2(-inf) = 0 exactly, and the first finite tile rescales the (zero) accumulators by exp2(-inf) = 0
    const float mc = (KMASK && m_run == -INFINITY) ? 0.f : m_run * p.scale_log2;
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[0][r], p.scale_log2, -mc));
      s[0][r] = e;
      ps += e;
    }
    l_run += ps;
    attn_pv<T, 1024>(o, s, sV, vofs);             // accumulator tile t2 = 32 d = 16 LDS rows of d pairs
  }

  if constexpr (SPLIT) {
    // ---------------- partial: the UNNORMALISED accumulators, relative to m_run, as fp32 rows o[q][d] (4 consecutive d = one 16-byte store), and
    // (m_run in raw score units, l) per query row.  Every row of the 128-row block is written: the workspace has n_qblk * 128 rows per (split, batch, head)
    const long R = (long)p.n_qblk * 128;
    const long wrow = (((long)ks * p.batch + b) * p.heads + h) * R + qrow;
    float* wp = p.ws + wrow * D + dbase;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = o[t][4 * g + j];
        *reinterpret_cast<f32x4*>(wp + t * 32 + 8 * g + 4 * hi) = v;
      }
    const float l = attn_row_sum<false>(o, l_run, hi);
    if (hi == 0 && dbase == 0) {                  // the column parts of d = 512 hold the same (m, l): one of them stores
      f32x2 ml;
      ml[0] = m_run; ml[1] = l;
      *reinterpret_cast<f32x2*>(p.ws + (long)p.splits * p.batch * p.heads * R * D + wrow * 2) = ml;
    }
  } else {
    // ---------------- normalise and store: O^T regs -> out[b, q, h*D + dbase + d], 4 consecutive d per 8-byte store; rows >= n_q are not written
    const float l = attn_row_sum<false>(o, l_run, hi);
    attn_scale_acc(o, (KMASK && !(l > 0.f)) ? 0.f : 1.f / l);      // a row with every key masked is outside the contract: zeros, not NaN
    if (q_ok) attn_store(o, reinterpret_cast<T*>(p.out) + (long)b * p.out_bs + qrow * p.out_ld + (long)h * D + dbase, hi, DO);
  }
}

template <typename T, int D, int DO, bool SPLIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void attention_wide_kernel(WideParams p) {
  attention_wide_body<T, D, DO, SPLIT, false>(p);
}

// KMASK: the same loop with a key-padding mask (tg_attention_wide_kmask).  A kernel of its own name: the instances above keep theirs
template <typename T, int D, int DO, bool SPLIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void attention_wide_kmask_kernel(WideParams p) {
  attention_wide_body<T, D, DO, SPLIT, true>(p);
}

// Combine of the key-split partials: one thread per 4 consecutive output columns of one (batch, head, query < n_q); 16-byte loads of o, 8-byte stores of out
// (exactly the elements the unsplit kernel writes).  fp32 throughout, s ascending (deterministic), one rounding.
template <typename T, int D, bool KMASK>
__device__ __forceinline__ void attention_wide_combine_body(CombineParams p) {
  typedef typename Vec<T>::v4 V4;
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  constexpr int TPR = D / 4, RPB = 256 / TPR;    // threads per row, rows per block
  const int tid = threadIdx.x;
  const long row = (long)blockIdx.x * RPB + tid / TPR;          // over batch x heads x n_q, query fastest
  if (row >= p.total) return;
  const int c = (tid % TPR) * 4;
  const int q = (int)(row % p.n_q);
  const long bh = row / p.n_q;
  const int h = (int)(bh % p.heads), b = (int)(bh / p.heads);
  const long sstride = (long)p.batch * p.heads * p.rows;          // workspace rows per split
  const long r0 = bh * p.rows + q;
  const float* wo = p.ws;
  const float* wml = p.ws + (long)p.splits * sstride * D;
  float M = -INFINITY;
  for (int s = 0; s < p.splits; ++s) M = fmaxf(M, wml[(r0 + s * sstride) * 2]);
  f32x4 acc;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = 0.f;
  float den = 0.f;
  for (int s = 0; s < p.splits; ++s) {
    const long r = r0 + s * sstride;
    const f32x2 ml = *reinterpret_cast<const f32x2*>(wml + r * 2);
    float w = __builtin_amdgcn_exp2f((ml[0] - M) * p.scale_log2);                // 1 for the split that holds the max, exactly 0 far below it
    if (KMASK && ml[0] == -INFINITY) w = 0.f;                                    // a split whose keys are all masked (m = -inf, l = 0, o = 0); -inf - -inf is NaN
    const f32x4 v = *reinterpret_cast<const f32x4*>(wo + r * D + c);
    den = __builtin_fmaf(w, ml[1], den);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(w, v[j], acc[j]);
  }
  const float inv = (KMASK && !(den > 0.f)) ? 0.f : 1.f / den;                 // every key of the row masked: zeros (outside the contract)
  V4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = from_f32<T>(acc[j] * inv);
  *reinterpret_cast<V4*>(reinterpret_cast<T*>(p.out) + (long)b * p.out_bs + (long)q * p.out_ld + (long)h * D + c) = o;
}

template <typename T, int D>
__global__ __launch_bounds__(256) void attention_wide_combine_kernel(CombineParams p) {
  attention_wide_combine_body<T, D, false>(p);
}

template <typename T, int D>
__global__ __launch_bounds__(256) void attention_wide_combine_kmask_kernel(CombineParams p) {
  attention_wide_combine_body<T, D, true>(p);
}

// S = 1: the unsplit kernel, no workspace.  S > 1: the partial launch (grid x S) and the combine launch, in this order on `st`
template <typename T, int D, int DO, bool SPLIT, bool KMASK = false>
int launch_wide(const tg_attn_desc* d, hipStream_t st, int S, float* ws, const char* who, const unsigned char* kmask = nullptr, long kmask_bs = 0) {
  WideParams p{};
  p.heads = d->heads; p.n_q = d->n_q; p.n_qblk = (d->n_q + 127) / 128;
  p.q = d->q; p.q_ld = d->q_ld; p.q_bs = d->q_bs;
  p.k = d->k0; p.k_ld = d->k0_ld; p.k_bs = d->k0_bs;
  p.vt = d->vt0; p.vt_ld = d->vt0_ld; p.vt_bs = d->vt0_bs;
  p.len = d->len0;
  p.scale_log2 = d->scale * 1.4426950408889634f;
  p.out = d->out; p.out_ld = d->out_ld; p.out_bs = d->out_bs;
  p.batch = d->batch; p.splits = S; p.ws = ws;
  p.kmask = kmask; p.kmask_bs = kmask_bs;
  const size_t lds = (size_t)2 * ((D / 64) * 32 * 64 + DO * 32) * sizeof(T);
  const long blocks = (long)p.n_qblk * d->heads * d->batch * (D / DO) * S;
  TG_CHECK(blocks <= 0x7fffffffL, TG_ERR_ARG, "%s: problem too large for one launch", who);
  constexpr int RPB = 256 / (D / 4);
  const long total = (long)d->batch * d->heads * d->n_q, cblocks = (total + RPB - 1) / RPB;
  TG_CHECK(cblocks <= 0x7fffffffL, TG_ERR_ARG, "%s: problem too large for one launch", who);
  auto k = KMASK ? attention_wide_kmask_kernel<T, D, DO, SPLIT> : attention_wide_kernel<T, D, DO, SPLIT>;
  // the dynamic LDS of a stage pair (96 KiB at d = 512) is above the default limit: raised once per device, and a refusal is this call's error
  static bool raised[64] = {};       // one table per instantiation of launch_wide, KMASK included; no lock: two threads that race here only repeat the same idempotent attribute call
  int dev = 0;
  TG_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, TG_ERR_LAUNCH, "%s: no current device", who);
  if (!raised[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    TG_CHECK(e == hipSuccess, TG_ERR_LAUNCH, "%s: cannot reserve %zu bytes of LDS per workgroup: %s", who, lds, hipGetErrorString(e));
    raised[dev] = true;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), lds, st, p);
  TG_LAUNCH_CHECK();
  if constexpr (SPLIT) {
    CombineParams c{};
    c.batch = d->batch; c.heads = d->heads; c.n_q = d->n_q; c.rows = p.n_qblk * 128; c.splits = S;
    c.total = total;
    c.ws = ws;
    c.scale_log2 = p.scale_log2;
    c.out = d->out; c.out_ld = d->out_ld; c.out_bs = d->out_bs;
    if constexpr (KMASK) hipLaunchKernelGGL((attention_wide_combine_kmask_kernel<T, D>), dim3((unsigned)cblocks), dim3(256), 0, st, c);
    else hipLaunchKernelGGL((attention_wide_combine_kernel<T, D>), dim3((unsigned)cblocks), dim3(256), 0, st, c);
    TG_LAUNCH_CHECK();
  }
  return TG_OK;
}

template <bool SPLIT>
int dispatch_wide(const tg_attn_desc* d, hipStream_t st, int S, float* ws, const char* who, const unsigned char* kmask = nullptr, long kmask_bs = 0) {
  const bool bf = d->dtype == TG_BF16;
  if (kmask) {
    if (d->head_dim == 256)
      return bf ? launch_wide<bf16_t, 256, 256, SPLIT, true>(d, st, S, ws, who, kmask, kmask_bs) : launch_wide<f16_t, 256, 256, SPLIT, true>(d, st, S, ws, who, kmask, kmask_bs);
    return bf ? launch_wide<bf16_t, 512, 256, SPLIT, true>(d, st, S, ws, who, kmask, kmask_bs) : launch_wide<f16_t, 512, 256, SPLIT, true>(d, st, S, ws, who, kmask, kmask_bs);
  }
  if (d->head_dim == 256) return bf ? launch_wide<bf16_t, 256, 256, SPLIT>(d, st, S, ws, who) : launch_wide<f16_t, 256, 256, SPLIT>(d, st, S, ws, who);
  return bf ? launch_wide<bf16_t, 512, 256, SPLIT>(d, st, S, ws, who) : launch_wide<f16_t, 512, 256, SPLIT>(d, st, S, ws, who);
}

// every check of the descriptor, on the host, in the documented order; `who` names the entry point in tg_last_error
int validate_wide(const tg_attn_desc* d, const char* who) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "%s: null descriptor", who);
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "%s: bad dtype", who);
  TG_CHECK(d->head_dim == 256 || d->head_dim == 512, TG_ERR_UNSUPPORTED,
           "%s: head_dim %d unsupported (256 or 512; tg_attention takes multiples of 8 up to 160)", who, d->head_dim);
  TG_CHECK(d->len1 == 0 && d->causal == 0 && d->mask == nullptr && d->w1_dev == nullptr, TG_ERR_UNSUPPORTED,
           "%s: one unmasked softmax segment only (len1 = 0, no causal, no mask, no w1_dev)", who);
  TG_CHECK(d->batch > 0 && d->heads > 0 && d->n_q > 0 && d->len0 > 0, TG_ERR_ARG, "%s: empty problem", who);
  TG_CHECK(d->len0 % 8 == 0, TG_ERR_ARG, "%s: len0 (%d) must be a multiple of 8", who, d->len0);
  TG_CHECK(d->scale > 0.f, TG_ERR_ARG, "%s: scale must be > 0", who);
  TG_CHECK(d->q && d->k0 && d->vt0 && d->out, TG_ERR_ARG, "%s: null q/k0/vt0/out", who);
  TG_CHECK(d->q_ld % 8 == 0 && d->k0_ld % 8 == 0 && d->vt0_ld % 8 == 0 && d->out_ld % 4 == 0, TG_ERR_ARG,
           "%s: pitches must keep 16-byte alignment", who);
  TG_CHECK(d->batch == 1 || (d->q_bs % 8 == 0 && d->k0_bs % 8 == 0 && d->vt0_bs % 8 == 0 && d->out_bs % 4 == 0), TG_ERR_ARG,
           "%s: batch strides must keep 16-byte alignment (q_bs, k0_bs, vt0_bs multiples of 8, out_bs of 4)", who);
  return TG_OK;
}

inline long wide_tiles(const tg_attn_desc* d) { return ((long)d->len0 + WKV - 1) / WKV; }
inline long wide_blocks(const tg_attn_desc* d) { return (((long)d->n_q + 127) / 128) * d->heads * d->batch * (d->head_dim == 512 ? 2 : 1); }

inline long wide_ws_bytes(const tg_attn_desc* d, long S) {
  return S * d->batch * d->heads * ((((long)d->n_q + 127) / 128) * 128) * (d->head_dim + 2) * (long)sizeof(float);
}

// The planner (requested == 0): 256 CUs at one workgroup per CU (the constant of tg_gemm_route.hip).  Cost of S splits = rounds of the grid x tiles a block
// walks = ceil(blocks S / 256) ceil(nt / S); the smallest S in 1 .. kSplitMax with the lowest cost, every split keeping >= kSplitMinTiles tiles and the
// grid at most two rounds (blocks S <= 512).  blocks >= 256 is S = 1.  A function of (batch, heads, head_dim, n_q, len0) alone.
constexpr long kCUs = 256, kSplitMax = 8, kSplitMinTiles = 8;

int plan_splits(const tg_attn_desc* d) {
  const long blocks = wide_blocks(d), nt = wide_tiles(d);
  if (blocks >= kCUs) return 1;
  long best = 1, best_cost = ((blocks + kCUs - 1) / kCUs) * nt;
  for (long S = 2; S <= kSplitMax; ++S) {
    if (S > nt || nt / S < kSplitMinTiles || blocks * S > 2 * kCUs) break;
    const long cost = ((blocks * S + kCUs - 1) / kCUs) * ((nt + S - 1) / S);
    if (cost < best_cost) { best = S; best_cost = cost; }
  }
  return (int)best;
}

}  // namespace

extern "C" int tg_attention_wide(const tg_attn_desc* d, void* stream) {
  const int rc = validate_wide(d, "tg_attention_wide");
  if (rc != TG_OK) return rc;
  return dispatch_wide<false>(d, reinterpret_cast<hipStream_t>(stream), 1, nullptr, "tg_attention_wide");
}

extern "C" int tg_attention_wide_splits(const tg_attn_desc* d, int32_t requested) {
  const int rc = validate_wide(d, "tg_attention_wide_splits");
  if (rc != TG_OK) return rc;
  TG_CHECK(requested >= 0, TG_ERR_ARG, "tg_attention_wide_splits: requested (%d) must be >= 0", requested);
  const long nt = wide_tiles(d);
  long S = requested;
  if (requested == 0) {
    // dev knob for A/Bs, read per call and never cached (as the GEMM planner's): TG_ATTN_WIDE_SPLIT=n forces n splits where the planner is asked
    const char* e = getenv("TG_ATTN_WIDE_SPLIT");
    const long forced = e ? strtol(e, nullptr, 0) : 0;
    S = forced >= 1 ? forced : plan_splits(d);
  }
  return (int)(S < nt ? S : nt);
}

extern "C" int64_t tg_attention_wide_workspace_bytes(const tg_attn_desc* d, int32_t splits) {
  if (validate_wide(d, "tg_attention_wide_workspace_bytes") != TG_OK) return 0;
  const long nt = wide_tiles(d), S = splits < nt ? splits : nt;
  return S <= 1 ? 0 : wide_ws_bytes(d, S);
}

extern "C" int tg_attention_wide_split(const tg_attn_desc* d, int32_t splits, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = validate_wide(d, "tg_attention_wide_split");
  if (rc != TG_OK) return rc;
  TG_CHECK(splits >= 1, TG_ERR_ARG, "tg_attention_wide_split: splits (%d) must be >= 1 (ask tg_attention_wide_splits for the planner's choice)", splits);
  const long nt = wide_tiles(d), S = splits < nt ? splits : nt;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (S == 1) return dispatch_wide<false>(d, st, 1, nullptr, "tg_attention_wide_split");          // the unsplit kernel: no workspace is touched
  TG_CHECK(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, TG_ERR_ARG,
           "tg_attention_wide_split: workspace must be non-null and 16-byte aligned");
  const long need = wide_ws_bytes(d, S);
  TG_CHECK(workspace_bytes >= need, TG_ERR_ARG, "tg_attention_wide_split: workspace of %lld bytes, %d splits need %ld", (long long)workspace_bytes, (int)S, need);
  return dispatch_wide<true>(d, st, (int)S, static_cast<float*>(workspace), "tg_attention_wide_split");
}

extern "C" int tg_attention_wide_kmask(const tg_attn_desc* d, const uint8_t* key_mask, int64_t key_mask_bs, int32_t splits, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  const char* who = "tg_attention_wide_kmask";
  const int rc = validate_wide(d, who);
  if (rc != TG_OK) return rc;
  TG_CHECK(key_mask != nullptr && (reinterpret_cast<uintptr_t>(key_mask) & 7) == 0, TG_ERR_ARG, "%s: key_mask must be non-null and 8-byte aligned", who);
  TG_CHECK(d->batch == 1 || (key_mask_bs >= d->len0 && key_mask_bs % 8 == 0), TG_ERR_ARG,
           "%s: key_mask_bs (%lld) must cover len0 and be a multiple of 8", who, (long long)key_mask_bs);
  TG_CHECK(splits >= 1, TG_ERR_ARG, "%s: splits (%d) must be >= 1 (ask tg_attention_wide_splits for the planner's choice)", who, splits);
  const long nt = wide_tiles(d), S = splits < nt ? splits : nt;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (S == 1) return dispatch_wide<false>(d, st, 1, nullptr, who, key_mask, key_mask_bs);
  TG_CHECK(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, TG_ERR_ARG, "%s: workspace must be non-null and 16-byte aligned", who);
  const long need = wide_ws_bytes(d, S);
  TG_CHECK(workspace_bytes >= need, TG_ERR_ARG, "%s: workspace of %lld bytes, %d splits need %ld", who, (long long)workspace_bytes, (int)S, need);
  return dispatch_wide<true>(d, st, (int)S, static_cast<float*>(workspace), who, key_mask, key_mask_bs);
}
