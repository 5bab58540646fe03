// Flash attention for WIDE heads on MFMA for gfx950 (include/theatergen_hip.h: tg_attention_wide): head_dim 256 / 512, one softmax segment
//
//   O = softmax(s Q K^T) V
//
// The VAE mid block's single-head d = C = 512 attention (theatergen_amd/vae.py) is the user: 4096 tokens at 512 x 512, 16384 at 1024 x 1024.  Nothing
// [n_q, len] exists in memory; scores are fp32 from the stored Q and K, the softmax is online (running max / sum in fp32), P is rounded to the storage dtype
// where it enters the PV product (as tg_attention does) and O is accumulated in fp32 and rounded once.
//
// Same formulation as tg_attention.hip (read its header first): everything is computed TRANSPOSED so that lane & 31 is the query,
//   S^T[key][q]  = mfma32x32x16(A = K rows,   B = Q rows)
//   O^T[d][q]   += mfma32x32x16(A = V^T rows, B = P^T)         P^T straight from the S^T registers (permuted key rows, one ds_read_b128 per fragment)
// block = 4 waves x 32 queries, K and V^T tiles staged once per block by LDS-DMA and shared by the four waves, two stages.
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
#include "tg_common.h"

namespace {

constexpr int WKV = 32;        // keys per tile

__device__ __attribute__((aligned(256))) unsigned char attn_wide_zero_page[256];

struct WideParams {
  int heads, n_q, n_qblk;
  const void* q; long q_ld, q_bs;
  const void* k; long k_ld, k_bs;
  const void* vt; long vt_ld, vt_bs;
  int len;
  float scale_log2;
  void* out; long out_ld, out_bs;
};

template <typename T, int D, int DO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void attention_wide_kernel(WideParams p) {
  typedef typename Vec<T>::v8 V8;
  typedef typename Vec<T>::v4 V4;
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
  // XCD-aware block order (speed only, as tg_attention): each XCD gets a contiguous chunk of the (batch, head, q-block, column part) space, so the
  // blocks that read one (batch, head)'s K / V^T share ONE private L2
  int lbid;
  {
    const int nb = gridDim.x, q8 = nb >> 3, r8 = nb & 7, xcd = blockIdx.x & 7;
    lbid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
  }
  const int dbase = (lbid % NSPLIT) * DO;        // first output column of this block
  const int lq = lbid / NSPLIT;
  const int qblk = lq % p.n_qblk;
  const int h = (lq / p.n_qblk) % p.heads, b = lq / (p.n_qblk * p.heads);
  const long qrow = (long)qblk * 128 + wave * 32 + l31;
  const bool q_ok = qrow < p.n_q;

  // Q fragments (B operand): this lane's query row, d = ks*16 + hi*8 .. +8; rows >= n_q are not read
  V8 qf[NKS];
  {
    const T* qp = reinterpret_cast<const T*>(p.q) + (long)b * p.q_bs + qrow * p.q_ld + (long)h * D;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      V8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = from_f32<T>(0.f);
      if (q_ok) v = *reinterpret_cast<const V8*>(qp + ks * 16 + hi * 8);
      qf[ks] = v;
    }
  }

  f32x16 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // ---- LDS-DMA tile loader
  const int lrow = lane >> 3, slot = lane & 7;
  const T* zero = reinterpret_cast<const T*>(attn_wide_zero_page);
  auto dma = [&](const T* src, T* lds_row_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_row_base, 16, 0, 0);
  };
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
      dma(src, sK + q * 512);
    }
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
      const int q = j * 4 + wave;
      const int R = 8 * q + lrow;                       // LDS row = the d pair 2R, 2R + 1
      const int ls = slot ^ ((R >> 1) & 7);
      const int d = 2 * R + (ls >> 2);
      const int c0 = kv0 + ((ls & 3) << 3);
      const T* src = c0 < p.len ? vb + (long)d * p.vt_ld + c0 : zero;
      dma(src, sV + q * 512);
    }
  };

  // per-lane LDS element offsets of the fragment reads (they only depend on the lane).  KEY PERMUTATION as in tg_attention.hip: MFMA row i of the score
  // tile is fed K row perm(i) = i with bits 2 and 3 swapped, so accumulator registers 8c .. 8c+7 hold the 8 CONSECUTIVE keys 16c + 8 hi + 0..7 and the
  // P^T fragment of chunk c pairs with ONE 16-byte V^T slot
  const int prow = (l31 & 19) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
  const int pkey = (prow >> 1) & 7;
  int kofs[4], vofs[2];
#pragma unroll
  for (int c = 0; c < 4; ++c) kofs[c] = prow * 64 + (((2 * c + hi) ^ pkey) << 3);
#pragma unroll
  for (int c = 0; c < 2; ++c) vofs[c] = (l31 >> 1) * 64 + (((((l31 & 1) << 2) + 2 * c + hi) ^ ((l31 >> 2) & 7)) << 3);

  const int nt = (p.len + WKV - 1) / WKV;
  issue(0, 0);
  for (int t = 0; t < nt; ++t) {
    const int st = t & 1, kv0 = t * WKV;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 < nt) issue(kv0 + WKV, st ^ 1);
    const T* sK = sbase + st * STAGE;
    const T* sV = sK + K_ELEMS;

    // RAW scores of the 32-key tile for this lane's query: register r holds key kv0 + 16 (r >> 3) + 8 hi + (r & 7)
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const V8 kf = *reinterpret_cast<const V8*>(sK + kofs[ks & 3] + (ks >> 2) * 2048);
      s = mfma32(kf, qf[ks], s);
    }
    if (kv0 + WKV > p.len) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kv0 + 16 * (r >> 3) + 8 * hi + (r & 7) >= p.len) s[r] = -INFINITY;
    }
    float tm;
    {
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
      // the other 16 keys of the row live in lane ^ 32 (inline asm and s_nop: see tile_max in tg_attention.hip)
      float a = mx, b2 = mx;
      asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b2));
      tm = fmaxf(a, b2);
    }
    // m_run in RAW score units, exp2 arguments fma(s, c, -m c) with c = scale * log2(e) > 0.  LAZY RUNNING MAX as in tg_attention.hip: O (DO / 2
    // accumulator registers, through v_accvgpr moves) is only rescaled when some row's tile max exceeds the reference by more than 2^LAZY_LOG2;
    // until then probabilities are at most 2^8 against the stale reference, which P's storage dtype and the fp32 accumulators hold
    constexpr float LAZY_LOG2 = 8.f;
    if (__any(tm * p.scale_log2 > m_run * p.scale_log2 + LAZY_LOG2)) {
      const float m_new = fmaxf(m_run, tm);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);     // first tile: exp2(-inf) = 0 on a zero accumulator
#pragma unroll
      for (int t2 = 0; t2 < DT; ++t2)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t2][r] *= alpha;
      l_run *= alpha;
      m_run = m_new;
    }
    const float mc = m_run * p.scale_log2;
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], p.scale_log2, -mc));
      s[r] = e;
      ps += e;
    }
    l_run += ps;
    // O^T += V^T * P^T: chunk c covers keys 16c + 8 hi + 0..7 = logical slot 2c + hi of the d row
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      V8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = from_f32<T>(s[8 * c + j]);
#pragma unroll
      for (int t2 = 0; t2 < DT; ++t2) {
        const V8 vf = *reinterpret_cast<const V8*>(sV + vofs[c] + t2 * 1024);
        o[t2] = mfma32(vf, pf, o[t2]);
      }
    }
  }

  // ---------------- normalise and store: O^T regs -> out[b, q, h*D + dbase + d], 4 consecutive d per 8-byte store; rows >= n_q are not written
  const float inv = 1.f / (l_run + __shfl_xor(l_run, 32, 64));
  if (q_ok) {
    T* op = reinterpret_cast<T*>(p.out) + (long)b * p.out_bs + qrow * p.out_ld + (long)h * D + dbase;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        V4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = from_f32<T>(o[t][4 * g + j] * inv);
        *reinterpret_cast<V4*>(op + t * 32 + 8 * g + 4 * hi) = v;
      }
  }
}

template <typename T, int D, int DO>
int launch_wide(const tg_attn_desc* d, hipStream_t st) {
  WideParams p{};
  p.heads = d->heads; p.n_q = d->n_q; p.n_qblk = (d->n_q + 127) / 128;
  p.q = d->q; p.q_ld = d->q_ld; p.q_bs = d->q_bs;
  p.k = d->k0; p.k_ld = d->k0_ld; p.k_bs = d->k0_bs;
  p.vt = d->vt0; p.vt_ld = d->vt0_ld; p.vt_bs = d->vt0_bs;
  p.len = d->len0;
  p.scale_log2 = d->scale * 1.4426950408889634f;
  p.out = d->out; p.out_ld = d->out_ld; p.out_bs = d->out_bs;
  const size_t lds = (size_t)2 * ((D / 64) * 32 * 64 + DO * 32) * sizeof(T);
  const long blocks = (long)p.n_qblk * d->heads * d->batch * (D / DO);
  TG_CHECK(blocks <= 0x7fffffffL, TG_ERR_ARG, "tg_attention_wide: problem too large for one launch");
  auto k = attention_wide_kernel<T, D, DO>;
  // the dynamic LDS of a stage pair (96 KiB at d = 512) is above the default limit: raised once per device, and a refusal is this call's error
  static bool raised[64] = {};       // no lock: two threads that race here only repeat the same idempotent attribute call
  int dev = 0;
  TG_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, TG_ERR_LAUNCH, "tg_attention_wide: no current device");
  if (!raised[dev]) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    TG_CHECK(e == hipSuccess, TG_ERR_LAUNCH, "tg_attention_wide: cannot reserve %zu bytes of LDS per workgroup: %s", lds, hipGetErrorString(e));
    raised[dev] = true;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), lds, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

}  // namespace

extern "C" int tg_attention_wide(const tg_attn_desc* d, void* stream) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_attention_wide: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_attention_wide: bad dtype");
  TG_CHECK(d->head_dim == 256 || d->head_dim == 512, TG_ERR_UNSUPPORTED,
           "tg_attention_wide: head_dim %d unsupported (256 or 512; tg_attention takes multiples of 8 up to 160)", d->head_dim);
  TG_CHECK(d->len1 == 0 && d->causal == 0 && d->mask == nullptr && d->w1_dev == nullptr, TG_ERR_UNSUPPORTED,
           "tg_attention_wide: one unmasked softmax segment only (len1 = 0, no causal, no mask, no w1_dev)");
  TG_CHECK(d->batch > 0 && d->heads > 0 && d->n_q > 0 && d->len0 > 0, TG_ERR_ARG, "tg_attention_wide: empty problem");
  TG_CHECK(d->len0 % 8 == 0, TG_ERR_ARG, "tg_attention_wide: len0 (%d) must be a multiple of 8", d->len0);
  TG_CHECK(d->scale > 0.f, TG_ERR_ARG, "tg_attention_wide: scale must be > 0");
  TG_CHECK(d->q && d->k0 && d->vt0 && d->out, TG_ERR_ARG, "tg_attention_wide: null q/k0/vt0/out");
  TG_CHECK(d->q_ld % 8 == 0 && d->k0_ld % 8 == 0 && d->vt0_ld % 8 == 0 && d->out_ld % 4 == 0, TG_ERR_ARG,
           "tg_attention_wide: pitches must keep 16-byte alignment");
  TG_CHECK(d->batch == 1 || (d->q_bs % 8 == 0 && d->k0_bs % 8 == 0 && d->vt0_bs % 8 == 0 && d->out_bs % 4 == 0), TG_ERR_ARG,
           "tg_attention_wide: batch strides must keep 16-byte alignment (q_bs, k0_bs, vt0_bs multiples of 8, out_bs of 4)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool bf = d->dtype == TG_BF16;
  if (d->head_dim == 256) return bf ? launch_wide<bf16_t, 256, 256>(d, st) : launch_wide<f16_t, 256, 256>(d, st);
  return bf ? launch_wide<bf16_t, 512, 256>(d, st) : launch_wide<f16_t, 512, 256>(d, st);
}
