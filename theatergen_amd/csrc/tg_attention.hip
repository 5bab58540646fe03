// Flash-style fused attention on MFMA for gfx950 (include/theatergen_hip.h: tg_attention, tg_attn_probs).
//
//   O = softmax(s Q K0^T) V0  +  w1 * softmax(s Q K1^T) V1        (segment 1 optional, len1 <= 64)
//
// No [B*h, N, Lk] probability tensor ever reaches HBM (the reference materialises it three times:
// ip_adapter/attention_processor.py:187-219).  Segment 1 is IP-Adapter's image-token K/V: it gets its OWN
// softmax (two independent normalisations, attention_processor.py:482, :503, :516) — its K/V tile is staged in
// the same LDS buffers right after the text segment and folded into the same accumulator as
// (w1 / l1) * exp(s1 - m1), so decoupled cross-attention costs one extra tile, not a second kernel.
//
// Work split: block = 4 waves x 32 queries; K tile [64 keys][d] and V^T tile [d][64 keys] in LDS, shared by
// the 4 waves, everything computed transposed.  tg_attn_fwd.h explains the formulation, the swizzle, the key
// permutation, the permlane exchange and the lazy running max, and holds the pieces shared with tg_attention_wide.hip
// and tg_attention_relpos.hip.  Every kernel of THIS file must keep its assembly when such a piece moves
// (scripts/dev_isa_diff.py): a piece that does not survive the move keeps its copy here and names the header function.
// head_dim 40 / 80 (SD-1.5) are zero-padded to 48 / 80 for QK^T (K of the MFMA) and 64 / 96 rows for PV.
#include "tg_attn_fwd.h"

namespace {

constexpr int KV = 64;        // keys per tile

// FOLD variants: K's first padding column (d = head dim) is fed 1.0 so that the QK^T MFMA adds the query's running-max bias
__device__ __attribute__((aligned(256))) const unsigned short attn_one0_bf16[8] = {0x3F80, 0, 0, 0, 0, 0, 0, 0};
__device__ __attribute__((aligned(256))) const unsigned short attn_one0_f16[8] = {0x3C00, 0, 0, 0, 0, 0, 0, 0};
template <typename T> __device__ __forceinline__ const T* one0_page();
template <> __device__ __forceinline__ const bf16_t* one0_page<bf16_t>() { return reinterpret_cast<const bf16_t*>(attn_one0_bf16); }
template <> __device__ __forceinline__ const f16_t* one0_page<f16_t>() { return reinterpret_cast<const f16_t*>(attn_one0_f16); }

struct AttnParams {
  int heads, hd, n_q, n_qblk;
  const void* q; long q_ld, q_bs;
  const void* k0; long k0_ld, k0_bs;
  const void* vt0; long vt0_ld, vt0_bs;
  int len0;
  const void* k1; long k1_ld, k1_bs;
  const void* vt1; long vt1_ld, vt1_bs;
  int len1;
  float scale_log2;
  float w1;
  const float* w1_dev;
  int w1_stride;                 // 0: w1_dev is one float; 1: one float per batch item (tg_attention_ps)
  void* out; long out_ld, out_bs;
  int causal;
  const float* mask; long mask_bs, mask_hs, mask_qs;   // MASK instances: additive score bias mask[b*bs + h*hs + q*qs + key] (fp32, score units)
  float inv_scale;
};

// Data path: K tile = NP panels of [64 keys][64 d] and V^T tile = [DV d][64 keys], swizzled 128-byte LDS rows filled by
// LDS-DMA.  Two stages: the DMA of tile t+1 is in flight while tile t is multiplied, one barrier per tile.
// ONES (variants whose DV exceeds the head dim; attn_row_sum): the PV MFMA accumulates the softmax denominator — the loop
// is VALU-bound (32 v_exp_f32 at quarter rate + ~100 other VALU ops against 14 MFMAs per wave-tile at head dim 40), so
// every removed VALU instruction counts.
// FOLD (head dim = DPAD - 8, i.e. 40 -> 48: the SD-1.5 level-0 layers that dominate attention time): the loop is VALU-bound and a
// quarter of its VALU instructions were the `fma(s, scale, -max)` in front of every exp2.  Q is pre-multiplied by scale * log2(e)
// once per block, and the spare K column of the padded QK^T contraction carries 1.0 while the query's spare element carries
// -(running reference) — so the MFMA itself delivers exp2's argument and the 32 fmas per tile disappear.  The reference is a
// storage-dtype value (softmax is invariant to it); it moves lazily as before, and a move shifts the current tile's scores by the
// exact difference of the two representable values.
// MASK (own instantiations, never the hot path): `attention_mask` of the diffusers processors — an additive bias on segment 0's scores
// (`baddbmm(mask, q, k^T, beta=1, alpha=scale)`, ip_adapter/attention_processor.py:193-206), broadcast over heads and / or queries by
// zero strides.  It is added in raw-score units (mask / scale) right after the QK^T tile, so the online softmax is unchanged.
template <typename T, int DPAD, int DV, bool ONES, bool FOLD, bool MASK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DV <= 64 ? 3 : (DV <= 96 ? 2 : 1)))) void attention_kernel(AttnParams p) {
  typedef typename Vec<T>::v8 V8;
  constexpr int NP = (DPAD + 63) / 64;          // K panels
  constexpr int NKS = DPAD / 16;
  constexpr int DT = DV / 32;
  constexpr int KJ = NP * 2;                    // K DMA instructions per wave per tile (8 rows x 8 slots each)
  constexpr int VJ = DV / 32;                   // V^T DMA instructions per wave per tile
  constexpr int K_ELEMS = NP * 64 * 64;
  constexpr int STAGE = K_ELEMS + DV * 64;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sbase = reinterpret_cast<T*>(smem);         // [2][ K: NP x 64 x 64 | V^T: DV x 64 ]

  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lbid = attn_xcd_block();             // over (batch, head, q-block), q-block fastest
  const int qblk = lbid % p.n_qblk;
  const int h = (lbid / p.n_qblk) % p.heads, b = lbid / (p.n_qblk * p.heads);
  const int HD = p.hd;
  const long qrow = (long)qblk * 128 + wave * 32 + l31;
  const bool q_ok = qrow < p.n_q;

  // Q fragments (B operand): this lane's query row, d = ks*16 + hi*8 .. +8
  V8 qf[NKS];
  {
    const T* qp = reinterpret_cast<const T*>(p.q) + (long)b * p.q_bs + qrow * p.q_ld + (long)h * HD;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int d = ks * 16 + hi * 8;
      V8 v = attn_q_frag(qp + d, q_ok && d < HD);
      if constexpr (FOLD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = from_f32<T>(to_f32<T>(v[j]) * p.scale_log2);
      }
      qf[ks] = v;
    }
  }
  float qbias = 0.f;                       // FOLD: value of the query's spare element qf[NKS - 1][0] (lanes hi = 1) = -reference, log2 units

  f32x16 o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // ---- LDS-DMA tile loader
  const int lrow_lane = lane >> 3, slot_lane = lane & 7;
  const T* zero = reinterpret_cast<const T*>(attn_zero_page);
  // mirrors attn_issue_tile (tg_attn_fwd.h), plus the FOLD page
  auto issue = [&](const T* kb, long k_ld, const T* vb, long vt_ld, int len, int kv0, int stage) {
    T* sK = sbase + stage * STAGE;
    T* sV = sK + K_ELEMS;
    // the lane's row and slot through an empty asm: the compiler must derive this call's addresses here, where they are used.  Otherwise it
    // hoists the tile-invariant part of every request of every call site out of the tile loop and holds it in registers across the loop
    // (2 per request, for a path that only ragged tiles and segment 1 take now; no instruction is emitted for the asm)
    int lrow = lrow_lane, slot = slot_lane;
    asm volatile("" : "+v"(lrow), "+v"(slot));
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int q = j * 4 + wave;                       // rows [8q, 8q+8) of the panel stack
      const int prow = 8 * q + lrow;
      const int r = prow & 63, panel = prow >> 6;
      const int d0 = panel * 64 + ((slot ^ ((r >> 1) & 7)) << 3);
      const bool ok = d0 < HD && kv0 + r < len;
      const T* src = ok ? kb + (long)(kv0 + r) * k_ld + d0 : zero;
      if (FOLD && d0 == HD) src = one0_page<T>();
      attn_dma16(src, sK + q * 512);
    }
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
      const int q = j * 4 + wave;
      const int d = 8 * q + lrow;
      const int c0 = kv0 + ((slot ^ ((d >> 1) & 7)) << 3);
      const T* src = (d < HD && c0 < len) ? vb + (long)d * vt_ld + c0 : zero;
      if (ONES && d == DV - 1) src = ones_page<T>();
      attn_dma16(src, sV + q * 512);
    }
  };
  // FULL tiles of segment 0 (kv0 + KV <= len0, not causal): nothing of a request's source address changes from tile to tile except a
  // uniform stride (KV rows of K, KV columns of V^T), and which lanes read a constant page (head-dim padding, the FOLD / ONES pages) is fixed
  // for the kernel.  So each request keeps a RUNNING source pointer: a full tile issues straight from it and advances it — no 64-bit
  // multiply, no key-range compare, no page select in the tile loop (the loop is VALU-bound; `issue` costs 11 VALU instructions a request).
  // Page lanes stay put: a K request's page lanes depend on the lane (d0 >= HD; the same lanes for both requests of a panel), so the K
  // stride is a per-lane byte count, one register pair per panel, 0 on page lanes; a V^T request is all tensor or all page (HD is a multiple
  // of 8, the request's rows start at a multiple of 8), so its stride is a scalar.  Ragged tiles, causal launches and segment 1 go
  // through `issue`; the pointers advance once per staged tile, so they are those of the tile to stage whenever that tile is full.
  const T* kb0 = reinterpret_cast<const T*>(p.k0) + (long)b * p.k0_bs + (long)h * HD;
  const T* vb0 = reinterpret_cast<const T*>(p.vt0) + (long)b * p.vt0_bs + (long)h * HD * p.vt0_ld;
  const bool fast = p.causal == 0;
  const T* kp[KJ];
  const T* vp[VJ];
  unsigned long kstep[NP], vstep[VJ];
#pragma unroll
  for (int j = 0; j < KJ; ++j) {
    const int q = j * 4 + wave;
    const int prow = 8 * q + lrow_lane;
    const int r = prow & 63, panel = prow >> 6;
    const int d0 = panel * 64 + ((slot_lane ^ ((r >> 1) & 7)) << 3);
    kp[j] = d0 < HD ? kb0 + (long)r * p.k0_ld + d0 : ((FOLD && d0 == HD) ? one0_page<T>() : zero);
    if ((j & 1) == 0) kstep[j >> 1] = d0 < HD ? (unsigned long)p.k0_ld * (KV * sizeof(T)) : 0ul;      // panel = j >> 1
  }
#pragma unroll
  for (int j = 0; j < VJ; ++j) {
    const int q = j * 4 + wave;
    const int d = 8 * q + lrow_lane;
    vp[j] = d < HD ? vb0 + (long)d * p.vt0_ld + ((slot_lane ^ ((d >> 1) & 7)) << 3) : ((ONES && d == DV - 1) ? ones_page<T>() : zero);
    vstep[j] = 8 * q < HD ? KV * sizeof(T) : 0ul;
  }
  // the advance as one tied instruction, pointer += bytes in place (`bytes`: a lane value for K, a scalar for V^T).  Written as `ptr + bytes` the
  // allocator keeps the old and the new pointer in different registers and pays a 64-bit move per request and tile
  auto bump_v = [](const T*& ptr, unsigned long bytes) { asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(ptr) : "v"(bytes)); };
  auto bump_s = [](const T*& ptr, unsigned long bytes) { asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(ptr) : "s"(bytes)); };
  auto issue_full = [&](int stage) {
    T* sK = sbase + stage * STAGE;
    T* sV = sK + K_ELEMS;
#pragma unroll
    for (int j = 0; j < KJ; ++j) attn_dma16(kp[j], sK + (j * 4 + wave) * 512);
#pragma unroll
    for (int j = 0; j < VJ; ++j) attn_dma16(vp[j], sV + (j * 4 + wave) * 512);
  };
  // on to the next tile.  Once per staged tile of segment 0, full or not and outside any branch (a branch around it is what makes the allocator
  // split the pointers' registers); pointers that have run past the last full tile are not used again
  auto advance = [&]() {
#pragma unroll
    for (int j = 0; j < KJ; ++j) bump_v(kp[j], kstep[j >> 1]);
#pragma unroll
    for (int j = 0; j < VJ; ++j) bump_s(vp[j], vstep[j]);
  };
  // segment 0's tile at keys kv0 .. kv0 + KV into `stage`
  auto issue0 = [&](int kv0, int stage) {
    if (fast && kv0 + KV <= p.len0) issue_full(stage);
    else issue(kb0, p.k0_ld, vb0, p.vt0_ld, p.len0, kv0, stage);
  };
  // the V^T fix-up of a ragged tile: only text 77 = 64 + 13 keys and 4 image tokens take this path
  auto fixup_v = [&](int rem, int stage) {
    if (tid < DV && tid < HD) attn_zero_vt_tail(sbase + stage * STAGE + K_ELEMS, tid, rem);
  };

  const int skey = (l31 >> 1) & 7;                       // swizzle key of this lane's fragment rows
  // per-lane LDS element offsets of the fragment reads (the keys are derived here, in this order: the assembly depends on it)
  const int prow = attn_perm_row(l31);
  const int pkey = (prow >> 1) & 7;
  int kofs[4], vofs[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) kofs[c] = attn_frag_ofs(prow, pkey, c, hi);
#pragma unroll
  for (int c = 0; c < 4; ++c) vofs[c] = attn_frag_ofs(l31, skey, c, hi);
  // RAW scores of one 64-key tile for this lane's query (the softmax scale is folded into the exp2 argument by one
  // fma per element); keys >= len are masked to -inf only on a ragged tile, full tiles take no compare/select at all.
  auto scores = [&](f32x16 (&s)[2], const T* sK, int len, int kv0, bool causal) {
    attn_qk<T>(s, sK, qf, kofs);
    if (kv0 + KV > len || causal) {
      // ragged tile and / or causal mask (key j visible to query i iff j <= i: key 0 is always visible, so a row's running
      // max is finite from the first tile on and fully masked later tiles contribute exp2(-inf) = 0)
      const int qmax = causal ? (int)qrow : 0x7fffffff;
#pragma unroll
      for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + kvt * 32 + 16 * (r >> 3) + 8 * hi + (r & 7);     // key held by register r (permuted rows)
          if (kv >= len || kv > qmax) s[kvt][r] = -INFINITY;
        }
    }
  };

  const T* kb1 =reinterpret_cast<const T*>(p.k1) + (long)b * p.k1_bs + (long)h * HD;
  const T* vb1 = reinterpret_cast<const T*>(p.vt1) + (long)b * p.vt1_bs + (long)h * HD * p.vt1_ld;

  // ---------------- segment 0: online softmax over len0 keys
  const int nt0 = (p.len0 + KV - 1) / KV;
  issue0(0, 0);
  advance();
  for (int t = 0; t < nt0; ++t) {
    const int st = t & 1, kv0 = t * KV;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kv0 + KV > p.len0 && ((p.len0 - kv0) & 7)) {
      fixup_v(p.len0 - kv0, st);
      __syncthreads();
    }
    if (t + 1 < nt0) issue0(kv0 + KV, st ^ 1);
    else if (p.len1 > 0) issue(kb1, p.k1_ld, vb1, p.vt1_ld, p.len1, 0, st ^ 1);
    advance();
    const T* sK = sbase + st * STAGE;
    f32x16 s[2];
    scores(s, sK, p.len0, kv0, p.causal != 0);
    if constexpr (MASK) {
      const float* mp = p.mask + (long)b * p.mask_bs + (long)h * p.mask_hs + (q_ok ? qrow : 0) * p.mask_qs;
#pragma unroll
      for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + kvt * 32 + 16 * (r >> 3) + 8 * hi + (r & 7);
          if (kv < p.len0) s[kvt][r] += mp[kv] * p.inv_scale;
        }
    }
    const float tm = attn_tile_max(s);
    // m_run is kept in RAW score units; exp2 arguments are formed as fma(s, c, -m*c) with c = scale * log2(e) > 0.
    // v_exp_f32 directly (__builtin_amdgcn_exp2f): results stay far inside the fp32 range, exp2(-inf) = 0 — none of
    // exp2f()'s denormal-range rescaling (v_ldexp + compares + selects per element) is needed.
    // The reference moves lazily (LAZY_LOG2); the generic branch mirrors attn_lazy_max, the rescale loops attn_scale_acc
    float ps = 0.f;
    float mc = 0.f;                                  // generic path: the reference in exp2 units
    if constexpr (FOLD) {
      // s already holds exp2's argument relative to the current reference (-qbias)
      if (t == 0 || __any(tm > LAZY_LOG2)) {
        const float sh = t == 0 ? tm : fmaxf(tm, 0.f);
        const float nb = to_f32<T>(from_f32<T>(qbias - sh));            // the new bias must be a storage-dtype value
        const float delta = nb - qbias;                                 // exact: both are representable
        const float alpha = t == 0 ? 1.0f : __builtin_amdgcn_exp2f(delta);   // first tile: O and l are still zero
#pragma unroll
        for (int t2 = 0; t2 < DT; ++t2)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[t2][r] *= alpha;
        if (!ONES) l_run *= alpha;
#pragma unroll
        for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[kvt][r] += delta;
        qbias = nb;
        if (hi) qf[NKS - 1][0] = from_f32<T>(nb);
      }
    } else {
      if (__any(tm * p.scale_log2 > m_run * p.scale_log2 + LAZY_LOG2)) {
        const float m_new = fmaxf(m_run, tm);
        // MASK: a row that has seen no visible key yet (every key of its tiles so far masked with -inf, or with a value whose mask / scale overflows
        // to it) takes this branch with the wave while m_run = m_new = -inf: its accumulators are zero and stay so, never exp2(-inf + inf)
        const float alpha = (MASK && m_new == -INFINITY) ? 1.0f : __builtin_amdgcn_exp2f((m_run - m_new) * p.scale_log2);
#pragma unroll
        for (int t2 = 0; t2 < DT; ++t2)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[t2][r] *= alpha;
        if (!ONES) l_run *= alpha;
        m_run = m_new;
      }
      // MASK: while no visible key has been seen the reference is 0 (tg_attention_wide_kmask's rule): exp2(fma(-inf, c, -0)) = 0 exactly
      mc = (MASK && m_run == -INFINITY) ? 0.f : m_run * p.scale_log2;
      if constexpr (MASK) {
        // a row whose every key so far carries a huge finite mask (-1e30: the reference is the mask itself): fma(x, c, -mc) leaves the rounding
        // error of mc = m_run * c, 2^-24 |mc|, as exp2's argument — a per-row constant that softmax forgives until it leaves exp2's range (+-inf
        // or 0 for every key of the row: NaN).  From |mc| = 2^24 on the argument is formed as (x - m_run) * c instead: x - 0 and c * 0 keep the
        // bits of every row below that
        const float far = __builtin_fabsf(mc) >= 16777216.f ? m_run : 0.f;
#pragma unroll
        for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[kvt][r] -= far;
        mc = far != 0.f ? 0.f : mc;
      }
    }
    // exp2 of one score register: FOLD scores are exp2's argument already
    auto ex = [&](float x) { return FOLD ? __builtin_amdgcn_exp2f(x) : __builtin_amdgcn_exp2f(__builtin_fmaf(x, p.scale_log2, -mc)); };
    const T* sV = sK + K_ELEMS;
#pragma unroll
    for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = ex(s[kvt][r]);
        s[kvt][r] = e;
        if (!ONES) ps += e;
      }
    if (!ONES) l_run += ps;
    attn_pv<T, 32 * 64>(o, s, sV, vofs);
  }
  {
    const float inv = 1.f / attn_row_sum<ONES>(o, l_run, hi);
#pragma unroll
    for (int t2 = 0; t2 < DT; ++t2)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t2][r] *= inv;
  }

  // ---------------- segment 1 (single tile, own softmax), folded in with weight w1 / l1
  if (p.len1 > 0) {
    const int st = nt0 & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (p.len1 < KV && (p.len1 & 7)) {
      fixup_v(p.len1, st);
      __syncthreads();
    }
    const T* sK = sbase + st * STAGE;
    f32x16 s[2];
    if constexpr (FOLD) {
      if (hi) qf[NKS - 1][0] = from_f32<T>(0.f);            // segment 1 has its own softmax: no carried reference
    }
    scores(s, sK, p.len1, 0, false);
    const float sc1 = FOLD ? 1.0f : p.scale_log2;           // FOLD: the scores are already in log2 units
    const float mc1 = attn_tile_max(s) * sc1;
    float ps = 0.f;
#pragma unroll
    for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kvt][r], sc1, -mc1));
        s[kvt][r] = e;
        ps += e;
      }
    const float l1 = ps + __shfl_xor(ps, 32, 64);
    // device value: the IP scale may change between replays of a captured graph.  One float, or one per batch item (w1_stride = 1: `b` is the
    // block's, so the load stays scalar); it enters as the same `w1 / l1` either way
    const float f = (p.w1_dev != nullptr ? p.w1_dev[(long)b * p.w1_stride] : p.w1) / l1;
#pragma unroll
    for (int kvt = 0; kvt < 2; ++kvt)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kvt][r] *= f;
    attn_pv<T, 32 * 64>(o, s, sK + K_ELEMS, vofs);
  }

  // ---------------- store: O^T regs -> out[b, q, h*HD + d], 4 consecutive d per 8-byte store
  if (q_ok) attn_store(o, reinterpret_cast<T*>(p.out) + (long)b * p.out_bs + qrow * p.out_ld + (long)h * HD, hi, HD);
}

template <typename T, int DPAD, int DV, bool ONES, bool FOLD = false, bool MASK = false>
int launch_attn(const tg_attn_desc* d, const AttnParams& p, hipStream_t st) {
  constexpr int NP = (DPAD + 63) / 64;
  const size_t lds = (size_t)2 * (NP * 64 * 64 + DV * 64) * sizeof(T);
  AttnParams pp = p;
  pp.n_qblk = (d->n_q + 127) / 128;
  dim3 grid((unsigned)(pp.n_qblk * d->heads * d->batch));
  auto k = attention_kernel<T, DPAD, DV, ONES, FOLD, MASK>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)attr;
  hipLaunchKernelGGL(k, grid, dim3(256), lds, st, pp);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

template <typename T>
int dispatch_attn(const tg_attn_desc* d, const AttnParams& p, hipStream_t st) {
  // ONES variants need a spare V^T row (DV > head dim): 40 -> (48, 64), 80 -> (80, 96), <= 16 -> (16, 32)
  const int hd = d->head_dim;
  if (p.mask != nullptr) {
    if (hd <= 16) return launch_attn<T, 16, 32, true, false, true>(d, p, st);
    if (hd <= 32) return launch_attn<T, 32, 32, false, false, true>(d, p, st);
    if (hd <= 48) return launch_attn<T, 48, 64, true, false, true>(d, p, st);
    if (hd <= 64) return launch_attn<T, 64, 64, false, false, true>(d, p, st);
    if (hd <= 80) return launch_attn<T, 80, 96, true, false, true>(d, p, st);
    if (hd <= 96) return launch_attn<T, 96, 96, false, false, true>(d, p, st);
    if (hd <= 128) return launch_attn<T, 128, 128, false, false, true>(d, p, st);
    return launch_attn<T, 160, 160, false, false, true>(d, p, st);
  }
  if (hd <= 16) return launch_attn<T, 16, 32, true>(d, p, st);
  if (hd <= 32) return launch_attn<T, 32, 32, false>(d, p, st);
  if (hd == 40) return launch_attn<T, 48, 64, true, true>(d, p, st);      // bias folded into QK^T
  if (hd <= 48) return launch_attn<T, 48, 64, true>(d, p, st);
  if (hd <= 64) return launch_attn<T, 64, 64, false>(d, p, st);
  if (hd <= 80) return launch_attn<T, 80, 96, true>(d, p, st);
  if (hd <= 96) return launch_attn<T, 96, 96, false>(d, p, st);
  if (hd <= 128) return launch_attn<T, 128, 128, false>(d, p, st);
  return launch_attn<T, 160, 160, false>(d, p, st);
}

// ---- attention-probability export (save_attn_to_dict side channel): one wave per query row --------------
template <typename T>
__global__ __launch_bounds__(256) void attn_probs_kernel(int b0, int heads, int hd, int n_q, const T* q, long q_ld, long q_bs,
                                                         const T* k, long k_ld, long k_bs, int len, float scale,
                                                         const int* tokens, int n_tokens, float* probs) {
  typedef typename Vec<T>::v8 V8;
  const int lane = threadIdx.x & 63;
  const long qi = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int h = blockIdx.y, bb = blockIdx.z, b = b0 + bb;
  if (qi >= n_q) return;
  const T* qp = q + (long)b * q_bs + qi * q_ld + (long)h * hd;
  const T* kp = k + (long)b * k_bs + (long)h * hd;
  constexpr int MAXJ = 4;  // keys per lane (len <= 256)
  float sc[MAXJ];
#pragma unroll
  for (int jj = 0; jj < MAXJ; ++jj) {
    const int j = lane + 64 * jj;
    float acc = 0.f;
    if (j < len) {
      for (int d = 0; d < hd; d += 8) {
        V8 a = *reinterpret_cast<const V8*>(qp + d);
        V8 c = *reinterpret_cast<const V8*>(kp + (long)j * k_ld + d);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += to_f32<T>(a[e]) * to_f32<T>(c[e]);
      }
    }
    sc[jj] = j < len ? acc * scale : -INFINITY;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int jj = 0; jj < MAXJ; ++jj) mx = fmaxf(mx, sc[jj]);
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int jj = 0; jj < MAXJ; ++jj) { sc[jj] = __expf(sc[jj] - mx); sum += sc[jj]; }
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  const int nt = tokens ? n_tokens : len;
  float* op = probs + (((long)bb * heads + h) * n_q + qi) * nt;
  if (!tokens) {
#pragma unroll
    for (int jj = 0; jj < MAXJ; ++jj) {
      const int j = lane + 64 * jj;
      if (j < len) op[j] = sc[jj] * inv;
    }
  } else {
    for (int t = 0; t < n_tokens; ++t) {
      const int j = tokens[t];
      const int owner = j & 63, slot = j >> 6;
      float v = 0.f;
#pragma unroll
      for (int jj = 0; jj < MAXJ; ++jj)
        if (jj == slot) v = sc[jj];
      v = __shfl(v, owner, 64);
      if (lane == 0) op[t] = v * inv;
    }
  }
}

}  // namespace

extern "C" int tg_attention_ps(const tg_attn_desc* d, int32_t ip_scale_count, void* stream) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_attention: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_attention: bad dtype");
  TG_CHECK(d->batch > 0 && d->heads > 0 && d->n_q > 0 && d->len0 > 0, TG_ERR_ARG, "tg_attention: empty problem");
  TG_CHECK(d->head_dim > 0 && d->head_dim % 8 == 0 && d->head_dim <= 160, TG_ERR_ARG,
           "tg_attention: head_dim %d unsupported (multiple of 8, <= 160)", d->head_dim);
  TG_CHECK(d->q && d->k0 && d->vt0 && d->out, TG_ERR_ARG, "tg_attention: null q/k0/vt0/out");
  TG_CHECK(d->q_ld % 8 == 0 && d->k0_ld % 8 == 0 && d->vt0_ld % 8 == 0 && d->out_ld % 4 == 0, TG_ERR_ARG,
           "tg_attention: pitches must keep 16-byte alignment");
  TG_CHECK(d->len1 >= 0 && d->len1 <= KV, TG_ERR_ARG, "tg_attention: len1 (%d) must be <= 64", d->len1);
  if (d->len1 > 0) TG_CHECK(d->k1 && d->vt1 && d->k1_ld % 8 == 0 && d->vt1_ld % 8 == 0, TG_ERR_ARG, "tg_attention: bad segment 1");
  // the lazy running max and the mask's 1 / scale assume c = scale * log2(e) > 0 (!(x > 0) also refuses NaN)
  TG_CHECK(d->scale > 0.f, TG_ERR_ARG, "tg_attention: scale must be > 0");
  // every K / V^T request is a 16-byte LDS-DMA, a Q fragment a 16-byte load, an output store 8 bytes, a mask element 4
  auto misaligned = [](const void* ptr, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(ptr) & (bytes - 1)) != 0; };
  TG_CHECK(!misaligned(d->q, 16) && !misaligned(d->k0, 16) && !misaligned(d->vt0, 16) && !misaligned(d->out, 8), TG_ERR_ARG,
           "tg_attention: q, k0 and vt0 must be 16-byte aligned, out 8-byte");
  TG_CHECK(d->vt0_ld >= d->len0, TG_ERR_ARG, "tg_attention: vt0_ld (%lld) must cover len0 (%d)", (long long)d->vt0_ld, d->len0);
  if (d->len1 > 0) {
    TG_CHECK(!misaligned(d->k1, 16) && !misaligned(d->vt1, 16), TG_ERR_ARG, "tg_attention: k1 and vt1 must be 16-byte aligned");
    TG_CHECK(d->vt1_ld >= d->len1, TG_ERR_ARG, "tg_attention: vt1_ld (%lld) must cover len1 (%d)", (long long)d->vt1_ld, d->len1);
  }
  TG_CHECK(d->mask == nullptr || !misaligned(d->mask, 4), TG_ERR_ARG, "tg_attention: mask must be 4-byte aligned");
  TG_CHECK(d->batch == 1 || (d->q_bs % 8 == 0 && d->k0_bs % 8 == 0 && d->vt0_bs % 8 == 0 && d->out_bs % 4 == 0), TG_ERR_ARG,
           "tg_attention: batch strides must keep 16-byte alignment (q_bs, k0_bs, vt0_bs multiples of 8, out_bs of 4)");
  TG_CHECK(d->batch == 1 || d->len1 == 0 || (d->k1_bs % 8 == 0 && d->vt1_bs % 8 == 0), TG_ERR_ARG,
           "tg_attention: segment 1's batch strides must keep 16-byte alignment (k1_bs, vt1_bs multiples of 8)");
  TG_CHECK(ip_scale_count == 0 || ip_scale_count == 1 || ip_scale_count == d->batch, TG_ERR_ARG,
           "tg_attention_ps: ip_scale_count = %d (0 or 1: w1_dev is one float; batch = %d: one per batch item)", ip_scale_count, d->batch);
  TG_CHECK(ip_scale_count <= 1 || d->w1_dev != nullptr, TG_ERR_ARG, "tg_attention_ps: ip_scale_count = %d needs w1_dev", ip_scale_count);
  AttnParams p{};
  p.heads = d->heads; p.hd = d->head_dim; p.n_q = d->n_q;
  p.q = d->q; p.q_ld = d->q_ld; p.q_bs = d->q_bs;
  p.k0 = d->k0; p.k0_ld = d->k0_ld; p.k0_bs = d->k0_bs; p.vt0 = d->vt0; p.vt0_ld = d->vt0_ld; p.vt0_bs = d->vt0_bs; p.len0 = d->len0;
  p.k1 = d->k1; p.k1_ld = d->k1_ld; p.k1_bs = d->k1_bs; p.vt1 = d->vt1; p.vt1_ld = d->vt1_ld; p.vt1_bs = d->vt1_bs; p.len1 = d->len1;
  p.scale_log2 = d->scale * 1.4426950408889634f;
  p.w1 = d->w1;
  p.w1_dev = d->w1_dev;
  p.w1_stride = ip_scale_count > 1 ? 1 : 0;
  p.out = d->out; p.out_ld = d->out_ld; p.out_bs = d->out_bs;
  p.causal = d->causal;
  if (d->mask != nullptr) {
    p.mask = d->mask; p.mask_bs = d->mask_bs; p.mask_hs = d->mask_hs; p.mask_qs = d->mask_qs;
    p.inv_scale = 1.0f / d->scale;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return dispatch_attn<bf16_t>(d, p, st);
  return dispatch_attn<f16_t>(d, p, st);
}

extern "C" int tg_attention(const tg_attn_desc* d, void* stream) { return tg_attention_ps(d, 0, stream); }

extern "C" int tg_attn_probs(int32_t dtype, int32_t batch, int32_t b0, int32_t heads, int32_t head_dim, int32_t n_q,
                             const void* q, int64_t q_ld, int64_t q_bs, const void* k, int64_t k_ld, int64_t k_bs,
                             int32_t len, float scale, const int32_t* tokens, int32_t n_tokens, float* probs, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_attn_probs: bad dtype");
  TG_CHECK(q && k && probs && batch > b0 && b0 >= 0 && heads > 0 && n_q > 0, TG_ERR_ARG, "tg_attn_probs: bad args");
  TG_CHECK(len > 0 && len <= 256 && head_dim > 0 && head_dim % 8 == 0, TG_ERR_ARG, "tg_attn_probs: len (%d) must be in 1..256, head_dim (%d) a positive multiple of 8", len,
           head_dim);
  TG_CHECK(q_ld % 8 == 0 && k_ld % 8 == 0, TG_ERR_ARG, "tg_attn_probs: q_ld (%lld) and k_ld (%lld) must keep the 16-byte loads aligned (multiples of 8)", (long long)q_ld,
           (long long)k_ld);
  TG_CHECK(tokens == nullptr || n_tokens > 0, TG_ERR_ARG, "tg_attn_probs: n_tokens (%d) must be positive when tokens is given", n_tokens);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)((n_q + 3) / 4), (unsigned)heads, (unsigned)(batch - b0));
  if (dtype == TG_BF16)
    hipLaunchKernelGGL(attn_probs_kernel<bf16_t>, grid, dim3(256), 0, st, b0, heads, head_dim, n_q, (const bf16_t*)q, q_ld, q_bs,
                       (const bf16_t*)k, k_ld, k_bs, len, scale, tokens, n_tokens, probs);
  else
    hipLaunchKernelGGL(attn_probs_kernel<f16_t>, grid, dim3(256), 0, st, b0, heads, head_dim, n_q, (const f16_t*)q, q_ld, q_bs,
                       (const f16_t*)k, k_ld, k_bs, len, scale, tokens, n_tokens, probs);
  TG_LAUNCH_CHECK();
  return TG_OK;
}
