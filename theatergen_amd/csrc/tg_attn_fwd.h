// Device pieces shared by the forward flash-attention kernels: tg_attention.hip (head dims 8-160), tg_attention_wide.hip (256 / 512) and
// tg_attention_relpos.hip (SAM's separable bias).  `__device__ __forceinline__` helpers and the constant pages only: no kernel, no instantiation, no
// host code, so including it does not touch a file's other kernels (scripts/dev_isa_diff.py compares the assembly of two trees).
//
// THE FORMULATION.  Block = 4 waves x 32 queries; a K tile [KVT * 32 keys][d] and a V^T tile in LDS, shared by the 4 waves, two stages.  Everything is
// computed TRANSPOSED so that lane & 31 is the query:
//   S^T[key][q]  = mfma32x32x16(A = K rows,   B = Q rows)      -> a lane holds half of the tile's scores of ITS query
//   O^T[d][q]   += mfma32x32x16(A = V^T rows, B = P^T)         -> P^T is consumed straight from the S^T registers
// (the MFMA C layout of S^T is a valid B-operand layout once V^T's keys are read in the matching permuted order), running max / sum / rescale are
// lane-local, and the only cross-lane traffic of the online softmax is one exchange with lane ^ 32.
// KVT = 32-key score tiles per key tile: 2 (64 keys) in tg_attention.hip and tg_attention_relpos.hip, 1 in tg_attention_wide.hip.
//
// THE SWIZZLE.  Tiles are 128-byte LDS rows filled by LDS-DMA (global_load_lds_dwordx4, no VGPR round trip, no ds_write pass) with the GEMM's XOR
// swizzle: 16-byte slot ^ ((row >> 1) & 7), applied on the request's source address and again on the fragment read (attn_frag_ofs).
#pragma once
#include "tg_common.h"

namespace {

// LDS-DMA sources for out-of-range pieces: head-dim / key padding reads zeros; the "ones row" reads 1.0
__device__ __attribute__((aligned(256))) unsigned char attn_zero_page[256];
#define TG_R8(x) x, x, x, x, x, x, x, x
__device__ __attribute__((aligned(256))) const unsigned short attn_ones_bf16[64] = {TG_R8(TG_R8(0x3F80))};
__device__ __attribute__((aligned(256))) const unsigned short attn_ones_f16[64] = {TG_R8(TG_R8(0x3C00))};
template <typename T> __device__ __forceinline__ const T* ones_page();
template <> __device__ __forceinline__ const bf16_t* ones_page<bf16_t>() { return reinterpret_cast<const bf16_t*>(attn_ones_bf16); }
template <> __device__ __forceinline__ const f16_t* ones_page<f16_t>() { return reinterpret_cast<const f16_t*>(attn_ones_f16); }

// XCD-aware block order (speed only): block b runs on XCD b % 8; give each XCD a contiguous chunk of the logical block space, so that the blocks
// which read one (batch, head)'s K / V^T (neighbours in that space) share them through ONE private L2.  Returns the logical block of blockIdx.x
__device__ __forceinline__ int attn_xcd_block() {
  const int nb = gridDim.x, q8 = nb >> 3, r8 = nb & 7, xcd = blockIdx.x & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
}

// one LDS-DMA request: 16 bytes per lane from `src` to 64 consecutive 16-byte slots (8 rows) from `lds_row_base` on
template <typename T>
__device__ __forceinline__ void attn_dma16(const T* src, T* lds_row_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_row_base, 16, 0, 0);
}

// a Q fragment (B operand): 8 head-dim elements of this lane's query row from `qp`, zeros where !ok (rows >= n_q, head-dim padding: not read)
template <typename T>
__device__ __forceinline__ typename Vec<T>::v8 attn_q_frag(const T* qp, bool ok) {
  typename Vec<T>::v8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = from_f32<T>(0.f);
  if (ok) v = *reinterpret_cast<const typename Vec<T>::v8*>(qp);
  return v;
}

// KEY PERMUTATION: MFMA row i of a 32-key score tile is fed K row perm(i) = i with bits 2 and 3 swapped.  The 32x32 accumulator gives lane-half `hi`
// the rows 8g + 4 hi + j in registers 4g + j; with the permutation registers 8cc .. 8cc+7 hold the 8 CONSECUTIVE keys 16cc + 8 hi + 0..7, i.e. the
// P^T fragment of the PV MFMA pairs with ONE 16-byte V^T slot (a single ds_read_b128 per fragment, no register shuffles) instead of two 8-byte halves
// of neighbouring slots.  So register r of score tile kvt holds key 32 kvt + 16 (r >> 3) + 8 hi + (r & 7).
__device__ __forceinline__ int attn_perm_row(int l31) { return (l31 & 19) | ((l31 & 4) << 1) | ((l31 & 8) >> 1); }

// per-lane LDS element offset of a fragment read: 16-byte slot 2c + hi of `row`, swizzled with key = (row >> 1) & 7.  Computed ONCE per lane (K: row =
// attn_perm_row, V^T of a 64-key tile: row = l31), so that inside the loop an access is (stage base + table entry + compile-time constant)
__device__ __forceinline__ int attn_frag_ofs(int row, int key, int c, int hi) { return row * 64 + (((2 * c + hi) ^ key) << 3); }

// RAW scores S^T of one key tile for this lane's query: K panels of [KVT * 32 keys][64 d] at sK, fragment offsets kofs[c] = attn_frag_ofs(perm row, c, hi)
template <typename T, int KVT, int NKS>
__device__ __forceinline__ void attn_qk(f32x16 (&s)[KVT], const T* sK, const typename Vec<T>::v8 (&qf)[NKS], const int (&kofs)[4]) {
  typedef typename Vec<T>::v8 V8;
#pragma unroll
  for (int kvt = 0; kvt < KVT; ++kvt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kvt][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      V8 kf = *reinterpret_cast<const V8*>(sK + kofs[ks & 3] + ((ks >> 2) * (KVT * 2048) + kvt * 32 * 64));
      s[kvt] = mfma32(kf, qf[ks], s[kvt]);
    }
  }
}

// max of this query's scores over the tile.  The other half of the row lives in lane ^ 32: v_permlane32_swap exchanges the upper 32 lanes of one copy
// with the lower 32 of the other (no LDS round trip, unlike the ds_bpermute behind __shfl_xor).  Inline asm: with the builtin hipcc drops the second
// result and the max with it; s_nop covers the VALU-write -> permlane-read hazard the assembler does not see
template <int KVT>
__device__ __forceinline__ float attn_tile_max(const f32x16 (&s)[KVT]) {
  float mx = -INFINITY;
#pragma unroll
  for (int kvt = 0; kvt < KVT; ++kvt)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kvt][r]);
  float a = mx, b = mx;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}

template <int DT>
__device__ __forceinline__ void attn_scale_acc(f32x16 (&o)[DT], float f) {
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] *= f;
}

// LAZY RUNNING MAX: softmax is invariant to the reference point, so m_run only moves (and O is only rescaled: 16 DT accumulator multiplies) when some
// row's tile max exceeds it by more than LAZY_LOG2 in exp2 units; until then probabilities are formed against the stale reference and are at most
// 2^LAZY_LOG2 (P's storage dtype and the fp32 accumulators have the range).  With a strict "any row has a new max" test the rescale ran on most tiles:
// over 32 rows a new maximum keeps turning up somewhere.  m_run and tm are in units of 1 / c exp2 units (c > 0: scale * log2(e) for raw scores, 1 for
// scores kept in exp2 units).  ONES: the denominator is an accumulator row (rescaled with O), l_run is unused
constexpr float LAZY_LOG2 = 8.f;
template <bool ONES, int DT>
__device__ __forceinline__ void attn_lazy_max(f32x16 (&o)[DT], float& m_run, float& l_run, float tm, float c) {
  if (__any(tm * c > m_run * c + LAZY_LOG2)) {
    const float m_new = fmaxf(m_run, tm);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);        // first tile: exp2(-inf) = 0 on a zero accumulator
    attn_scale_acc(o, alpha);
    if (!ONES) l_run *= alpha;
    m_run = m_new;
  }
}

// O^T += V^T * P^T for one key tile; P^T comes straight from the score registers: chunk c = (kvt, cc) covers keys 32 kvt + 16 cc + 8 hi + 0..7, one
// 16-byte V^T slot at vofs[c]; accumulator tile t (32 head-dim rows) starts VT elements after tile t - 1
template <typename T, int VT, int KVT, int DT>
__device__ __forceinline__ void attn_pv(f32x16 (&o)[DT], const f32x16 (&s)[KVT], const T* sV, const int (&vofs)[2 * KVT]) {
  typedef typename Vec<T>::v8 V8;
#pragma unroll
  for (int c = 0; c < 2 * KVT; ++c) {
    const int kvt = c >> 1, cc = c & 1;
    V8 pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[j] = from_f32<T>(s[kvt][8 * cc + j]);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const V8 vf = *reinterpret_cast<const V8*>(sV + vofs[c] + t * VT);
      o[t] = mfma32(vf, pf, o[t]);
    }
  }
}

// the softmax denominator of this lane's query.  ONES (variants whose DV exceeds the head dim): V^T row DV - 1 is fed from a page of 1.0, so the PV
// MFMA itself accumulates l = sum_k p[k] in accumulator row DV - 1 = tile DT - 1, register 15 of the lanes with hi = 1 (rescaled with O for free) and
// the per-tile v_add_f32 of the row sum disappear; otherwise the two half-row sums l_run
template <bool ONES, int DT>
__device__ __forceinline__ float attn_row_sum(const f32x16 (&o)[DT], const float& l_run, int hi) {
  float l_tot;
  if (ONES) {
    const float c = hi ? o[DT - 1][15] : 0.f;
    l_tot = c + __shfl_xor(c, 32, 64);
  } else {
    l_tot = l_run + __shfl_xor(l_run, 32, 64);
  }
  return l_tot;
}

// store: O^T regs -> op[d] (this lane's output row), 4 consecutive d per 8-byte store, d < hd
template <typename T, int DT>
__device__ __forceinline__ void attn_store(const f32x16 (&o)[DT], T* op, int hi, int hd) {
  typedef typename Vec<T>::v4 V4;
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = t * 32 + 8 * g + 4 * hi;
      if (d < hd) {
        V4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = from_f32<T>(o[t][4 * g + j]);
        *reinterpret_cast<V4*>(op + d) = v;
      }
    }
}

// ---- the 64-key tile: K = NP panels of [64 keys][64 d], V^T = [DV d][64 keys] ----------------------------------------------------------------------
// Generic loader of one tile at keys kv0 .. kv0 + 64 of a segment of `len` keys: every request derives its source from (kv0, len, hd); pieces past the
// head dim or the segment come from the zero page.  wave / lrow / slot: the wave and the lane's row (lane >> 3) and 16-byte slot (lane & 7) of a request.
// ONES: V^T row DV - 1 comes from the page of 1.0
template <typename T, int NP, int DV, bool ONES>
__device__ __forceinline__ void attn_issue_tile(T* sK, T* sV, const T* kb, long k_ld, const T* vb, long vt_ld, int len, int kv0, int hd, int wave,
                                                int lrow, int slot) {
  const T* zero = reinterpret_cast<const T*>(attn_zero_page);
#pragma unroll
  for (int j = 0; j < NP * 2; ++j) {
    const int q = j * 4 + wave;                       // rows [8q, 8q+8) of the panel stack
    const int prow = 8 * q + lrow;
    const int r = prow & 63, panel = prow >> 6;
    const int d0 = panel * 64 + ((slot ^ ((r >> 1) & 7)) << 3);
    const bool ok = d0 < hd && kv0 + r < len;
    const T* src = ok ? kb + (long)(kv0 + r) * k_ld + d0 : zero;
    attn_dma16(src, sK + q * 512);
  }
#pragma unroll
  for (int j = 0; j < DV / 32; ++j) {
    const int q = j * 4 + wave;
    const int d = 8 * q + lrow;
    const int c0 = kv0 + ((slot ^ ((d >> 1) & 7)) << 3);
    const T* src = (d < hd && c0 < len) ? vb + (long)d * vt_ld + c0 : zero;
    if (ONES && d == DV - 1) src = ones_page<T>();
    attn_dma16(src, sV + q * 512);
  }
}

// a 16-byte V^T chunk that straddles the segment's end brought columns >= len along (they may hold anything, and 0 * NaN = NaN in the PV MFMA): zero
// them in LDS.  One thread per V^T row d < head dim; rem = keys of the ragged tile, (rem & 7) != 0
template <typename T>
__device__ __forceinline__ void attn_zero_vt_tail(T* sV, int d, int rem) {
  const int ch = rem >> 3;
  T* rowp = sV + d * 64 + ((ch ^ ((d >> 1) & 7)) << 3);
  for (int c = rem & 7; c < 8; ++c) rowp[c] = from_f32<T>(0.f);
}

}  // namespace
