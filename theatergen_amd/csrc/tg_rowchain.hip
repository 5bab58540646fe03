// Row-chain kernels (round 4): the ROW-LOCAL layers of a transformer block at K = C <= 640 — every projection, the decoupled
// text + image cross-attention against its short key set, the GEGLU feed-forward, the residual adds — with the token on the LANE.
//
// Why: at the UNet's first level (65536 tokens x 320 channels at CFG batch 16) the 128 x 128 LDS-tiled GEMM spends 34-39 us on a
// 320 -> 320 projection whose operands cross HBM in 14-21 us and whose MFMAs take 6 us (profiles/r4_per_shape_eager.txt): the K loop is
// five tiles long and the tile's fixed costs (operand fetch round trip, LDS bounce epilogue) are not amortised.  Here a WAVE owns 32
// tokens for the whole layer (or chain of layers):
//   * activations live in REGISTERS in MFMA B-operand form (lane & 31 = token, lane >> 5 = which half of a 64-channel group, 8
//     consecutive channels per k-step): loaded once from HBM with 16-byte accesses (a token pair covers whole 128-byte lines);
//   * weights are the A operand, packed ONCE on the host in fragment order (1 KiB per (32 output rows, 16 k) block, lane-linear), so a
//     64-row chunk is one contiguous 128 K-byte piece of memory: it goes L2 -> LDS by straight LDS-DMA and every fragment read is a
//     conflict-free linear ds_read_b128 shared by all waves of the workgroup;
//   * the weight rows of a chunk are PERMUTED (pi below) so that the fp32 accumulators of two 32-row MFMA tiles, rounded to the storage
//     dtype, ARE the next layer's B operand for four k-steps (and 64 contiguous bytes of the output row): a chain of row-local layers
//     never leaves the registers, and a store is four 16-byte pieces per lane.
// Index maps (c = 64-row chunk, u = MFMA tile of the chunk, r = MFMA row, s = k-step, hi = lane >> 5, j = element of the fragment):
//   output channel of (c, u, r)      = 64 c + 32 ((r >> 2) & 1) + 16 u + 4 (r >> 3) + (r & 3)     (accumulator register rho of lane half
//                                       hi holds channel 64 c + 32 hi + 16 u + rho)
//   input channel of (s, hi, j)      = 64 (s >> 2) + 32 hi + 8 (s & 3) + j                         (lane half hi owns channels [32 hi, 32 hi + 32)
//                                       of every 64-channel group: 64 contiguous bytes per lane and group)
// Reference layers: `Attention.to_q / to_out[0]` (ip_adapter/attention_processor.py:113-128), `Transformer2DModel.proj_in / proj_out`
// (models/transformer_2d.py:150-163, 286-327), `BasicTransformerBlock.norm1/2/3` folded as in tg_gemm_glds.h, `FeedForward`
// (models/attention.py:226-236, 337-338).
#include "tg_common.h"

#include <type_traits>
#include <utility>

// rc_xattn_kernel keeps its timing switches as RUN-TIME branches on the (always zero, C entry checked) dbg word: with them compiled out hipcc's allocator spills
// 99-111 VGPRs in the image-token instances (448 B scratch; profiles/r6_kernel_resources.json gate) — the branches are scheduling fences it relies on.
#define RC_DBG_RT(bit) ((p.dbg & (bit)) != 0)

namespace {

struct RcLinearParams {
  const void* x;      // [M, K] storage dtype, row pitch ldx
  long ldx;
  const void* wpk;    // packed weights: N / 64 chunks of (128 K + 1024) bytes (rc_pack in theatergen_amd/weights_pack.py)
  const void* res;    // [M, N] residual or NULL
  long ldres;
  void* out;          // [M, N]
  long ldc;
  long M;
  int N, K;
  float ln_eps;
  long c_dup;         // tg_rc_linear_dup: every output row is stored again c_dup elements further on, 0 = off
};

// Workgroup -> row block, XCD-aware (speed only): the dispatcher places block b on XCD b % 8 and every XCD has a private L2.  The LDS-tiled
// GEMM / conv kernels give XCD x a CONTIGUOUS eighth of the token rows (tg_gemm_common.h), so a row-chain kernel that sits between them must
// use the same partition — with the natural order its output is striped over the eight L2s and the next kernel finds none of its rows in
// its own L2 (measured: the rc_linear swaps alone made the graph-replayed step 1.4 % SLOWER although each launch is 20 % shorter).
// Global-address-space accesses through a pointer whose provenance hipcc cannot see (the opaque `asm("" : "+s"(ptr))` copies below): a plain dereference
// becomes a FLAT instruction, which counts in lgkmcnt as well as vmcnt — the next `s_waitcnt lgkmcnt(0)` in front of an LDS fragment's first MFMA then sits out a
// whole global-memory round trip.
template <typename V>
__device__ __forceinline__ V gld(const void* ptr) { return *(const __attribute__((address_space(1))) V*)ptr; }
template <typename V>
__device__ __forceinline__ void gst(void* ptr, V v) { *(__attribute__((address_space(1))) V*)ptr = v; }

__device__ __forceinline__ int rc_block_id(int bid, int nblocks) {
  const int q = nblocks >> 3, r = nblocks & 7;
  const int xcd = bid & 7;
  const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return start + (bid >> 3);
}

template <typename T> __device__ __forceinline__ typename Vec<T>::v8 pack8(const float* f) {
  typename Vec<T>::v8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(f[e]);
  return o;
}

// 4 x 4 transpose of 16-byte pieces inside every quad of lanes: in  = lane b holds piece i of ITS row in p[i];
//                                                              out = lane b holds piece b of row i (of the quad) in p[i]   (an involution).
// Why: a lane owns a token ROW, so a naive load / store instruction touches 64 different rows with 16 bytes each — measured 2 TB/s on
// this chip (the vector-memory path processes one 16-byte request per lane and row).  Transposed, the quad's four lanes cover 64
// contiguous bytes of ONE row and lane ^ 32 the other half of the 128-byte line: every instruction moves 8 whole lines.
// Two butterfly stages of quad-permute DPP selects (v_cndmask_b32_dpp: 2 instructions per dword pair and stage = 32 per 64-byte group).
// d[k] = mask[lane] ? y[k] : x[k] of the quad-permuted lane, four dwords per statement (VOP2-DPP selects; hipcc does not fold a DPP move
// into a select that has two uses, and VOP2 takes its condition from VCC only).  The two s_mov in front are also the two wait states a
// DPP read needs behind a VALU write of its source (nothing pads an asm statement).
#define TG_SEL4_DPP(QP, MASK, D, X, Y)                                                                          \
  asm volatile("s_mov_b32 vcc_lo, " MASK "\n\ts_mov_b32 vcc_hi, " MASK "\n\t"                                    \
               "v_cndmask_b32_dpp %0, %4, %8, vcc quad_perm:" QP " row_mask:0xf bank_mask:0xf\n\t"               \
               "v_cndmask_b32_dpp %1, %5, %9, vcc quad_perm:" QP " row_mask:0xf bank_mask:0xf\n\t"               \
               "v_cndmask_b32_dpp %2, %6, %10, vcc quad_perm:" QP " row_mask:0xf bank_mask:0xf\n\t"              \
               "v_cndmask_b32_dpp %3, %7, %11, vcc quad_perm:" QP " row_mask:0xf bank_mask:0xf"                   \
               : "=&v"(D[0]), "=&v"(D[1]), "=&v"(D[2]), "=&v"(D[3])                                             \
               : "v"(X[0]), "v"(X[1]), "v"(X[2]), "v"(X[3]), "v"(Y[0]), "v"(Y[1]), "v"(Y[2]), "v"(Y[3])         \
               : "vcc")
template <typename V8> __device__ __forceinline__ void quad_transpose(V8& p0, V8& p1, V8& p2, V8& p3) {
  unsigned x[4][4], y[4][4];
  {
    const u32x4 t0 = __builtin_bit_cast(u32x4, p0), t1 = __builtin_bit_cast(u32x4, p1), t2 = __builtin_bit_cast(u32x4, p2), t3 = __builtin_bit_cast(u32x4, p3);
#pragma unroll
    for (int d = 0; d < 4; ++d) { x[0][d] = t0[d]; x[1][d] = t1[d]; x[2][d] = t2[d]; x[3][d] = t3[d]; }
  }
  // stage 1 (lane bit 0 <-> piece bit 0): y[pr] = odd lane ? partner's x[pr + 1] : x[pr];  y[pr + 1] = odd lane ? x[pr + 1] : partner's x[pr]
  TG_SEL4_DPP("[1,0,3,2]", "0x55555555", y[0], x[1], x[0]);
  TG_SEL4_DPP("[1,0,3,2]", "0x55555555", y[2], x[3], x[2]);
  TG_SEL4_DPP("[1,0,3,2]", "0xaaaaaaaa", y[1], x[0], x[1]);
  TG_SEL4_DPP("[1,0,3,2]", "0xaaaaaaaa", y[3], x[2], x[3]);
  // stage 2 (lane bit 1 <-> piece bit 1)
  TG_SEL4_DPP("[2,3,0,1]", "0x33333333", x[0], y[2], y[0]);
  TG_SEL4_DPP("[2,3,0,1]", "0x33333333", x[1], y[3], y[1]);
  TG_SEL4_DPP("[2,3,0,1]", "0xcccccccc", x[2], y[0], y[2]);
  TG_SEL4_DPP("[2,3,0,1]", "0xcccccccc", x[3], y[1], y[3]);
  u32x4 o0, o1, o2, o3;
#pragma unroll
  for (int d = 0; d < 4; ++d) { o0[d] = x[0][d]; o1[d] = x[1][d]; o2[d] = x[2][d]; o3[d] = x[3][d]; }
  p0 = __builtin_bit_cast(V8, o0); p1 = __builtin_bit_cast(V8, o1); p2 = __builtin_bit_cast(V8, o2); p3 = __builtin_bit_cast(V8, o3);
}

// KS = K / 16 k-steps (20: K = 320), NW waves per workgroup.  A chunk in memory = 2 KS KiB of weight fragments + one 1-KiB vector page (v[64] fp32, u[64] fp32, pad).
template <typename T, int KS, int NW, bool LN>
__global__ __launch_bounds__(NW * 64) void rc_linear_kernel(RcLinearParams p) {
  typedef typename Vec<T>::v8 V8;
  constexpr int NBUF = 2;               // chunk buffers in LDS
  constexpr int NP = 2 * KS + 1;        // 1-KiB DMA pieces per chunk
  constexpr int CB = NP * 1024;         // bytes of a chunk
  constexpr int PPW = (NP + NW - 1) / NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int lbid = rc_block_id((int)blockIdx.x, (int)gridDim.x);
  const long tok0 = ((long)lbid * NW + wave) * 32;             // the wave's first token; lane (t, hi) computes token tok0 + t
  // memory instruction i of a 4-piece group: this lane moves piece (lane & 3) of row tok0 + (t & ~3) + i (quad_transpose)
  const int qb = lane & 3;
  long mrow[4];
  bool mok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long r = tok0 + (l31 & ~3) + i;
    mok[i] = r < p.M;
    mrow[i] = mok[i] ? r : p.M - 1;
  }
  const int NC = p.N >> 6;
  const char* wpk = reinterpret_cast<const char*>(p.wpk);

  auto issue_chunk = [&](int c, int buf) {
    const char* src = wpk + (long)c * CB + lane * 16;
    char* dst = smem + buf * CB;
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int i = j * NW + wave;
      if (i < NP)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i * 1024),
                                         (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
    }
  };
  // (a loop of one iteration: written as a plain `if`, hipcc schedules the prologue differently and every instance grows by 9 - 12 instructions)
#pragma unroll
  for (int b = 0; b < NBUF - 1; ++b)
    if (b < NC) issue_chunk(b, b);

  // the wave's 32 token rows as B operands: B[4 q + i] = channels [64 q + 32 hi + 8 i, + 8)
  V8 B[KS];
  {
    const T* xp = reinterpret_cast<const T*>(p.x) + 32 * hi + 8 * qb;
#pragma unroll
    for (int s = 0; s < KS; ++s) B[s] = *reinterpret_cast<const V8*>(xp + mrow[s & 3] * p.ldx + 64 * (s >> 2));
#pragma unroll
    for (int q = 0; q < KS / 4; ++q) quad_transpose(B[4 * q], B[4 * q + 1], B[4 * q + 2], B[4 * q + 3]);
  }
  float ln_rstd = 1.f, ln_std = 1.f, ln_nmean = 0.f;
  if constexpr (LN) {
    // two-pass row statistics on the stored values (what nn.LayerNorm reads), the token's other 160 channels sit in lane ^ 32
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += to_f32<T>(B[s][e]);
    sum += __shfl_xor(sum, 32, 64);
    const float inv_k = 1.0f / (float)p.K;
    const float mean = sum * inv_k;
    float c2 = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      asm volatile("" : "+v"(B[s]));      // second pass converts again: 160 fp32 copies of the row must not stay live
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = to_f32<T>(B[s][e]) - mean; c2 = __builtin_fmaf(d, d, c2); }
    }
    c2 += __shfl_xor(c2, 32, 64);
    const float var = c2 * inv_k + p.ln_eps;
    ln_rstd = __builtin_amdgcn_rsqf(var);
    ln_std = var * ln_rstd;
    ln_nmean = -mean;
  } else {
    // the compiler must see the row loads consumed BEFORE the loop, or it waits vmcnt(0) in front of the first MFMA of every iteration
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(B[s]));
  }

  const T* resp = reinterpret_cast<const T*>(p.res);
  T* outp = reinterpret_cast<T*>(p.out);
  // the stores of chunk c are issued at the top of iteration c + 1, BEHIND the wait for chunk c + 1's DMA: the only vmcnt(0) of the loop
  // then waits for operations that were issued a whole MFMA block earlier (stores are vector-memory operations on gfx9: they count)
  V8 pend[4];
  long pend_ch = -1;
  for (int c = 0; c < NC; ++c) {
    const int buf = c % NBUF;
    // chunk c has landed (this wave's pieces; the barrier covers the other waves') and every wave is done with chunk c - 1's buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (c + NBUF - 1 < NC) issue_chunk(c + NBUF - 1, (c + NBUF - 1) % NBUF);
    if (pend_ch >= 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (mok[i]) *reinterpret_cast<V8*>(outp + mrow[i] * p.ldc + pend_ch + 8 * qb) = pend[i];
      if (p.c_dup != 0) {                      // wave-uniform: the second destination of tg_rc_linear_dup
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (mok[i]) *reinterpret_cast<V8*>(outp + mrow[i] * p.ldc + pend_ch + 8 * qb + p.c_dup) = pend[i];
      }
    }
    const long ch0 = 64 * (long)c + 32 * hi;
    V8 r8[4];
    if (resp != nullptr) {
#pragma unroll
      for (int i = 0; i < 4; ++i) r8[i] = *reinterpret_cast<const V8*>(resp + mrow[i] * p.ldres + ch0 + 8 * qb);
    }
    const char* cbase = smem + buf * CB;
    // accumulators start from the layer's vector terms (fp32, broadcast reads of the chunk's vector page):
    //   plain: v;   LayerNorm fold: std * v - mean * u, scaled by rstd at the end = rstd * (x W'^T - mean u) + v
    f32x16 acc[2];
    {
      const float* vec = reinterpret_cast<const float*>(cbase + 2 * KS * 1024) + 32 * hi;
#pragma unroll
      for (int uu = 0; uu < 2; ++uu)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 v4 = *reinterpret_cast<const f32x4*>(vec + 16 * uu + 4 * g);
          if constexpr (LN) {
            const f32x4 u4 = *reinterpret_cast<const f32x4*>(vec + 64 + 16 * uu + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[uu][4 * g + e] = __builtin_fmaf(ln_nmean, u4[e], ln_std * v4[e]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[uu][4 * g + e] = v4[e];
          }
        }
    }
    const char* cb = cbase + lane * 16;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const V8 a0 = *reinterpret_cast<const V8*>(cb + s * 1024);
      const V8 a1 = *reinterpret_cast<const V8*>(cb + (KS + s) * 1024);
      acc[0] = mfma32(a0, B[s], acc[0]);
      acc[1] = mfma32(a1, B[s], acc[1]);
    }
    // epilogue: accumulator register rho of tile uu = channel ch0 + 16 uu + rho
    float o[32];
#pragma unroll
    for (int uu = 0; uu < 2; ++uu)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[16 * uu + r] = LN ? acc[uu][r] * ln_rstd : acc[uu][r];
    if (resp != nullptr) {
      quad_transpose(r8[0], r8[1], r8[2], r8[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[8 * i + e] += to_f32<T>(r8[i][e]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) pend[i] = pack8<T>(o + 8 * i);
    quad_transpose(pend[0], pend[1], pend[2], pend[3]);
    pend_ch = ch0;
  }
  if (pend_ch >= 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (mok[i]) *reinterpret_cast<V8*>(outp + mrow[i] * p.ldc + pend_ch + 8 * qb) = pend[i];
    if (p.c_dup != 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (mok[i]) *reinterpret_cast<V8*>(outp + mrow[i] * p.ldc + pend_ch + 8 * qb + p.c_dup) = pend[i];
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// rc_xattn_kernel: the whole cross-attention sub-block of a first-level BasicTransformerBlock in ONE launch, for SD-1.5's geometry
// (C = 320 = 8 heads x 40, 77 text keys + IPT image keys):
//     h2 = to_out( softmax(q Kt^T) Vt + w_ip softmax(q Kip^T) Vip ) + bias + h1,      q = to_q(LayerNorm(h1))
// (models/attention.py:206-224 norm2 + attn2 + residual; IPAttnProcessor, ip_adapter/attention_processor.py:445-529: two independent
// softmaxes; AttnProcessor :282-393 with IPT = 0).  Today that is three launches (LayerNorm-folded q GEMM 37 us, attention 53 us,
// to_out GEMM 39 us at 65536 tokens) and 7 HBM passes over the [tokens, 320] tensor; here q, the scores, the probabilities and the
// attention output never leave the registers of the wave that owns the 32 tokens: 2 HBM passes (+ the residual re-read).
// A wave's life:  load h1 rows -> row statistics -> 5 weight chunks of to_q (LayerNorm folded; softmax scale * log2 e folded) -> per
// head: S^T = K q^T (MFMA, keys on the accumulator rows), softmax over the registers (+ one lane ^ 32 exchange), P^T straight from the
// accumulator registers as the next MFMA's B operand, O^T = V^T P^T with V^T's spare rows fed with ones (row 40 / 44 of the second
// tile = the softmax denominator), the image keys as one more k-step -> O^T rounded = B operand of to_out -> 5 chunks -> + h1 -> store.
// Slot layout of q / O inside the 20 k-steps (a head pair = 80 channels = 5 k-steps; m = pair):
//   q:  k-step 5m, 5m+1: head 2m, d = 16 w + 8 hi + j;   5m+2: hi = 0 -> head 2m, d = 32 + j;  hi = 1 -> head 2m+1, d = j;
//       k-step 5m+3, 5m+4: head 2m+1, d = 8 + 16 (w-1) + 8 hi + j (w = 1, 2).   K fragments hold zeros in the other head's half.
//   O:  k-step 5m + 3 hh + gg (gg = 0, 1): head 2m+hh, d = 16 gg + 8 (j >> 2) + 4 hi + (j & 3)   (accumulator registers 8 gg .. 8 gg + 7);
//       k-step 5m+2: j < 4 -> head 2m, d = 32 + 4 hi + j;  j >= 4 -> head 2m+1, d = 32 + 4 hi + j - 4.
// Both are absorbed by the host-side row / column permutations of the packed weights (theatergen_amd/rowchain.py).
// LDS: a ring of three 24-KiB slots fed by LDS-DMA two stages ahead: 10 to_q tiles (21 KiB each), 8 per-head K / V^T fragment sets of the
// workgroup's batch item (24 KiB, packed by rc_kv_pack_kernel when the conditioning is projected), 10 to_out tiles.  4-wave workgroups of 128
// tokens, 72 KiB: two per CU (the first version — one 8-wave workgroup, two 48-KiB slots — took 67 us against this one's 55).
struct RcXattnParams {
  const void* h;        // [M, 320] the stream before norm2 (= residual)
  long ldh;
  const void* wq;       // 5 chunks (rc_pack of the permuted, LayerNorm-folded, scaled to_q)
  const void* kv;       // [batch][8 heads][24 KiB] K / V^T fragments (rc_kv_pack_kernel)
  const void* wo;       // 5 chunks (rc_pack of the column-permuted to_out[0] + bias)
  void* out;            // [M, 320]
  long ldc;
  long M;
  int rows_per_batch;   // tokens per batch item (multiple of 32 * NW)
  float ln_eps;
  const float* ip_scale;  // device scalar (IPAttnProcessor.scale), one per batch item (ip_stride = 1, tg_rc_xattn_ps) or NULL (1.0)
  int dbg;                // always 0 (RC_DBG_RT): 1 no to_q MFMAs, 2 no attention, 4 no to_out MFMAs, 8 no stage DMA, 16 no barriers
  int ip_stride;          // 0: ip_scale[0] for every workgroup; 1: ip_scale[the workgroup's batch item]
};

template <typename T> __device__ __forceinline__ typename Vec<T>::v8 pack8r(const f32x16& a, int r0) {
  typename Vec<T>::v8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(a[r0 + e]);
  return o;
}

template <typename T, int NW, int TEXT, int IPT>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void rc_xattn_kernel(RcXattnParams p) {
  typedef typename Vec<T>::v8 V8;
  constexpr int KS = 20;
  constexpr int TBW = (KS + 1) * 1024;         // weight TILE: 20 fragment blocks + one vector page (v[32], u[32] fp32 in accumulator order)
  constexpr int KVH = 24 * 1024;               // K (12 KiB) + V^T (12 KiB) fragments of one head
  constexpr int SLOT = 24 * 1024;
  static_assert(TEXT > 64 && TEXT <= 80, "text keys: three 32-key tiles, five 16-key PV steps");
  static_assert(IPT == 0 || IPT == 4 || IPT == 16, "image tokens");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int lbid = rc_block_id((int)blockIdx.x, (int)gridDim.x);
  const long tok0 = ((long)lbid * NW + wave) * 32;
  const int qb = lane & 3;
  long mrow[4];
  bool mok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long r = tok0 + (l31 & ~3) + i;
    mok[i] = r < p.M;
    mrow[i] = mok[i] ? r : p.M - 1;
  }
  const long bi = ((long)lbid * NW * 32) / p.rows_per_batch;            // the workgroup's batch item (uniform)
  const char* kvb = reinterpret_cast<const char*>(p.kv) + bi * (8 * KVH);

  // every stage is 24 KiB = 6 pieces per wave, unconditionally (a 21-KiB weight tile drags the next 3 KiB along: the packed streams are
  // padded by 3 KiB): the same number of vector-memory operations per wave and stage, so the stage waits below can be COUNTED.
  // FOUR waves per workgroup and 72 KiB of LDS: two workgroups share a CU and drift apart, so one's memory phases (row loads, residual
  // re-read, stores: 26 of the first version's 57 us with one 8-wave workgroup per CU) run under the other's MFMA phases.
  static_assert(NW == 4, "six 1-KiB pieces per wave and stage");
  auto issue = [&](const char* src, int slot) {
    const char* s0 = src + lane * 16 + wave * 1024;
    char* dst = smem + slot * SLOT + wave * 1024;
#pragma unroll
    for (int j = 0; j < 6; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s0 + j * NW * 1024),
                                       (__attribute__((address_space(3))) void*)(dst + j * NW * 1024), 16, 0, 0);
  };
  // stage st (0..27): 0-9 to_q tiles, 10-17 K / V^T of the heads, 18-27 to_out tiles; slot = st % 3, fetched TWO stages ahead
  auto issue_stage = [&](int st) {
    if (st < 10) issue(reinterpret_cast<const char*>(p.wq) + (long)st * TBW, st % 3);
    else if (st < 18) issue(kvb + (long)(st - 10) * KVH, st % 3);
    else if (st < 28) issue(reinterpret_cast<const char*>(p.wo) + (long)(st - 18) * TBW, st % 3);
  };
  // dev: phase stagger of the two co-resident workgroups of a CU (dbg 32: odd blocks, 64: second half of the grid; delay = dbg >> 8 x ~3.5 us)
  if ((RC_DBG_RT(32) && (blockIdx.x & 1)) || (RC_DBG_RT(64) && blockIdx.x >= gridDim.x / 2)) {
    for (int i = 0; i < (p.dbg >> 8); ++i) __builtin_amdgcn_s_sleep(127);
  }
  issue_stage(0);
  issue_stage(1);

  // rows -> B operands
  V8 H[KS];
  {
    const T* xp = reinterpret_cast<const T*>(p.h) + 32 * hi + 8 * qb;
#pragma unroll
    for (int s = 0; s < KS; ++s) H[s] = *reinterpret_cast<const V8*>(xp + mrow[s & 3] * p.ldh + 64 * (s >> 2));
#pragma unroll
    for (int q = 0; q < KS / 4; ++q) quad_transpose(H[4 * q], H[4 * q + 1], H[4 * q + 2], H[4 * q + 3]);
  }
  float ln_rstd, ln_std, ln_nmean;
  {
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += to_f32<T>(H[s][e]);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / 320.0f);
    float c2 = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      asm volatile("" : "+v"(H[s]));
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = to_f32<T>(H[s][e]) - mean; c2 = __builtin_fmaf(d, d, c2); }
    }
    c2 += __shfl_xor(c2, 32, 64);
    const float var = c2 * (1.0f / 320.0f) + p.ln_eps;
    ln_rstd = __builtin_amdgcn_rsqf(var);
    ln_std = var * ln_rstd;
    ln_nmean = -mean;
  }

  // stage st's pieces have landed when at most `younger` vector-memory operations of this wave are outstanding (they complete in
  // issue order): the 6 pieces of stage st + 1, and in the to_out phase the previous stage's 4 residual loads and 4 deferred stores
  auto stage_begin = [&](int st, int younger) {
    if (younger >= 22) asm volatile("s_waitcnt vmcnt(22)" ::: "memory");
    else if (younger >= 18) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    else if (younger >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (younger >= 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
    else if (younger >= 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if (younger >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (younger >= 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (younger >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!RC_DBG_RT(16)) __builtin_amdgcn_s_barrier();
    if (!RC_DBG_RT(8)) issue_stage(st + 2);
  };
  // One 32-row weight tile = a stream of 20 fragments consumed by 20 MFMAs on one accumulator, read PD steps ahead of their MFMA with the
  // order PINNED (hipcc otherwise sinks every ds_read next to its MFMA: ~150 exposed cycles per MFMA).  The accumulator is seeded from
  // the tile's vector page: v (plain) or std * v - mean * u (LayerNorm fold; times rstd at the end).
  auto tile_stream = [&](const char* cbase, const V8 (&Bop)[KS], bool fold, auto pd_c) __attribute__((always_inline)) -> f32x16 {
    constexpr int PD = decltype(pd_c)::value;
    const char* cb = cbase + lane * 16;
    const float* vec = reinterpret_cast<const float*>(cbase + KS * 1024) + 16 * hi;
    V8 a[KS];
#pragma unroll
    for (int x = 0; x < PD; ++x) a[x] = *reinterpret_cast<const V8*>(cb + x * 1024);
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(vec + 4 * g);
      if (fold) {
        const f32x4 u4 = *reinterpret_cast<const f32x4*>(vec + 32 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * g + e] = __builtin_fmaf(ln_nmean, u4[e], ln_std * v4[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * g + e] = v4[e];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int x = 0; x < KS; ++x) {
      if (x + PD < KS) a[x + PD] = *reinterpret_cast<const V8*>(cb + (x + PD) * 1024);
      __builtin_amdgcn_sched_barrier(0);
      acc = mfma32(a[x], Bop[x], acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    return acc;
  };

  // ---- to_q (LayerNorm folded): tile t = 2 c + u of chunk c gives Q[2 t], Q[2 t + 1] = B operands of the score MFMAs
  V8 Q[KS];
#pragma unroll
  for (int t = 0; t < 10; ++t) {
    stage_begin(t, 6);
    if RC_DBG_RT(1) continue;
    f32x16 acc = tile_stream(smem + (t % 3) * SLOT, H, true, std::integral_constant<int, 4>{});
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] *= ln_rstd;
    Q[2 * t] = pack8r<T>(acc, 0);
    Q[2 * t + 1] = pack8r<T>(acc, 8);
  }

  // ---- attention, one head per stage; O pieces overwrite the head's dead q pieces.  Per head a stream of 12 K fragments (key tile
  // major) and 12 V^T fragments (PV step major), each read 6 ahead of its MFMA; the V^T reads are issued before the softmax arithmetic.
  float w_ip = 1.0f;
  if (IPT > 0 && p.ip_scale != nullptr) w_ip = p.ip_scale[bi * p.ip_stride];      // bi is the workgroup's: a scalar load either way
  const float NEG = -1.0e30f;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    typename Vec<T>::v4 third0;        // head 2m's O, d = 32 .. 39 (held until head 2m+1 has read its q from the shared k-step)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      stage_begin(10 + 2 * m + hh, 6);
      if RC_DBG_RT(2) continue;
      const char* kb = smem + ((10 + 2 * m + hh) % 3) * SLOT + lane * 16;
      const char* vb = kb + 12 * 1024;
      const int s0 = 5 * m + 2 * hh;          // the head's three q k-steps: s0, s0 + 1, s0 + 2
      constexpr int NKF = 9;                  // text K fragments: (key tile, w)
      constexpr int WN = 6;
      V8 kf[NKF];
#pragma unroll
      for (int x = 0; x < WN; ++x) kf[x] = *reinterpret_cast<const V8*>(kb + x * 1024);
      f32x16 S[3];
#pragma unroll
      for (int r = 0; r < 16; ++r) { S[0][r] = 0.f; S[1][r] = 0.f; S[2][r] = 0.f; }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int x = 0; x < NKF; ++x) {
        if (x + WN < NKF) kf[x + WN] = *reinterpret_cast<const V8*>(kb + (x + WN) * 1024);
        __builtin_amdgcn_sched_barrier(0);
        S[x / 3] = mfma32(kf[x], Q[s0 + x % 3], S[x / 3]);
        __builtin_amdgcn_sched_barrier(0);
      }
      // V^T fragments in PV order: (step kk, tile u) -> block u * 6 + kk; the first six are in flight during the softmax
      constexpr int NVF = 10;
      V8 vf[NVF];
#pragma unroll
      for (int x = 0; x < WN; ++x) vf[x] = *reinterpret_cast<const V8*>(vb + ((x & 1) * 6 + (x >> 1)) * 1024);
      __builtin_amdgcn_sched_barrier(0);
      // text softmax over the registers that can hold a real key: tiles 0, 1 whole, tile 2 registers with 64 + (r & 3) + 8 (r >> 2) < TEXT
      // (hi = 1 adds 4: masked per lane half where that crosses TEXT)
      constexpr int R2 = ((TEXT - 64 + 7) / 8) * 4;          // registers of tile 2 in use (multiple of 4; <= 8 by the static_assert)
#pragma unroll
      for (int r = 0; r < R2; ++r) {
        const int k0 = 64 + (r & 3) + 8 * (r >> 2);
        if (k0 >= TEXT) S[2][r] = NEG;
        else if (k0 + 4 >= TEXT) S[2][r] = hi ? NEG : S[2][r];
      }
      float mx = NEG;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fmaxf(S[0][r], S[1][r]));
#pragma unroll
      for (int r = 0; r < R2; ++r) mx = fmaxf(mx, S[2][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
#pragma unroll
      for (int r = 0; r < 16; ++r) { S[0][r] = __builtin_amdgcn_exp2f(S[0][r] - mx); S[1][r] = __builtin_amdgcn_exp2f(S[1][r] - mx); }
#pragma unroll
      for (int r = 0; r < 8; ++r) S[2][r] = r < R2 ? __builtin_amdgcn_exp2f(S[2][r] - mx) : 0.f;
      V8 pk[5];
#pragma unroll
      for (int kk = 0; kk < 5; ++kk) pk[kk] = pack8r<T>(S[kk >> 1], 8 * (kk & 1));
      f32x16 O[2];
#pragma unroll
      for (int uu = 0; uu < 2; ++uu)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[uu][r] = 0.f;
      V8 kfi[3], vfi[2];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int x = 0; x < NVF; ++x) {
        if (x + WN < NVF) vf[x + WN] = *reinterpret_cast<const V8*>(vb + (((x + WN) & 1) * 6 + ((x + WN) >> 1)) * 1024);
        if constexpr (IPT > 0) {
          // the image tile's K fragments (blocks 9..11) and V^T fragments (step 5 of both tiles) ride behind the text stream
          if (x >= 4 && x < 7) kfi[x - 4] = *reinterpret_cast<const V8*>(kb + (9 + x - 4) * 1024);
          if (x >= 7 && x < 9) vfi[x - 7] = *reinterpret_cast<const V8*>(vb + ((x - 7) * 6 + 5) * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
        O[x & 1] = mfma32(vf[x], pk[x >> 1], O[x & 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (IPT > 0) {
        // image keys: their own softmax (second segment of the decoupled cross-attention), weight w_ip, accumulated into the same O
        f32x16 Si;
#pragma unroll
        for (int r = 0; r < 16; ++r) Si[r] = 0.f;
#pragma unroll
        for (int w = 0; w < 3; ++w) Si = mfma32(kfi[w], Q[s0 + w], Si);
        __builtin_amdgcn_sched_barrier(0);
      // rows 8 / 12 of the second tile (accumulator register 4 of both lane halves) carry sum_j p_j  (text part: scaled while the image
      // scores are in the matrix pipe)
        const float inv_t = __builtin_amdgcn_rcpf(O[1][4]);
#pragma unroll
        for (int r = 0; r < 16; ++r) O[0][r] *= inv_t;
#pragma unroll
        for (int r = 0; r < 4; ++r) O[1][r] *= inv_t;
        constexpr int RI = IPT >= 8 ? (IPT / 8) * 4 : 4;       // registers in use: keys (r & 3) + 8 (r >> 2) (+ 4 in the upper lane half)
#pragma unroll
        for (int r = 0; r < RI; ++r) {
          const int k0 = (r & 3) + 8 * (r >> 2);
          if (k0 + 4 >= IPT) Si[r] = hi ? NEG : Si[r];
        }
        float mi = NEG;
#pragma unroll
        for (int r = 0; r < RI; ++r) mi = fmaxf(mi, Si[r]);
        mi = fmaxf(mi, __shfl_xor(mi, 32, 64));
        float si = 0.f;
#pragma unroll
        for (int r = 0; r < RI; ++r) { Si[r] = __builtin_amdgcn_exp2f(Si[r] - mi); si += Si[r]; }
        si += __shfl_xor(si, 32, 64);
        const float wi = w_ip * __builtin_amdgcn_rcpf(si);
        f32x16 pi;
#pragma unroll
        for (int r = 0; r < 16; ++r) pi[r] = r < RI ? Si[r] * wi : 0.f;
        const V8 pk5 = pack8r<T>(pi, 0);
        O[0] = mfma32(vfi[0], pk5, O[0]);
        O[1] = mfma32(vfi[1], pk5, O[1]);
      } else {
        const float inv_t = __builtin_amdgcn_rcpf(O[1][4]);
#pragma unroll
        for (int r = 0; r < 16; ++r) O[0][r] *= inv_t;
#pragma unroll
        for (int r = 0; r < 4; ++r) O[1][r] *= inv_t;
      }
      // O^T -> to_out's B operands, in place of the head's q pieces
      Q[5 * m + 3 * hh] = pack8r<T>(O[0], 0);
      Q[5 * m + 3 * hh + 1] = pack8r<T>(O[0], 8);
      typename Vec<T>::v4 th;
#pragma unroll
      for (int e = 0; e < 4; ++e) th[e] = from_f32<T>(O[1][e]);
      if (hh == 0) third0 = th;
      else {
        V8 mg;
#pragma unroll
        for (int e = 0; e < 4; ++e) { mg[e] = third0[e]; mg[4 + e] = th[e]; }
        Q[5 * m + 2] = mg;
      }
    }
  }

  // ---- to_out + bias + residual
  V8 pend[4], r8[4];
#pragma unroll
  for (int c = 0; c < 5; ++c) {
#pragma unroll
    for (int uu = 0; uu < 2; ++uu) {
      const int st = 18 + 2 * c + uu;
      stage_begin(st, st == 18 ? 6 : st <= 20 ? 10 : st == 27 ? 8 : 14);
      if (uu == 0) {
        // (opaque copies of the base pointers: hipcc otherwise forms all forty row addresses of this phase in the prologue and spills them)
        const T* hp = reinterpret_cast<const T*>(p.h);
        T* outp = reinterpret_cast<T*>(p.out);
        asm volatile("" : "+s"(hp), "+s"(outp));
        const long ch0 = 64 * (long)c + 32 * hi;
        if (c > 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (mok[i]) gst<V8>(outp + mrow[i] * p.ldc + (ch0 - 64) + 8 * qb, pend[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) r8[i] = gld<V8>(hp + mrow[i] * p.ldh + ch0 + 8 * qb);
      }
      f32x16 acc;
      if (!RC_DBG_RT(4)) acc = tile_stream(smem + (st % 3) * SLOT, Q, false, std::integral_constant<int, 8>{});
      if (uu == 0) quad_transpose(r8[0], r8[1], r8[2], r8[3]);
      float o[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = acc[r] + to_f32<T>(r8[2 * uu + (r >> 3)][r & 7]);
      pend[2 * uu] = pack8<T>(o);
      pend[2 * uu + 1] = pack8<T>(o + 8);
      if (uu == 1) quad_transpose(pend[0], pend[1], pend[2], pend[3]);
    }
  }
  {
    T* outp = reinterpret_cast<T*>(p.out);
    const long ch0 = 64 * 4 + 32 * hi;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (mok[i]) *reinterpret_cast<V8*>(outp + mrow[i] * p.ldc + ch0 + 8 * qb) = pend[i];
  }
}

// K / V^T of one conditioning -> the fragment blocks rc_xattn_kernel streams: per (batch item, head) 24 blocks of 1 KiB:
//   blocks 0..11  K:   (key tile kt = blk / 3: 0..2 text keys 32 kt + r, 3 image keys r;  w = blk % 3 = the head's w-th q k-step)
//   blocks 12..23 V^T: (tile u = (blk - 12) / 6: rows d = 32 u + r;  step kk = (blk - 12) % 6: 0..4 text keys 16 kk + 8 (j >> 2) + 4 hi + (j & 3),
//                       5 image keys 8 (j >> 2) + 4 hi + (j & 3));  rows d = 40, 44 of the TEXT steps hold 1.0 for real keys (denominator)
template <typename T>
__global__ __launch_bounds__(64) void rc_kv_pack_kernel(const T* k, const T* vt, long ldt, const T* kip, const T* vtip, long ldi,
                                                      int L, int Tn, T* out) {
  typedef typename Vec<T>::v8 V8;
  const int blk = blockIdx.x % 24, h = (blockIdx.x / 24) % 8, b = blockIdx.x / (24 * 8);
  const int lane = threadIdx.x, r = lane & 31, hi = lane >> 5;
  const int inner = 320;
  V8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = from_f32<T>(0.f);
  if (blk < 12) {
    const int kt = blk / 3, w = blk % 3;
    const bool ip = kt == 3;
    const int key = ip ? r : 32 * kt + r;
    const int len = ip ? Tn : L;
    int d0 = -1;                                   // d of element j = 0 (8 consecutive d), -1: the other head's half / nothing
    if ((h & 1) == 0) d0 = w < 2 ? 16 * w + 8 * hi : (hi == 0 ? 32 : -1);
    else d0 = w == 0 ? (hi == 1 ? 0 : -1) : 8 + 16 * (w - 1) + 8 * hi;
    if (key < len && d0 >= 0) {
      const T* src = (ip ? kip + ((long)b * Tn + key) * inner : k + ((long)b * L + key) * inner) + 40 * h + d0;
      o = *reinterpret_cast<const V8*>(src);
    }
  } else {
    const int u = (blk - 12) / 6, kk = (blk - 12) % 6;
    const bool ip = kk == 5;
    const int d = 32 * u + r;
    const int len = ip ? Tn : L;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = (ip ? 0 : 16 * kk) + 8 * (j >> 2) + 4 * hi + (j & 3);
      if (key >= len) continue;
      if (d < 40) o[j] = ip ? vtip[((long)b * inner + 40 * h + d) * ldi + key] : vt[((long)b * inner + 40 * h + d) * ldt + key];
      else if (!ip && (d == 40 || d == 44)) o[j] = from_f32<T>(1.0f);
    }
  }
  *reinterpret_cast<V8*>(out + (((long)b * 8 + h) * 24 + blk) * 512 + lane * 8) = o;
}

template <typename T, int IPT>
int launch_rc_xattn(const tg_rc_xattn_desc* d, const RcXattnParams& p, hipStream_t st) {
  constexpr int NW = 4;
  const size_t lds = 3 * 24 * 1024;
  const long grid = (d->M + NW * 32 - 1) / (NW * 32);
  auto k = rc_xattn_kernel<T, NW, 77, IPT>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)attr;
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(NW * 64), lds, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

template <typename T>
int dispatch_rc_xattn(const tg_rc_xattn_desc* d, const RcXattnParams& p, hipStream_t st) {
  if (d->ip_tokens == 0) return launch_rc_xattn<T, 0>(d, p, st);
  if (d->ip_tokens == 4) return launch_rc_xattn<T, 4>(d, p, st);
  return launch_rc_xattn<T, 16>(d, p, st);
}


// ---------------------------------------------------------------------------------------------------------------------------------
// rc_front_kernel: the FRONT of a first-level Transformer2DModel in one launch (SD-1.5 geometry, 320 channels):
//     y = proj_in(GroupNorm(x)) + b;      [Q | K | V] = to_qkv(LayerNorm1(y))      (Q | K token-major [M, 640], V TRANSPOSED per batch item)
// (models/transformer_2d.py:285-296 norm + proj_in; models/attention.py:186-204 norm1 + attn1's projections; today: GroupNorm apply pass,
// proj_in launch, LayerNorm-folded q|k|v GEMM with its V^T epilogue).  GroupNorm arrives as per-(image, channel) coefficients (a, d) from
// tg_groupnorm_coef — the statistics pass stays a launch, the normalised tensor never exists: x * a + d is applied to the row registers
// (fp32, one rounding: what the apply pass stores).  40 weight tiles through the 3 x 24-KiB ring: 10 of proj_in, 30 of the LayerNorm-folded
// q|k|v; y, Q | K leave through quad-transposed 128-byte-line stores (deferred by one stage), V^T through 2-byte stores (lane = token is the
// contiguous direction of V^T: 64 bytes per channel and wave).
struct RcFrontParams {
  const void* x;          // [M, 320] block input (token-major)
  long ldx;
  const float* coef;      // fp32 [batch][2][320]: a, d of tg_groupnorm_coef
  const void* win;        // proj_in: rc_pack_tiles stream (10 tiles)
  const void* wqkv;       // LayerNorm-folded to_q ; to_k ; to_v: rc_pack_tiles stream (30 tiles, v / u pages)
  void* y;                // [M, 320]
  long ldy;
  void* qk;               // [M, 640]
  long ldqk;
  void* vt;               // [batch, 320, ldt]
  long ldt;
  long M;
  int rows_per_batch;
  float ln_eps;
};

// NW = 4: two 128-token workgroups per CU, ring of 3 stages (fetched 2 ahead)
template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void rc_front_kernel(RcFrontParams p) {
  typedef typename Vec<T>::v8 V8;
  constexpr int KS = 20, NST = 40;
  constexpr int DEPTH = 2, NSLOT = DEPTH + 1, PPW = 24 / NW;
  constexpr int TBW = (KS + 1) * 1024, SLOT = 24 * 1024;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int lbid = rc_block_id((int)blockIdx.x, (int)gridDim.x);
  const long tok0 = ((long)lbid * NW + wave) * 32;
  const int qb = lane & 3;
  long mrow[4];
  bool mok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long r = tok0 + (l31 & ~3) + i;
    mok[i] = r < p.M;
    mrow[i] = mok[i] ? r : p.M - 1;
  }
  const long bi = ((long)lbid * NW * 32) / p.rows_per_batch;            // the workgroup's batch item (uniform)
  auto issue_stage = [&](int st) __attribute__((always_inline)) {
    if (st >= NST) return;
    const char* src = (st < 10 ? reinterpret_cast<const char*>(p.win) + (long)st * TBW
                               : reinterpret_cast<const char*>(p.wqkv) + (long)(st - 10) * TBW) + lane * 16 + wave * 1024;
    char* dst = smem + (st % NSLOT) * SLOT + wave * 1024;
#pragma unroll
    for (int j = 0; j < PPW; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + j * NW * 1024),
                                       (__attribute__((address_space(3))) void*)(dst + j * NW * 1024), 16, 0, 0);
  };
  issue_stage(0);
  issue_stage(1);

  // rows -> registers, GroupNorm applied in place (fp32 x * a + d, one rounding), B-operand layout
  V8 X[KS];
  {
    const T* xp = reinterpret_cast<const T*>(p.x) + 32 * hi + 8 * qb;
#pragma unroll
    for (int s = 0; s < KS; ++s) X[s] = *reinterpret_cast<const V8*>(xp + mrow[s & 3] * p.ldx + 64 * (s >> 2));
#pragma unroll
    for (int q = 0; q < KS / 4; ++q) quad_transpose(X[4 * q], X[4 * q + 1], X[4 * q + 2], X[4 * q + 3]);
    // the batch item's 2 x 320 coefficients through LDS (behind the ring): one coalesced 2.5-KiB load per workgroup, broadcast reads
    float* cl = reinterpret_cast<float*>(smem + NSLOT * SLOT);
    if (tid < 160) *reinterpret_cast<f32x4*>(cl + 4 * tid) = *reinterpret_cast<const f32x4*>(p.coef + bi * 640 + 4 * tid);
    __syncthreads();
    const float* ca = cl + 32 * hi;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float* c0 = ca + 64 * (s >> 2) + 8 * (s & 3);
      float f[8];
#pragma unroll
      for (int h4 = 0; h4 < 2; ++h4) {
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(c0 + 4 * h4);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(c0 + 320 + 4 * h4);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[4 * h4 + e] = __builtin_fmaf(to_f32<T>(X[s][4 * h4 + e]), a4[e], d4[e]);
      }
      X[s] = pack8<T>(f);
    }
  }

  float ln_rstd = 1.f, ln_std = 1.f, ln_nmean = 0.f;
  // stores produced by stage k (issued at the top of stage k + 1): a finished 64-channel chunk = 4 x 16 bytes, a V tile = 16 x 2 bytes
  auto n_stores = [](int k) { return k < 10 ? 0 : k < 30 ? ((k & 1) ? 4 : 0) : k < NST ? 16 : 0; };
  // y stores issued IN stage k (right behind its weight pieces): chunk k - 10 of the finished proj_in output, once the rows' registers are free
  auto y_stores = [](int k) { return k >= 10 && k < 15 ? 4 : 0; };
  // operations issued behind stage st's pieces when stage st begins: the deferred stores of stages st - DEPTH - 1 .. st - 2 and the pieces of the stages
  // fetched since (st + 1 .. st + DEPTH - 1)
  auto younger_of = [&](int st) __attribute__((always_inline)) {
    int y = 0;
    for (int k = st - DEPTH - 1; k <= st - 2; ++k) y += n_stores(k);
    for (int k = st - DEPTH; k <= st - 1; ++k) y += y_stores(k);
    for (int j = st + 1; j <= st + DEPTH - 1; ++j) y += j < NST ? PPW : 0;
    return y;
  };
  // counted wait (the value is a compile-time constant after unrolling)
  auto wait_vm = [&](int n) __attribute__((always_inline)) {
    switch (n) {
#define TG_VM_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
      TG_VM_CASE(1) TG_VM_CASE(2) TG_VM_CASE(3) TG_VM_CASE(4) TG_VM_CASE(5) TG_VM_CASE(6) TG_VM_CASE(7) TG_VM_CASE(8) TG_VM_CASE(9) TG_VM_CASE(10) TG_VM_CASE(11) TG_VM_CASE(12) TG_VM_CASE(13) TG_VM_CASE(14) TG_VM_CASE(15)
      TG_VM_CASE(16) TG_VM_CASE(17) TG_VM_CASE(18) TG_VM_CASE(19) TG_VM_CASE(20) TG_VM_CASE(21) TG_VM_CASE(22) TG_VM_CASE(23) TG_VM_CASE(24) TG_VM_CASE(25) TG_VM_CASE(26) TG_VM_CASE(27) TG_VM_CASE(28) TG_VM_CASE(29) TG_VM_CASE(30) TG_VM_CASE(31)
      TG_VM_CASE(32) TG_VM_CASE(33) TG_VM_CASE(34) TG_VM_CASE(35) TG_VM_CASE(36) TG_VM_CASE(37) TG_VM_CASE(38) TG_VM_CASE(39) TG_VM_CASE(40) TG_VM_CASE(41) TG_VM_CASE(42) TG_VM_CASE(43) TG_VM_CASE(44) TG_VM_CASE(45) TG_VM_CASE(46) TG_VM_CASE(47)
      TG_VM_CASE(48) TG_VM_CASE(49) TG_VM_CASE(50) TG_VM_CASE(51) TG_VM_CASE(52) TG_VM_CASE(53) TG_VM_CASE(54) TG_VM_CASE(55) TG_VM_CASE(56) TG_VM_CASE(57) TG_VM_CASE(58) TG_VM_CASE(59) TG_VM_CASE(60) TG_VM_CASE(61) TG_VM_CASE(62) TG_VM_CASE(63)
#undef TG_VM_CASE
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };
  V8 pend[4];
  auto flush = [&](int k) __attribute__((always_inline)) {      // the stores of stage k
    if (k < 0 || n_stores(k) == 0) return;
    if (k < 30) {
      T* base = reinterpret_cast<T*>(p.qk);
      asm volatile("" : "+s"(base));
      const long ch0 = 64 * (long)((k - 10) >> 1) + 32 * hi;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (mok[i]) gst<V8>(base + mrow[i] * p.ldqk + ch0 + 8 * qb, pend[i]);
    } else {
      // V tile t = k - 30 (chunk c = t >> 1, tile u = t & 1): register rho = channel 64 c + 32 hi + 16 u + rho, lane = token
      T* vb = reinterpret_cast<T*>(p.vt);
      asm volatile("" : "+s"(vb));
      const int t = k - 30;
      const long tok = tok0 + l31;
      const long tin = tok - bi * p.rows_per_batch;
      T* vrow = vb + (bi * 320 + 64 * (t >> 1) + 32 * hi + 16 * (t & 1)) * p.ldt + tin;
      if (tok < p.M) {
#pragma unroll
        for (int r = 0; r < 16; ++r) gst<T>(vrow + (long)r * p.ldt, pend[r >> 3][r & 7]);
      }
    }
  };
  auto stage_begin = [&](int st) __attribute__((always_inline)) {
    wait_vm(younger_of(st));
    __builtin_amdgcn_s_barrier();
    issue_stage(st + DEPTH);
    flush(st - 1);
  };
  auto tile_stream = [&](const char* cbase, const V8 (&Bop)[KS], bool fold, auto pd_c) __attribute__((always_inline)) -> f32x16 {
    constexpr int PD = decltype(pd_c)::value;      // fragment read-ahead: 4 while the rows AND the growing outputs are live, 8 after
    const char* cb = cbase + lane * 16;
    const float* vec = reinterpret_cast<const float*>(cbase + KS * 1024) + 16 * hi;
    V8 a[KS];
#pragma unroll
    for (int x = 0; x < PD; ++x) a[x] = *reinterpret_cast<const V8*>(cb + x * 1024);
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(vec + 4 * g);
      if (fold) {
        const f32x4 u4 = *reinterpret_cast<const f32x4*>(vec + 32 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * g + e] = __builtin_fmaf(ln_nmean, u4[e], ln_std * v4[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * g + e] = v4[e];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int x = 0; x < KS; ++x) {
      if (x + PD < KS) a[x + PD] = *reinterpret_cast<const V8*>(cb + (x + PD) * 1024);
      __builtin_amdgcn_sched_barrier(0);
      acc = mfma32(a[x], Bop[x], acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    return acc;
  };

  // ---- proj_in: Y = B operands of the q|k|v phase, and the stream the block's residual adds read back
  // (y itself is stored from the first five q | k | v stages: while the rows AND the growing Y are live there is no room for transposed copies)
  V8 Y[KS];
#pragma unroll
  for (int t = 0; t < 10; ++t) {
    stage_begin(t);
    const f32x16 acc = tile_stream(smem + (t % NSLOT) * SLOT, X, false, std::integral_constant<int, 4>{});
    Y[2 * t] = pack8r<T>(acc, 0);
    Y[2 * t + 1] = pack8r<T>(acc, 8);
    // opaque: hipcc otherwise ALSO keeps the sixteen rounded values unpacked for the LayerNorm statistics below (160 registers, all spilled)
    asm volatile("" : "+v"(Y[2 * t]), "+v"(Y[2 * t + 1]));
  }
  {
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += to_f32<T>(Y[s][e]);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / 320.0f);
    float c2 = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      asm volatile("" : "+v"(Y[s]));
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = to_f32<T>(Y[s][e]) - mean; c2 = __builtin_fmaf(d, d, c2); }
    }
    c2 += __shfl_xor(c2, 32, 64);
    const float var = c2 * (1.0f / 320.0f) + p.ln_eps;
    ln_rstd = __builtin_amdgcn_rsqf(var);
    ln_std = var * ln_rstd;
    ln_nmean = -mean;
  }
  // ---- q | k | v (LayerNorm folded).  The rounding / packing / transposing of tile t - 1 runs in stage t BEHIND the first fragment and seed
  // reads of tile t (a lone wave otherwise sits out one LDS round trip per stage before its first MFMA), its stores right behind that.
  V8 half[2];
  auto qkv_epilogue = [&](int t, f32x16 acc) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] *= ln_rstd;
    if (t < 20) {
      if (t & 1) {
        pend[0] = half[0]; pend[1] = half[1]; pend[2] = pack8r<T>(acc, 0); pend[3] = pack8r<T>(acc, 8);
        quad_transpose(pend[0], pend[1], pend[2], pend[3]);
      } else {
        half[0] = pack8r<T>(acc, 0); half[1] = pack8r<T>(acc, 8);
      }
    } else {
      pend[0] = pack8r<T>(acc, 0); pend[1] = pack8r<T>(acc, 8);
    }
  };
  auto y_chunk_store = [&](int c) __attribute__((always_inline)) {
    V8 t0 = Y[4 * c], t1 = Y[4 * c + 1], t2 = Y[4 * c + 2], t3 = Y[4 * c + 3];
    quad_transpose(t0, t1, t2, t3);
    T* base = reinterpret_cast<T*>(p.y);
    asm volatile("" : "+s"(base));
    const long ch0 = 64 * (long)c + 32 * hi + 8 * qb;
    if (mok[0]) gst<V8>(base + mrow[0] * p.ldy + ch0, t0);
    if (mok[1]) gst<V8>(base + mrow[1] * p.ldy + ch0, t1);
    if (mok[2]) gst<V8>(base + mrow[2] * p.ldy + ch0, t2);
    if (mok[3]) gst<V8>(base + mrow[3] * p.ldy + ch0, t3);
  };
  f32x16 acc_prev;
#pragma unroll
  for (int t = 0; t < 30; ++t) {
    const int st = 10 + t;
    wait_vm(younger_of(st));
    __builtin_amdgcn_s_barrier();
    issue_stage(st + DEPTH);
    if (y_stores(st)) { y_chunk_store(t); __builtin_amdgcn_sched_barrier(0); }
    constexpr int PD = 8;
    const char* cbase = smem + (st % NSLOT) * SLOT;
    const char* cb = cbase + lane * 16;
    const float* vec = reinterpret_cast<const float*>(cbase + KS * 1024) + 16 * hi;
    V8 a[KS];
#pragma unroll
    for (int x = 0; x < PD; ++x) a[x] = *reinterpret_cast<const V8*>(cb + x * 1024);
    f32x4 v4[4], u4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { v4[g] = *reinterpret_cast<const f32x4*>(vec + 4 * g); u4[g] = *reinterpret_cast<const f32x4*>(vec + 32 + 4 * g); }
    __builtin_amdgcn_sched_barrier(0);
    if (t > 0) qkv_epilogue(t - 1, acc_prev);
    flush(st - 1);
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[4 * g + e] = __builtin_fmaf(ln_nmean, u4[g][e], ln_std * v4[g][e]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int x = 0; x < KS; ++x) {
      if (x + PD < KS) a[x + PD] = *reinterpret_cast<const V8*>(cb + (x + PD) * 1024);
      __builtin_amdgcn_sched_barrier(0);
      acc = mfma32(a[x], Y[x], acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    acc_prev = acc;
  }
  qkv_epilogue(29, acc_prev);
  flush(NST - 1);
}

template <typename T>
int launch_rc_front(const tg_rc_front_desc* d, const RcFrontParams& p, hipStream_t st) {
  const size_t lds = 3 * 24 * 1024 + 2560;
  auto k = rc_front_kernel<T, 4>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)attr;
  hipLaunchKernelGGL(k, dim3((unsigned)((d->M + 127) / 128)), dim3(256), lds, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

// (Round 4's rc_linear_wide_kernel — the K = 640 projections of the 32 x 32 level in row-chain form, one wave per SIMD — measured 37.3 us against tg_gemm's
// 30.2 on 16384 x 640 x 640 + residual and was never selected; removed in round 5, where the 128 x 160 tiles take the same launches in 27.4 us.)
// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{})  (asm immediates need constants)
template <int... X, class F> __device__ __forceinline__ void static_for_impl(std::integer_sequence<int, X...>, F&& f) {
  (f(std::integral_constant<int, X>{}), ...);
}
template <int N, class F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }
// fragment read / counted wait as asm: hipcc waits lgkmcnt(0) in front of most MFMAs of a long read-ahead stream (every such wait exposes a
// full LDS round trip: the read-ahead would hide nothing); the wait is tied to the fragment register so the MFMA cannot be moved above it
template <int OFF, typename V8> __device__ __forceinline__ void lds_read16(V8& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
template <int N, typename V8> __device__ __forceinline__ void lds_wait(V8& frag) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(frag) : "n"(N));
}
// one wait for the three fragments of a slot group (every asm statement costs its own issue slot plus the s_nop hipcc puts behind it)
template <int N, typename V8> __device__ __forceinline__ void lds_wait3(V8& f0, V8& f1, V8& f2) {
  asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(f0), "+v"(f1), "+v"(f2) : "n"(N));
}

struct RcFfParams {
  const void* h;        // [M, 320] the stream before norm3 (= the residual)
  long ldh;
  const void* w1;       // rowchain.pack_ff2: n_slices x 41 KiB (+ 3 KiB pad)
  const void* w2;       // n_slices x 20 KiB, of the same pack function
  const float* b2;      // fp32 [320]
  const void* wpo;      // proj_out as rowchain.pack_po2 stream, or NULL (then `out` = h3)
  const void* res0;     // [M, 320] residual of proj_out
  long ldres;
  void* out;
  long ldc;
  long M;
  int n_slices;         // inner / 32, even, >= 2
  float ln_eps;
};

// ---------------------------------------------------------------------------------------------------------------------------------
// rc_ff2_kernel: norm3 + FeedForward (GEGLU) + residual, and optionally Transformer2DModel.proj_out + its residual, of a first-level block
// in ONE launch (reference models/attention.py:226-236 `ff(norm3(x)) + x`, :328-338 GEGLU; models/transformer_2d.py:316-327 proj_out):
//     h3 = net2( a * gelu(g) ) + b2 + h,   [a | g] = proj(LayerNorm(h)) + b1;        out = proj_out(h3) + b + res0
// As separate launches: layernorm (16 us) + 256 x 256 GEGLU GEMM (148 us at 65536 tokens: K = 320 is five K-tiles long) + net.2 GEMM (92 us) +
// proj_out (27-39 us), and the [tokens, 1280] hidden tensor (168 MB) written and read back.  Here the hidden activations exist 32 channels at a time,
// in the registers of the wave that owns the tokens: per 32-channel SLICE j the wave runs 40 MFMAs of proj (20 value + 20 gate fragments over the
// normalised rows), GEGLU on the accumulator registers, and 20 MFMAs of net.2 (20 output tiles of 16 channels, one k-step of 32) into accumulators that
// live for the whole kernel.
// TWO waves per SIMD: a single wave per SIMD (the retired one-wave kernel of 32-token waves on 32x32x16 MFMAs, profiles/rc_ff2_findings.md) runs this
// interleaved stream at the SUM of its MFMA and VALU issue times (profiles/r4_rowchain_findings.md) and sits in its row-load / store phases with nothing
// else on the SIMD.  ONE 8-wave workgroup per CU shares one weight stream of 128 tokens, and a wave owns 16 tokens on v_mfma_f32_16x16x32: 80 net.2
// accumulator registers (20 tiles of 16 channels), two projection slots of 16, the normalised rows as 10 B pieces of 32 channels — within 256 registers.
// Pipeline, software-pipelined by hand and pinned by sched_barrier: iteration j issues, interleaved 2 : 1, proj(j)'s 40 MFMAs and net.2(j - 2)'s 20
// MFMAs (60 slots), and between consecutive MFMAs the micro-steps of GEGLU(j - 1) (8 elements x 4 parts = 32 per iteration, a few VALU instructions each).
// LDS (128 KiB): two 44-KiB proj slots (41 KiB of a slice + 3 KiB of the next slice / the pad) + two 20-KiB net.2 slots, filled by LDS-DMA one iteration
// ahead; the proj_out phase reuses them as a ring of three 24-KiB stages (21 KiB used).  Fragment reads are asm ds_read_b128 with counted lgkmcnt waits
// (lds_read16 / lds_wait above): hipcc's own waits are lgkmcnt(0) in front of most MFMAs, which turns the nine-slot read-ahead into one LDS round
// trip per MFMA.
// Index maps (n = lane & 15 the token, g = lane >> 4, e = element of a 16-byte piece):
//   rows as B operand, k-step s                 lane (n, g) element e = channel 32 s + 8 g + e                    (16 contiguous bytes of the row)
//   proj tile (value / gate, u) of slice j      MFMA row r = hidden channel 32 j + 16 u + r; accumulator register i of lane group g = row 4 g + i
//   hidden piece of slice j (net.2's B operand) element e = [u = e >> 2][i = e & 3] = hidden channel 32 j + 16 (e >> 2) + 4 g + (e & 3)
//   net.2 / proj_out tile t = 2 s + u           MFMA row r = output channel 32 s + 8 (r >> 2) + 4 u + (r & 3): registers i of tiles 2 s, 2 s + 1 of lane
//                                               group g ARE elements 0..3, 4..7 of the rows' B piece s (the residual, proj_out's operand, the store)
// Streams: rowchain.pack_ff2 (41 KiB + 20 KiB per slice) / pack_po2 (21 KiB per stage), fragments in the order above; fragment k = 2 s + u so that
// consecutive MFMAs of one kind alternate between two accumulators.
template <typename T, bool PROJ>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void rc_ff2_kernel(RcFfParams p) {
  typedef typename Vec<T>::v8 V8;
  constexpr int KS = 10, NW = 8;
  constexpr int W1B = 41 * 1024, W1SLOT = 44 * 1024, W2B = 20 * 1024;
  constexpr int W2OFF = 2 * W1SLOT;
  constexpr int TBW = 21 * 1024, SLOT = 24 * 1024;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int lbid = rc_block_id((int)blockIdx.x, (int)gridDim.x);
  const long tok = ((long)lbid * NW + wave) * 16 + n;
  const bool ok = tok < p.M;
  const long row = ok ? tok : p.M - 1;
  const int NS = p.n_slices;
  const char* w1g = reinterpret_cast<const char*>(p.w1) + lane * 16 + wave * 1024;
  const char* w2g = reinterpret_cast<const char*>(p.w2) + lane * 16 + wave * 1024;
  auto issue_w1 = [&](int j) __attribute__((always_inline)) {      // slice j -> proj slot j & 1: 44 KiB-pieces over 8 waves (41 KiB + 3 KiB of the next slice / the pad)
    const char* s0 = w1g + (long)j * W1B;
    char* dst = smem + (j & 1) * W1SLOT + wave * 1024;
#pragma unroll
    for (int q = 0; q < 6; ++q)
      if (q < 5 || wave < 4)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s0 + q * NW * 1024),
                                         (__attribute__((address_space(3))) void*)(dst + q * NW * 1024), 16, 0, 0);
  };
  auto issue_w2 = [&](int j) __attribute__((always_inline)) {      // slice j -> net.2 slot j & 1: 20 KiB-pieces over 8 waves
    const char* s0 = w2g + (long)j * W2B;
    char* dst = smem + W2OFF + (j & 1) * W2B + wave * 1024;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (q < 2 || wave < 4)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s0 + q * NW * 1024),
                                         (__attribute__((address_space(3))) void*)(dst + q * NW * 1024), 16, 0, 0);
  };
  issue_w1(0);

  // the wave's 16 rows -> normalised B pieces (what norm3 hands to the feed-forward); the rows themselves are read again for the residual
  V8 HN[KS];
  {
    V8 H[KS];
    const T* xp = reinterpret_cast<const T*>(p.h) + row * p.ldh + 8 * g;
#pragma unroll
    for (int s = 0; s < KS; ++s) H[s] = *reinterpret_cast<const V8*>(xp + 32 * s);
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += to_f32<T>(H[s][e]);
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / 320.0f);
    float c2 = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      asm volatile("" : "+v"(H[s]));
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = to_f32<T>(H[s][e]) - mean; c2 = __builtin_fmaf(d, d, c2); }
    }
    c2 += __shfl_xor(c2, 16, 64);
    c2 += __shfl_xor(c2, 32, 64);
    const float rstd = __builtin_amdgcn_rsqf(c2 * (1.0f / 320.0f) + p.ln_eps);
    const float nm = -mean * rstd;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      asm volatile("" : "+v"(H[s]));
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = __builtin_fmaf(to_f32<T>(H[s][e]), rstd, nm);
      HN[s] = pack8<T>(f);
    }
  }
  // net.2's accumulators for the whole kernel: tile t = 2 s + u, register i <-> channel 32 s + 8 g + 4 u + i; seeded with b2
  f32x4 out[20];
#pragma unroll
  for (int t = 0; t < 20; ++t) out[t] = *reinterpret_cast<const f32x4*>(p.b2 + 32 * (t >> 1) + 8 * g + 4 * (t & 1));

  f32x4 acc_a[2][2], acc_g[2][2];
  V8 hid[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) hid[q][e] = from_f32<T>(0.f);

  // one pipeline iteration: proj(j) [F1], GEGLU(j - 1) [GG], net.2(j - 2) [F2]; PAR = j & 1 selects slots / accumulator sets
  auto iteration = [&](int j, auto par_c, auto f1_c, auto gg_c, auto f2_c) __attribute__((always_inline)) {
    constexpr int PAR = decltype(par_c)::value;
    constexpr bool F1 = decltype(f1_c)::value, GG = decltype(gg_c)::value, F2 = decltype(f2_c)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (j + 1 < NS) issue_w1(j + 1);
    if (j >= 1 && j - 1 < NS) issue_w2(j - 1);
    // slot x = 3 k + {0: value fragment k, 1: gate fragment k, 2: net.2 tile k}, k = 2 s + u for the projections; the fragment of slot x is read
    // LA slots ahead of its MFMA (asm reads, counted waits: see lds_read16)
    constexpr int LA = 9;
    const unsigned lbase = (unsigned)reinterpret_cast<size_t>((__attribute__((address_space(3))) char*)smem);
    const unsigned a1 = lbase + PAR * W1SLOT + lane * 16, a2 = lbase + W2OFF + PAR * W2B + lane * 16;
    V8 fr[60];
    auto rd = [&](auto xc) __attribute__((always_inline)) {
      constexpr int x = decltype(xc)::value;
      constexpr int k = x / 3, w = x % 3;
      if constexpr (w == 0) { if constexpr (F1) lds_read16<k * 1024>(fr[x], a1); }
      else if constexpr (w == 1) { if constexpr (F1) lds_read16<(20 + k) * 1024>(fr[x], a1); }
      else { if constexpr (F2) lds_read16<k * 1024>(fr[x], a2); }
    };
    // the projection accumulators start from the slice's bias page (register i of lane group g <- bias[16 u + 4 g + i]): asm reads as well, IN FRONT of the
    // fragment reads (LDS returns in order: they have landed with slot 0's fragment) — a plain load here costs an lgkmcnt(0) over the whole read-ahead
    if constexpr (F1) {
      const unsigned ap = lbase + PAR * W1SLOT + 40 * 1024 + g * 16;
      lds_read16<0>(acc_a[PAR][0], ap);
      lds_read16<64>(acc_a[PAR][1], ap);
      lds_read16<128>(acc_g[PAR][0], ap);
      lds_read16<192>(acc_g[PAR][1], ap);
    }
    static_for<LA>([&](auto xc) __attribute__((always_inline)) { rd(xc); });
    // GEGLU micro-step state (one element in flight).  gelu(g) = g (0.5 + 0.5 erf(g / sqrt 2)) with erf(z) = z P(z^2) on |z| <= 3 (degree-7 minimax fit
    // in z^2, |error| <= 8.1e-5, clamped beyond: erf(3) = 1 - 2.2e-5): fourteen plain VALU instructions per element and no transcendental (the quarter-rate
    // rcp + exp2 of the Abramowitz-Stegun form cost the stream more than their issue time).  8 elements x 4 parts = 32 micro-steps spread over the 60 slots
    float ge_z = 0.f, ge_t = 0.f, ge_p = 0.f;
    float hv[8];
    auto geglu_micro = [&](int mstep) __attribute__((always_inline)) {
      const int e = mstep >> 2, part = mstep & 3;
      const float a = acc_a[PAR ^ 1][e >> 2][e & 3], gt = acc_g[PAR ^ 1][e >> 2][e & 3];
      if (part == 0) {
        ge_z = __builtin_amdgcn_fmed3f(gt * 0.70710678118654752440f, -3.0f, 3.0f);
        ge_t = ge_z * ge_z;
      } else if (part == 1) {
        float q = __builtin_fmaf(-4.0553346e-07f, ge_t, 1.7159753e-05f);
        q = __builtin_fmaf(q, ge_t, -3.1459445e-04f);
        q = __builtin_fmaf(q, ge_t, 3.3187051e-03f);
        ge_p = __builtin_fmaf(q, ge_t, -2.2685785e-02f);
      } else if (part == 2) {
        float q = __builtin_fmaf(ge_p, ge_t, 1.0771781e-01f);
        q = __builtin_fmaf(q, ge_t, -3.7323141e-01f);
        q = __builtin_fmaf(q, ge_t, 1.1278958f);
        ge_p = q * ge_z;                                     // erf(g / sqrt 2)
      } else {
        hv[e] = a * gt * __builtin_fmaf(0.5f, ge_p, 0.5f);
        if (e == 7) hid[PAR ^ 1] = pack8<T>(hv);
      }
    };
    __builtin_amdgcn_sched_barrier(0);
    static_for<60>([&](auto xc) __attribute__((always_inline)) {
      constexpr int x = decltype(xc)::value;
      constexpr int k = x / 3, w = x % 3;
      constexpr bool act = (w == 2) ? F2 : F1;
      if constexpr (F1 && F2) {
        if constexpr (w == 0) {      // the three reads of the group LA slots ahead, in one go
          if constexpr (x + LA < 60) rd(std::integral_constant<int, (x + LA < 60 ? x + LA : 59)>{});
          if constexpr (x + LA + 1 < 60) rd(std::integral_constant<int, (x + LA + 1 < 60 ? x + LA + 1 : 59)>{});
          if constexpr (x + LA + 2 < 60) rd(std::integral_constant<int, (x + LA + 2 < 60 ? x + LA + 2 : 59)>{});
        }
      } else {
        if constexpr (x + LA < 60) rd(std::integral_constant<int, (x + LA < 60 ? x + LA : 59)>{});
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (act) {
        // reads issued after this slot's: the active slots in (x, min(59, x + LA)]
        constexpr int hi_x = x + LA < 60 ? x + LA : 59;
        constexpr int n_f1 = ((hi_x / 3) * 2 + (hi_x % 3 >= 1 ? 2 : 1)) - ((x / 3) * 2 + (x % 3 >= 1 ? 2 : 1));
        constexpr int n_f2 = (hi_x + 1) / 3 - (x + 1) / 3;
        constexpr int younger = (F1 ? n_f1 : 0) + (F2 ? n_f2 : 0);
        if constexpr (F1 && F2) {
          // steady state: one wait per slot group (value, gate, net.2 fragments of k): counted for the group's LAST fragment
          if constexpr (w == 0) {
            constexpr int hi3 = x + 2 + LA < 60 ? x + 2 + LA : 59;
            lds_wait3<(hi3 - (x + 2) > 15 ? 15 : hi3 - (x + 2))>(fr[x], fr[x + 1], fr[x + 2]);
          }
        } else {
          lds_wait<(younger > 15 ? 15 : younger)>(fr[x]);
        }
        if constexpr (F1 && x == 0) asm volatile("" : "+v"(acc_a[PAR][0]), "+v"(acc_a[PAR][1]), "+v"(acc_g[PAR][0]), "+v"(acc_g[PAR][1]));
        if constexpr (w == 0) acc_a[PAR][k & 1] = mfma16(fr[x], HN[k >> 1], acc_a[PAR][k & 1]);
        else if constexpr (w == 1) acc_g[PAR][k & 1] = mfma16(fr[x], HN[k >> 1], acc_g[PAR][k & 1]);
        else out[k] = mfma16(fr[x], hid[PAR], out[k]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (GG) {
        constexpr int m0 = 32 * x / 60, m1 = 32 * (x + 1) / 60;     // 0 or 1 micro-steps per slot
        if constexpr (m1 > m0) {
          geglu_micro(m0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    });
    // anchor: the hidden piece is consumed one iteration later, in another basic block — without a use HERE the compiler sinks this iteration's GEGLU
    // arithmetic down to that block (one lump of VALU instructions with the matrix pipe idle)
    if constexpr (GG) asm volatile("" :: "v"(hid[PAR ^ 1]));
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  using Tt = std::true_type;
  using Ff = std::false_type;
  iteration(0, C0{}, Tt{}, Ff{}, Ff{});
  iteration(1, C1{}, Tt{}, Tt{}, Ff{});
  for (int j = 2; j < NS; j += 2) {
    iteration(j, C0{}, Tt{}, Tt{}, Tt{});
    iteration(j + 1, C1{}, Tt{}, Tt{}, Tt{});
  }
  iteration(NS, C0{}, Ff{}, Tt{}, Tt{});
  iteration(NS + 1, C1{}, Ff{}, Ff{}, Tt{});

  // h3 = net.2 + b2 + h: the rows are read again (L2 / Infinity Cache); their B piece s IS the register layout of tiles 2 s, 2 s + 1
  {
    const T* hb = reinterpret_cast<const T*>(p.h);
    asm volatile("" : "+s"(hb));
    const T* xp = hb + row * p.ldh + 8 * g;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const V8 hr = gld<V8>(xp + 32 * s);
#pragma unroll
      for (int e = 0; e < 8; ++e) out[2 * s + (e >> 2)][e & 3] += to_f32<T>(hr[e]);
    }
  }
  auto pack_rows = [&](int s) __attribute__((always_inline)) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = out[2 * s + (e >> 2)][e & 3];
    return pack8<T>(f);
  };

  T* outp = reinterpret_cast<T*>(p.out);
  if constexpr (!PROJ) {
    asm volatile("" : "+s"(outp));
    T* op = outp + row * p.ldc + 8 * g;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const V8 pc = pack_rows(s);
      if (ok) gst<V8>(op + 32 * s, pc);
    }
  } else {
    // proj_out over the rounded h3 rows: 10 stages of 32 output channels (20 fragments + the bias page = 21 KiB) in a ring of three 24-KiB slots (the
    // feed-forward slots are dead behind this barrier); every wave moves 3 KiB of a stage
    V8 HB[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) HB[s] = pack_rows(s);
    const char* wpg = reinterpret_cast<const char*>(p.wpo) + lane * 16 + wave * 1024;
    auto issue_po = [&](int st) __attribute__((always_inline)) {
      if (st >= 10) return;
      const char* s0 = wpg + (long)st * TBW;
      char* dst = smem + (st % 3) * SLOT + wave * 1024;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s0 + q * NW * 1024),
                                         (__attribute__((address_space(3))) void*)(dst + q * NW * 1024), 16, 0, 0);
    };
    __builtin_amdgcn_s_barrier();
    issue_po(0);
    issue_po(1);
    const T* rp = reinterpret_cast<const T*>(p.res0);
    asm volatile("" : "+s"(rp), "+s"(outp));
    rp += row * p.ldres + 8 * g;
    T* op = outp + row * p.ldc + 8 * g;
    const unsigned pbase = (unsigned)reinterpret_cast<size_t>((__attribute__((address_space(3))) char*)smem) + lane * 16;
#pragma unroll
    for (int st = 0; st < 10; ++st) {
      // stage st has landed when at most `younger` vector-memory operations are outstanding.  Counted are only the operations EVERY wave issues behind
      // the stage's three pieces — later stages' pieces and the residual loads (clamped rows: unconditional); the stores are predicated and may be
      // absent, so they are not counted (when present the wait is slightly early, never late).
      //   order: P0 P1 | st 0: L0 P2 (S0) | st 1: L1 P3 (S1) | ...   behind P(st): L(st - 1), P(st + 1)
      if (st == 0) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else if (st == 9) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // the residual piece as an asm load with its own counted wait (behind it: the three pieces of stage st + 2): hipcc's wait for a load that sits between
      // LDS-DMA issues is vmcnt(0), which would end every stage on the round trip of the prefetch it has just issued
      V8 r8;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r8) : "v"(rp + 32 * st) : "memory");
      issue_po(st + 2);
      // fragments and the bias page by asm reads with counted waits (see lds_read16; a plain LDS load behind the stage's LDS-DMA issue makes hipcc wait
      // vmcnt(0) in front of it: the prefetch would not be one)
      const unsigned cb = pbase + (st % 3) * SLOT;
      constexpr int PD = 8;
      V8 a[20];
      f32x4 acc[2];
      lds_read16<20 * 1024>(acc[0], cb - lane * 16 + g * 16);
      lds_read16<20 * 1024 + 64>(acc[1], cb - lane * 16 + g * 16);
      static_for<PD>([&](auto xc) __attribute__((always_inline)) { constexpr int x = decltype(xc)::value; lds_read16<x * 1024>(a[x], cb); });
      __builtin_amdgcn_sched_barrier(0);
      static_for<20>([&](auto xc) __attribute__((always_inline)) {
        constexpr int x = decltype(xc)::value;
        if constexpr (x + PD < 20) lds_read16<(x + PD < 20 ? x + PD : 0) * 1024>(a[x + PD < 20 ? x + PD : 0], cb);
        lds_wait<(x + PD < 20 ? PD : 19 - x)>(a[x]);
        if constexpr (x == 0) asm volatile("" : "+v"(acc[0]), "+v"(acc[1]));
        __builtin_amdgcn_sched_barrier(0);
        acc[x & 1] = mfma16(a[x], HB[x >> 1], acc[x & 1]);
        __builtin_amdgcn_sched_barrier(0);
      });
      if (st + 2 < 10) asm volatile("s_waitcnt vmcnt(3)" : "+v"(r8));
      else asm volatile("s_waitcnt vmcnt(0)" : "+v"(r8));
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = acc[e >> 2][e & 3] + to_f32<T>(r8[e]);
      const V8 pc = pack8<T>(o);
      if (ok) gst<V8>(op + 32 * st, pc);
    }
  }
}

// one 8-wave workgroup per 128 tokens; one instantiation, hence one `static` attribute call, per kernel instance
template <typename T, bool PROJ>
int launch_rc_ff(const tg_rc_ff_desc* d, const RcFfParams& p, hipStream_t st) {
  const size_t lds = 2 * 44 * 1024 + 2 * 20 * 1024;
  auto k = rc_ff2_kernel<T, PROJ>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)attr;
  hipLaunchKernelGGL(k, dim3((unsigned)((d->M + 127) / 128)), dim3(512), lds, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

// one 8-wave workgroup per CU, two chunk buffers
template <typename T>
int launch_rc_linear(const tg_rc_linear_desc* d, const RcLinearParams& p, hipStream_t st) {
  constexpr int KS = 20, NW = 8;
  const size_t lds = (size_t)2 * (2 * KS + 1) * 1024;
  const long grid = (d->M + NW * 32 - 1) / (NW * 32);
  if (d->ln) {
    auto k = rc_linear_kernel<T, KS, NW, true>;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)attr;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(NW * 64), lds, st, p);
  } else {
    auto k = rc_linear_kernel<T, KS, NW, false>;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)attr;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(NW * 64), lds, st, p);
  }
  TG_LAUNCH_CHECK();
  return TG_OK;
}

// every row / weight-stream operand is moved in 16-byte pieces (global loads and stores, LDS-DMA, f32x4 coefficient reads)
inline bool rc_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

extern "C" int tg_rc_linear(const tg_rc_linear_desc* d, void* stream) { return tg_rc_linear_dup(d, 0, stream); }

extern "C" int tg_rc_linear_dup(const tg_rc_linear_desc* d, int64_t c_dup_offset, void* stream) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_rc_linear: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_rc_linear: dtype %d", d->dtype);
  TG_CHECK(d->K == 320, TG_ERR_ARG, "tg_rc_linear: K = %d (320: the token row lives in registers; the K = 640 variant of round 4 was removed)", d->K);
  TG_CHECK(d->N > 0 && d->N % 64 == 0, TG_ERR_ARG, "tg_rc_linear: N = %d must be a positive multiple of 64", d->N);
  TG_CHECK(d->variant == 0, TG_ERR_ARG, "tg_rc_linear: variant = %d (reserved, must be 0)", d->variant);
  TG_CHECK(d->M > 0 && d->x && d->wpk && d->out, TG_ERR_ARG, "tg_rc_linear: null operand or M <= 0");
  TG_CHECK(d->ldx >= d->K && d->ldx % 8 == 0 && d->ldc >= d->N && d->ldc % 8 == 0, TG_ERR_ARG, "tg_rc_linear: row pitches must be multiples of 8 elements");
  TG_CHECK(!d->res || (d->ldres >= d->N && d->ldres % 8 == 0), TG_ERR_ARG, "tg_rc_linear: residual pitch");
  TG_CHECK(rc_al16(d->x) && rc_al16(d->wpk) && rc_al16(d->res) && rc_al16(d->out), TG_ERR_ARG, "tg_rc_linear: x, wpk, res and out must be 16-byte aligned");
  TG_CHECK(c_dup_offset == 0 || (c_dup_offset % 8 == 0 && c_dup_offset >= (d->M - 1) * d->ldc + d->N), TG_ERR_ARG,
           "tg_rc_linear_dup: c_dup_offset = %lld must be a multiple of 8 elements past the first destination", (long long)c_dup_offset);
  RcLinearParams p;
  p.c_dup = (long)c_dup_offset;
  p.x = d->x; p.ldx = d->ldx; p.wpk = d->wpk; p.res = d->res; p.ldres = d->ldres;
  p.out = d->out; p.ldc = d->ldc; p.M = d->M; p.N = d->N; p.K = d->K; p.ln_eps = d->ln_eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return launch_rc_linear<bf16_t>(d, p, st);
  return launch_rc_linear<f16_t>(d, p, st);
}

extern "C" int tg_rc_xattn_ps(const tg_rc_xattn_desc* d, int32_t ip_scale_count, void* stream) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_rc_xattn: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_rc_xattn: dtype %d", d->dtype);
  TG_CHECK(d->h && d->wq && d->kv && d->wo && d->out && d->M > 0, TG_ERR_ARG, "tg_rc_xattn: null operand or M <= 0");
  TG_CHECK(d->text_len == 77, TG_ERR_ARG, "tg_rc_xattn: %d text keys (built for CLIP's 77)", d->text_len);
  TG_CHECK(d->ip_tokens == 0 || d->ip_tokens == 4 || d->ip_tokens == 16, TG_ERR_ARG, "tg_rc_xattn: %d image tokens (0, 4 or 16)", d->ip_tokens);
  TG_CHECK(d->rows_per_batch > 0 && d->rows_per_batch % 128 == 0 && d->M % d->rows_per_batch == 0, TG_ERR_ARG,
           "tg_rc_xattn: rows_per_batch = %d must be a multiple of 128 that divides M (a workgroup's 128 tokens share one key set)", d->rows_per_batch);
  TG_CHECK(d->ldh >= 320 && d->ldh % 8 == 0 && d->ldc >= 320 && d->ldc % 8 == 0, TG_ERR_ARG, "tg_rc_xattn: row pitches");
  TG_CHECK(rc_al16(d->h) && rc_al16(d->wq) && rc_al16(d->kv) && rc_al16(d->wo) && rc_al16(d->out), TG_ERR_ARG,
           "tg_rc_xattn: h, wq, kv, wo and out must be 16-byte aligned");
  TG_CHECK(ip_scale_count == 0 || ip_scale_count == 1 || ip_scale_count == d->M / d->rows_per_batch, TG_ERR_ARG,
           "tg_rc_xattn_ps: ip_scale_count = %d (0 or 1: ip_scale is one float; M / rows_per_batch = %lld: one per batch item)", ip_scale_count,
           (long long)(d->M / d->rows_per_batch));
  TG_CHECK(ip_scale_count <= 1 || d->ip_scale != nullptr, TG_ERR_ARG, "tg_rc_xattn_ps: ip_scale_count = %d needs ip_scale", ip_scale_count);
  RcXattnParams p;
  p.h = d->h; p.ldh = d->ldh; p.wq = d->wq; p.kv = d->kv; p.wo = d->wo; p.out = d->out; p.ldc = d->ldc; p.M = d->M;
  p.rows_per_batch = d->rows_per_batch; p.ln_eps = d->ln_eps; p.ip_scale = d->ip_scale; p.dbg = 0;
  p.ip_stride = ip_scale_count > 1 ? 1 : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return dispatch_rc_xattn<bf16_t>(d, p, st);
  return dispatch_rc_xattn<f16_t>(d, p, st);
}

extern "C" int tg_rc_xattn(const tg_rc_xattn_desc* d, void* stream) { return tg_rc_xattn_ps(d, 0, stream); }

extern "C" int tg_rc_kv_pack(int32_t dtype, int32_t batch, const void* k, const void* vt, int64_t ldt, int32_t text_len, const void* kip,
                             const void* vtip, int64_t ldi, int32_t ip_tokens, void* out, void* stream) {
  TG_CHECK(dtype == TG_BF16 || dtype == TG_F16, TG_ERR_ARG, "tg_rc_kv_pack: dtype %d", dtype);
  TG_CHECK(batch > 0 && k && vt && out, TG_ERR_ARG, "tg_rc_kv_pack: null operand");
  TG_CHECK(text_len > 0 && text_len <= 80 && ip_tokens >= 0 && ip_tokens <= 16 && (ip_tokens == 0 || (kip && vtip)), TG_ERR_ARG,
           "tg_rc_kv_pack: %d text keys (<= 80), %d image keys (<= 16)", text_len, ip_tokens);
  TG_CHECK(ldt >= text_len && (ip_tokens == 0 || ldi >= ip_tokens), TG_ERR_ARG,
           "tg_rc_kv_pack: V^T row pitches %lld / %lld below the key counts %d / %d", (long long)ldt, (long long)ldi, text_len, ip_tokens);
  TG_CHECK(rc_al16(k) && rc_al16(out) && (ip_tokens == 0 || rc_al16(kip)), TG_ERR_ARG, "tg_rc_kv_pack: k, kip and out must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)batch * 8 * 24;
  if (dtype == TG_BF16)
    hipLaunchKernelGGL(rc_kv_pack_kernel<bf16_t>, dim3(grid), dim3(64), 0, st, (const bf16_t*)k, (const bf16_t*)vt, (long)ldt,
                       (const bf16_t*)kip, (const bf16_t*)vtip, (long)ldi, text_len, ip_tokens, (bf16_t*)out);
  else
    hipLaunchKernelGGL(rc_kv_pack_kernel<f16_t>, dim3(grid), dim3(64), 0, st, (const f16_t*)k, (const f16_t*)vt, (long)ldt,
                       (const f16_t*)kip, (const f16_t*)vtip, (long)ldi, text_len, ip_tokens, (f16_t*)out);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

extern "C" int tg_rc_ff(const tg_rc_ff_desc* d, void* stream) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_rc_ff: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_rc_ff: dtype %d", d->dtype);
  TG_CHECK(d->h && d->w1 && d->w2 && d->b2 && d->out && d->M > 0, TG_ERR_ARG, "tg_rc_ff: null operand or M <= 0");
  TG_CHECK(d->inner >= 64 && d->inner % 64 == 0, TG_ERR_ARG, "tg_rc_ff: inner = %d must be a multiple of 64", d->inner);
  TG_CHECK(d->ldh >= 320 && d->ldh % 8 == 0 && d->ldc >= 320 && d->ldc % 8 == 0, TG_ERR_ARG, "tg_rc_ff: row pitches");
  TG_CHECK(!d->wpo || (d->res0 && d->ldres >= 320 && d->ldres % 8 == 0), TG_ERR_ARG, "tg_rc_ff: proj_out needs its residual");
  TG_CHECK(d->dbg != 0, TG_ERR_ARG,
           "tg_rc_ff: dbg = 0: the one-wave kernel and its stream format were retired; pack with rowchain.pack_ff2 / pack_po2 and set TG_RC_FF_TWO_WAVE");
  TG_CHECK(d->dbg == TG_RC_FF_TWO_WAVE, TG_ERR_ARG, "tg_rc_ff: dbg = %d (must be TG_RC_FF_TWO_WAVE, the stream-format tag; the rest is reserved)", d->dbg);
  RcFfParams p;
  p.h = d->h; p.ldh = d->ldh; p.w1 = d->w1; p.w2 = d->w2; p.b2 = d->b2; p.wpo = d->wpo; p.res0 = d->res0; p.ldres = d->ldres;
  p.out = d->out; p.ldc = d->ldc; p.M = d->M; p.n_slices = d->inner / 32; p.ln_eps = d->ln_eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return d->wpo ? launch_rc_ff<bf16_t, true>(d, p, st) : launch_rc_ff<bf16_t, false>(d, p, st);
  return d->wpo ? launch_rc_ff<f16_t, true>(d, p, st) : launch_rc_ff<f16_t, false>(d, p, st);
}

extern "C" int tg_rc_front(const tg_rc_front_desc* d, void* stream) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_rc_front: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_rc_front: dtype %d", d->dtype);
  TG_CHECK(d->x && d->coef && d->win && d->wqkv && d->y && d->qk && d->vt && d->M > 0, TG_ERR_ARG, "tg_rc_front: null operand or M <= 0");
  TG_CHECK(d->rows_per_batch > 0 && d->rows_per_batch % 128 == 0 && d->M % d->rows_per_batch == 0, TG_ERR_ARG,
           "tg_rc_front: rows_per_batch = %d must be a multiple of 128 that divides M", d->rows_per_batch);
  TG_CHECK(d->ldx >= 320 && d->ldx % 8 == 0 && d->ldy >= 320 && d->ldy % 8 == 0 && d->ldqk >= 640 && d->ldqk % 8 == 0 && d->ldt >= d->rows_per_batch,
           TG_ERR_ARG, "tg_rc_front: row pitches");
  TG_CHECK(d->dbg == 0, TG_ERR_ARG, "tg_rc_front: dbg = %d (reserved, must be 0)", d->dbg);
  TG_CHECK(rc_al16(d->x) && rc_al16(d->coef) && rc_al16(d->win) && rc_al16(d->wqkv) && rc_al16(d->y) && rc_al16(d->qk), TG_ERR_ARG,
           "tg_rc_front: x, coef, win, wqkv, y and qk must be 16-byte aligned");
  RcFrontParams p;
  p.x = d->x; p.ldx = d->ldx; p.coef = d->coef; p.win = d->win; p.wqkv = d->wqkv; p.y = d->y; p.ldy = d->ldy; p.qk = d->qk; p.ldqk = d->ldqk;
  p.vt = d->vt; p.ldt = d->ldt; p.M = d->M; p.rows_per_batch = d->rows_per_batch; p.ln_eps = d->ln_eps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return launch_rc_front<bf16_t>(d, p, st);
  return launch_rc_front<f16_t>(d, p, st);
}
