// conv_halo_kernel: conv3x3 (stride 1, pad 1) with an LDS-staged halo window; launched from tg_gemm.hip through
// tg_conv_halo_launch (own translation unit: compile time).
#include "tg_gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// conv3x3 with an LDS-STAGED HALO WINDOW (stride 1, pad 1, image width 16 / 32 / 64).
// The implicit-GEMM kernel above fetches every activation row 9 times (once per tap) through L2; the GEMM family is
// bound by L2 -> LDS operand delivery (profiles/r1_gemm_findings.md), so here a block = 128 output pixels = TH full
// image rows stages the (TH+2) x (W+2) input halo of ONE 64-channel chunk in LDS once and serves all 9 taps from
// it: the MFMA B-operand (lane = pixel) is read at slab row (py+ky)*(W+2) + px+kx.  K runs chunk-major / tap-minor;
// only the 128x64 weight tile streams per K-step (double-buffered).  Activation L2 traffic drops 9x, total operand
// traffic per FLOP by ~1.7x.  Same swizzle, same accumulator layout and the same epilogue as the GEMM kernel
// (full-width rows make the block's pixels contiguous in the token-major tensor).
// (Round 5 built a 128 x 160-channel instance for the 8 x 8 level — 64 tiles x 4 K splits = exactly one workgroup per CU, double-buffered window, five-stage
// weight ring, then eight waves sharing each K-step — parity-tested, and measured it at 55.2-57.8 us against this kernel's 56.9 (K = 11520) and SLOWER on the
// two-source layers (93 vs 86 us): a K-step takes ~0.9-1.0 us whatever the structure; removed.  profiles/r5_t160_findings.md.)
// UPS = true: the same for Upsample2D (nearest x2 then conv3x3): WI is the OUTPUT width, the slab holds the
// (TH/2 + 2) x (WI/2 + 2) INPUT pixels the block's upsampled window maps to (input pixel = upsampled coordinate >> 1).
// FOLD = true (tg_conv_up2): Upsample2D with the nearest x2 FOLDED INTO THE WEIGHTS.  The nine taps of output pixel (2i + py, 2j + px) touch only the
// 2 x 2 input pixels (i + py + ty - 1, j + px + tx - 1), so each parity class cls = 2 py + px is a 2 x 2-tap conv on the LOW-RESOLUTION grid with
// weights that are sums of the original taps (weights_pack.pack_conv3x3_up2: [4][N][4 C], tap-major (ty, tx, c)): 4/9 of the MFMAs.  WI is the
// low-resolution width, the block = 128 low-resolution pixels of ONE class x 128 channels, the slab is the plain (UPS = false) geometry, the K loop runs
// 4 taps per channel chunk, and the epilogue scatters local row (img, i, j) to token (img 2H + 2i + py) 2W + 2j + px.  No K split, bias only.
template <typename T, int WI, bool UPS, bool FOLD = false>
__global__ __launch_bounds__(256) void conv_halo_kernel(GemmParams p) {
  constexpr int BM = 128, BN = 128, NW = 4, TM = 2, TN = 2, WAVES_N = 2;
  // WI = 8 (the 8x8 level): a block's 128 pixels are TWO whole 8x8 images; their two 10x10 padded windows are stacked
  // in the slab (20 slab rows of width 10), everything else is unchanged
  constexpr bool MULTI = WI == 8;
  static_assert(!(MULTI && UPS), "no upsample variant at width 8");
  static_assert(!(FOLD && UPS), "the folded instance runs on the low-resolution grid");
  constexpr int NT = FOLD ? 4 : 9;                    // taps = K-steps per channel chunk
  constexpr int TH = BM / WI, WIN = UPS ? WI / 2 : WI, SW = WIN + 2, SROWS = MULTI ? 20 : (UPS ? TH / 2 + 2 : TH + 2);
  constexpr int SLAB = SROWS * SW, NI = (SLAB + 7) / 8, SJ = (NI + NW - 1) / NW;
  constexpr int WJ = BN / (8 * NW);
  typedef typename Vec<T>::v8 V8;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sS = reinterpret_cast<T*>(smem);                 // [NI*8][64]   halo slab of the current channel chunk
  // weight-tile ring: 3 stages (2 tiles in flight) wherever slab + 3 x 16 KB still lets two blocks share a CU (every
  // variant but the 64-wide one): a K-step's period was one DMA round trip of the next W tile, not its 16 MFMAs
  constexpr int WST = ((size_t)NI * 8 * BK + 3 * BN * BK) * sizeof(T) <= 80 * 1024 ? 3 : 2;
  constexpr int WD = WST - 1;                          // W tiles issued ahead of the one being multiplied
  T* sW = sS + NI * 8 * BK;                           // [WST][BN][64]  weight tiles

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / WAVES_N;
  const int wave_n = wave % WAVES_N;
  int lbid, split = 0, part = -1;     // same work-item scheme as gemm_glds_kernel; the K split runs over channel chunks
  int cls = 0;                        // FOLD: output parity class 2 py + px of this work item
  if ((int)blockIdx.x < p.full_tiles) {
    lbid = xcd_chunked_block_id(blockIdx.x, p.full_tiles);
    // the four classes of one (row tile, column tile) are neighbours in the walk: same XCD, same time, one input window in L2
    if (FOLD) { cls = lbid & 3; lbid >>= 2; }
  } else {
    const int j = (int)blockIdx.x - p.full_tiles;
    lbid = p.full_tiles + j / p.tail_s;
    split = j - (j / p.tail_s) * p.tail_s;
    part = j;
  }
  const int tile_n = lbid % p.tiles_n;
  const int tile_m = lbid / p.tiles_n;
  const long m0 = (long)tile_m * BM;
  const long n0 = (long)tile_n * BN;
  const int H = p.in_h;                               // INPUT height (output height = 2H when UPS)
  const int HO = UPS ? 2 * H : H;
  const int img = (int)(m0 / ((long)HO * WI));
  const int y0 = (int)((m0 - (long)img * HO * WI) / WI);
  const int iy0 = UPS ? y0 / 2 - 1 : y0 - 1;          // input row held by slab row 0

  const int lrow = lane >> 3;
  const int slot = lane & 7;
  const int wkey = (4 * (wave & 1) + (lane >> 4)) & 7;
  const int chunk = slot ^ wkey;

  const T* A0 = reinterpret_cast<const T*>(p.a0);
  const T* A1 = reinterpret_cast<const T*>(p.a1);
  const T* Wp = reinterpret_cast<const T*>(p.w) + (FOLD ? (long)cls * p.N * p.K : 0L);   // FOLD: p.K = 4 C, the row pitch inside one class
  const int cpy = cls >> 1, cpx = cls & 1;
  const T* zero = reinterpret_cast<const T*>(tg_zero_page);
  const int ctot = p.c0 + p.c1;
  const int nchunks = ctot / BK;

  int spix[SJ];                                       // input pixel feeding this lane's slab row (-1: zero padding)
#pragma unroll
  for (int j = 0; j < SJ; ++j) {
    const int sr = (j * NW + wave) * 8 + lrow;
    const int sy = sr / SW, sx = sr - sy * SW;
    int iy = iy0 + sy, im = img;
    if (MULTI) { im = img + sy / 10; iy = sy % 10 - 1; }       // slab rows [10 i, 10 i + 10) = padded window of image img + i
    const int ix = sx - 1;
    const bool ok = sr < SLAB && iy >= 0 && iy < H && ix >= 0 && ix < WIN && (m0 < p.M);
    spix[j] = ok ? (im * H + iy) * WIN + ix : -1;
  }
  const T* wrow[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    const long n = n0 + (j * NW + wave) * 8 + lrow;
    wrow[j] = n < p.N ? Wp + n * p.K : nullptr;
  }

  auto dma = [&](const T* src, T* lds_row_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_row_base, 16, 0, 0);
  };
  auto issue_slab = [&](int cc) {
    int c = cc * BK;
    const T* base = A0;
    int pitch = p.c0;
    if (c >= p.c0) { base = A1; pitch = p.c1; c -= p.c0; }
    c += chunk * 8;
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
      if (j * NW + wave < NI) {
        const T* src = spix[j] >= 0 ? base + (long)spix[j] * pitch + c : zero;
        dma(src, sS + (j * NW + wave) * 8 * BK);
      }
    }
  };
  // weight tile requests of a column tile wholly inside N: wave-uniform base (weight pointer + the K-step's column offset) + this lane's constant 32-bit byte offset
  // (tg_gemm_glds.h, round 6: no 64-bit pointer arithmetic / zero-page select per request in the K loop)
  const unsigned lds_sw = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)sW;
  const bool fastw = n0 + BN <= p.N && (long)p.N * p.K * (long)sizeof(T) < (1L << 31);
  unsigned voffw[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) voffw[j] = (unsigned)(((n0 + (j * NW + wave) * 8 + lrow) * p.K + chunk * 8) * (long)sizeof(T));
  auto dma_s = [&](const T* base, unsigned voff, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(base), "s"(lds_byte_addr) : "memory");
  };
  auto issue_w = [&](int cc, int tap, int buf) {
    if (fastw) {
      const T* wb = Wp + ((long)tap * ctot + cc * BK);
#pragma unroll
      for (int j = 0; j < WJ; ++j) dma_s(wb, voffw[j], lds_sw + (unsigned)((buf * BN * BK + (j * NW + wave) * 8 * BK) * sizeof(T)));
      return;
    }
    const long kc = (long)tap * ctot + cc * BK + chunk * 8;
    T* dw = sW + buf * BN * BK;
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      const T* src = wrow[j] != nullptr ? wrow[j] + kc : zero;
      dma(src, dw + (j * NW + wave) * 8 * BK);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int rkey = (l31 >> 1) & 7;
  int ppy[TM], ppx[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int pm = wave_m * TM * 32 + i * 32 + l31;
    ppy[i] = MULTI ? (pm >> 6) * 10 + ((pm & 63) >> 3) : pm / WI;
    ppx[i] = pm % WI;
  }

  // channel chunks of this work item (kt_per_split counts chunks here)
  const int c_begin = part >= 0 ? split * p.kt_per_split : 0;
  int c_end = part >= 0 ? c_begin + p.kt_per_split : nchunks;
  if (c_end > nchunks) c_end = nchunks;

  const int nkt = (c_end - c_begin) * NT;
  int icc = c_begin, itap = 0;                         // (chunk, tap) of the next W tile to request
  issue_slab(c_begin);
#pragma unroll
  for (int s_ = 0; s_ < WD; ++s_) {
    if (s_ < nkt) {
      issue_w(icc, itap, s_);
      if (++itap == NT) { itap = 0; ++icc; }
    }
  }
  if (WD == 2 && nkt >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WJ) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  int cc = c_begin, tap = 0;
  int buf = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    int ky = tap / 3, kx = tap - ky * 3;
    if (FOLD) { ky = cpy + (tap >> 1); kx = cpx + (tap & 1); }   // tap (ty, tx) of class (py, px) reads slab row (y + py + ty) * SW + x + px + tx
    const T* bw = sW + buf * BN * BK + (wave_n * TN * 32 + l31) * BK;
    V8 xf[BK / 16][TM], wf[BK / 16][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int sr = UPS ? (((ppy[i] + ky - 1) >> 1) + 1) * SW + ((ppx[i] + kx - 1) >> 1) + 1
                         : (ppy[i] + ky) * SW + ppx[i] + kx;
      const int key = (sr >> 1) & 7;
      const T* bx = sS + sr * BK;
#pragma unroll
      for (int ks = 0; ks < BK / 16; ++ks) xf[ks][i] = *reinterpret_cast<const V8*>(bx + ((2 * ks + hi) ^ key) * 8);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      const int so = ((2 * ks + hi) ^ rkey) * 8;
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[ks][j] = *reinterpret_cast<const V8*>(bw + j * 32 * BK + so);
    }
    __builtin_amdgcn_sched_barrier(0);
    int ncc = cc, ntap = tap + 1;
    if (ntap == NT) { ntap = 0; ncc = cc + 1; }
    if (kt + 1 < nkt) {
      if (ntap == 0) {
        // the next K-step starts a new channel chunk: every wave must have its LAST-tap fragments (tap 8; FOLD: tap 3) in registers before
        // the slab is overwritten; the slab DMA then overlaps this step's 16 MFMAs.  Nothing here depends on the number of taps per chunk:
        // write-after-read — the fragments of the chunk's earlier taps were consumed by their own steps' MFMAs, which every wave finished
        // before that step's closing barrier, and this step's reads are covered by the lgkmcnt(0) + barrier below; read-after-write — the
        // slab request is OLDER than this step's W request, so the closing vmcnt(WJ) (or vmcnt(0)) + barrier of this step sees it landed
        // before the next step's first fragment read.  With FOLD the extra barrier fires every 4th step instead of every 9th.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        issue_slab(ncc);
      }
    }
    if (kt + WD < nkt) {
      int nb = buf + WD;
      if (nb >= WST) nb -= WST;
      issue_w(icc, itap, nb);
      if (++itap == NT) { itap = 0; ++icc; }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(wf[ks][j], xf[ks][i], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
    // the W tile of step kt+1 (and a slab requested in this step, which is older than this step's W request) must have
    // landed; the W tile requested in this step may stay in flight
    if (WD == 2 && kt + 2 < nkt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WJ) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    cc = ncc;
    tap = ntap;
    buf = buf + 1 == WST ? 0 : buf + 1;
  }

  if constexpr (FOLD) {
    // Mapped-row LDS epilogue (precedent: the slab conv's patch rows, PR / patch_token in tg_gemm_common.h).  Same bounce as epilogue_rows_lds —
    // the operand stages are dead after the K loop's last barrier, each wave owns 32 x 68 floats — and the same fp32 expression (acc + bias, one
    // rounding; the host admits bias only: no residual, per-batch vector, activation, scale, n_split or GroupNorm partials), so an exact-arithmetic
    // input gives the unfolded kernel's bits.  Lane = (row r0 + 8 it, 8-channel piece c): 16-byte stores, 128 contiguous bytes per token row.
    constexpr int RS = TN * 32 + 4;
    float* scr = reinterpret_cast<float*>(smem) + wave * (32 * RS);
    const int c8 = lane & 7, r0 = lane >> 3;
    const long n = n0 + wave_n * TN * 32 + c8 * 8;
    const bool n_ok = n < p.N;
    float bias_f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias_f[e] = 0.f;
    if (p.bias != nullptr) {
      const V8 b8 = *reinterpret_cast<const V8*>(reinterpret_cast<const T*>(p.bias) + (n_ok ? n : 0));
#pragma unroll
      for (int e = 0; e < 8; ++e) bias_f[e] = to_f32<T>(b8[e]);
    }
    T* outp = reinterpret_cast<T*>(p.out);
    const int hw = H * WI;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 o = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          *reinterpret_cast<f32x4*>(scr + l31 * RS + 32 * j + 8 * g + 4 * hi) = o;
        }
      __builtin_amdgcn_wave_barrier();
      f32x4 lo[4], hi4[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        lo[it] = *reinterpret_cast<const f32x4*>(scr + (it * 8 + r0) * RS + c8 * 8);
        hi4[it] = *reinterpret_cast<const f32x4*>(scr + (it * 8 + r0) * RS + c8 * 8 + 4);
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int ml = (int)m0 + wave_m * TM * 32 + i * 32 + it * 8 + r0;     // low-resolution pixel (img, yi, xj)
        const int im = ml / hw, rem = ml - im * hw;
        const int yi = rem / WI, xj = rem - yi * WI;
        const long tok = ((long)im * 2 * H + 2 * yi + cpy) * (2 * WI) + 2 * xj + cpx;
        V8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = from_f32<T>(lo[it][e] + bias_f[e]); o[4 + e] = from_f32<T>(hi4[it][e] + bias_f[4 + e]); }
        if (ml < p.M && n_ok) *reinterpret_cast<V8*>(outp + tok * p.ldc + n) = o;
      }
    }
  } else {
    epilogue_tile_lds<T, TM, TN, 0>(p, acc, m0 + wave_m * TM * 32, n0 + wave_n * TN * 32, lane,
                                   reinterpret_cast<float*>(smem) + wave * (32 * (TN * 32 + 4)), part, m0, n0);
  }
}

template <typename T, int WI, bool UPS, bool FOLD = false>
int launch_halo(const GemmParams& p, int grid, hipStream_t st) {
  constexpr int TH = 128 / WI, SLAB = WI == 8 ? 200 : (UPS ? (TH / 2 + 2) * (WI / 2 + 2) : (TH + 2) * (WI + 2)), NI = (SLAB + 7) / 8;
  const int wst = ((size_t)NI * 8 * BK + 3 * 128 * BK) * sizeof(T) <= 80 * 1024 ? 3 : 2;
  const size_t lds = ((size_t)NI * 8 * BK + wst * 128 * BK) * sizeof(T);
  auto k = conv_halo_kernel<T, WI, UPS, FOLD>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)attr;
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), lds, st, p);
  TG_LAUNCH_CHECK();
  return TG_OK;
}

template <typename T>
int dispatch_halo(const tg_gemm_desc* d, const GemmParams& p, int grid, hipStream_t st) {
  if (d->upsample) {
    if (d->out_w == 64) return launch_halo<T, 64, true>(p, grid, st);
    if (d->out_w == 32) return launch_halo<T, 32, true>(p, grid, st);
    return launch_halo<T, 16, true>(p, grid, st);
  }
  if (d->out_w == 64) return launch_halo<T, 64, false>(p, grid, st);
  if (d->out_w == 32) return launch_halo<T, 32, false>(p, grid, st);
  if (d->out_w == 8) return launch_halo<T, 8, false>(p, grid, st);
  return launch_halo<T, 16, false>(p, grid, st);
}

template <typename T>
int dispatch_up2(const tg_gemm_desc* d, const GemmParams& p, int grid, hipStream_t st) {
  if (d->in_w == 64) return launch_halo<T, 64, false, true>(p, grid, st);
  if (d->in_w == 32) return launch_halo<T, 32, false, true>(p, grid, st);
  if (d->in_w == 16) return launch_halo<T, 16, false, true>(p, grid, st);
  return launch_halo<T, 8, false, true>(p, grid, st);
}

// tg_conv_up2's host-side contract (include/theatergen_hip.h); every check runs before any launch
int up2_validate(const tg_gemm_desc* d) {
  TG_CHECK(d != nullptr, TG_ERR_ARG, "tg_conv_up2: null descriptor");
  TG_CHECK(d->dtype == TG_BF16 || d->dtype == TG_F16, TG_ERR_ARG, "tg_conv_up2: bad dtype %d", d->dtype);
  TG_CHECK(d->a0 && d->w && d->out, TG_ERR_ARG, "tg_conv_up2: null a0/w/out");
  TG_CHECK((reinterpret_cast<uintptr_t>(d->a0) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->w) & 15) == 0, TG_ERR_ARG,
           "tg_conv_up2: a0 / w must be 16-byte aligned (a0=%p w=%p)", d->a0, d->w);
  TG_CHECK(d->mode == 1 && d->upsample == 1 && d->stride == 1 && d->pad_mode == 0, TG_ERR_ARG,
           "tg_conv_up2: the descriptor must be mode 1, upsample 1, stride 1, pad_mode 0");
  TG_CHECK(d->a1 == nullptr, TG_ERR_ARG, "tg_conv_up2: single source only (a1 must be NULL)");
  TG_CHECK(d->batch > 0 && d->in_h > 0 && d->in_w > 0 && d->c0 > 0 && d->N > 0, TG_ERR_ARG, "tg_conv_up2: empty problem");
  TG_CHECK(d->K == 16L * d->c0, TG_ERR_ARG, "tg_conv_up2: K must be 16*c0 (four classes of four folded taps), got K=%lld c0=%d", (long long)d->K, d->c0);
  TG_CHECK(d->out_h == 2 * d->in_h && d->out_w == 2 * d->in_w, TG_ERR_ARG, "tg_conv_up2: out %dx%d inconsistent with in %dx%d",
           d->out_h, d->out_w, d->in_h, d->in_w);
  TG_CHECK(d->M == (int64_t)d->batch * d->out_h * d->out_w, TG_ERR_ARG, "tg_conv_up2: M != batch*out_h*out_w");
  TG_CHECK(d->bvec == nullptr && d->res == nullptr && d->act == TG_ACT_NONE && !d->geglu && d->n_split <= 0 && d->out_scale == 1.0f &&
           d->a_coef == nullptr && d->ln_u == nullptr && d->ln_v == nullptr && d->ln_rows == nullptr && d->out_gn_partials == nullptr &&
           d->force_split_k <= 1 && d->force_tile == 0 && d->lda <= 0 && d->ldw <= 0 && d->a_rows_per_batch <= 0,
           TG_ERR_UNSUPPORTED, "tg_conv_up2: bias is the only epilogue term (no residual / per-batch vector / activation / scale / split / fold / forced plan)");
  TG_CHECK(d->c0 % BK == 0, TG_ERR_UNSUPPORTED, "tg_conv_up2: c0 %% 64 required (c0=%d)", d->c0);
  const long mlo = (long)d->batch * d->in_h * d->in_w;
  bool geo = mlo % 128 == 0;
  if (d->in_w == 8) geo = geo && d->in_h == 8;                                      // two whole 8 x 8 images per block
  else geo = geo && (d->in_w == 16 || d->in_w == 32 || d->in_w == 64) && d->in_h % (128 / d->in_w) == 0;   // whole image rows, blocks inside one image
  TG_CHECK(geo, TG_ERR_UNSUPPORTED, "tg_conv_up2: low-resolution map %dx%d x batch %d is not 128-pixel blocks of whole rows at width 8 / 16 / 32 / 64",
           d->in_h, d->in_w, d->batch);
  TG_CHECK(d->N % 8 == 0 && d->ldc % 8 == 0 && d->ldc >= d->N && (reinterpret_cast<uintptr_t>(d->out) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(d->bias) & 15) == 0, TG_ERR_UNSUPPORTED, "tg_conv_up2: N %% 8, ldc %% 8 and 16-byte aligned out / bias required");
  // 32-bit byte offsets of the LDS-DMA requests and int pixel / token indices in the kernel
  const long esz = 2;
  TG_CHECK(mlo * d->c0 * esz < (1L << 31) && d->M * d->ldc * esz < (1L << 31) && d->N * 4L * d->c0 * esz < (1L << 31), TG_ERR_UNSUPPORTED,
           "tg_conv_up2: an operand extent reaches 2^31 bytes");
  return TG_OK;
}

}  // namespace

extern "C" int tg_conv_up2_eligible(const tg_gemm_desc* d) { return up2_validate(d) == TG_OK ? 1 : 0; }

extern "C" int tg_conv_up2(const tg_gemm_desc* d, void* stream) {
  const int rc = up2_validate(d);
  if (rc != TG_OK) return rc;
  GemmParams p{};
  p.a0 = d->a0; p.c0 = d->c0;
  p.in_h = d->in_h; p.in_w = d->in_w; p.out_h = d->out_h; p.out_w = d->out_w; p.stride = 1; p.upsample = 1; p.pad_lo = 1;
  p.w = d->w;
  p.M = (long)d->batch * d->in_h * d->in_w;        // the kernel's rows are LOW-RESOLUTION pixels
  p.N = d->N;
  p.K = 4L * d->c0;                                // weight row pitch inside one parity class
  p.bias = d->bias; p.rows_per_batch = p.M; p.out_scale = 1.0f;
  p.out = d->out; p.ldc = d->ldc;
  p.tiles_n = (int)((d->N + 127) / 128);
  p.full_tiles = (int)(p.M / 128) * 4 * p.tiles_n; p.tail_s = 1; p.tile_bm = 128; p.tile_bn = 128;
  p.patch_np = 1; p.epi_lds = 1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return dispatch_up2<bf16_t>(d, p, p.full_tiles, st);
  return dispatch_up2<f16_t>(d, p, p.full_tiles, st);
}

// grid = full tiles + tail tiles * K splits (the caller, tg_gemm.hip, owns the plan and launches the split reduce)
int tg_conv_halo_launch(const tg_gemm_desc* d, const void* params, int grid, void* stream) {
  const GemmParams& p = *reinterpret_cast<const GemmParams*>(params);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return dispatch_halo<bf16_t>(d, p, grid, st);
  return dispatch_halo<f16_t>(d, p, grid, st);
}
