// MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (see include/theatergen_hip.h: tg_gemm).
//
// out[m, n] = epilogue( sum_k A[m, k] * W[n, k] ),  A token-major activations, W [N, K] (K contiguous).
// The MFMA is issued "swapped": A-operand = W rows (n), B-operand = activation rows (m), so the
// 32x32 accumulator tile has lane&31 = token and 4 consecutive registers = 4 consecutive output
// channels -> 8-byte stores / 8-byte bias+residual loads in the epilogue, and per-token quantities
// stay lane-local.
//
// Block tile BM(tokens) x BN(channels) x BK=64, 256 threads = 4 waves (WAVES_M x WAVES_N), each wave
// TM x TN tiles of v_mfma_f32_32x32x16.  Operands are register-staged (global_load_dwordx4 issued
// before the MFMA block of the current tile, ds_write_b128 after it) into double-buffered LDS with a
// 144-byte row pitch (128 B of K + 16 B pad): ds_read_b128 of 16 rows x one 16-B column hits 16 distinct
// 4-bank slots (conflict-free), ds_write_b128 rows are contiguous.
//
// Conv mode gathers the A rows on the fly (no im2col buffer): K is tap-major (ky, kx, c); a BK chunk
// never straddles a tap because channel counts are multiples of 64, so each A row of a K-tile is one
// contiguous 128-B segment of a shifted input pixel (or zeros at the border).  Stride-2 (Downsample2D),
// nearest-x2 upsampled input (Upsample2D) and a two-source channel concat (skip connection) are folded
// into the gather.
#include "tg_gemm_common.h"
#include "tg_gemm_glds.h"
#include "tg_gemm_route.h"

namespace {

template <typename T>
__global__ void splitk_reduce_kernel(GemmParams p);

// sums the `s` fp32 partials of each of the `tail` last tiles and runs the regular epilogue (nothing to do without a K split)
template <typename T>
int launch_reduce(const GemmParams& p, int tail, int s, hipStream_t st) {
  if (s > 1) {
    hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3((unsigned)tail * 8), dim3(256), 0, st, p);
    TG_LAUNCH_CHECK();
  }
  return TG_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmParams p) {
  // 8 blocks per tail tile (row slices): sum its tail_s fp32 partials in split order, then the regular epilogue
  const int t = blockIdx.x >> 3, slice = blockIdx.x & 7;
  const int lbid = p.full_tiles + t;
  const long m0 = (long)(lbid / p.tiles_n) * p.tile_bm, n0 = (long)(lbid % p.tiles_n) * p.tile_bn;
  const int q4 = p.tile_bn / 4;
  const int rows = p.tile_bm / 8;
  const long tile_elems = (long)p.tile_bm * p.tile_bn;
  const float* base = p.ws + (long)t * p.tail_s * tile_elems;
  for (int q = threadIdx.x; q < rows * q4; q += blockDim.x) {
    const int lr = slice * rows + q / q4, lc = (q % q4) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < p.tail_s; ++z) s += *reinterpret_cast<const f32x4*>(base + z * tile_elems + (long)lr * p.tile_bn + lc);
    // slab conv patch tiles: partial rows are in tile-local order, the token comes from the patch geometry
    const long m = p.patch_pwl > 0 ? patch_token(p, lbid / p.tiles_n, lr) : m0 + lr;
    epilogue_store4<T>(p, m, n0 + lc, s[0], s[1], s[2], s[3]);
  }
}

template <typename T, int BM, int BN, int WM, int WN, bool CONV, int STAGES, int BKT, int EPI>
void launch_glds(const GemmParams& p, dim3 grid, size_t lds, hipStream_t st) {
  auto k = gemm_glds_kernel<T, BM, BN, WM, WN, CONV, STAGES, BKT, EPI>;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)attr;
  hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, st, p);
}

template <typename T, int BM, int BN, int WM, int WN, int STAGES, int BKT = 64>
int launch_cfg2(const tg_gemm_desc* d, const GemmParams& p, const GemmTilePlan& pl, hipStream_t st) {
  const size_t lds = (size_t)STAGES * (BM + BN) * BKT * sizeof(T);
  dim3 grid((unsigned)(pl.full + pl.tail * pl.s));
  // epilogue kind: 0 = linear only, 1 = generic (activation / GEGLU on any tile), 2 = GEGLU on the default plain tile
  constexpr bool kMainTile = (BM == 128 && BN == 128 && STAGES == 2) || (BM == 256 && BN == 256);   // tiles with a GEGLU-only instance
  const int epi = d->geglu ? ((kMainTile && d->mode != 1) ? 2 : 1) : (d->act == TG_ACT_NONE ? 0 : 1);
  if (d->mode == 1) {
    if (epi == 0) launch_glds<T, BM, BN, WM, WN, true, STAGES, BKT, 0>(p, grid, lds, st);
    else launch_glds<T, BM, BN, WM, WN, true, STAGES, BKT, 1>(p, grid, lds, st);
  } else {
    if (epi == 0) launch_glds<T, BM, BN, WM, WN, false, STAGES, BKT, 0>(p, grid, lds, st);
    else if (epi == 2) {
      if constexpr (kMainTile) launch_glds<T, BM, BN, WM, WN, false, STAGES, BKT, 2>(p, grid, lds, st);
    } else launch_glds<T, BM, BN, WM, WN, false, STAGES, BKT, 1>(p, grid, lds, st);
  }
  TG_LAUNCH_CHECK();
  return launch_reduce<T>(p, pl.tail, pl.s, st);
}

}  // namespace
// big-tile kernel (tg_gemm_bt.hip): bt_tile 2 = 256 x 256 (the 128 x 320 instance, bt_tile 1, was removed in round 5)
int tg_gemm_bt_launch(const tg_gemm_desc* d, const void* params, int bt_tile, void* stream);
// slab conv kernel (tg_conv_slab.hip): BM x 320 output tiles, GroupNorm(+SiLU) prologue on the staged window; two_wave = conv_slab_pp_kernel
int tg_conv_slab_launch(const tg_gemm_desc* d, const void* params, int splits, bool two_wave, void* stream);
// LayerNorm-fused projections (tg_gemm_ln.hip): 128 x 128 tiles, no K split
int tg_gemm_ln_launch(const tg_gemm_desc* d, const void* params, int short_k, int grid, void* stream);
// 128 x 160 tiles (tg_gemm_t160.hip): variant 0 = BK 64 x 3 stages, 1 = BK 32 x 4 stages, 2 = BK 64 x 2 stages
int tg_gemm_t160_launch(const tg_gemm_desc* d, const void* params, int variant, int grid, void* stream);
// LDS-halo conv (tg_conv_halo.hip): grid = full tiles + tail tiles * K splits
int tg_conv_halo_launch(const tg_gemm_desc* d, const void* params, int grid, void* stream);
// ping-pong 256 x 256 tiles (tg_gemm_pp.hip, round 6): 8 waves in two groups one barrier apart, persistent
int tg_gemm_pp_launch(const tg_gemm_desc* d, const void* params, void* stream);
// the same structure on 256 x 160 tiles (tg_gemm_pp160.hip): the N = 640 / 1920 / 320 projections
int tg_gemm_pp160_launch(const tg_gemm_desc* d, const void* params, void* stream);
namespace {

// Fill GemmParams, then launch the kernel family the route (tg_gemm_route.hip) names.  No selection rule lives here.
template <typename T>
int launch_gemm(const tg_gemm_desc* d, hipStream_t st) {
  GemmRoute r;
  gemm_route(d, &r);
  const GemmTilePlan& pl = r.plan;
  GemmParams p{};
  p.a0 = d->a0; p.a1 = d->a1; p.c0 = d->c0; p.c1 = d->a1 ? d->c1 : 0;
  p.in_h = d->in_h; p.in_w = d->in_w; p.out_h = d->out_h; p.out_w = d->out_w;
  p.stride = d->stride; p.upsample = d->upsample; p.pad_lo = d->pad_mode == 1 ? 0 : 1;
  p.w = d->w; p.M = d->M; p.N = d->N; p.K = d->K;
  p.bias = d->bias; p.bvec = d->bvec; p.ldbvec = d->ldbvec;
  p.rows_per_batch = d->rows_per_batch > 0 ? d->rows_per_batch : d->M;
  p.res = d->res; p.ldres = d->ldres; p.act = d->act; p.geglu = d->geglu; p.out_scale = d->out_scale;
  p.out = d->out; p.ldc = d->ldc; p.n_split = d->n_split; p.out_t = d->out_t; p.ldt = d->ldt;
  p.ws = reinterpret_cast<float*>(d->workspace);
  p.full_tiles = pl.full; p.tail_s = pl.s; p.kt_per_split = pl.kps; p.tiles_n = (int)pl.tiles_n;
  p.tile_bm = pl.bm; p.tile_bn = pl.bn;
  p.a_rpb = d->mode == 0 ? d->a_rows_per_batch : 0; p.a_bs = d->a_batch_stride;
  p.lda = d->lda > 0 ? d->lda : p.c0; p.ldw = d->ldw > 0 ? d->ldw : d->K;
  p.a_coef = d->a_coef; p.a_silu = d->a_silu;
  p.patch_pwl = 0; p.patch_np = 1;
  p.ln_u = d->ln_u; p.ln_v = d->ln_v; p.ln_eps = d->ln_eps; p.ln_rows = d->ln_rows;
  p.epi_lds = r.epi_lds;
  p.slab_order = r.column_major ? 1 : 0;
  p.gn_part = d->out_gn_partials; p.gn_cpg = d->out_gn_partials ? (int)(d->N / d->out_gn_groups) : 0;
  TG_CHECK(d->out_gn_partials == nullptr || r.gn_partial_blocks > 0, TG_ERR_UNSUPPORTED,
           "tg_gemm: out_gn_partials needs an unsplit stride-1 conv on the two-wave slab kernel with 80 %% (N / groups) == 0 (ask tg_gemm_gn_partial_blocks)");
  TG_CHECK(r.refusal == TG_OK, r.refusal, "%s", r.refusal_msg);
  TG_CHECK(r.workspace_bytes == 0 || (d->workspace != nullptr && d->workspace_bytes >= r.workspace_bytes), TG_ERR_ARG,
           r.kind == kKindSlab ? "tg_gemm conv: the K split needs %lld workspace bytes, got %lld" : "tg_gemm: the K-split tail needs %lld workspace bytes, got %lld",
           (long long)r.workspace_bytes, (long long)d->workspace_bytes);
  const int grid = pl.full + pl.tail * pl.s;
  switch (r.kind) {
    case kKindPingPong:
      return r.pp_bn == 256 ? tg_gemm_pp_launch(d, &p, st) : tg_gemm_pp160_launch(d, &p, st);
    case kKindLnFold: {
      // whole rows per workgroup (no K split), in XCD-chunked order
      const long tiles_n = (d->N + r.tile_n - 1) / r.tile_n, tiles = ((d->M + 127) / 128) * tiles_n;
      p.full_tiles = (int)tiles; p.tail_s = 1; p.tiles_n = (int)tiles_n; p.tile_bm = r.tile_m; p.tile_bn = r.tile_n;
      p.kt_per_split = 0;
      return tg_gemm_ln_launch(d, &p, r.ln_variant, (int)tiles, st);
    }
    case kKindSlab: {
      p.patch_np = r.slab_np;
      if (r.slab_patch) { int l = 0; while ((1 << l) < r.slab_pw) ++l; p.patch_pwl = l; }
      const int rc = tg_conv_slab_launch(d, &p, r.splits, r.two_wave, st);
      if (rc != TG_OK || r.splits == 1) return rc;
      const long tiles = (d->M / 128) * (d->N / 320);
      p.tiles_n = (int)(d->N / 320); p.full_tiles = 0; p.tail_s = r.splits; p.tile_bm = 128; p.tile_bn = 320;
      return launch_reduce<T>(p, (int)tiles, r.splits, st);
    }
    case kKindBigTile:
      return tg_gemm_bt_launch(d, &p, 2, st);
    case kKindHalo: {
      const int rc = tg_conv_halo_launch(d, &p, grid, st);
      return rc != TG_OK ? rc : launch_reduce<T>(p, pl.tail, pl.s, st);
    }
    case kKindGemm:
    case kKindConv:
      break;
  }
  switch (pl.tile) {
    case 0: return launch_cfg2<T, 128, 128, 2, 2, 2>(d, p, pl, st);
    case 1: return launch_cfg2<T, 64, 64, 2, 2, 3>(d, p, pl, st);
    case 2: return launch_cfg2<T, 128, 64, 4, 1, 3>(d, p, pl, st);
    case 3: return launch_cfg2<T, 64, 128, 1, 4, 3>(d, p, pl, st);
    case 4: return launch_cfg2<T, 128, 128, 2, 2, 3>(d, p, pl, st);   // 3 stages, 96 KB: 1 block / CU (forced only)
    case 6: return launch_cfg2<T, 128, 128, 2, 2, 3, 32>(d, p, pl, st);   // three 16 KB K stages: 3 blocks / CU
    case 7: case 8: case 9: {                                             // 128 x 160 tiles (tg_gemm_t160.hip): 7 = 1 block / CU, 8 / 9 = 2 blocks / CU
      const int rc = tg_gemm_t160_launch(d, &p, pl.tile - 7, grid, st);
      return rc != TG_OK ? rc : launch_reduce<T>(p, pl.tail, pl.s, st);
    }
    default: return launch_cfg2<T, 256, 256, 2, 4, 2>(d, p, pl, st);   // 8 waves of 128x64, 128 KB, 1 block / CU
  }
}

}  // namespace

extern "C" int tg_gemm(const tg_gemm_desc* d, void* stream) {
  int rc = gemm_validate(d);
  if (rc != TG_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == TG_BF16) return launch_gemm<bf16_t>(d, st);
  return launch_gemm<f16_t>(d, st);
}
