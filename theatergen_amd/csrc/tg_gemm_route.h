// Which kernel runs a tg_gemm descriptor: the ONE place that decides (tg_gemm_route.hip).  Host logic only — no kernels, no
// tg_gemm_glds.h — so a planner edit recompiles in seconds.  tg_gemm (tg_gemm.hip) fills GemmParams and switches on the route;
// tg_gemm_plan / tg_gemm_workspace_bytes / tg_gemm_gn_partial_blocks / tg_gemm_kernel_name copy fields out of it.
#pragma once
#include <stdint.h>

#include "../../include/theatergen_hip.h"

// tg_gemm_plan's kernel_kind (5, round 2's loader / compute GEMM, was removed in round 5)
enum GemmKind {
  kKindGemm = 0,      // gemm_glds_kernel, plain GEMM (128 x 160 tiles: tg_gemm_t160.hip)
  kKindConv = 1,      // gemm_glds_kernel, implicit-GEMM conv
  kKindHalo = 2,      // conv_halo_kernel (tg_conv_halo.hip)
  kKindBigTile = 3,   // bt_gemm_kernel, 256 x 256 (tg_gemm_bt.hip)
  kKindSlab = 4,      // conv_slab_kernel / conv_slab_pp_kernel, 128 x 320 (tg_conv_slab.hip, tg_conv_slab_pp.hip)
  kKindLnFold = 6,    // gemm_glds_kernel with the LayerNorm fold (tg_gemm_ln.hip)
  kKindPingPong = 7,  // pp_gemm_kernel 256 x 256 / pp160_gemm_kernel 256 x 160 (tg_gemm_pp.hip, tg_gemm_pp160.hip)
};

// tg_gemm_desc.force_tile (tests / dev sweeps; 0 = heuristic): 1 .. 8 = 1 + glds tile id, 9 = round 2's 128 x 320 big tile (removed: plans as tile id 8),
// 13 / 14 = round 2's loader / compute GEMM (removed: plan as the default tile)
enum GemmForceTile {
  kForceBigTile = 10,      // 256 x 256 big tile (a problem it cannot take plans as glds tile id 9)
  kForceSlab = 11,         // slab conv with force_split_k (default 1) splits
  kForceSlab2 = 12,        // slab conv, two splits
  kForceT160First = 21,    // 21 / 22 / 23 = glds tile ids 7 / 8 / 9 (128 x 160)
  kForceT160Last = 23,
  kForcePingPong = 24,     // ping-pong 256 x 256
  kForcePingPong160 = 25,  // ping-pong 256 x 160
};

// The dev A/B knobs of the planner.  Read once per route, never cached: tests and A/B scripts change them inside one process.
struct GemmKnobs {
  long flags;     // TG_GEMM_FLAGS (default 0), the router's five bits and nothing else: bit 3 no big tile, 7 no slab kernel, 10 no patch tiles, 11 / 12 the slab split
                  // rules.  Every other bit of the variable is masked off (kGemmRouterFlags): no kernel and no launcher sees the word
  int pp;         // TG_PP (15): 1 = GEGLU, 2 = linear / activation, 4 = LayerNorm-folded launches on the ping-pong tiles, 8 = the 256 x 160 tiles
  int t160;       // TG_T160 (7): 1 = 128 x 160 tiles for plain GEMMs where they fill whole rounds, 2 = for the LayerNorm-folded projections, 4 = N = 2.5 / 7.5 tiles of 128
  long t64_max;   // TG_T64_MAX (128): 128 x 128 tile counts up to this take the 64 x 64 tile
  long t3_max;    // TG_T3_MAX (256): ... up to this the 128 x 64 tile
  long t7_maxk;   // TG_T7_MAXK (640): plain GEMMs with K up to this take the 32-wide K stages
  bool t7_fit;    // TG_T7_FIT=1: also longer-K GEMMs whose tiles fit one round of three workgroups per CU
  int slab_pp;    // TG_SLAB_PP (3): 0 = one-wave slab kernel everywhere, 1 = two-wave on 64-wide rows, 2 = + 32 / 16-wide rows, 3 = + patch tiles
};
GemmKnobs gemm_knobs();

// glds tile `tile` (kTiles id); the first `full` tiles are computed whole, each of the `tail` last tiles is cut into `s` K-ranges of `kps` units
// (K-tiles, or 64-channel chunks for the halo kernel); grid = full + tail * s work items.  What GemmParams' tile bookkeeping starts from in EVERY family.
struct GemmTilePlan { int tile, bm, bn; bool halo; int full, tail, s, kps; long tiles_m, tiles_n; };

struct GemmRoute {
  GemmKind kind;
  int tile_m, tile_n, splits;   // what tg_gemm_plan reports
  GemmTilePlan plan;
  int slab_pw, slab_np;         // kKindSlab: patch width, patches per 128-pixel tile,
  bool slab_patch, two_wave;    //   patch tiles (not whole image rows), conv_slab_pp_kernel (two compute waves per SIMD)
  int ln_variant;               // kKindLnFold: 0 = 128 x 128, 1 = the same on 32-wide K stages (K <= 640), 160 / 161 = 128 x 160 with three / two stages
  int pp_bn;                    // kKindPingPong: 256 or 160
  int64_t workspace_bytes;      // fp32 partials of the K split (0 = none)
  int gn_partial_blocks;        // > 0: the kernel can write GroupNorm partial sums of its output: 64-pixel blocks per batch item
  const char* kernel;           // the kernel template's name
  bool epi_lds;                 // operands / strides allow the LDS-transposed, 16-byte-coalesced epilogue (GemmParams::epi_lds)
  bool column_major;            // kKindSlab / kKindPingPong: the persistent grid walks column tiles outermost (GemmParams::slab_order): the weight is the larger operand
  // tg_gemm refuses the descriptor with this code / message (TG_OK: it launches).  The queries answer for such a descriptor as they always have.
  int refusal;
  const char* refusal_msg;
};

// Walks the precedence chain once for a VALIDATED descriptor: ping-pong 256 x 256, ping-pong 256 x 160, LayerNorm fold, slab conv, big tile, halo conv, glds tile.
// Returns route->refusal.
int gemm_route(const tg_gemm_desc* d, GemmRoute* route);
// argument checks of tg_gemm and its queries (sets the error message)
int gemm_validate(const tg_gemm_desc* d);
