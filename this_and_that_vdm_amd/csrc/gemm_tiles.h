// gemm_tiles.h -- the tables of the tiled template (gemm_kernel.h): every tile shape, every KMODE_ that is built and on which tiles, the
// tiles whose wide variant is built.  No kernel code: gemm.hip plans and names instances from these tables, gemm_launch.h generates
// the launch switches from them, so the two cannot drift apart.
#pragma once

namespace ttg {

// ---- which instance of gemm_kernel a launch on a tile runs: the ONE place that says so.  launch_cfg dispatches on the answer and
// tt_gemm_kernel (gemm.hip) prints it.  KMODE_ = the base mode 0..5 (0 / 1 / 2: the gather of p.mode; 3 / 4: LayerNorm folded over the rows of
// A / of W; 5: the mode-3 gather) + 8 split-fp16 products (TT_F32) + 16 / + 32 W / A arrives pre-split + 64 the wide (windowed) variant.
// lnok / m3ok: the tile's LNOK / M3OK columns.  -1: mode 3 on a tile without the gather (tt_gemm refuses it before it gets here).
// Wide: modes 0 / 1 / 2, operands not pre-split, no fold (tt_gemm refuses the rest).  Pre-split: W wherever its rows are not the
// LayerNorm's, A only as a Linear operand whose rows are not (convs: only the weight is ever pre-split).
constexpr int tile_kmode(int mode, int ln_fold, int presplit, bool f32_split, bool wide, bool lnok, bool m3ok) {
  const int gather = mode == 0 ? 0 : (mode == 1 ? 1 : 2), split = f32_split ? 8 : 0;
  const int w_pre = f32_split && (presplit & 2) ? 16 : 0, a_pre = f32_split && (presplit & 1) ? 32 : 0;
  if (wide) return 64 + split + gather;
  if (mode == 3) return m3ok ? 5 + split + w_pre : -1;
  if (lnok && ln_fold == 1) return 3 + split + w_pre;
  if (lnok && ln_fold == 2) return 4 + split + a_pre;
  return gather + split + w_pre + (mode == 0 ? a_pre : 0);
}
// Every KMODE_ that is built, with the tiles it is built on: X(KMODE_, condition) over F32 (the TT_F32 tiles), LNOK / M3OK (the tile's
// columns) and WIDE (the units of TT_GEMM_WIDE_TILES).  A row more is a kernel more per tile: compile time and library size.
#define TT_GEMM_KMODES(X) \
  X(0, !WIDE) X(1, !WIDE) X(2, !WIDE) X(3, !WIDE && LNOK) X(4, !WIDE && LNOK) X(5, !WIDE && M3OK) \
  X(8, !WIDE && F32) X(8 + 16, !WIDE && F32) X(8 + 32, !WIDE && F32) X(8 + 48, !WIDE && F32) \
  X(9, !WIDE && F32) X(9 + 16, !WIDE && F32) X(10, !WIDE && F32) X(10 + 16, !WIDE && F32) \
  X(11, !WIDE && F32 && LNOK) X(11 + 16, !WIDE && F32 && LNOK) X(12, !WIDE && F32 && LNOK) X(12 + 32, !WIDE && F32 && LNOK) \
  X(13, !WIDE && F32 && M3OK) X(13 + 16, !WIDE && F32 && M3OK) \
  X(64, WIDE) X(64 + 1, WIDE) X(64 + 2, WIDE) X(64 + 8, WIDE && F32) X(64 + 9, WIDE && F32) X(64 + 10, WIDE && F32)

// LNOK: also instantiate the fused-LayerNorm variants (only the tile shapes the planner picks; gemm.hip keeps LayerNorm
// problems on them).  M3OK: likewise the mode-3 gather (KMODE 5).  Both are columns of the tile table below.
// ---- the tile table: every tile shape of gemm_kernel is written down here, once.  X(index, BM, BN, BK, NST, WGM, WGN, LNOK, M3OK);
// launch<Tag>() below, the planner's kCfgs[] / kCfgsF32[] and its "is the fused-LayerNorm / mode-3 variant built" answers
// (gemm.hip: ln_capable, mode3_capable) are all generated from these two lists, so they cannot drift apart.
#define TT_GEMM_TILES(X) \
  X( 0, 128, 128,  64, 2, 2, 2, false, false)   /* 4 waves, 64 KiB, 2 blocks/CU */ \
  X( 1, 128,  64,  64, 3, 2, 2, true,  true )   /* 72 KiB */ \
  X( 2,  64,  64,  64, 4, 2, 2, true,  true )   /* small problems, deep ring (64 KiB) */ \
  X( 3, 256, 128,  32, 3, 4, 2, true,  false)   /* 8 waves, 72 KiB -> 2 blocks/CU */ \
  X( 4, 256, 256,  32, 3, 2, 4, false, false)   /* 8 waves, 96 KiB */ \
  X( 5, 128, 128,  32, 3, 2, 2, false, false)   /* 48 KiB -> 3 blocks/CU */ \
  X( 6, 256, 128,  64, 3, 4, 2, false, false)   /* 8 waves, 144 KiB */ \
  X( 7, 128, 160,  64, 2, 4, 1, true,  false)   /* N = 320 without tile waste, wave tile 32x160, 72 KiB */ \
  X( 8, 128, 320,  32, 3, 4, 2, false, false)   /* 8 waves, wave tile 32x160, 84 KiB */ \
  X( 9, 256, 256,  64, 2, 2, 4, true,  false)   /* 8 waves, wave tile 128x64, 128 KiB, plain double buffer */ \
  X(10, 128, 128,  64, 4, 2, 2, false, false)   /* 128 KiB, 1 block/CU, prefetch distance 3 */ \
  X(11, 128, 128,  64, 2, 4, 2, true,  true )   /* 8 waves (wave tile 32x64), 64 KiB -> 16 waves/CU */ \
  X(12, 256, 160,  32, 3, 8, 1, false, false)   /* N = 320/960, 8 waves (wave tile 32x160), 78 KiB -> 2 blocks/CU */ \
  X(13, 256, 128,  32, 4, 4, 2, false, false)   /* like 3 with one more stage (96 KiB, 1 block/CU) */ \
  X(14, 128, 128,  32, 5, 4, 2, false, false)   /* 8 waves, 80 KiB, prefetch distance 4 (x32) -> 2 blocks/CU */ \
  X(15, 128, 128,  64, 3, 4, 2, false, false)   /* 8 waves, 96 KiB, prefetch distance 2 -> 1 block/CU */ \
  X(16, 128, 128,  64, 4, 4, 2, true,  true )   /* 8 waves, 128 KiB, prefetch distance 3 -> 1 block/CU */ \
  X(17, 256, 256,  32, 4, 2, 4, false, false)   /* 8 waves, wave tile 128x64, 128 KiB: three 32 KiB tiles in flight */ \
  X(18, 256, 128,  64, 2, 4, 2, false, false)   /* 8 waves, wave tile 64x64, 96 KiB, plain double buffer */ \
  X(19, 256, 128,  32, 5, 4, 2, false, false)   /* 8 waves, wave tile 64x64, 120 KiB: four 24 KiB tiles in flight */ \
  X(20, 128, 128, 128, 2, 4, 2, false, false)   /* 8 waves, 128-deep K steps (256-byte rows), 128 KiB double buffer: half the barriers per MFMA (opt-in, see make_plan) */
// TT_F32 (reference-precision mode): two tile shapes of the same kernel template.  BK counts elements, so 32 fp32
// elements give the 128-byte tile rows of the 16-bit BK = 64 configurations.
#define TT_GEMM_TILES_F32(X) \
  X( 0, 128, 128,  32, 2, 2, 2, true,  true ) \
  X( 1,  64,  64,  32, 4, 2, 2, true,  true )

struct TileCfg { int idx, bm, bn, bk, nst, wgm, wgn; bool ln, m3; };
#define TT_TILE_ROW(i, bm, bn, bk, nst, wgm, wgn, ln, m3) {i, bm, bn, bk, nst, wgm, wgn, ln, m3},
constexpr TileCfg kCfgs[] = {TT_GEMM_TILES(TT_TILE_ROW)};
constexpr TileCfg kCfgsF32[] = {TT_GEMM_TILES_F32(TT_TILE_ROW)};
#undef TT_TILE_ROW
constexpr int kNumCfgs = sizeof(kCfgs) / sizeof(kCfgs[0]);
template <int N> constexpr bool tiles_in_order(const TileCfg (&t)[N]) {
  for (int i = 0; i < N; ++i) if (t[i].idx != i) return false;
  return true;
}
static_assert(tiles_in_order(kCfgs) && tiles_in_order(kCfgsF32), "a tile's index is its position in the table (the planner and launch() both go by it)");

// ---- the tile shapes whose wide variant is built, by index into the tables above: what the planner gives a problem with an operand of
// 2 GiB or more -- 128 x 128 with 8 waves from 384 tiles on (16-bit) / from 256 tiles on (TT_F32) -- and what it gives the small strided
// problems of the tests (one block per CU with the 4-deep ring; the 64 x 64 TT_F32 tile).  X(index, BM, BN, BK, NST, WGM, WGN)
#define TT_GEMM_WIDE_TILES(X) \
  X(11, 128, 128,  64, 2, 4, 2) \
  X(16, 128, 128,  64, 4, 4, 2)
#define TT_GEMM_WIDE_TILES_F32(X) \
  X( 0, 128, 128,  32, 2, 2, 2) \
  X( 1,  64,  64,  32, 4, 2, 2)
#define TT_WIDE_SAME(i, bm_, bn_, bk_, nst_, wgm_, wgn_) && t[i].bm == bm_ && t[i].bn == bn_ && t[i].bk == bk_ && t[i].nst == nst_ && t[i].wgm == wgm_ && t[i].wgn == wgn_
template <int N> constexpr bool wide_tiles_match16(const TileCfg (&t)[N]) { return true TT_GEMM_WIDE_TILES(TT_WIDE_SAME); }
template <int N> constexpr bool wide_tiles_match32(const TileCfg (&t)[N]) { return true TT_GEMM_WIDE_TILES_F32(TT_WIDE_SAME); }
#undef TT_WIDE_SAME
static_assert(wide_tiles_match16(kCfgs) && wide_tiles_match32(kCfgsF32), "a wide tile is the narrow tile of the same index");
#define TT_WIDE_IS(i, bm, bn, bk, nst, wgm, wgn) || cfg == i
constexpr bool wide_capable(bool f32, int cfg) { return f32 ? (false TT_GEMM_WIDE_TILES_F32(TT_WIDE_IS)) : (false TT_GEMM_WIDE_TILES(TT_WIDE_IS)); }
#undef TT_WIDE_IS

}  // namespace ttg
