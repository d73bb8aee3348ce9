// tt_gemm: gather-GEMM on gfx950 MFMA (v_mfma_f32_32x32x16_{bf16,f16}).
//
//   out[m][n] = epilogue( sum_{tap,src,c} A_src[rowmap(m,tap)][c] * W[n][(tap,src,c)] )
//
// One kernel family covers nn.Linear, 1x1 conv, 3x3 conv (stride 1/2, fused nearest-x2 upsample),
// and the (3,1,1) temporal conv, with up to two channel sources (skip-concat without a concat
// buffer).  Structure:
//   * BM x BN x BK tiles, WGM x WGN waves (4 or 8), each wave owns (BM/WGM) x (BN/WGN) as 32x32 MFMA fragments;
//   * A and W tiles go HBM -> LDS by 16-byte LDS-DMA (global_load_lds) into an NST-deep ring: tile kt+NST-1 is
//     issued while tile kt is computed, and the wait before tile kt is a COUNTED s_waitcnt vmcnt(G*(NST-2)), so
//     NST-2 tiles stay in flight across the (raw) s_barrier -- one barrier per K step, no vmcnt(0) in the loop
//     (cdna guide T3+T4).  Out-of-range rows / conv halo / K tails point their lane at a zero page;
//   * LDS image is lane-linear with the XOR swizzle applied on the SOURCE chunk and on the read
//     (conflict-free ds_read_b128, see common.h);
//   * MFMA operands are swapped (W fragment as the MFMA "A" operand) so each lane ends up with 4
//     consecutive output columns of one row: 8-byte epilogue loads/stores;
//   * every lane addresses an operand with a 32-bit byte offset into a buffer descriptor.  The narrow instances (and the persistent /
//     big-tile / streaming kernels) put the descriptor on the operand's base: operands below 2 GiB.  A problem in which a0, out, residual
//     or blend spans 2 GiB or more runs the template's WIDE variant (KMODE + 64, gemm_inst_wide_*.hip), in which each workgroup rebases
//     its descriptors once per tile, in 64-bit scalar arithmetic, onto the first row the tile can touch: same tile, ring, K order and
//     epilogue arithmetic, the same bits (the temporal VAE decoder at 576x1024: 302 MB of activations per frame).
//
// Host side of this file: the per-route predicates (pp_ok, sq320_ok, w320_route, ... -- each with the measurements behind its thresholds),
// ONE resolver that sequences them (wanted_route / granted_route -> Route), and five short entry points that read its answer.
// The tile shapes live in one table (TT_GEMM_TILES in gemm_tiles.h); the tuning knobs in one struct read once (knobs()).
#include <stdlib.h>
#include "gemm_params.h"
#include "gemm_splitk.h"
#include "gemm_sq320.h"
#include "gemm_tiles.h"

namespace ttg {
// per-dtype instantiation units (gemm_inst_*.hip)
void launch_bf16(GemmP& p, int cfg, hipStream_t st);
void launch_f16(GemmP& p, int cfg, hipStream_t st);
void launch_f32(GemmP& p, int cfg, hipStream_t st);
void launch_wide_bf16(GemmP& p, int cfg, hipStream_t st);   // gemm_inst_wide_*.hip: the windowed variants (operands of 2 GiB and more)
void launch_wide_f16(GemmP& p, int cfg, hipStream_t st);
void launch_wide_f32(GemmP& p, int cfg, hipStream_t st);
void launch_sq320_bf16(const GemmP& p, hipStream_t st);
void launch_sq320_f16(const GemmP& p, hipStream_t st);
void launch_pp_bf16(GemmP& p, hipStream_t st);         // gemm_pp.hip: persistent 256 x 256 x 64 ping-pong kernel
void launch_pp_f16(GemmP& p, hipStream_t st);
void launch_w320(GemmP& p, hipStream_t st, int bm, bool bf16);      // gemm_w320.hip: 256 x 320 x 64 tiles for N = 320 t at the finest UNet level; bm = 128: the variant (two K halves per slab) for problems with fewer rows
}
using namespace ttg;

namespace {
// taps per output row: 9 for both 3x3 gathers (mode 1: pad 1 all round, mode 3: pad on the bottom / right only), 3 for the temporal conv
inline int gemm_taps(int mode) { return mode == 1 || mode == 3 ? 9 : (mode == 2 ? 3 : 1); }

// upsample = 2: the nearest-x2 upsampling 3x3 conv on phase-packed weights (packing.pack_upsample_phases: [n, 16 * k0], phase-major).  An
// output pixel of phase (py, px) = (Y & 1, X & 1) sees 2 x 2 distinct low-res pixels, so its nine taps collapse onto four whose weights
// were added at pack time: 4/9 of the products of upsample = 1.  One launch of the tiled template: blocks tile the LOW-RES rows, the four
// phases of a tile are neighbouring slices (each walks its 4 taps and owns its output rows: no slab, no reduction pass).
inline bool is_up2(const TtGemmArgs* a) { return a->mode == 1 && a->upsample == 2; }
// what such a problem may carry (tt_gemm and tt_gemm_plan refuse the rest alike): one source, bias, stride 1, any storage type
const char* up2_refusal(const TtGemmArgs* a) {
  if (a->stride != 1 || a->hout != 2 * a->hin || a->wout != 2 * a->win) return "stride 1 with hout = 2 hin and wout = 2 win";
  if (a->a1 || a->k1) return "one source (no a1 / k1)";
  if (a->residual || a->blend || a->rowvec) return "a bias-only epilogue (no residual / blend / rowvec)";
  if (a->stats_out || a->gn_out) return "no stats_out / gn_out";
  if (a->geglu || a->ln_fold || a->out_fp8 || a->out_f32 || a->out_col_hw) return "no geglu / ln_fold / out_fp8 / out_f32 / out_col_hw";
  return nullptr;
}

// Every tuning knob of the planner.  All of them are read from the environment together, once per process, by the first call that asks
// for one (the function-local static of knobs(): initialised exactly once, also under concurrent callers); the four tt_gemm_set_*
// setters overwrite theirs afterwards.  What each one steers is written at the predicate that reads it.
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
// tt_gemm_set_big_tile / TT_GEMM_W320 -> bit 0 the 256 x 320 kernel, bit 1 its 128 x 320 variant, bit 2: that one for conv3x3 only, bit 3: its split-K route
int big_tile_bits(int on) { return on == 0 ? 0 : (on == 2 ? 1 : (on == 3 ? 11 : (on == 4 ? 7 : 15))); }
struct Knobs {
  int forced_cfg = env_int("TT_GEMM_CFG", -1);                    // tt_gemm_set_tile_override
  int group_m = env_int("TT_GEMM_GROUP_M", 0);                    // tuning switch: <rows> overrides the group height of the tile order (gemm_launch.h: tile_params picks it otherwise)
  int forced_split = env_int("TT_GEMM_SPLITK", -1);
  int deep = env_int("TT_GEMM_DEEP", 1);
  int small64 = env_int("TT_GEMM_SMALL64", 2);
  int sq320 = env_int("TT_GEMM_SQ320", 2);                        // tt_gemm_set_streaming_square
  int sq320_rowvec = env_int("TT_SQ320_ROWVEC", 1);
  int sq320_min_rows = env_int("TT_SQ320_MIN_ROWS", 131072);
  int pp = env_int("TT_GEMM_PP", 1);
  int pp_geglu_min_tiles = env_int("TT_PP_GEGLU_MIN_TILES", 400);
  int pp_geglu_min_fill = env_int("TT_PP_GEGLU_MIN_FILL", 75);
  int pp_min_tiles = env_int("TT_PP_MIN_TILES", 460);
  int pp_min_fill = env_int("TT_PP_MIN_FILL", 90);
  int pp_split_whole = env_int("TT_PP_SPLIT_WHOLE", 1);
  int w320 = big_tile_bits(env_int("TT_GEMM_W320", 1));           // tt_gemm_set_big_tile
  int w320_force = env_int("TT_W320_FORCE", 0);
  int w320_min_fill = env_int("TT_W320_MIN_FILL", 60);
  int f32_split = env_int("TT_F32_SPLIT", 0) ? 1 : 0;             // tt_gemm_set_f32_split
  int f32_split_min_tiles = env_int("TT_F32_SPLIT_MIN_TILES", 160);
  int f32_splitk = env_int("TT_F32_SPLITK", 1);
  int wide = env_int("TT_GEMM_WIDE", 1);                          // tt_gemm_set_wide
};
Knobs& knobs() { static Knobs k; return k; }

// Tile + split-K plan, tuned on MI355X with tools/gemm_bench.py (shapes of the SVD UNet at 256x448 and 512x896):
//   * N = 320 / 960 (multiple of 160 but not of 128): 128x160 tiles, no column waste;
//   * tall problems with wide N: 256x128, 8 waves;
//   * otherwise the largest of 128x128 / 128x64 / 64x64 that still yields ~1.5 workgroups per CU;
//   * few tiles but a long K (convs at the two coarsest levels): 128x128 tiles with the K loop split over S
//     workgroups, fp32 slabs reduced in fixed order by a second kernel.
struct Plan { int cfg, splitk; };

// `wide_ok`: the 256x128 tile pays for tall-and-wide problems (GEGLU projections, fused QKV) unless the epilogue reads
// per-row tensors (residual / blend / row vector): its 128-VGPR budget has no room to preload them, so they would be read
// between the stores (measured: 16 us epilogue instead of 3)
// `forced`: the tile shape to take whatever the problem (tt_gemm_set_tile_override / TT_GEMM_CFG), -1 for the planner's own choice
Plan make_plan(int forced, int m, int n, long ktot, bool allow_split, bool wide_ok = true, bool mode0 = false, bool k128 = false) {
  Plan pl{0, 1};
  const int f = forced;
  const long b128 = (long)ceil_div(m, 128) * ceil_div(n, 128);
  const long b12864 = (long)ceil_div(m, 128) * ceil_div(n, 64);
  if (f >= 0 && f < kNumCfgs) pl.cfg = f;
  else if (n % 160 == 0 && n % 128 != 0 && n <= 960 && m >= 2048) pl.cfg = 7;
  // (256x256 tiles -- cfg 9 -- win 6..25 % on the wide GEGLU / QKV projections in isolation (tools/gemm_cold.py) but lose
  // inside the two-branch step graph, where one 128 KiB block per CU shuts the other branch's kernels out: FF1 at 32x56
  // 144 vs 137 us, QKV at 16x28 60 vs 48 us per launch -- profiles/r2_*_kernel_by_grid.txt history.  Not routed.)
  else if (m >= 8192 && n >= 1024 && wide_ok) pl.cfg = 3;
  else if (m < 2048 && n >= 2560 && n % 160 == 0) pl.cfg = 7;
  else if (b128 >= 384) pl.cfg = 11;                 // 128x128 with 8 waves (32x64 wave tiles): 16 waves per CU
  else if (b12864 >= 384) pl.cfg = 1;
  else pl.cfg = 2;
  const int fs = knobs().forced_split;
  if (fs >= 1) { pl.splitk = allow_split ? fs : 1; return pl; }
  const long kt = (ktot + 63) / 64;
  const int deep = knobs().deep;
  if (deep && f < 0 && b128 <= 256 && ktot > 0) {
    // at most one 128x128 tile per CU: LDS is free for a 4-deep ring (prefetch distance 3), which beats two resident
    // blocks with a double buffer once the loads really overlap the MFMAs; K is split only as far as whole CUs are idle.
    // (128-deep K steps for channel counts that are multiples of 128 -- cfg 20, one barrier pair per 16 MFMAs of a wave -- are faster
    // in isolation: FF2 at 3136 rows 690 -> 791 TFLOP/s, K = 1280 509 -> 556, the 3x3 conv 792 -> 848 (tools/gemm_bench.py 16 20), and
    // slower in the step: 31.19 / 31.23 -> 31.48 / 31.51 ms, restricted to K >= 4096 30.83 / 31.08 -> 31.26 / 31.17: a double buffer
    // has one K step of prefetch where the 4-deep ring has three.  Opt-in: TT_GEMM_DEEP=2.)
    // Short-K linears that leave half of the CUs without a 128 x 128 tile (the half-row output projections of the cross-attentions at the
    // third level, everything K = C at the coarsest one) on 64 x 64 tiles, two blocks per CU, all resident at once: faster on warm operands
    // (tools/small_gemm_sweep.py, us in a graph of ten launches: 1568 x 1280 x 1280 16.8 -> 12.3, 784 rows 16.6 -> 11.3, 392 rows 13.7 -> 10.0),
    // NOT in the step, where every weight comes from HBM once and 64-row tiles fetch it twice as often: 29.06 / 29.18 -> 29.10 / 29.10 ms
    // (one call, interleaved).  Opt-in: TT_GEMM_SMALL64=1.  Default (2): only wide problems (n >= 4096) of at most 64 rows -- the 64-row tail of the third level's
    // GEGLU projection (3136 = 12 x 256 + 64 rows; 21 launches per step), half of whose 128-row tiles was padding: 29.78 / 29.76 -> 29.70 / 29.67 ms.
    const int small64 = knobs().small64;
    if (small64 && (small64 != 2 || (m <= 64 && n >= 4096)) && mode0 && ktot <= 2048 && (long)ceil_div(m, 64) * ceil_div(n, 64) <= 512) { pl.cfg = 2; return pl; }   // (2: only the <= 64-row tails)
    // (Round 6, tools/coarse_conv_probe.py / profiles/r6_coarse_conv_probe.txt: on cold weights in isolation the 70-tile convs of the coarsest
    // level are 18-20 % faster as two resident double-buffered 8-wave workgroups per CU with six K slices -- cfg 11: 53.6 -> 43.9 us,
    // 92.7 -> 74.2 us, reduction pass included -- and the step does not move: 28.97 / 29.06 vs 29.05 / 29.00 ms, one call, interleaved.
    // Not routed: once more, an isolated sweep does not predict the step.)
    pl.cfg = (deep == 2 && k128) ? 20 : 16;
    long s = allow_split ? 256 / b128 : 1;
    if (s > kt / 8) s = kt / 8;
    if (s > 16) s = 16;
    pl.splitk = s >= 2 ? (int)s : 1;
    return pl;
  }
  if (allow_split && f < 0 && b128 < 384 && kt >= 40) {
    long s = (512 + b128 - 1) / b128;
    if (s > kt / 8) s = kt / 8;
    if (s > 16) s = 16;
    if (s >= 2) { pl.cfg = 11; pl.splitk = (int)s; }
  }
  return pl;
}

int plan_f32(int m, int n, int min_tiles = 256) { return (long)ceil_div(m, 128) * ceil_div(n, 128) >= min_tiles ? 0 : 1; }

// ---- the per-route predicates
// a row vector the streaming kernel can carry: at most two distinct rows over the launch (both preloaded), on the residual form
bool sq320_rowvec_ok(const TtGemmArgs* a) {
  if (!a->rowvec) return true;
  if (!knobs().sq320_rowvec || !a->residual) return false;     // (TT_SQ320_ROWVEC=0: A/B)
  if (a->rowvec_mod == 2 && a->rowvec_rows == 1) return true;
  return a->rowvec_mod == 0 && a->rowvec_rows >= 32 && a->rowvec_rows % 32 == 0 && (long)a->rowvec_rows * 2 >= a->m;
}
bool sq320_ok(const TtGemmArgs* a) {
  // 0 off, 1 on, 2 (default) by size: at 64x112 latents (200 704 rows: 784 big tiles = 3.06 rounds of 196) the 32-row streaming kernel wins
  // (block l0hi 5.46 -> 5.39 ms, fp8 4.995 -> 4.91; 512x896 step 109.6 -> 109.1 ms), at 32x56 it loses (29.04 -> 29.32 ms): one call each, interleaved
  const int on = knobs().sq320;                                // (TT_GEMM_SQ320, the size bar TT_SQ320_MIN_ROWS)
  if (on == 2 && a->m < knobs().sq320_min_rows) return false;
  return on && a->dtype != TT_F32 && !a->ln_fold && !a->out_fp8 && knobs().forced_cfg < 0 && a->mode == 0 && a->k1 == 0 && a->k0 == SQ_K && a->n == SQ_N && a->m >= 4096 &&
         !a->geglu && sq320_rowvec_ok(a) && !a->out_f32 && !a->out_col_hw &&
         (!a->blend || (a->blend == a->residual && a->ld_blend == a->ld_res));
}
// The persistent big-tile kernel (gemm_pp.hip) takes tall-and-wide Linear problems without per-row epilogue operands when every CU
// gets about two or more 256 x 256 tiles and the last round of tiles is nearly full: the GEGLU projections at the three finest UNet
// levels (1960 / 980 / 480 tiles).  A problem whose row count is not a multiple of 256 and that only qualifies without its
// ragged last tile row is launched in two parts -- whole tile rows on the persistent kernel, the remaining < 256 rows on the tiled
// kernel (3136 rows: 480 tiles = 1.9 rounds + 64 rows, instead of 520 tiles = 3 rounds; the persistent kernel has no short cut for
// a ragged tile -- its out-of-range rows are zero-filled by the DMA bounds check and multiplied like any others, so it costs a
// whole tile time -- and cutting tiles along K stream-K fashion costs more in partial-tile traffic than it saves: DESIGN.md
// section 6.0).  TT_GEMM_PP=0 keeps everything on the tiled kernels (A/B).
// The constants below (256 CUs, one workgroup per CU) are MI355X in SPX mode: the only target of this library (gfx950, tt_target_arch).
bool pp_ok(const TtGemmArgs* a) {
  const Knobs& k = knobs();
  if (!k.pp || k.forced_cfg >= 0 || a->dtype == TT_F32 || a->mode != 0 || a->k1 != 0 || a->ln_fold > 1 || a->out_fp8 || a->residual || a->blend ||
      a->rowvec || a->out_f32 || a->out_col_hw || (a->k0 & 63) || a->k0 < 128 || (a->n & 15) || (a->ldo & 7))
    return false;
  const long tiles = (long)ceil_div(a->m, 256) * ceil_div(a->n, 256);
  const long rounds = (tiles + 255) / 256;
  // The GEGLU projections have their own, lower bar (TT_PP_GEGLU_MIN_TILES / _MIN_FILL, A/B): their alternative is the tiled template at
  // 640-670 TFLOP/s, which a persistent launch beats even with a 75 %-full last round -- 256x384: 10752 x 5120 (840 tiles, 82 %) and
  // 2688 x 10240 (400 whole tiles, 78 %): --res ref 27.72 -> 27.06 ms with 400 / 75 against 460 / 90 (one call, interleaved).  256x448 and
  // 512x896 do not change: their projections pass either bar or fall below both.
  if (a->geglu) return tiles >= k.pp_geglu_min_tiles && tiles * 100 >= rounds * 256 * k.pp_geglu_min_fill;
  // (TT_PP_MIN_TILES / TT_PP_MIN_FILL, A/B)
  return tiles >= k.pp_min_tiles && tiles * 100 >= rounds * 256 * k.pp_min_fill;      // ~2 rounds of tiles per CU or more, last round >= 90 % full on average
}
// The 256 x 320 big-tile kernel (gemm_w320.hip) takes 16-bit problems whose output width is a multiple of 320 and whose row count
// fills most of a round of 256 CUs with 256-row tiles (the finest UNet level: 50176 rows = 196 tiles): Linear (one or two sources,
// optional LayerNorm fold of the A rows), conv3x3 stride 1 and the temporal conv, with bias / scale / row vector (groups of >= 32
// rows) / residual / AlphaBlender epilogues.  TT_GEMM_W320=0 keeps them on the tiled kernels (A/B).
// what both kernels of gemm_w320.hip need of a problem
bool w320_eligible(const TtGemmArgs* a) {
  if (!knobs().w320 || knobs().forced_cfg >= 0 || a->mode == 3 || a->dtype == TT_F32 || a->n % 320 || (a->k0 & 63) || (a->k1 & 63) || gemm_taps(a->mode) * (a->k0 + a->k1) < 128 || a->geglu ||
      a->out_fp8 || a->out_f32 || a->out_col_hw || a->ln_fold > 1 || (a->ln_fold && (a->mode != 0 || a->k1)))
    return false;
  if (a->mode == 1 && (a->stride != 1 || a->upsample || a->hin != a->hout || a->win != a->wout || a->win >= 32768 || a->hin >= 32768)) return false;
  if (a->rowvec && a->rowvec_rows < 32 && !(a->rowvec_rows == 1 && a->rowvec_mod == 2)) return false;
  // 8-byte (16-bit operands) / 16-byte (fp32 vectors) epilogue accesses
  if ((a->ldo & 3) || (a->residual && (a->ld_res & 3)) || (a->blend && (a->ld_blend & 3)) || (a->rowvec && (a->ld_rowvec & 3))) return false;
  if ((((size_t)a->out | (size_t)a->residual | (size_t)a->blend) & 7) || (((size_t)a->rowvec | (size_t)a->bias) & 15)) return false;
  return true;
}
// 0: not served; 1: 256 x 320 tiles (gemm_w320_kernel); 2: 128 x 320 tiles (gemm_w320h_kernel: problems whose 256-row tiles would fill
// less than 70 % of a round, e.g. the second UNet level at 32x56 latents -- 12544 rows, N = 640: 98 x 2 = 196 tiles of 128 rows).
// By default the variant takes conv3x3 problems only: A/B in the step 31.06 (256-row kernel only) / 31.01 (variant for all modes) /
// 30.84 ms (variant for the convs); in isolation +9..16 % on the convs, +-0 on the linears and temporal convs (tools/w320_bench.py).
// TT_W320_MIN_FILL: percent of the CU x round slots the tiles must fill (A/B).  Tuning aid: TT_W320_FORCE=1|2 routes every eligible
// problem to the 256- / 128-row kernel whatever the fill.
int w320_route(const TtGemmArgs* a) {
  if (!w320_eligible(a)) return 0;
  const Knobs& k = knobs();
  if (k.w320_force == 1 || k.w320_force == 2) return k.w320_force;
  for (int half = 0; half < 2; ++half) {
    if (half && (!(k.w320 & 2) || ((k.w320 & 4) && a->mode != 1))) break;     // tt_gemm_set_big_tile(2): the 256-row kernel only
    const long tiles = (long)ceil_div(a->m, half ? 128 : 256) * (a->n / 320);
    const long rounds = (tiles + 255) / 256;
    if (tiles * 100 >= rounds * 256 * k.w320_min_fill) return 1 + half;   // >= 70 % of the CU x round slots busy (196 / 392 / 588 / 784 tiles: 77 %)
  }
  return 0;
}
// Split-K route of the 128 x 320 kernel for the coarse UNet levels (3136 / 784 rows at 32x56 latents: 100 / 28 tiles), where no tile
// shape fills the chip and the tiled 128 x 128 kernel keeps the matrix pipe 35 % busy (profiles/r4_gemm_sq_counters.txt): S workgroups
// per tile, each with >= 20 (conv3x3) / 32 (Linear) slabs of K, at most 256 workgroups and at least 160; the fp32 slabs are summed in a
// fixed order by splitk_epilogue_kernel.  Returns S (0: not served).  Measured (tools/w320_split_probe.py, us, tiled -> split):
//   conv3x3 at 3136 rows, 1280 / 1920 / 2560 -> 1280 channels   129.7 -> 108.5   173.2 -> 145.3   231.0 -> 190.3   (S = 2)
//   FF2 at 3136 rows (K = 5120, S = 2) 64.2 -> 63.5;   conv3x3 at 784 rows (S = 9) 46.4 -> 47.1, 79.7 -> 75.6
// -- the second pass and the fp32 slabs cost ~25 us per problem, so by default only the 3x3 convs with >= 64 tiles take the route;
// tt_gemm_set_big_tile(3) opens it to the Linear problems and the 28-tile level as well (tests, A/B).
// (Asked only of problems that w320_route does not serve: the resolver's order.)
int w320_split(const TtGemmArgs* a) {
  const int bits = knobs().w320;
  if (!w320_eligible(a) || !(bits & 8) || a->ln_fold || a->mode == 2) return 0;
  const long tiles = (long)ceil_div(a->m, 128) * (a->n / 320);
  if ((bits & 4) && (a->mode != 1 || tiles < 64)) return 0;
  const long slabs = (long)gemm_taps(a->mode) * (a->k0 + a->k1) / 64;
  long s = 256 / tiles;
  const long by_k = slabs / (a->mode == 1 ? 20 : 32);
  if (s > by_k) s = by_k;
  if (s > 16) s = 16;
  if (s < 2 || tiles * s < 160 || s * a->m * a->n * 4 >= (1L << 31)) return 0;
  return (int)s;
}
size_t slab_bytes(const TtGemmArgs* a, int split) { return (size_t)split * a->m * a->n * sizeof(float); }
bool ws_fits(const TtGemmArgs* a, int split) { return a->ws && (size_t)a->ws_bytes >= slab_bytes(a, split); }
// rows the persistent kernel takes when the problem is launched in two parts (0: one launch)
// (also for row counts that ARE whole tile rows but leave the last round of tiles poorly filled: 10752 x 5120 at 256x384 -- 840 tiles = 3.3
// rounds -- runs its first 38 tile rows, 2.97 rounds, on the persistent kernel and the last 1024 rows on the tiled one; at most 1/8 of the
// rows go to the tail)
// `served`: a big-tile kernel of its own (sq320 / w320) takes the whole problem.  Asked only of problems that pp_ok refuses as a whole.
int pp_head_rows(const TtGemmArgs* a, bool served) {
  if (a->m < 512) return 0;
  // TT_PP_SPLIT_WHOLE=0: ragged row counts only (A/B)
  if ((a->m & 255) == 0 && (!knobs().pp_split_whole || served)) return 0;       // (whole tile rows: only problems no big-tile kernel of their own serves)
  TtGemmArgs head = *a;
  for (int tr = a->m >> 8; tr >= 2 && (long)(a->m - tr * 256) * 8 <= a->m; --tr) {
    head.m = tr * 256;
    if (head.m < a->m && pp_ok(&head)) return head.m;
  }
  return 0;
}
void pp_split(const TtGemmArgs* a, int rows, TtGemmArgs* head, TtGemmArgs* tail) {
  const size_t es = 2;                                      // 16-bit storage (pp_ok)
  *head = *a; *tail = *a;
  head->m = rows;
  tail->m = a->m - rows;
  tail->a0 = (const char*)a->a0 + (size_t)rows * a->lda0 * es;
  tail->out = (char*)a->out + (size_t)rows * a->ldo * es;
}

// ---- plans of the tiled template
const TileCfg& tile_of(int dtype, int cfg) { return dtype == TT_F32 ? kCfgsF32[cfg] : kCfgs[cfg]; }
// tile shapes whose fused-LayerNorm variants are built: the ones the planner picks (the LNOK column of the tile table)
bool ln_capable(int cfg) { return kCfgs[cfg].ln; }
// 16-bit tile shapes whose mode-3 gather is built (the M3OK column; TT_F32: both of its shapes): what mode3_plan maps every
// plan of a mode-3 problem onto.  A forced tile shape outside this set is refused (TT_EUNSUPPORTED), never replaced.
bool mode3_capable(int cfg) { return kCfgs[cfg].m3; }
Plan mode3_plan(const TtGemmArgs* a, Plan pl) {
  if (a->mode != 3 || a->dtype == TT_F32 || knobs().forced_cfg >= 0 || mode3_capable(pl.cfg)) return pl;
  if (pl.cfg == 20) return Plan{16, pl.splitk};          // (TT_GEMM_DEEP=2: the 4-deep ring's split plan instead of the 128-deep K steps)
  const long b128 = (long)ceil_div(a->m, 128) * ceil_div(a->n, 128), b12864 = (long)ceil_div(a->m, 128) * ceil_div(a->n, 64);
  return Plan{b128 >= 384 ? 11 : (b12864 >= 384 ? 1 : 2), 1};   // (the wide / N = 160 t shapes: make_plan's choice for the other sizes)
}
// do the products of `a` run split (GemmP.f32_split)?
int f32_split_of(const TtGemmArgs* a) { return a->dtype == TT_F32 ? knobs().f32_split : 0; }
bool mode3_served(const TtGemmArgs* a, const Plan& pl) { return a->mode != 3 || tile_of(a->dtype, pl.cfg).m3; }
// TT_F32 products: 0 = exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, 157 TFLOP/s peak), 1 = "split16": every fp32 operand split on the fly into
// fp16 hi + lo, three 16-bit MFMAs per product block (gemm_kernel.h, `mma`): ~2^-21 relative per product at 3 / 16 of the issue time.
// upsample = 2: never split along K (the four phase slices are the launch's slices).  Tile by the number of blocks, phases included:
// two resident double-buffered 128 x 128 workgroups per CU from more than one block per CU on, else one with the 4-deep ring.
Plan up2_plan(const TtGemmArgs* a) {
  const long blocks = 4L * ceil_div(a->m / 4, 128) * ceil_div(a->n, 128);
  if (a->dtype == TT_F32) return Plan{blocks >= 256 ? 0 : 1, 1};
  const int f = knobs().forced_cfg;
  if (f >= 0 && f < kNumCfgs) return Plan{f, 1};
  return Plan{blocks > 256 ? 11 : 16, 1};
}
Plan plan_for(const TtGemmArgs* a) {
  if (is_up2(a)) return up2_plan(a);
  if (a->dtype == TT_F32) {
    // split16: the 64 x 64 tiles' 32 x 32 wave tiles convert two operand fragments per product block (VALU-bound, ~110 TFLOP/s against
    // ~210 on the 128 x 128 tiles' 64 x 64 wave tiles), so the big tile is taken from 160 tiles on (3136 x 1280: 250 tiles = one round)
    const int split_min = knobs().f32_split_min_tiles;          // (TT_F32_SPLIT_MIN_TILES)
    // (256 x 128 tiles with 8 waves -- the same wave tiles, 25 % less LDS fill per flop, one workgroup per CU -- measured SLOWER:
    // 109.3 -> 114.1 ms / step, one call; the loop is bound by the VALU conversions + MFMA issue of its two waves per SIMD, not by the fill)
    // Other shapes of the big tile, each one gpurun call against 106-108 ms / step for this one: 128 x 128 x 16 with a 4-deep / 3-deep ring
    // (three / two tiles in flight instead of one) 112.7 / 112.0; x 32 with a 3-deep ring (96 KiB: one workgroup per CU) 135.5; 8 waves
    // as 4 x 2 / 2 x 4 (wave tiles 32 x 64 / 64 x 32 at a 128-register budget) 123.4 / 234.2; 128 x 64 x 32, 3-deep 127.7.
    // (4 waves as 4 x 1 -- every A fragment converted by one wave instead of two -- 105.1 -> 104.0 ms, within the noise; as 1 x 4 149.6.)
    // Where the time goes (ablation builds `make variant DEFS=-DTT_SPLIT_ABL=1|2|3`, wrong numbers, one call; the flag ended with commit 83d2c66,
    // the last that builds it): 105.4 ms as built; without
    // any conversion 74.8; with one MFMA per product block instead of three 75.1; with neither 65.9 -- conversions and the two extra MFMAs
    // cost ~9 ms each on their own and ~40 ms together: inside one wave they run back to back (the fragment consumers are pinned by
    // sched_barrier: the raw-read hazard of gemm_kernel.h), so the matrix pipe idles while a wave converts.
    if (knobs().f32_split) {
      // split16, few tiles and a long K (the coarsest level's convs: 784 rows x 1280 x 11 520 = 70 tiles of 128 x 128, 360 K steps of 32): the
      // 64 x 64 tiles ran them at ~100 TFLOP/s (260 workgroups, one round, VALU-bound wave tiles).  The K loop split over S workgroups per
      // 128 x 128 tile, fp32 slabs summed in a fixed order by the reduction pass (the 16-bit modes' plan for these shapes; bit-reproducible).
      // (TT_F32_SPLITK=0: A/B)
      const long b128 = (long)ceil_div(a->m, 128) * ceil_div(a->n, 128);
      const long kt = (long)gemm_taps(a->mode) * (a->k0 + a->k1) / 32;
      if (knobs().f32_splitk && !a->geglu && !a->ln_fold && !a->out_col_hw && b128 < split_min && kt >= 64) {
        long sp = 448 / b128;
        if (sp > kt / 16) sp = kt / 16;
        if (sp > 16) sp = 16;
        if (sp >= 2) return Plan{0, (int)sp};
      }
    }
    return Plan{plan_f32(a->m, a->n, knobs().f32_split ? split_min : 256), 1};
  }
  const long ktot = (long)gemm_taps(a->mode) * (a->k0 + a->k1);
  const bool allow = !a->geglu && !a->ln_fold && !a->out_fp8;       // a K slice would see only part of a LayerNorm row
  const bool k128 = (a->k0 & 127) == 0 && (a->k1 & 127) == 0;
  const bool wide_ok = !(a->residual || a->blend || a->rowvec);
  Plan pl = make_plan(knobs().forced_cfg, a->m, a->n, ktot, allow, wide_ok, a->mode == 0, k128);
  if (a->ln_fold && !ln_capable(pl.cfg))             // a forced tile shape without the fused variant: planner's own choice
    pl = make_plan(-1, a->m, a->n, ktot, false, wide_ok, a->mode == 0);
  return mode3_plan(a, pl);
}
// the plan of a problem whose split plan cannot be served (no / too small a workspace)
Plan unsplit_plan(const TtGemmArgs* a) {
  if (a->dtype == TT_F32) return Plan{plan_f32(a->m, a->n, 256), 1};
  return mode3_plan(a, Plan{make_plan(knobs().forced_cfg, a->m, a->n, 0, false, !(a->residual || a->blend || a->rowvec)).cfg, 1});
}

// ---- the route resolver: the ONE place that sequences the predicates above.  Every entry point below reads its answer.
//   wanted_route: the kernel a problem would run on if it were handed the workspace tt_gemm_ws_bytes asks for;
//   granted_route: what it gets with the ws / ws_bytes it carries (a split plan without its slabs falls back, never fails).
// Order: persistent kernel (whole, then head + tail) > streaming 320 x 320 > 256 x 320 / 128 x 320 > 128 x 320 split-K > tiled template.
// Where the entry points disagree (each one's observable answer is pinned by tests/test_gemm_routes_cpu.py and kept as it was):
//   * slabs of 2 GiB or more: tt_gemm_ws_bytes reports a tiled split plan's size from the WANTED route; tt_gemm, tt_gemm_plan,
//     tt_gemm_stats_rows and tt_gemm_gn_fused take the granted one, which un-splits such a plan whatever the workspace;
//   * a 128 x 320 split-K problem without its workspace falls to the tiled template's plan, which may be a split plan of a different
//     slab count: tt_gemm_ws_bytes never reports that second size;
//   * TT_F32 split16: an un-split plan takes the 128 x 128 tile from 256 tiles on, the plan it replaces from TT_F32_SPLIT_MIN_TILES on;
//   * a two-part problem: tt_gemm_plan / tt_gemm_stats_rows / tt_gemm_gn_fused answer for the head (the persistent kernel),
//     tt_gemm_ws_bytes for the tail; the tail's own route is visible only by asking about the tail;
//   * tt_gemm_stats_rows tells "big-tile kernel" from "tiled template" by the tile (BN = 320 or no ring), so a forced 128 x 320 x 32
//     tile (cfg 8) gets the big-tile kernels' answer.
enum class Kind { PP, PP_TWO_PART, SQ320, W320, W320H, W320H_SPLIT, TILED, UNSUPPORTED };
struct Route { Kind kind; int cfg; int splitk; int head_rows; bool wide; };       // cfg: tile table index (TILED / UNSUPPORTED); head_rows: PP_TWO_PART; wide: the windowed variant of the tile

Route tiled_route(const TtGemmArgs* a, Plan pl) { return Route{mode3_served(a, pl) ? Kind::TILED : Kind::UNSUPPORTED, pl.cfg, pl.splitk, 0, false}; }
Route wanted_route(const TtGemmArgs* a) {
  if (pp_ok(a)) return Route{Kind::PP, -1, 1, 0, false};
  const bool sq = sq320_ok(a);
  const int big = w320_route(a);
  if (const int rows = pp_head_rows(a, sq || big)) return Route{Kind::PP_TWO_PART, -1, 1, rows, false};
  if (sq) return Route{Kind::SQ320, -1, 1, 0, false};
  if (big) return Route{big == 1 ? Kind::W320 : Kind::W320H, -1, 1, 0, false};
  if (const int split = w320_split(a)) return Route{Kind::W320H_SPLIT, -1, split, 0, false};
  return tiled_route(a, plan_for(a));
}
Route granted_route(const TtGemmArgs* a, Route r) {
  if (r.kind == Kind::W320H_SPLIT && !ws_fits(a, r.splitk)) r = tiled_route(a, plan_for(a));
  // no workspace, or slabs beyond the 32-bit offsets: un-split plan (still correct)
  if (r.kind == Kind::TILED && r.splitk > 1 && (!ws_fits(a, r.splitk) || slab_bytes(a, r.splitk) >= ((size_t)1 << 31))) r = tiled_route(a, unsplit_plan(a));
  return r;
}

// ---- the wide route: the tiled template's windowed variant (gemm_kernel.h, KMODE + 64) for problems in which a0, a1, out, residual or
// blend spans 2 GiB or more -- every other kernel, and the narrow template, index an operand with 32-bit byte offsets from its base.
// tt_gemm_set_wide / TT_GEMM_WIDE: 0 never (such a problem is refused, as before the route existed), 1 (default) the problems that need
// it, 2 every problem it can serve (tests, A/B measurements: the same bits as the narrow route).
struct Extents { long a0, a1, w, out, res, blend, rowvec; };          // bytes from each operand's base to the end of its last row
Extents extents_of(const TtGemmArgs* a) {
  const long es = a->dtype == TT_F32 ? 4 : 2;
  const long rows = a->mode == 1 || a->mode == 3 ? (long)a->nimg * a->hin * a->win : (long)a->m;
  const long taps = is_up2(a) ? 16 : gemm_taps(a->mode);
  const long n_out = a->geglu ? a->n / 2 : a->n;
  const bool f32o = a->dtype != TT_F32 && a->out_f32;
  Extents e;
  e.a0 = ((rows - 1) * a->lda0 + a->k0) * es;
  e.a1 = a->k1 ? ((rows - 1) * a->lda1 + a->k1) * es : 16;
  e.w = ((long)(a->n - 1) * a->ldw + taps * (a->k0 + a->k1)) * es;
  e.out = ((long)(a->m - 1) * a->ldo + (a->out_col_hw > 0 ? a->ldo : n_out)) * (f32o ? 4 : (a->out_fp8 ? 1 : es));
  e.res = a->residual ? ((long)(a->m - 1) * a->ld_res + a->n) * es : 0;
  e.blend = a->blend ? ((long)(a->m - 1) * a->ld_blend + a->n) * es : 0;
  long rv_last = a->rowvec && a->rowvec_rows > 0 ? (a->m - 1) / a->rowvec_rows : 0;   // last row-vector index the kernel can form
  if (a->rowvec_mod > 0 && rv_last > a->rowvec_mod - 1) rv_last = a->rowvec_mod - 1;
  e.rowvec = a->rowvec ? (rv_last * a->ld_rowvec + a->n) * 4 : 0;
  return e;
}
constexpr long k2G = 1L << 31;
bool needs_wide(const TtGemmArgs* a) {
  const Extents e = extents_of(a);
  return e.a0 >= k2G || e.a1 >= k2G || e.out >= k2G || e.res >= k2G || e.blend >= k2G;
}
// what the wide variant does not carry (nullptr: nothing)
const char* wide_unserved(const TtGemmArgs* a) {
  if (a->mode == 3) return "mode 3";
  if (a->a1 || a->k1) return "a second source (a1 / k1)";
  if (a->geglu) return "geglu";
  if (a->ln_fold) return "ln_fold";
  if (a->rowvec) return "rowvec";
  if (a->gn_out) return "gn_out";
  if (a->out_fp8) return "out_fp8";
  if (a->out_col_hw) return "out_col_hw";
  if (a->presplit) return "presplit operands";
  return nullptr;
}
// The plan of a wide launch: the narrow plan of the same problem, un-split (the window arithmetic covers `out`, not fp32 slabs), on its
// own tile where that tile's wide variant is built, else on the 128 x 128 tile the planner gives every large problem.
Plan wide_plan(const TtGemmArgs* a) {
  Plan pl = plan_for(a);
  if (pl.splitk > 1) pl = unsplit_plan(a);
  const bool f32 = a->dtype == TT_F32;
  if (!wide_capable(f32, pl.cfg)) pl.cfg = f32 ? 0 : 11;
  return Plan{pl.cfg, 1};
}
// Rows and bytes one tile's window spans per operand, worst case over the tiles (the kernel's origins: gemm_kernel.h, WIDE).
struct Windows { long a_rows, a_bytes, o_rows, o_bytes, e_rows, r_bytes, b_bytes; };
Windows wide_windows(const TtGemmArgs* a, int bm) {
  const long es = a->dtype == TT_F32 ? 4 : 2;
  Windows w;
  const long tile_m = is_up2(a) ? (long)a->nimg * a->hin * a->win : (long)a->m;      // rows of the tile domain
  const long tm = bm < tile_m ? bm : tile_m;
  if (a->mode == 1) {                      // from the start of the first image a tile touches to the end of the last
    const long hwo = is_up2(a) ? (long)a->hin * a->win : (long)a->hout * a->wout;
    long imgs = (tm - 2 + hwo) / hwo + 1;
    if (imgs > a->nimg) imgs = a->nimg;
    w.a_rows = imgs * a->hin * a->win;
  } else if (a->mode == 2) {               // one frame before the tile's first row to one frame behind its last
    w.a_rows = tm + 2L * a->hw < a->m ? tm + 2L * a->hw : a->m;
  } else {
    w.a_rows = tm;
  }
  w.a_bytes = ((w.a_rows - 1) * a->lda0 + a->k0) * es;
  // out: the tile's rows; phase-packed upsampling conv: low-res row gm -> output row 4 gm - 2 x + (py 2 win + px)
  w.o_rows = is_up2(a) ? 4L * tm + 4L * a->win + 2 : tm;
  if (w.o_rows > a->m) w.o_rows = a->m;
  w.o_bytes = (a->dtype != TT_F32 && a->out_f32) ? 0 : ((w.o_rows - 1) * a->ldo + a->n) * es;     // (fp32 out of 16-bit storage: 64-bit pointers)
  w.e_rows = tm;
  w.r_bytes = a->residual ? ((tm - 1) * a->ld_res + a->n) * es : 0;
  w.b_bytes = a->blend ? ((tm - 1) * a->ld_blend + a->n) * es : 0;
  return w;
}
// nullptr if `a` can run wide on tile row count bm; else the reason (names the window and the rows it spans)
const char* wide_window_refusal(const TtGemmArgs* a, int bm) {
  static thread_local char msg[192];
  const Windows w = wide_windows(a, bm);
  const char* which = nullptr; long rows = 0, bytes = 0;
  if (w.a_bytes >= k2G) { which = "a0"; rows = w.a_rows; bytes = w.a_bytes; }
  else if (w.o_bytes >= k2G) { which = "out"; rows = w.o_rows; bytes = w.o_bytes; }
  else if (w.r_bytes >= k2G) { which = "residual"; rows = w.e_rows; bytes = w.r_bytes; }
  else if (w.b_bytes >= k2G) { which = "blend"; rows = w.e_rows; bytes = w.b_bytes; }
  if (!which) return nullptr;
  snprintf(msg, sizeof msg, "the window of one tile on %s spans %ld rows = %ld bytes (2 GiB or more)", which, rows, bytes);
  return msg;
}
// does tt_gemm ask for the wide route for `a` (before looking at what it can serve)?
bool wide_asked(const TtGemmArgs* a) { const int on = knobs().wide; return on == 2 || (on == 1 && needs_wide(a)); }
// Which problems go wide, and on which tile.  (1) A problem whose own plan is the tiled template, un-split (with or without a workspace),
// on a tile whose wide variant is built: the same plan with the windowed kernel -- no answer of tt_gemm_plan / tt_gemm_ws_bytes /
// tt_gemm_stats_rows / tt_gemm_gn_fused changes, and tt_gemm_set_wide(2) takes exactly these.  (2) A problem whose a0 itself spans 2 GiB
// or more: no other kernel can read it, so the wide route comes before every other one, on wide_plan()'s tile (the decoder's 1 x 1
// shortcut at 576x1024 would otherwise be the persistent kernel's).  A problem in which only out / residual / blend reach 2 GiB and that
// the planner gives to the persistent / big-tile / streaming kernels, to a split plan or to another tile keeps that plan and its refusal
// by tt_gemm (those kernels are as they were; tests/golden/gemm_route_census.json pins their answers at such sizes).
bool wide_own_plan(const TtGemmArgs* a, const Route& narrow) {
  return narrow.kind == Kind::TILED && narrow.splitk == 1 && wide_capable(a->dtype == TT_F32, narrow.cfg);
}
bool wide_plan_of(const TtGemmArgs* a, Plan* pl) {
  const Route narrow = wanted_route(a);
  if (wide_own_plan(a, narrow)) { *pl = Plan{narrow.cfg, 1}; return true; }
  if (knobs().wide != 0 && extents_of(a).a0 >= k2G) { *pl = wide_plan(a); return true; }
  return false;
}
// tt_gemm only: the reason a problem that needs the wide route and would get it cannot have it (nullptr: it can, does not need it, or
// stays with the narrow route's own refusal)
const char* wide_refusal(const TtGemmArgs* a) {
  if (knobs().wide == 0 || !needs_wide(a)) return nullptr;
  if (extents_of(a).w >= k2G) return nullptr;                // (W stays refused with the narrow route's message)
  if (const char* what = wide_unserved(a)) { static thread_local char msg[160]; snprintf(msg, sizeof msg, "the wide route (an operand of 2 GiB or more) does not serve %s", what); return msg; }
  Plan pl;
  if (!wide_plan_of(a, &pl)) return nullptr;
  return wide_window_refusal(a, tile_of(a->dtype, pl.cfg).bm);
}
Route resolve(const TtGemmArgs* a) {
  if (wide_asked(a) && !wide_unserved(a) && extents_of(a).w < k2G) {
    Plan pl;
    if (wide_plan_of(a, &pl) && !wide_window_refusal(a, tile_of(a->dtype, pl.cfg).bm)) return Route{Kind::TILED, pl.cfg, 1, 0, true};
  }
  return granted_route(a, wanted_route(a));
}

// the tile of a route as tt_gemm_plan reports it: nst = 0 marks the kernels that are not the tiled template's ring
TileCfg route_tile(const TtGemmArgs* a, const Route& r) {
  switch (r.kind) {
    case Kind::PP: case Kind::PP_TWO_PART: return TileCfg{-1, 256, 256, 64, 0, 2, 4};       // gemm_pp_kernel<dtype, ln, geglu> (all or all but the last rows)
    case Kind::SQ320: return TileCfg{-1, SQ_ROWS, SQ_N, SQ_K, a->residual ? 3 : 5, 1, SQ_WAVES};   // the streaming kernel: 32-row tiles, ring depth 3 (5 without residual)
    case Kind::W320: return TileCfg{-1, 256, 320, 64, 0, 4, 2};                               // gemm_w320_kernel<dtype, mode, ln>: 4 x 2 waves
    case Kind::W320H: case Kind::W320H_SPLIT: return TileCfg{-1, 128, 320, 64, 0, 2, 2};      // gemm_w320h_kernel: 2 x 2 waves
    default: return tile_of(a->dtype, r.cfg);
  }
}

// tt_gemm_stats_rows on a resolved route
int32_t stats_rows_on(const TtGemmArgs* a, const Route& r) {
  if (is_up2(a)) return 0;                                             // bias-only epilogue
  if (a->geglu || a->out_fp8 || a->out_f32 || a->out_col_hw > 0 || a->ln_fold == 2) return 0;
  if (r.kind == Kind::PP || r.kind == Kind::PP_TWO_PART || r.kind == Kind::SQ320 || r.kind == Kind::UNSUPPORTED) return 0;
  // the statistics variants exist for the straight-line epilogues: bias / scale / row vector of >= 32-row groups (or the even / odd
  // form) / residual / a blend with the residual itself -- not for the in-pass operand loads (gemm_kernel.h, `inpass`)
  const int seg = a->stats_seg;
  if (r.splitk != 1) {                                                 // split-K: the reduction kernel takes the sums, on tiles of any height:
    if (seg <= 0) return 0;                                            // the largest divisor of the consumer's segment up to 128 rows
    for (int rows = seg < 128 ? seg : 128; rows > 0; --rows)
      if (seg % rows == 0) return a->m % rows == 0 ? rows : 0;
    return 0;
  }
  const TileCfg t = route_tile(a, r);
  if (a->blend && !(a->blend == a->residual && a->ld_blend == a->ld_res)) return 0;
  if (a->rowvec && a->rowvec_rows < 32 && !(a->rowvec_rows == 1 && a->rowvec_mod == 2)) return 0;
  if (t.bm > 128 && t.bn != 320 && a->residual) return 0;             // 256-row tiles of the tiled template read the residual in-pass
  if (a->dtype == TT_F32 && knobs().f32_split && a->residual) return 0;      // ... and so do the split-fp16 product variants on every tile shape
  if (t.bn == 320 || t.nst == 0) {                                     // the big-tile kernels: whole tiles; the 128-row one also the 64 rows of a wave row
    if (a->m % t.bm) return 0;
    return (t.bm == 128 && seg > 0 && seg % 128 && seg % 64 == 0) ? 64 : t.bm;
  }
  // the tiled template: whole tiles (BM rows) if they divide the segment (or no hint), else the rows of one wave row (BM / WGM: 32 or 64)
  const int wave_rows = t.bm / t.wgm;
  const int rows = (seg <= 0 || seg % t.bm == 0) ? t.bm : (seg % wave_rows == 0 ? wave_rows : t.bm);
  return a->m % rows == 0 ? rows : 0;
}
// tt_gemm_gn_fused on a resolved route
int32_t gn_fused_on(const TtGemmArgs* a, const Route& r) {
  if (is_up2(a) || r.wide) return 0;
  if (a->dtype == TT_F32 || a->geglu || a->out_fp8 || a->out_f32 || a->out_col_hw > 0 || a->stats_out) return 0;
  const int seg = a->stats_seg;
  if (seg <= 0 || a->m % seg || (a->n & 127)) return 0;               // 32 groups of a whole number of column quads
  if (r.kind != Kind::W320H_SPLIT && r.kind != Kind::TILED) return 0;
  if (r.splitk <= 1) return 0;                                         // only where a reduction pass runs anyway
  return splitk_gn_rows(seg, a->n, nullptr) > 0 ? 1 : 0;
}
}  // namespace

int tt_internal_f32_split() { return knobs().f32_split; }
extern "C" int32_t tt_gemm_get_f32_split(void) { return knobs().f32_split; }

extern "C" int tt_gemm_set_tile_override(int32_t cfg) {
  if (cfg < -1 || cfg >= kNumCfgs) TT_FAIL(TT_EINVAL, "tt_gemm_set_tile_override: cfg %d (valid -1..%d)", cfg, kNumCfgs - 1);
  knobs().forced_cfg = cfg;
  return TT_OK;
}
extern "C" int tt_gemm_set_streaming_square(int32_t on) {
  knobs().sq320 = on == 2 ? 2 : (on ? 1 : 0);          // 2: by size (the default)
  return TT_OK;
}
extern "C" int tt_gemm_set_f32_split(int32_t on) { knobs().f32_split = on ? 1 : 0; return TT_OK; }
extern "C" int tt_gemm_set_big_tile(int32_t on) { knobs().w320 = big_tile_bits(on); return TT_OK; }
extern "C" int tt_gemm_set_wide(int32_t on) {
  if (on < 0 || on > 2) TT_FAIL(TT_EINVAL, "tt_gemm_set_wide: %d (0 never, 1 when an operand needs it, 2 whenever it can serve)", on);
  knobs().wide = on;
  return TT_OK;
}
extern "C" int32_t tt_gemm_is_wide(const TtGemmArgs* a) {
  if (!a || a->m <= 0 || a->n <= 0) return 0;
  return resolve(a).wide ? 1 : 0;
}

namespace {
// what the two host-only queries below refuse, and the route of everything else
int queried_route(const char* who, const TtGemmArgs* a, const void* result, Route* r) {
  if (!a || !result || a->m <= 0 || a->n <= 0) TT_FAIL(TT_EINVAL, "%s: bad arguments", who);
  if (is_up2(a)) if (const char* why = up2_refusal(a)) TT_FAIL(TT_EINVAL, "%s: upsample = 2 needs %s", who, why);
  *r = resolve(a);
  if (r->kind == Kind::UNSUPPORTED)
    TT_FAIL(TT_EUNSUPPORTED, "%s: forced tile configuration %d has no mode-3 variant (mode 3 is built for 1, 2, 11, 16)", who, r->cfg);
  return TT_OK;
}
}  // namespace

extern "C" int tt_gemm_plan(const TtGemmArgs* a, int32_t cfg[7]) {
  Route r;
  if (const int rc = queried_route("tt_gemm_plan", a, cfg, &r)) return rc;
  const TileCfg t = route_tile(a, r);              // (stages = 0: not the tiled template)
  cfg[0] = t.bm; cfg[1] = t.bn; cfg[2] = t.bk; cfg[3] = t.nst; cfg[4] = t.wgm; cfg[5] = t.wgn; cfg[6] = r.splitk;
  return TT_OK;
}

// The instance of the route's kernel: each family's selector (gemm_params.h, gemm_tiles.h) is asked what its launcher asks it, with the fields
// fill_params copies into GemmP unchanged.  A two-part problem: the head's kernel; a split plan: the main kernel (not the reduction pass).
extern "C" int tt_gemm_kernel(const TtGemmArgs* a, char* name, int32_t cap) {
  Route r;
  if (const int rc = queried_route("tt_gemm_kernel", a, name, &r)) return rc;
  const char* who = "tt_gemm_kernel", *tag = tt_tag_name(a->dtype);
  switch (r.kind) {
    case Kind::PP: case Kind::PP_TWO_PART: {
      const PpInst i = pp_inst(a->ln_fold, a->geglu);
      return tt_put_name(who, name, cap, "gemm_pp_kernel<%s, %d, %d>", tag, i.lnrows, i.geglu);
    }
    case Kind::SQ320: {
      const Sq320Inst i = sq320_inst(a->residual, a->rowvec);
      return tt_put_name(who, name, cap, "sq320_kernel<%s, %s, %s>", tag, i.has_res ? "true" : "false", i.has_rv ? "true" : "false");
    }
    case Kind::W320: case Kind::W320H: case Kind::W320H_SPLIT: {
      const W320Inst i = w320_inst(a->mode, a->ln_fold);
      return tt_put_name(who, name, cap, "gemm_w320%s_kernel<%s, %d, %d>", r.kind == Kind::W320 ? "" : "h", tag, i.mode, i.lnrows);
    }
    default: {
      const TileCfg t = tile_of(a->dtype, r.cfg);
      const int kmode = tile_kmode(a->mode, a->ln_fold, a->presplit, f32_split_of(a), r.wide, t.ln, t.m3);
      return tt_put_name(who, name, cap, "gemm_kernel<%s, %d, %d, %d, %d, %d, %d, %d>", tag, t.bm, t.bn, t.bk, t.nst, t.wgm, t.wgn, kmode);
    }
  }
}

// rows per statistics tile of the route tt_gemm takes (0: no statistics epilogue on it); see include/ttvdm.h
extern "C" int32_t tt_gemm_stats_rows(const TtGemmArgs* a) {
  if (!a || a->m <= 0 || a->n <= 0) return 0;
  return stats_rows_on(a, resolve(a));
}

// GroupNorm inside the split-K reduction (TtGemmArgs.gn_out): see include/ttvdm.h
extern "C" int32_t tt_gemm_gn_fused(const TtGemmArgs* a) {
  if (!a || a->m <= 0 || a->n <= 0) return 0;
  return gn_fused_on(a, resolve(a));
}

// the slabs of the wanted route (a two-part launch: of its tail, the only part that may split)
extern "C" size_t tt_gemm_ws_bytes(const TtGemmArgs* a) {
  if (!a || a->m <= 0 || a->n <= 0) return 0;
  if (resolve(a).wide) return 0;                        // never split along K
  const Route r = wanted_route(a);
  if (r.kind == Kind::PP_TWO_PART) { TtGemmArgs head, tail; pp_split(a, r.head_rows, &head, &tail); return tt_gemm_ws_bytes(&tail); }
  return (r.kind == Kind::W320H_SPLIT || r.kind == Kind::TILED) && r.splitk > 1 ? slab_bytes(a, r.splitk) : 0;
}

namespace {
// what tt_gemm checks of a problem after its route is known, and the launch parameters of that route
int fill_params(const TtGemmArgs* a, const Route& r, GemmP& p) {
  if (a->geglu && ((a->n & 15) || a->residual || a->blend || a->rowvec || a->out_f32 || a->out_col_hw))
    TT_FAIL(TT_EINVAL, "tt_gemm: geglu needs n %% 16 == 0 and no other epilogue terms");
  if (a->rowvec && a->rowvec_rows <= 0) TT_FAIL(TT_EINVAL, "tt_gemm: rowvec_rows");
  if (a->gn_out) {
    if (!a->gn_gamma || !a->gn_beta || (a->ld_gn & 3) || ((size_t)a->gn_out & 7)) TT_FAIL(TT_EINVAL, "tt_gemm: gn_out needs gn_gamma, gn_beta, ld_gn %% 4 == 0 and an 8-byte aligned pointer");
    if (!gn_fused_on(a, r)) TT_FAIL(TT_EUNSUPPORTED, "tt_gemm: gn_out on a problem without a split-K reduction pass (tt_gemm_gn_fused(args) == 0)");
  }
  if (a->stats_out && stats_rows_on(a, r) == 0)
    TT_FAIL(TT_EUNSUPPORTED, "tt_gemm: stats_out on a route without a statistics epilogue (tt_gemm_stats_rows(args) == 0)");
  if (a->rowvec_mod < 0 || (a->rowvec_mod > 0 && !a->rowvec)) TT_FAIL(TT_EINVAL, "tt_gemm: rowvec_mod %d (>= 0, needs rowvec)", a->rowvec_mod);
  if (a->ln_fold < 0 || a->ln_fold > 2) TT_FAIL(TT_EINVAL, "tt_gemm: ln_fold %d (0 none, 1 rows of A, 2 rows of W)", a->ln_fold);
  if (a->ln_fold && (a->mode != 0 || a->k1 != 0 || !(a->ln_eps > 0.f)))
    TT_FAIL(TT_EINVAL, "tt_gemm: ln_fold needs mode 0, one source spanning the whole LayerNorm row (k0 = C) and ln_eps > 0");
  if (a->ln_fold == 2 && a->geglu) TT_FAIL(TT_EINVAL, "tt_gemm: ln_fold 2 (columns) cannot be combined with geglu");
  if (a->out_fp8 && (a->dtype == TT_F32 || a->mode != 0 || a->geglu || a->residual || a->blend || a->rowvec || a->out_f32 || (a->ldo & 3)))
    TT_FAIL(TT_EINVAL, "tt_gemm: out_fp8 is for plain 16-bit linears (no geglu / residual / blend / rowvec / fp32 out), ldo %% 4 == 0");
  p.a0 = (const char*)a->a0; p.a1 = (const char*)a->a1; p.k0 = a->k0; p.k1 = a->k1;
  p.lda0 = a->lda0; p.lda1 = a->lda1; p.w = (const char*)a->w; p.ldw = a->ldw;
  p.m = a->m; p.n = a->n; p.mode = a->mode;
  p.nimg = a->nimg; p.hin = a->hin; p.win = a->win; p.hout = a->hout; p.wout = a->wout;
  p.stride = a->stride; p.upsample = a->upsample; p.frames = a->frames; p.hw = a->hw;
  p.bias = a->bias; p.acc_scale = a->acc_scale;
  p.rowvec = a->rowvec; p.rowvec_rows = a->rowvec_rows; p.ld_rowvec = a->ld_rowvec; p.rowvec_mod = a->rowvec ? a->rowvec_mod : 0;
  p.geglu = a->geglu; p.residual = (const char*)a->residual; p.ld_res = a->ld_res;
  p.blend = (const char*)a->blend; p.ld_blend = a->ld_blend; p.alpha = a->alpha;
  const int es = a->dtype == TT_F32 ? 4 : 2;         // bytes per stored element
  p.out = (char*)a->out; p.ldo = a->ldo; p.out_f32 = a->dtype == TT_F32 ? 0 : a->out_f32;   // TT_F32 stores fp32 anyway
  p.out_col_hw = a->out_col_hw; p.out_col_hwp = a->out_col_hwp;
  p.ln_fold = a->ln_fold; p.ln_eps = a->ln_eps; p.out_fp8 = a->out_fp8; p.stats = a->stats_out; p.stat_rows = a->gn_out ? a->stats_seg : (a->stats_out ? stats_rows_on(a, r) : 0);
  p.f32_split = f32_split_of(a);
  p.presplit = a->presplit;
  if (a->presplit) {
    if ((a->presplit & ~3) || a->dtype != TT_F32 || !p.f32_split)
      TT_FAIL(TT_EINVAL, "tt_gemm: presplit operands need TT_F32 with tt_gemm_set_f32_split(1)");
    if (((a->presplit & 1) && a->ln_fold == 1) || ((a->presplit & 2) && a->ln_fold == 2))
      TT_FAIL(TT_EINVAL, "tt_gemm: the LayerNorm statistics cannot be taken from a pre-split operand");
    if ((a->presplit & 1) && a->mode != 0) TT_FAIL(TT_EINVAL, "tt_gemm: a pre-split A operand is a Linear operand (mode 0)");
  }
  p.gn_out = (char*)a->gn_out; p.ld_gn = a->ld_gn; p.gn_gamma = a->gn_gamma; p.gn_beta = a->gn_beta; p.gn_eps = a->gn_eps; p.gn_silu = a->gn_silu;
  if (p.mode == 1 || p.mode == 3) {
    if (p.nimg <= 0 || p.hin <= 0 || p.win <= 0 || p.hout <= 0 || p.wout <= 0 || p.stride < 1)
      TT_FAIL(TT_EINVAL, "tt_gemm: conv geometry");
    if ((long)p.nimg * p.hout * p.wout != p.m) TT_FAIL(TT_EINVAL, "tt_gemm: m != nimg*hout*wout");
  }
  if (p.mode == 2) {
    if (p.frames <= 0 || p.hw <= 0 || p.m % ((long)p.frames * p.hw)) TT_FAIL(TT_EINVAL, "tt_gemm: tconv geometry");
  }
  p.taps = is_up2(a) ? 16 : gemm_taps(p.mode);            // (upsample = 2: 4 phases x 4 taps of the phase-packed weight)
  {
    const long rows = p.mode == 1 || p.mode == 3 ? (long)p.nimg * p.hin * p.win : (long)p.m;
    long a0b = ((rows - 1) * p.lda0 + p.k0) * es;
    const long a1b = p.k1 ? ((rows - 1) * p.lda1 + p.k1) * es : 16;
    const long wb = ((long)(p.n - 1) * p.ldw + (long)p.taps * (p.k0 + p.k1)) * es;
    if (r.wide && a0b >= (1L << 31)) a0b = (1L << 31) - 1;           // (the wide variant windows a0 itself: the field is not read)
    if (a0b >= (1L << 31) || a1b >= (1L << 31) || wb >= (1L << 31))
      TT_FAIL(TT_EUNSUPPORTED, "tt_gemm: operand larger than 2 GiB (32-bit buffer offsets)");
    p.a0_bytes = (unsigned)a0b; p.a1_bytes = (unsigned)a1b; p.w_bytes = (unsigned)wb;
    // epilogue operands (bounds-checked descriptors; 0 bytes = absent -> loads return 0)
    const long n_out = p.geglu ? p.n / 2 : p.n;
    long outb = ((long)(p.m - 1) * p.ldo + (p.out_col_hw > 0 ? p.ldo : n_out)) * (p.out_f32 ? 4 : (p.out_fp8 ? 1 : es));
    long resb = p.residual ? ((long)(p.m - 1) * p.ld_res + p.n) * es : 0;
    long blb = p.blend ? ((long)(p.m - 1) * p.ld_blend + p.n) * es : 0;
    if (r.wide) {                                                     // (windowed by the kernel / reached through 64-bit pointers: not read)
      const long cap = (1L << 31) - 1;
      if (outb > cap) outb = cap;
      if (resb > cap) resb = cap;
      if (blb > cap) blb = cap;
    }
    long rv_last = p.rowvec ? (p.m - 1) / p.rowvec_rows : 0;             // last row-vector index the kernel can form
    if (p.rowvec_mod > 0 && rv_last > p.rowvec_mod - 1) rv_last = p.rowvec_mod - 1;
    const long rvb = p.rowvec ? (rv_last * p.ld_rowvec + p.n) * 4 : 0;
    if (outb >= (1L << 31) || resb >= (1L << 31) || blb >= (1L << 31) || rvb >= (1L << 31))
      TT_FAIL(TT_EUNSUPPORTED, "tt_gemm: epilogue operand larger than 2 GiB (32-bit buffer offsets)");
    p.out_bytes = (unsigned)outb; p.res_bytes = (unsigned)resb; p.blend_bytes = (unsigned)blb;
    p.bias_bytes = p.bias ? (unsigned)p.n * 4u : 0u; p.rowvec_bytes = (unsigned)rvb;
  }
  // the tile order's group height: launch_cfg / the persistent kernel pick it unless TT_GEMM_GROUP_M says otherwise; the workspace only where K is split
  p.splitk = r.splitk; p.group_m = 1;
  p.group_m_override = r.kind == Kind::PP || r.kind == Kind::TILED ? knobs().group_m : 0;
  p.ws = r.splitk > 1 ? (float*)a->ws : nullptr;
  p.ws_bytes = r.splitk > 1 ? (unsigned)slab_bytes(a, r.splitk) : 0u;
  p.slices = r.splitk; p.phases = 0;
  if (is_up2(a)) {                                   // the tile domain is the low-res image; the extents above are those of the real operands
    if (r.kind != Kind::TILED || r.splitk != 1) TT_FAIL(TT_EUNSUPPORTED, "tt_gemm: upsample = 2 runs on the tiled template, unsplit");
    p.phases = 1; p.upsample = 0;
    p.m = p.nimg * p.hin * p.win; p.hout = p.hin; p.wout = p.win;
  }
  return TT_OK;
}
}  // namespace

extern "C" int tt_gemm(const TtGemmArgs* a, tt_stream_t stream) {
  if (!a || !a->a0 || !a->w || !a->out) TT_FAIL(TT_EINVAL, "tt_gemm: null operand");
  if (a->m <= 0 || a->n <= 0 || a->k0 <= 0) TT_FAIL(TT_EINVAL, "tt_gemm: empty problem m=%d n=%d k0=%d", a->m, a->n, a->k0);
  if (a->dtype != TT_BF16 && a->dtype != TT_F16 && a->dtype != TT_F32) TT_FAIL(TT_EINVAL, "tt_gemm: bad dtype");
  if ((a->k0 & 7) || (a->k1 & 7) || (a->n & 3)) TT_FAIL(TT_EINVAL, "tt_gemm: k0/k1 must be multiples of 8 and n of 4");
  if ((a->lda0 & 7) || (a->k1 && (a->lda1 & 7)) || (a->ldw & 7)) TT_FAIL(TT_EINVAL, "tt_gemm: row strides must be multiples of 8 elements");
  if (a->k1 && !a->a1) TT_FAIL(TT_EINVAL, "tt_gemm: k1 > 0 without a1");
  if (a->mode < 0 || a->mode > 3) TT_FAIL(TT_EINVAL, "tt_gemm: bad mode %d", a->mode);
  if (a->mode == 3 && a->upsample) TT_FAIL(TT_EINVAL, "tt_gemm: mode 3 (bottom / right zero padding) has no fused upsample");
  if (is_up2(a)) if (const char* why = up2_refusal(a)) TT_FAIL(TT_EINVAL, "tt_gemm: upsample = 2 needs %s", why);
  if (const char* why = wide_refusal(a)) TT_FAIL(TT_EUNSUPPORTED, "tt_gemm: %s", why);
  const Route r = resolve(a);
  if (r.kind == Kind::PP_TWO_PART) {                        // whole tile rows -> persistent kernel, the rest -> whatever serves it; each half is checked in full below
    TtGemmArgs head, tail;
    pp_split(a, r.head_rows, &head, &tail);
    const int rc = tt_gemm(&head, stream);
    return rc != TT_OK ? rc : tt_gemm(&tail, stream);
  }
  GemmP p;
  if (const int rc = fill_params(a, r, p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool bf16 = a->dtype == TT_BF16;
  switch (r.kind) {
    case Kind::PP: if (bf16) launch_pp_bf16(p, st); else launch_pp_f16(p, st); break;
    case Kind::SQ320: if (bf16) launch_sq320_bf16(p, st); else launch_sq320_f16(p, st); break;
    case Kind::W320: launch_w320(p, st, 256, bf16); break;
    case Kind::W320H: case Kind::W320H_SPLIT: launch_w320(p, st, 128, bf16); break;
    case Kind::TILED:
      if (r.wide) {
        if (bf16) launch_wide_bf16(p, r.cfg, st);
        else if (a->dtype == TT_F16) launch_wide_f16(p, r.cfg, st);
        else launch_wide_f32(p, r.cfg, st);
      } else if (bf16) launch_bf16(p, r.cfg, st);
      else if (a->dtype == TT_F16) launch_f16(p, r.cfg, st);
      else launch_f32(p, r.cfg, st);
      break;
    default:
      TT_FAIL(TT_EUNSUPPORTED, "tt_gemm: forced tile configuration %d has no mode-3 variant (mode 3 is built for 1, 2, 11, 16)", r.cfg);
  }
  TT_CHECK_LAUNCH("tt_gemm");
  return TT_OK;
}
