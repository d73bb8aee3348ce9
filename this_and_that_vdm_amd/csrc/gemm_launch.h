// gemm_launch.h -- the launchers of the tiled template: per tile shape the derived launch parameters (tile_params), the KMODE_ switch
// (launch_cfg) and the launch itself (launch_mode), and launch<Tag>() over the tile table.  Included by the instantiation units
// gemm_inst_*.hip, which compile in parallel.
#pragma once
#include "gemm_kernel.h"
#include "gemm_splitk.h"
#include "gemm_tiles.h"

namespace ttg {

// ---- configurations: {BM, BN, BK, NST, WGM, WGN}
template <typename Tag, int BM, int BN, int BK, int NST, int WGM, int WGN, int MODE>
void launch_mode(const GemmP& p, hipStream_t st) {
  constexpr int NT_ = 64 * WGM * WGN, CPR_ = BK / Elem<Tag>::EPC;
  constexpr size_t lds = (size_t)NST * (((BM * CPR_ + NT_ - 1) / NT_) + ((BN * CPR_ + NT_ - 1) / NT_)) * NT_ * 16
                         + ((MODE & 7) == 4 ? WGM * WGN * 1024 : 0);    // + the per-wave column-scale arrays  (MODE + 8: split-fp16 products, TT_F32)
  static_assert(lds + (size_t)WGM * WGN * 2 * (BN / WGN) * sizeof(float) <= 160 * 1024, "LDS ring (+ the statistics staging rows) exceeds 160 KiB");
  static_assert((MODE & 7) != 4 || BN / WGN <= 256, "column-scale array: 1 KiB per wave");
  constexpr size_t stat_lds = (size_t)WGM * WGN * 2 * (BN / WGN) * sizeof(float);        // per wave: sum and sum-of-squares rows of its columns
  static unsigned long long attr_done = 0;     // per kernel instance, one bit per device (see tt_lds_opt_in)
  tt_lds_opt_in((const void*)gemm_kernel<Tag, BM, BN, BK, NST, WGM, WGN, MODE>, (int)(lds + stat_lds), &attr_done);
  hipLaunchKernelGGL((gemm_kernel<Tag, BM, BN, BK, NST, WGM, WGN, MODE>), dim3(p.tiles_m * p.tiles_n * p.slices),
                     dim3(64 * WGM * WGN), (p.stats && p.splitk == 1) ? lds + stat_lds : lds, st, p);
  if constexpr ((MODE & 64) == 0) {            // (the wide variant never splits along K)
    if (p.splitk > 1) launch_splitk_epilogue<Tag>(p, st);
  }
}

// multiply-shift pairs of every launch-uniform divisor the kernel meets (tile order, K split, conv / frame geometry, row groups)
static inline void fill_fastdivs(GemmP& p) {
  p.fd_splitk = make_fastdiv(p.slices);
  p.fd_per_group = make_fastdiv((long)p.group_m * p.tiles_n);
  p.fd_group_m = make_fastdiv(p.group_m);
  p.fd_last_rows = make_fastdiv(p.tiles_m % p.group_m ? p.tiles_m % p.group_m : p.group_m);
  p.fd_per_tap = make_fastdiv(p.nk0 + p.nk1);
  p.fd_hwo = make_fastdiv((long)p.hout * p.wout);
  p.fd_wout = make_fastdiv(p.wout);
  p.fd_hw = make_fastdiv(p.hw);
  p.fd_frames = make_fastdiv(p.frames);
  p.fd_rv_rows = make_fastdiv(p.rowvec ? p.rowvec_rows : 1);
  p.fd_rv_mod = make_fastdiv(p.rowvec_mod > 0 ? p.rowvec_mod : 1);
}

// what every launch on a tile shape derives from the problem first: tile counts, the launch order's group height, K steps, divisors
template <typename Tag, int BM, int BN, int BK, int NST, int WGM, int WGN>
void tile_params(GemmP& p) {
  p.tiles_m = ceil_div(p.m, BM);
  p.tiles_n = ceil_div(p.n, BN);
  {
    // group height that balances the A rows and W columns of one XCD's resident window (32 CUs x blocks per CU)
    constexpr int NT_ = 64 * WGM * WGN, CPR_ = BK / Elem<Tag>::EPC;
    constexpr long lds_ = (long)NST * (((BM * CPR_ + NT_ - 1) / NT_) + ((BN * CPR_ + NT_ - 1) / NT_)) * NT_ * 16;
    const int window = 32 * (lds_ * 2 <= 160 * 1024 ? 2 : 1);
    int gm = p.group_m_override;
    if (gm <= 0) {
      gm = 1;
      // few columns: a row's tiles are all resident together anyway and row-major keeps neighbouring rows (conv halos) adjacent
      if (p.tiles_n > 8)
        while (gm * 2 * BM * gm * 2 <= (long)window * BN && gm * 2 <= p.tiles_m) gm *= 2;    // gm^2 * BM <= window * BN
    }
    p.group_m = gm < 1 ? 1 : (gm > p.tiles_m ? p.tiles_m : gm);
  }
  p.nk0 = ceil_div(p.k0, BK); p.nk1 = p.k1 ? ceil_div(p.k1, BK) : 0;
  p.kt_total = p.taps * (p.nk0 + p.nk1);
  p.slices = p.phases ? 4 : p.splitk;
  fill_fastdivs(p);
}

template <typename Tag, int BM, int BN, int BK, int NST, int WGM, int WGN, bool LNOK = false, bool M3OK = false, bool WIDE = false>
void launch_cfg(GemmP& p, hipStream_t st) {
  constexpr bool F32 = std::is_same<Tag, f32_tag>::value;
  tile_params<Tag, BM, BN, BK, NST, WGM, WGN>(p);
  switch (tile_kmode(p.mode, p.ln_fold, p.presplit, p.f32_split, WIDE, LNOK, M3OK)) {
#define TT_KMODE_CASE(km, built) case km: if constexpr (built) launch_mode<Tag, BM, BN, BK, NST, WGM, WGN, km>(p, st); break;
    TT_GEMM_KMODES(TT_KMODE_CASE)
#undef TT_KMODE_CASE
  }
}

#define TT_WIDE_CASE(i, bm, bn, bk, nst, wgm, wgn) case i: launch_cfg<Tag, bm, bn, bk, nst, wgm, wgn, false, false, true>(p, st); break;

// cfg = index into the table of Tag's storage type; an index outside it launches nothing (the planner hands out none)
#define TT_TILE_CASE(i, bm, bn, bk, nst, wgm, wgn, ln, m3) case i: launch_cfg<Tag, bm, bn, bk, nst, wgm, wgn, ln, m3>(p, st); break;
template <typename Tag>
void launch(GemmP& p, int cfg, hipStream_t st) {
  switch (cfg) { TT_GEMM_TILES(TT_TILE_CASE) }
}
template <> void launch<f32_tag>(GemmP& p, int cfg, hipStream_t st);      // TT_GEMM_TILES_F32: defined in its own unit, gemm_inst_f32.hip

}  // namespace ttg
