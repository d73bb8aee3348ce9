// gemm_kernel.h -- the tiled template of tt_gemm: gemm_kernel and the pieces it is built from (namespace ttg).  Launched through
// gemm_launch.h (the per-dtype instantiation units gemm_inst_*.hip); the tile shapes and KMODE_ values are listed in gemm_tiles.h.
#pragma once
#include "gemm_params.h"

namespace ttg {

// The pass-loop epilogue arithmetic of one element with its contractions written out operation by operation: add, fma, [add,] mul, fma
// -- what hipcc makes of `(t + bias) * scale + rowvec`, `+ residual` and `alpha * blend + (1 - alpha) * w` in every narrow instance
// (disassembly).  The WIDE instances call it: in their slightly different surroundings hipcc fused some elements of the loose
// expression and not others, which costs the last bit of an fp32 result; written out, their bits are the narrow ones' by construction.
// The narrow instances keep the loose expression (adopting this form there is a change of source form whose bits are
// pinned by tests/test_gemm_tiled_bits_gpu.py but whose instruction counts have not been compared).  INPASS: the row vector (zero
// where absent) rides on the scale's fma and the residual is added after it; otherwise the residual rides on the fma.
// BLEND_MUL_FIRST: the instances that read the residual in-pass (the split16 ones among the wide tiles) form alpha * blend first and
// fuse (1 - alpha) * w onto it; the ones that preload it fuse alpha * blend onto (1 - alpha) * w.
template <bool INPASS, bool BLEND_MUL_FIRST>
__device__ __forceinline__ float epi_elem(float t, float bias, float scale, float rv, float res, float bl, float alpha, float one_m_alpha) {
#pragma clang fp contract(off)
  const float u = t + bias;
  float w;
  if constexpr (INPASS) { w = __builtin_fmaf(scale, u, rv); w = w + res; }
  else w = __builtin_fmaf(scale, u, res);
  if constexpr (BLEND_MUL_FIRST) { const float x = alpha * bl; return __builtin_fmaf(one_m_alpha, w, x); }
  const float x = one_m_alpha * w;
  return __builtin_fmaf(alpha, bl, x);
}

// wait until at most `tiles` of the G-load groups issued last are still in flight (tiles <= 3)
template <int G> __device__ __forceinline__ void wait_tiles(int tiles) {
  static_assert(3 * G <= 63, "vmcnt field is 6 bits");
  if (tiles <= 0) wait_vmcnt<0>();
  else if (tiles == 1) wait_vmcnt<G>();
  else if (tiles == 2) wait_vmcnt<2 * G>();
  else wait_vmcnt<3 * G>();
}

// LDS bytes of one workgroup and the waves per SIMD the register allocator must leave room for: as many workgroups per
// CU as the 160 KiB of LDS admit (at most 2 -- more did not pay), i.e. blocks * waves / 4 SIMDs.  Declaring it keeps e.g.
// the 256x128 8-wave kernel at <= 128 VGPRs (130 would halve its occupancy).
constexpr int gemm_lds_bytes(int BM, int BN, int CPR, int NST, int NT) {      // CPR = 16-byte chunks per tile row
  return NST * (((BM * CPR + NT - 1) / NT) + ((BN * CPR + NT - 1) / NT)) * NT * 16;
}
constexpr int gemm_min_waves(int BM, int BN, int CPR, int NST, int NT) {
  const int blocks = (160 * 1024) / gemm_lds_bytes(BM, BN, CPR, NST, NT) >= 2 ? 2 : 1;
  const int w = blocks * (NT / 64) / 4;
  return w < 1 ? 1 : w;
}

// ---- the pieces gemm_kernel is built from.

// WIDE: descriptor on the window of operand `base` (row stride ld elements of ES bytes, `total` bytes in all) from row `row0` on
template <int ES>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t window_rsrc(const char* base, long row0, long ld, long total) {
  const long off = row0 * ld * ES;
  long rest = total - off;
  if (rest > 0x7fffffffL) rest = 0x7fffffffL;
  return make_rsrc(base + off, (!base || rest < 0) ? 0u : (unsigned)rest);
}

// the epilogue strip of one wave: 32 rows x 256 bytes, 16-byte quads XOR-swizzled by the row (no padding: 8 KiB per wave)
__device__ __forceinline__ int strip_off(int row, int quad, int nq) { return row * 256 + ((quad ^ (row & (nq - 1))) << 4); }

// ---- split16: conversion of one fragment set (4 fp32 values) into its fp16 (h, l) halves.  An operand the caller pre-split
// (GemmP.presplit: packed weights) arrives as (h01, h23, l01, l23) already: no VALU at all.
// split_f32x4_mix: 10 VALU -- two packed scalings, two packed conversions for h, and one v_fma_mixlo / mixhi_f16 per value for
// l = fp16(8 x - 2048 h): the instruction widens its fp16 operand, fuses and rounds once.
__device__ __forceinline__ void split_f32x4_mix(const raw_u32x4_t& f, bool pre, uint2& h, uint2& l) {
  if (pre) { h = make_uint2(f.x, f.y); l = make_uint2(f.z, f.w); return; }
  const float kM2048 = -2048.0f;
  const f32x2_t v01 = (f32x2_t){__uint_as_float(f.x), __uint_as_float(f.y)}, v23 = (f32x2_t){__uint_as_float(f.z), __uint_as_float(f.w)};
  const f16x2_t h01 = __builtin_convertvector(v01 * 0.00390625f, f16x2_t), h23 = __builtin_convertvector(v23 * 0.00390625f, f16x2_t);   // fp16(x 2^-8)
  h = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
  const f32x2_t e01 = v01 * 8.0f, e23 = v23 * 8.0f;                      // (x - 2^8 h) 2^3 = 8 x - 2048 h, exact in fp32
  unsigned l01, l23;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(l01) : "v"(h.x), "v"(kM2048), "v"(e01.x));
  asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l01) : "v"(h.x), "v"(kM2048), "v"(e01.y));
  asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(l23) : "v"(h.y), "v"(kM2048), "v"(e23.x));
  asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l23) : "v"(h.y), "v"(kM2048), "v"(e23.y));
  l = make_uint2(l01, l23);
}
// split_f32x4: the same conversion in plain C (14 VALU, no inline asm: every instruction is visible to the scheduler, which is asked to
// alternate them with the pending MFMAs); used where the conversion is hidden under MFMAs anyway
__device__ __forceinline__ void split_f32x4(const raw_u32x4_t& f, bool pre, uint2& h, uint2& l) {
  if (pre) { h = make_uint2(f.x, f.y); l = make_uint2(f.z, f.w); return; }
  const f32x2_t v01 = (f32x2_t){__uint_as_float(f.x), __uint_as_float(f.y)}, v23 = (f32x2_t){__uint_as_float(f.z), __uint_as_float(f.w)};
  const f16x2_t h01 = __builtin_convertvector(v01 * 0.00390625f, f16x2_t), h23 = __builtin_convertvector(v23 * 0.00390625f, f16x2_t);
  h = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
  const f32x2_t r01 = v01 * 8.0f - __builtin_convertvector(h01, f32x2_t) * 2048.0f, r23 = v23 * 8.0f - __builtin_convertvector(h23, f32x2_t) * 2048.0f;
  l = make_uint2(__builtin_bit_cast(unsigned, __builtin_convertvector(r01, f16x2_t)), __builtin_bit_cast(unsigned, __builtin_convertvector(r23, f16x2_t)));
}

// ---- the arms of the strip pass epilogue: one struct of compile-time flags per arm (a run-time `if` inside the pass loops breaks the
// straight-line code).
//   FILM   the row vector (time-embedding FiLM term, one vector per rowvec_rows output rows) of the <= 2 row groups a 32-row
//          fragment spans is loaded up front and selected per row;
//   INPASS operands that cannot be held in registers are loaded inside the pass batches: a blend tensor distinct from the
//          residual, a row vector with groups shorter than 32 rows, and -- on the 256-row tiles, whose 128-VGPR budget has no
//          room for the preload, and in the split16 variants -- the residual.  A load issued after a store waits for that store
//          (in-order vmcnt), so each batch loads first and stores last; the planner keeps such epilogues off the 256-row tiles;
//   OUT8   the output is stored as e4m3 bytes;
//   STATS  GemmP.stats: column sums of the stored values beside the passes (colstat_strip);
//   PHASE  GemmP.phases (bias-only epilogue): tile row gm is low-res pixel (img, y, x); slice (py, px) stores output row
//          (img * 2 hin + 2 y + py) * 2 win + 2 x + px -- the other launches do not pay for the row map.
template <bool FILM_, bool INPASS_, bool OUT8_, bool STATS_, bool PHASE_>
struct EpiArm { static constexpr bool FILM = FILM_, INPASS = INPASS_, OUT8 = OUT8_, STATS = STATS_, PHASE = PHASE_; };
// Every arm that is built: X(name, FILM, INPASS, OUT8, STATS, PHASE) -- a line more is a pass loop more in every instance that can
// reach it.  The dispatch in gemm_kernel names its arms from this list and nothing else.
#define TT_GEMM_EPI_ARMS(X) \
  X(Plain,      0, 0, 0, 0, 0)   /* bias / scale / preloaded residual / blend with the residual as its source */ \
  X(PlainStats, 0, 0, 0, 1, 0)   /* ... whose consumer is a GroupNorm (tt_gemm_stats_rows > 0) */ \
  X(Film,       1, 0, 0, 0, 0)   /* + a row vector in groups of >= 32 rows, or the even / odd form (ResBlock time embedding, zero-context bias) */ \
  X(FilmStats,  1, 0, 0, 1, 0)   /* ... with the sums (a ResBlock's first conv feeds the second norm) */ \
  X(InPass,     0, 1, 0, 0, 0)   /* a distinct blend tensor, short row-vector groups, a residual that is not preloaded: never with sums */ \
  X(Out8,       0, 0, 1, 0, 0)   /* Q | K and V^T of the fp8 attention path: Linear, 16-bit storage, no residual */ \
  X(Phase,      0, 0, 0, 0, 1)   /* the four slices of a phase-packed upsampling conv: bias only (tt_gemm refuses the rest) */
namespace epi_arm {
#define TT_EPI_ARM_TYPE(name, film, inpass, out8, stats, phase) using name = EpiArm<film, inpass, out8, stats, phase>;
TT_GEMM_EPI_ARMS(TT_EPI_ARM_TYPE)
#undef TT_EPI_ARM_TYPE
}  // namespace epi_arm

// KMODE: 0 Linear, 1 conv3x3, 2 temporal conv, and two Linear variants with a fused LayerNorm (transformer blocks):
//   3  out = LN(A rows) W^T        4  out = A LN(W rows)^T   (the swapped V^T projection: the tokens are the "W" operand)
//   5  conv3x3 with zero padding on the bottom / right only (tt_gemm mode 3: the VAE encoder's Downsample2D(padding=0) after
//      F.pad(x, (0, 1, 0, 1))): the mode-1 gather with tap (ky, kx) reading pixel (y*stride + ky, x*stride + kx), built only for
//      the tile shapes the planner gives mode-3 problems (M3OK in launch_cfg)
// The caller folds gamma into the weights, centres them over k (rows sum to zero, so the mean of x drops out of x W^T) and
// folds beta into the bias; what remains is the per-token 1/sigma.  Every lane sees ALL K values of "its" operand row pass
// through its registers as MFMA fragments (row l31, chunk parity hi), so sum and sum of squares cost two packed dot
// products per dword next to the MFMAs -- no statistics pass, no extra memory traffic, no normalised copy of the tensor.
// One-pass variance (E[x^2] - E[x]^2, fp32 sums): relative error ~6e-8 * (1 + mean^2 / var), i.e. fine for |row mean| <= ~50 sigma
// (tests/test_ops_gpu.py::test_gemm_fused_layernorm_rows_with_large_row_means); far beyond that use tt_layernorm + a plain GEMM.
template <typename Tag, int BM, int BN, int BK, int NST, int WGM, int WGN, int KMODE_>
__global__ __launch_bounds__(64 * WGM * WGN, gemm_min_waves(BM, BN, BK / Elem<Tag>::EPC, NST, 64 * WGM * WGN))
void gemm_kernel(const GemmP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool SPLIT = (KMODE_ & 8) != 0;            // f32_tag only: KMODE + 8 = the same kernel with split-fp16 products (see `mma`)
  constexpr bool PRE_B = (KMODE_ & 16) != 0, PRE_A = (KMODE_ & 32) != 0;      // ... + 16 / + 32: the W / A operand arrives pre-split (GemmP.presplit)
  // + 64: the WINDOWED ("wide") variant for operands of 2 GiB and more.  The narrow kernel puts one descriptor on each operand's base and
  // gives every lane a 32-bit byte offset into it; here every workgroup rebases the descriptors of a0 / out / residual / blend once per
  // tile in 64-bit scalar arithmetic -- onto the first row the tile can touch -- and the lanes' offsets count from that row.  num_records
  // is the rest of the operand capped below 2^31, so an offset of 0x80000000 still reads zeros / drops the store; tt_gemm refuses a
  // problem in which one tile's window itself reaches 2 GiB.  Same tile, ring, K order and epilogue arithmetic as KMODE_ - 64: the same
  // bits.  Built for modes 0 / 1 / 2 with the bias / scale / residual / blend / fp32-out epilogues and stats_out (tile_kmode).
  constexpr bool WIDE = (KMODE_ & 64) != 0;
  constexpr int KMODE = KMODE_ & 7;
  static_assert(SPLIT || (!PRE_A && !PRE_B), "pre-split operands belong to the split variants");
  static_assert(!SPLIT || std::is_same<Tag, f32_tag>::value, "split products are a TT_F32 mode");
  static_assert(!WIDE || ((KMODE_ & 7) <= 2 && !PRE_A && !PRE_B), "the wide variant: modes 0 / 1 / 2, operands not pre-split");
  constexpr bool PAD_BR = KMODE == 5;                  // mode-3 conv: taps start at the output pixel's own (strided) position
  constexpr int MODE = PAD_BR ? 1 : (KMODE >= 3 ? 0 : KMODE);                   // gather mode
  constexpr int LN = KMODE == 3 || KMODE == 4 ? KMODE - 2 : 0;                  // 0 none, 1 statistics of A rows, 2 of W rows
  TL(0);
  kernarg_touch<sizeof(GemmP)>();
  typedef typename Elem<Tag>::quad_t quad_t;
  constexpr int ES = Elem<Tag>::ES, EPC = Elem<Tag>::EPC;   // bytes per element, elements per 16-byte chunk
  constexpr int NT = 64 * WGM * WGN;                   // threads
  constexpr int CPR = BK / EPC;                        // 16-byte chunks per tile row
  constexpr int WTM = BM / WGM, WTN = BN / WGN, FM = WTM / 32, FN = WTN / 32;
  // 16-byte chunks staged per thread per tile; when the tile does not divide evenly the last pass is padded
  // (rows >= BM/BN of the LDS image are never read; their lanes load the zero page so every wave issues the
  // same number of loads and the counted vmcnt stays valid)
  constexpr int AR = (BM * CPR + NT - 1) / NT, BR = (BN * CPR + NT - 1) / NT;
  constexpr int A_BYTES = AR * NT * 16, B_BYTES = BR * NT * 16, STAGE = A_BYTES + B_BYTES;
  constexpr int G = AR + BR;
  constexpr int RPI = NT / CPR;                        // tile rows covered per staging pass
  static_assert(NT % CPR == 0 && NST >= 2 && NST <= 5 && WTM % 32 == 0 && WTN % 32 == 0, "tile/threads mismatch");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- the tile walk: block id -> (tile_m, tile_n, split) and the K-step range [kt_lo, kt_lo + KT)
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  int split = 0;                                           // slices of one tile sit next to each other
  if (p.slices > 1) { const int t = fdiv(bid, p.fd_splitk); split = bid - t * p.slices; bid = t; }
  // Within an XCD's run the tiles go in groups of `group_m` tile rows, column by column inside a group: the ~64 workgroups
  // that are resident on an XCD at a time then cover group_m rows x 64/group_m columns, i.e. every K slice they fetch is
  // shared by group_m (W) or 64/group_m (A) of them instead of the whole window sharing ONE A row and streaming every W
  // column.  The K loop is bound by the LDS fill (ablation in DESIGN.md section 6: without the loads the same loop runs
  // ~2x faster, without the MFMAs only ~1.2x), and what misses L2 pays the fabric latency.
  int tile_m, tile_n;
  {
    const int gm = p.group_m;
    const int per_group = gm * p.tiles_n;
    const int grp = fdiv(bid, p.fd_per_group);
    const int first = grp * gm;
    const int r = bid - grp * per_group;
    // every group has gm tile rows except a ragged last one (tiles_m % gm rows): two precomputed divisors
    const bool full = first + gm <= p.tiles_m;
    const int rows = full ? gm : p.tiles_m - first;
    tile_n = full ? fdiv(r, p.fd_group_m) : fdiv(r, p.fd_last_rows);
    tile_m = first + (r - tile_n * rows);
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  // K-tile range of this block
  // (kt_total * splitk < 2^31: at most a few thousand K steps, splitk <= 16; the 4 phases of an upsample = 2 conv: 4 of its 16 taps each)
  const int kt_lo = p.slices > 1 ? fdiv(p.kt_total * split, p.fd_splitk) : 0;
  const int KT = p.slices > 1 ? fdiv(p.kt_total * (split + 1), p.fd_splitk) - kt_lo : p.kt_total;

  // ---- staging: buffer_load ... lds through 128-bit resource descriptors.  Every lane owns a 32-bit byte offset per
  // staged 16-byte chunk (computed once per tile, or once per conv tap); the K position is a SCALAR offset.  Lanes that
  // must read zeros (ragged M/N, conv halo, K tail) use an offset beyond num_records: the hardware bounds check returns 0.
  // This keeps the per-K-step instruction count at ~1 per load (the loop is otherwise instruction-issue bound).
  constexpr int INV = (int)0x80000000;
  long a_org = 0;                   // WIDE: first row of a0 the tile can read -- the window's origin
  if constexpr (WIDE) {
    if constexpr (MODE == 0) a_org = m0;
    else if constexpr (MODE == 1) a_org = (long)fdiv(m0, p.fd_hwo) * p.hin * p.win;       // start of the image that holds output row m0
    else {                                                                              // m0 - hw, not before the start of m0's frame group
      const int grp0 = fdiv(fdiv(m0, p.fd_hw), p.fd_frames) * p.frames * p.hw;
      a_org = m0 - p.hw > grp0 ? m0 - p.hw : grp0;
    }
  }
  const long a_rows_all = MODE == 1 ? (long)p.nimg * p.hin * p.win : (long)p.m;
  const __amdgpu_buffer_rsrc_t ra0 = WIDE ? window_rsrc<ES>(p.a0, a_org, p.lda0, ((a_rows_all - 1) * p.lda0 + p.k0) * ES)
                                          : __builtin_amdgcn_make_buffer_rsrc((void*)p.a0, 0, p.a0_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ra1 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.a1 ? p.a1 : p.a0), 0, p.a1_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
  const int crow = tid / CPR, cchunk = tid % CPR;
  int a_chunk[AR];              // source chunk (swizzled) per staged row
  int va0[AR], va1[AR];         // byte offsets into a0 / a1 for the current tap
  int a_img[AR], a_y[AR], a_x[AR];
  bool a_valid[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int r = i * RPI + crow;
    a_chunk[i] = cchunk ^ tile_swz<CPR>(r);
    const int gm = m0 + r;
    a_valid[i] = gm < p.m && r < BM;
    const int g = a_valid[i] ? gm : 0;
    va0[i] = va1[i] = INV;
    a_img[i] = a_y[i] = a_x[i] = 0;
    if constexpr (MODE == 0) {
      if (a_valid[i]) {
        va0[i] = (int)(((long)(g - a_org) * p.lda0 + a_chunk[i] * EPC) * ES);
        va1[i] = (int)(((long)g * p.lda1 + a_chunk[i] * EPC) * ES);
      }
    } else if constexpr (MODE == 1) {
      const int hwo = p.hout * p.wout;
      a_img[i] = fdiv(g, p.fd_hwo);
      const int rem = g - a_img[i] * hwo;
      a_y[i] = fdiv(rem, p.fd_wout);
      a_x[i] = rem - a_y[i] * p.wout;
    } else {
      const int fr = fdiv(g, p.fd_hw);
      a_img[i] = fr - fdiv(fr, p.fd_frames) * p.frames;   // frame index
      a_y[i] = g;                         // row
    }
  }
  int b_chunk[BR], vb[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) {
    const int r = i * RPI + crow;
    b_chunk[i] = cchunk ^ tile_swz<CPR>(r);
    const int gn = n0 + r;
    vb[i] = (gn < p.n && r < BN) ? (int)(((long)gn * p.ldw + b_chunk[i] * EPC) * ES) : INV;
  }

  // K-step iterator state for the NEXT tile to stage (uniform)
  int s_tap, s_src, s_kc;
  {
    const int per_tap = p.nk0 + p.nk1;
    s_tap = kt_lo ? fdiv(kt_lo, p.fd_per_tap) : 0;
    const int rem = kt_lo - s_tap * per_tap;
    s_src = rem >= p.nk0 ? 1 : 0;
    s_kc = rem - (s_src ? p.nk0 : 0);
  }
  bool tap_dirty = true;
  auto stage = [&](int slot) {
    if constexpr (MODE != 0) {
      if (tap_dirty) {                       // new tap: refresh the per-lane row offsets (uniform branch)
        tap_dirty = false;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
          bool ok = a_valid[i];
          long row;
          if constexpr (MODE == 1) {
            constexpr int OFF = PAD_BR ? 0 : 1;          // taps -1..1 (pad 1 all round) or 0..2 (pad on the bottom / right only)
            int dy = s_tap / 3 - OFF, dx = s_tap - (dy + OFF) * 3 - OFF;
            // phase (py, px) of a phase-packed upsampling conv: tap (r, c) = (s_tap & 3) reads low-res pixel (y + r - 1 + py, x + c - 1 + px)
            if (!PAD_BR && p.phases) { dy = ((s_tap >> 1) & 1) - 1 + (split >> 1); dx = (s_tap & 1) - 1 + (split & 1); }
            int iy = a_y[i] * p.stride + dy, ix = a_x[i] * p.stride + dx;
            const bool up = !PAD_BR && p.upsample;     // (tt_gemm refuses upsample with mode 3)
            const int hv = up ? p.hin * 2 : p.hin, wv = up ? p.win * 2 : p.win;
            ok = ok && iy >= 0 && iy < hv && ix >= 0 && ix < wv;
            if (up) { iy >>= 1; ix >>= 1; }
            row = ((long)a_img[i] * p.hin + iy) * p.win + ix;
          } else {
            const int f = a_img[i] + s_tap - 1;
            ok = ok && f >= 0 && f < p.frames;
            row = (long)a_y[i] + (long)(s_tap - 1) * p.hw;
          }
          va0[i] = ok ? (int)(((row - a_org) * p.lda0 + a_chunk[i] * EPC) * ES) : INV;
          va1[i] = ok ? (int)((row * p.lda1 + a_chunk[i] * EPC) * ES) : INV;
        }
      }
    }
    // everything below is wave-uniform except the per-lane offsets; force the scalars into SGPRs so the buffer
    // instructions get their soffset / descriptor without waterfall loops (cdna guide T20)
    const int src = __builtin_amdgcn_readfirstlane(s_src);
    const int ksrc = src ? p.k1 : p.k0;
    const int kbase = __builtin_amdgcn_readfirstlane(s_kc) * BK;
    const bool tail = kbase + BK > ksrc;     // only the last K step of a source can have dead chunks
    char* lds_a = smem + slot * STAGE + wid * 1024;
    char* lds_b = smem + slot * STAGE + A_BYTES + wid * 1024;
    const int soff_a = kbase * ES;
    const int soff_w = __builtin_amdgcn_readfirstlane(
        (int)(((long)s_tap * (p.k0 + p.k1) + (src ? p.k0 : 0) + kbase) * ES));
    auto issue = [&](const __amdgpu_buffer_rsrc_t& ra, const int (&va)[AR], auto has_tail) {
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        int v = va[i];
        if constexpr (decltype(has_tail)::value) { if (kbase + a_chunk[i] * EPC >= ksrc) v = INV; }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)(lds_a + i * (NT * 16)), 16, v, soff_a, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        int v = vb[i];
        if constexpr (decltype(has_tail)::value) { if (kbase + b_chunk[i] * EPC >= ksrc) v = INV; }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(lds_b + i * (NT * 16)), 16, v, soff_w, 0, 0);
      }
    };
    if (!tail) {
      if (!src) issue(ra0, va0, std::false_type{}); else issue(ra1, va1, std::false_type{});
    } else {
      if (!src) issue(ra0, va0, std::true_type{}); else issue(ra1, va1, std::true_type{});
    }
    if (++s_kc == (s_src ? p.nk1 : p.nk0)) {
      s_kc = 0;
      if (s_src == 0 && p.nk1 > 0) s_src = 1;
      else { s_src = 0; ++s_tap; tap_dirty = true; }
    }
  };

  const int wr = wid / WGN, wc = wid - wr * WGN;
  f32x16_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int l31 = lane & 31, hi = lane >> 5;
  int a_lds_row[FM], b_lds_row[FN];
#pragma unroll
  for (int i = 0; i < FM; ++i) a_lds_row[i] = wr * WTM + i * 32 + l31;
#pragma unroll
  for (int j = 0; j < FN; ++j) b_lds_row[j] = wc * WTN + j * 32 + l31;

  constexpr int KS = CPR / 2;                 // fragment reads per tile row (one chunk per lane half): MFMA k sub-steps (even)
  static_assert(KS % 2 == 0, "the pipelined loop reads fragment sets in pairs");
  // Fragment reads are raw ds_read_b128 (common.h): with compiler-visible LDS loads hipcc puts `s_waitcnt vmcnt(0)` in
  // front of the first read of every K step -- AFTER the next tile's DMA has been issued -- so load latency and MFMA time
  // add up instead of overlapping (1.1-1.5 us per 64-deep step, measured).  The reads of one fragment set are retired
  // by lds_wait<reads issued after them>() before the MFMAs that consume them.
  constexpr int NF = FM + FN;                 // ds_read_b128 per fragment set
  const unsigned lds_base = lds_addr(smem);
  auto read_frags = [&](unsigned sa, int ks, raw_u32x4_t (&af)[FM], raw_u32x4_t (&bf)[FN]) {
    const unsigned sb = sa + A_BYTES;
    const int chunk = ks * 2 + hi;
#pragma unroll
    for (int i = 0; i < FM; ++i) af[i] = lds_read16_raw(sa + tile_off<CPR>(a_lds_row[i], chunk));
#pragma unroll
    for (int j = 0; j < FN; ++j) bf[j] = lds_read16_raw(sb + tile_off<CPR>(b_lds_row[j], chunk));
  };
  constexpr int NLN = LN == 1 ? FM : (LN == 2 ? FN : 1);
  float ln_s[NLN], ln_q[NLN];
#pragma unroll
  for (int i = 0; i < NLN; ++i) ln_s[i] = ln_q[i] = 0.f;
  constexpr bool LN_SHIFT = LN != 0 && std::is_same<Tag, f32_tag>::value;     // see ln_stat_shifted
  float ln_c[LN_SHIFT ? NLN : 1];
  if constexpr (LN_SHIFT) {
#pragma unroll
    for (int i = 0; i < NLN; ++i) {
      const int row = LN == 1 ? m0 + a_lds_row[i] : n0 + b_lds_row[i];
      const bool ok = row < (LN == 1 ? p.m : p.n);
      ln_c[i] = ok ? *(const float*)((LN == 1 ? p.a0 : p.w) + (long)row * (LN == 1 ? p.lda0 : p.ldw) * 4) : 0.f;
    }
  }
  // TT_F32 "split16" (round 6): fp32-class products at the 16-bit matrix rate.  Every fp32 operand x is split on the fly into two fp16
  // parts on DIFFERENT binary scales,
  //     h = fp16(x 2^-8),   l = fp16((x - 2^8 h) 2^3)          x = 2^8 h + 2^-3 l  up to  max(2^-22 |x|, 2^-28)
  // so that |x| up to 2^24 fits (an unscaled fp16 hi part overflows at 65504: proj_in of the tiny test model sees 1.8e5, and inf x 0
  // is NaN) while the lo part -- which also repairs the denormal quantisation of h for |x| < 2^-6 -- stays a normal fp16 number for
  // every x whose h is normal (fp16 denormals are KEPT by the gfx950 MFMA: tools/mfma_split_probe.hip).  Then
  //     a b = 2^16 a_h b_h + 2^5 (a_h b_l + a_l b_h) + 2^-6 a_l b_l (dropped: 2^-22 of the product)
  // runs as three v_mfma_f32_32x32x16_f16 per product block into TWO fp32 accumulators (the hi x hi sum and the cross-term sum carry
  // different scales), combined once after the K loop.  One 16-deep MFMA needs 8 k-values per lane: two consecutive fragment sets
  // (4 fp32 each) -- the loops below consume the sets in pairs already, so the even set is split and parked in registers (phase 0)
  // and the odd set triggers the MFMAs (phase 1).  Both operands use the same (lane half, slot) -> k map, which is all the instruction
  // needs.  Per 32 x 32 x 16 block: 3 x 8 passes against 8 x 16 passes of v_mfma_f32_32x32x2_f32.
  uint2 sp_ah[SPLIT ? FM : 1], sp_al[SPLIT ? FM : 1], sp_bh[SPLIT ? FN : 1], sp_bl[SPLIT ? FN : 1];
  f32x16_t accx[SPLIT ? FM : 1][SPLIT ? FN : 1];        // cross terms a_h b_l + a_l b_h
  if constexpr (SPLIT) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[i][j][r] = 0.f;
  }
  constexpr bool pre_a = PRE_A, pre_b = PRE_B;         // compile-time: a branch would cut the block the scheduler interleaves
  // Software pipeline of the split products: the MFMAs of chunk pair p are ISSUED during the conversion of the even chunk of pair
  // p + 1 -- an in-order wave can only overlap its own VALU with its own MFMAs if they alternate in program order (the ablation of
  // 6.R6: conversions and the two extra MFMAs cost 9 ms each alone and 40 ms together when they run back to back).  The operands of
  // the pending pair wait in op_* (32 registers for a 64 x 64 wave tile; the pair's temporaries before); the first phase 0 of a launch
  // issues MFMAs on zero operands (adds nothing), the last pair is flushed after the K loop.  All block rows of the pending pair go
  // under the EVEN chunk's conversion -- spreading them (1 of 2 rows) keeps the odd chunk's halves in temporaries next to the pending
  // operands and spills 40-88 bytes per lane on the 64 x 64 wave tiles: 93.4 -> 104.2 ms / step (one call, interleaved).
  uint4 op_ah[SPLIT ? FM : 1], op_al[SPLIT ? FM : 1], op_bh[SPLIT ? FN : 1], op_bl[SPLIT ? FN : 1];
  if constexpr (SPLIT) {
#pragma unroll
    for (int i = 0; i < FM; ++i) op_ah[i] = op_al[i] = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < FN; ++j) op_bh[j] = op_bl[j] = make_uint4(0, 0, 0, 0);
  }
  auto issue_pending = [&]() {               // the three MFMA sweeps of the pair whose operands wait in op_*: the two MFMAs into one
   if constexpr (SPLIT) {                    // cross-term accumulator sit FM x FN x 2 instructions apart (back to back they wait for each other's result)
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) accx[i][j] = Cvt<f16_tag>::mfma32(op_bl[j], op_ah[i], accx[i][j]);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = Cvt<f16_tag>::mfma32(op_bh[j], op_ah[i], acc[i][j]);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) accx[i][j] = Cvt<f16_tag>::mfma32(op_bh[j], op_al[i], accx[i][j]);
   }
  };
  auto mma = [&](const raw_u32x4_t (&af)[FM], const raw_u32x4_t (&bf)[FN], int phase) {
    if constexpr (LN == 1) {
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if constexpr (LN_SHIFT) ln_stat_shifted(af[i], ln_c[i], ln_s[i], ln_q[i]); else ln_stat<Tag>(af[i], ln_s[i], ln_q[i]);
      }
    } else if constexpr (LN == 2) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        if constexpr (LN_SHIFT) ln_stat_shifted(bf[j], ln_c[j], ln_s[j], ln_q[j]); else ln_stat<Tag>(bf[j], ln_s[j], ln_q[j]);
      }
    }
    if constexpr (SPLIT) {
      if (phase == 0) {                      // (constant after unrolling) even chunk: convert it UNDER the MFMAs of the previous pair
#pragma unroll
        for (int i = 0; i < FM; ++i) split_f32x4(af[i], pre_a, sp_ah[i], sp_al[i]);
#pragma unroll
        for (int j = 0; j < FN; ++j) split_f32x4(bf[j], pre_b, sp_bh[j], sp_bl[j]);
        issue_pending();
        // ask for MFMA, VALU, VALU, ... (one MFMA holds the matrix pipe for 8 passes; two or three conversions fit under it)
#pragma unroll
        for (int g = 0; g < 3 * FM * FN; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        }
      } else {                               // odd chunk: convert (no MFMAs left to hide it under: the 10-VALU asm form), combine with the parked even half
        uint2 th[FM], tl[FM], ubh[FN], ubl[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) split_f32x4_mix(af[i], pre_a, th[i], tl[i]);
#pragma unroll
        for (int j = 0; j < FN; ++j) split_f32x4_mix(bf[j], pre_b, ubh[j], ubl[j]);
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          op_ah[i] = make_uint4(sp_ah[i].x, sp_ah[i].y, th[i].x, th[i].y); op_al[i] = make_uint4(sp_al[i].x, sp_al[i].y, tl[i].x, tl[i].y);
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          op_bh[j] = make_uint4(sp_bh[j].x, sp_bh[j].y, ubh[j].x, ubh[j].y); op_bl[j] = make_uint4(sp_bl[j].x, sp_bl[j].y, ubl[j].x, ubl[j].y);
        }
      }
      __builtin_amdgcn_sched_barrier(0);     // conversions and MFMAs stay in front of the next raw fragment read
    } else {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = Cvt<Tag>::mfma32(make_uint4(bf[j].x, bf[j].y, bf[j].z, bf[j].w), make_uint4(af[i].x, af[i].y, af[i].z, af[i].w), acc[i][j]);
    }
    // The fragment registers are written by raw asm ds_reads whose data lands later (cdna guide 5.7 item 1).  If the
    // scheduler sinks the statistics VALU below the NEXT raw read of the same fragment set, the two values are live at once,
    // the new read gets other registers and a v_mov copies them back at the loop edge -- before the data has landed
    // (NaNs under load, measured).  Pin everything that reads the fragments in front of whatever follows.
    if constexpr (LN != 0) __builtin_amdgcn_sched_barrier(0);
  };

  // residual operands of every (row, quad) this lane will finish (epilogue layout, see below): ONE batch of loads.
  // Tiles with register headroom issue it BEFORE the main loop so the whole K loop hides the latency; the 256-row
  // tiles (128-VGPR budget) issue it at the top of the epilogue, where it overlaps the barrier and the LDS transposition.
  // (The AlphaBlender source is usually the residual tensor itself -- temporal ResBlock -- and then shares the
  // preloaded value; a distinct blend tensor is read in-pass.)
  constexpr int NCH = (FN + 1) / 2;                    // 64-column chunks per fragment row
  constexpr bool EARLY_RES = BM <= 128 && !SPLIT;     // (the split variant needs the 64 registers for its operand halves)
  quad_t resv[EARLY_RES ? FM : 1][EARLY_RES ? NCH : 1][8];   // 256-row tiles read the residual inside the passes
  const bool direct = (p.out_col_hw > 0 || p.out_f32) && p.splitk == 1;   // rare layouts keep the simple per-fragment path
  const bool blend_is_res = p.blend && p.blend == p.residual && p.ld_blend == p.ld_res;
  const int e_org = WIDE ? m0 : 0;       // WIDE: first row of the tile -- origin of the residual / blend / out windows
  auto preload_residual = [&]() {
    if constexpr (EARLY_RES) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int pass = 0; pass < 8; ++pass) resv[i][c][pass] = zero_quad<Tag>();
    }
    // (no residual: nothing is requested -- loads through a 0-byte descriptor return 0, but still cost their issue slots in the
    // texture addresser: 0.5 us per launch for two resident 128 x 128 tiles, tools/gemm_timeline.py)
    if constexpr (EARLY_RES) if (!direct && !p.geglu && p.splitk == 1 && p.residual) {
      const __amdgpu_buffer_rsrc_t r_res = WIDE ? window_rsrc<ES>(p.residual, e_org, p.ld_res, ((long)(p.m - 1) * p.ld_res + p.n) * ES) : make_rsrc(p.residual, p.res_bytes);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int nfr = (2 * c + 1 < FN) ? 2 : 1;
          const int q_per_row = nfr * 8, rows_per_pass = 64 / q_per_row;
          const int gn = n0 + wc * WTN + c * 64 + (lane % q_per_row) * 4;
#pragma unroll
          for (int pass = 0; pass < 8; ++pass) {
            resv[i][c][pass] = zero_quad<Tag>();
            if (pass * rows_per_pass < 32) {
              const int gm = m0 + wr * WTM + i * 32 + pass * rows_per_pass + lane / q_per_row;
              resv[i][c][pass] = ldq<Tag>(r_res, (gm < p.m && gn < p.n) ? (int)(((long)(gm - e_org) * p.ld_res + gn) * ES) : kInv);
            }
          }
        }
    }
  };
  if constexpr (NST == 2) {
    // plain double buffer: wait tile kt, barrier, issue tile kt+1, compute tile kt.  The first tile is requested before
    // the residual batch (whose address arithmetic costs ~2 us); the first wait covers both.
    TL(6);
    stage(0);
    TL(7);
    // (requested behind the SECOND tile instead -- under the MFMAs of the first K step -- the batch disturbs the K loop's DMA stream:
    // 12544 x 640 x 640 + residual 18.7 -> 19.3 us, K = 2560 49.3 -> 51.9 us, step 30.67 -> 30.72 ms, one call; round 5)
    preload_residual();
    TL(1);
    for (int kt = 0; kt < KT; ++kt) {
      wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#ifdef TT_GEMM_TIMELINE
      if (kt == 0) TL(2);
#endif
      if (kt + 1 < KT) stage((kt + 1) & 1);
      const unsigned sa = lds_base + (kt & 1) * STAGE;
      raw_u32x4_t af[2][FM], bf[2][FN];         // fragment sets double-buffered: set ks+1 is read under the MFMAs of ks
      read_frags(sa, 0, af[0], bf[0]);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) {
          read_frags(sa, ks + 1, af[(ks + 1) & 1], bf[(ks + 1) & 1]);
          lds_wait<NF>();
        } else {
          lds_wait<0>();
        }
        mma(af[ks & 1], bf[ks & 1], ks & 1);
      }
    }
  } else {
    TL(6);
    preload_residual();                       // before the ring fill: the counted waits below assume the DMAs come last
    TL(1);
    // software pipeline: fragments double-buffered in registers; the wait+barrier for tile kt+1 sits BEFORE the last
    // MFMA group of tile kt, so the first fragments of tile kt+1 are read (and tile kt+NST-1 is issued) under MFMAs.
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
      if (s < KT) stage(s);
    wait_tiles<G>(min(KT - 1, NST - 2));      // tile 0 landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    raw_u32x4_t afA[FM], bfA[FN], afB[FM], bfB[FN];
    read_frags(lds_base, 0, afA, bfA);
    int slot = 0, fill = NST - 1;             // slot of tile kt ; slot the next staged tile goes to
    // The last tile is peeled: inside the steady loop set A is (re)defined by the raw read at ONE program point on every
    // path, so no value merge of "old fragments / new fragments" exists and hipcc has no reason to copy raw-read registers
    // (a copy would run before the data has landed: cdna guide 5.7 item 1).
    auto tile = [&](int kt, auto last_tag) {
      constexpr bool LAST = decltype(last_tag)::value;
      const unsigned sa = lds_base + slot * STAGE;
      const int nslot = slot + 1 == NST ? 0 : slot + 1;
#pragma unroll
      for (int ks = 0; ks < KS; ks += 2) {
        read_frags(sa, ks + 1, afB, bfB);
        lds_wait<NF>();                       // set A (issued before set B) has landed
        mma(afA, bfA, 0);
        if (ks + 2 < KS) {
          read_frags(sa, ks + 2, afA, bfA);
          lds_wait<NF>();                     // set B has landed
        } else if constexpr (!LAST) {
          // tile kt+1 must have landed; tiles kt+2 .. min(KT-1, kt+NST-2) may stay in flight
          wait_tiles<G>(min(KT - 2 - kt, NST - 3));
          __builtin_amdgcn_s_barrier();       // all waves: tile kt+1 visible, tile kt-1's slot free
          asm volatile("" ::: "memory");
          if (kt + NST - 1 < KT) stage(fill);
          read_frags(lds_base + nslot * STAGE, 0, afA, bfA);
          lds_wait<NF>();
        } else {
          lds_wait<0>();
        }
        mma(afB, bfB, 1);
      }
      slot = nslot;
      fill = fill + 1 == NST ? 0 : fill + 1;
    };
    for (int kt = 0; kt + 1 < KT; ++kt) tile(kt, std::false_type{});
    tile(KT - 1, std::true_type{});
  }

  if constexpr (SPLIT) issue_pending();                // the last chunk pair's MFMAs
  if constexpr (SPLIT) {                               // 2^16 (hi x hi) + 2^5 (cross terms)
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = fmaf(accx[i][j][r], 32.0f, acc[i][j][r] * 65536.0f);
  }
  // ---- fused LayerNorm: 1/sigma of the operand rows from the sums gathered beside the MFMAs (the two lane halves hold the
  // even / odd chunks of a row).  Rows: scale the accumulators now (lane <-> row l31).  Columns: the lane that owns W row
  // l31 of fragment j publishes 1/sigma of output column j*32 + l31 in a wave-private LDS array behind the ring; the
  // epilogue multiplies by it where a lane holds four consecutive columns.
  constexpr int CS_OFF = NST * STAGE;                  // MODE 4 only: WGM*WGN KiB more dynamic LDS (launch_mode)
  constexpr int STAT_OFF = NST * STAGE + (KMODE == 4 ? WGM * WGN * 1024 : 0);    // GemmP.stats: 8 * BN * WGM bytes more (launch_mode)
  if constexpr (LN != 0) {
    const float inv_k = 1.0f / (float)p.k0;
    float rs[NLN];
#pragma unroll
    for (int i = 0; i < NLN; ++i) {
      const float sm = (ln_s[i] + __shfl_xor(ln_s[i], 32)) * inv_k, sq = (ln_q[i] + __shfl_xor(ln_q[i], 32)) * inv_k;
      rs[i] = rsqrtf(fmaxf(sq - sm * sm, 0.f) + p.ln_eps);
    }
    if constexpr (LN == 1) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] *= rs[i];
    } else {
      float* cs = (float*)(smem + CS_OFF + wid * 1024);
#pragma unroll
      for (int j = 0; j < FN; ++j) cs[j * 32 + l31] = rs[j];          // both lane halves write the same value
    }
  }
  const float* colscale = (const float*)(smem + CS_OFF + wid * 1024);   // read only when LN == 2

  // ---- epilogue.  The MFMA layout gives a lane row m = .. + l31 and columns n = .. + 8g + 4hi + {0..3}: stored
  // directly, one instruction would touch 32 rows x 16 bytes.  Instead each wave transposes its accumulators through a
  // private LDS strip (fp32, 32 rows x 64 columns at a time) and re-reads them so that 16 consecutive lanes cover 64
  // consecutive columns of one row: every residual/blend load and every store instruction then covers 4 rows x 128
  // contiguous bytes.  All global accesses go through bounds-checked descriptors (see make_rsrc) so the pass loops are
  // straight-line code; the arithmetic (fp32, same order) is what epilogue_quad does.
  TL(3);
  if (!direct) {
    const __amdgpu_buffer_rsrc_t r_bias = make_rsrc(p.bias, p.bias_bytes);
    // WIDE (never split along K): the out window starts at the tile's first output row; phase-packed form: slice (py, px) stores low-res
    // row gm = (img, y, x) to output row 4 gm - 2 x + (py 2 win + px), which grows with gm -- the origin is that of m0 in phase (0, 0)
    const int o_org = !WIDE ? 0 : ((MODE == 1 && !PAD_BR && p.phases) ? 4 * m0 - 2 * (m0 - fdiv(m0, p.fd_wout) * p.win) : m0);
    const long o_rows_all = (MODE == 1 && !PAD_BR && p.phases) ? 4L * p.m : (long)p.m;
    const __amdgpu_buffer_rsrc_t r_out = WIDE ? window_rsrc<ES>(p.out, o_org, p.ldo, ((o_rows_all - 1) * p.ldo + p.n) * ES)
                                         : (p.splitk > 1 ? make_rsrc(p.ws, p.ws_bytes) : make_rsrc(p.out, p.out_bytes));
    char* ebuf = smem + wid * 8192;
    static_assert(WGM * WGN * 8192 <= NST * STAGE, "epilogue strips do not fit the ring");
    if (WIDE || !p.geglu) {
      // bias of the 4 columns this lane finishes in each 64-column chunk (row-independent: loaded once)
      float4 bias4[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int q_per_row = ((2 * c + 1 < FN) ? 2 : 1) * 8;
        const int gn = n0 + wc * WTN + c * 64 + (lane % q_per_row) * 4;
        bias4[c] = ld128f(r_bias, gn < p.n ? gn * 4 : kInv);
      }
      const float alpha = p.blend ? p.alpha : 0.0f, one_m_alpha = 1.0f - alpha;
      __syncthreads();                                 // all waves are done with the operand ring
      TL(4);
      // one arm of TT_GEMM_EPI_ARMS (uniform dispatch below, each arm straight-line)
      auto run = [&](auto arm) {
        using Arm = decltype(arm);
        constexpr bool FILM = Arm::FILM, INPASS = Arm::INPASS, OUT8 = Arm::OUT8, STATS = Arm::STATS, PHASE = Arm::PHASE;
        const int ph_row0 = (split >> 1) * 2 * p.win + (split & 1), ph_hw = p.hin * p.win;
        const __amdgpu_buffer_rsrc_t r_rv = make_rsrc(p.rowvec, (FILM || INPASS) ? p.rowvec_bytes : 0);
        const __amdgpu_buffer_rsrc_t r_bl = (WIDE && INPASS) ? window_rsrc<ES>(p.blend, e_org, p.ld_blend, ((long)(p.m - 1) * p.ld_blend + p.n) * ES)
                                                             : make_rsrc(p.blend, INPASS ? p.blend_bytes : 0);
        const __amdgpu_buffer_rsrc_t r_res = (WIDE && INPASS && !EARLY_RES) ? window_rsrc<ES>(p.residual, e_org, p.ld_res, ((long)(p.m - 1) * p.ld_res + p.n) * ES)
                                                                            : make_rsrc(p.residual, (INPASS && !EARLY_RES) ? p.res_bytes : 0);
        const int rv_rows = p.rowvec ? p.rowvec_rows : 1;
        // periodic row vector (rowvec_mod): group indices wrap; the even / odd form (one row per group, period 2) stays on the
        // two-vector path below with the row's parity as the selector
        const bool parity = FILM && p.rowvec_mod == 2 && rv_rows == 1;
        auto wrap = [&](int g) { return p.rowvec_mod > 0 ? g - fdiv(g, p.fd_rv_mod) * p.rowvec_mod : g; };
        float* sstage = (float*)(smem + STAT_OFF) + wid * (2 * WTN);      // staging rows behind the ring (launch_mode adds the bytes)
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int mb = m0 + wr * WTM + i * 32;
          const int grp_raw = fdiv(mb, p.fd_rv_rows);    // row group of the fragment's first row (uniform)
          const int grp0 = parity ? 0 : wrap(grp_raw), grp1 = parity ? 1 : wrap(grp_raw + 1);
          const int grp_split = parity ? mb : (grp_raw + 1) * rv_rows;    // first row of the next group (parity: see the selector)
          const int sel_split = parity ? 0x7fffffff : grp_split, sel_odd = parity ? 1 : 0;
#pragma unroll
          for (int jc = 0; jc < FN; jc += 2) {
            const int nfr = (jc + 1 < FN) ? 2 : 1;       // fragments in this chunk (compile-time after unrolling)
            const int q_per_row = nfr * 8;               // 4-column quads per strip row
            const int rows_per_pass = 64 / q_per_row;
            const int qq = lane % q_per_row, rr = lane / q_per_row;
            const int gn = n0 + wc * WTN + jc * 32 + qq * 4;
            const float4 b4 = bias4[jc / 2];
            float4 cs4 = make_float4(1.f, 1.f, 1.f, 1.f);
            if constexpr (LN == 2) cs4 = *(const float4*)(colscale + jc * 32 + qq * 4);
            float4 film_lo = make_float4(0.f, 0.f, 0.f, 0.f), film_hi = film_lo;
            if constexpr (FILM) {
              film_lo = ld128f(r_rv, (mb < p.m && gn < p.n) ? (int)(((long)grp0 * p.ld_rowvec + gn) * 4) : kInv);
              film_hi = ld128f(r_rv, (grp_split < p.m && gn < p.n) ? (int)(((long)grp1 * p.ld_rowvec + gn) * 4) : kInv);
            }
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
              if (jc + jj < FN) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                  *(float4*)(ebuf + strip_off(l31, jj * 8 + 2 * g + hi, nfr * 8)) =
                      make_float4(acc[i][jc + jj][g * 4], acc[i][jc + jj][g * 4 + 1], acc[i][jc + jj][g * 4 + 2], acc[i][jc + jj][g * 4 + 3]);
              }
            }
            constexpr int PB = INPASS ? (BM > 128 ? 2 : 4) : 8;   // passes per batch, sized to the register budget
#pragma unroll
            for (int pb = 0; pb < 8; pb += PB) {
              quad_t rqv[PB], blv[PB];
              float4 rvv[PB];
#pragma unroll
              for (int k = 0; k < PB; ++k) {
                const int pass = pb + k;
                rqv[k] = blv[k] = zero_quad<Tag>();
                rvv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pass * rows_per_pass < 32) {
                  const int gm = mb + pass * rows_per_pass + rr;
                  const bool ok = gm < p.m && gn < p.n;
                  if constexpr (EARLY_RES) rqv[k] = resv[i][jc / 2][pass];
                  else if constexpr (INPASS) rqv[k] = ldq<Tag>(r_res, ok ? (int)(((long)(gm - e_org) * p.ld_res + gn) * ES) : kInv);
                  if constexpr (INPASS) {
                    rvv[k] = ld128f(r_rv, ok ? (int)(((long)wrap(fdiv(gm, p.fd_rv_rows)) * p.ld_rowvec + gn) * 4) : kInv);
                    blv[k] = ldq<Tag>(r_bl, ok ? (int)(((long)(gm - e_org) * p.ld_blend + gn) * ES) : kInv);
                  }
                }
              }
#pragma unroll
              for (int k = 0; k < PB; ++k) {
                const int pass = pb + k;
                if (pass * rows_per_pass < 32) {
                  const int r = pass * rows_per_pass + rr;
                  const float4 t = *(const float4*)(ebuf + strip_off(r, qq, q_per_row));
                  const int gm = mb + r;
                  const bool ok = gm < p.m && gn < p.n;
                  int orow = gm;                           // row of `out`
                  if constexpr (PHASE) {
                    const int img = fdiv(gm, p.fd_hwo), rem = gm - img * ph_hw, y = fdiv(rem, p.fd_wout), x = rem - y * p.win;
                    orow = (img * p.hin + y) * 4 * p.win + 2 * x + ph_row0;      // (img * 2 hin + 2 y) * 2 win + 2 x + (py * 2 win + px)
                  }
                  if (p.splitk > 1) {                    // uniform: fp32 partial sums of K slice `split`
                    st128f(r_out, ok ? (int)((((long)split * p.m + gm) * p.n + gn) * 4) : kInv, t);
                  } else {
                    float v[4];
                    if constexpr (WIDE) {                // written out (epi_elem): no FILM arm, no column scale
                      const quad_t rq = rqv[k];
                      quad_t bq = rq;
                      if constexpr (INPASS) bq = (p.blend && !blend_is_res) ? blv[k] : rq;
                      float r4[4], b4v[4];
                      quad_to_f32<Tag>(rq, r4);
                      quad_to_f32<Tag>(bq, b4v);
                      const float tv[4] = {t.x, t.y, t.z, t.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w}, rv4[4] = {rvv[k].x, rvv[k].y, rvv[k].z, rvv[k].w};
#pragma unroll
                      for (int e = 0; e < 4; ++e) v[e] = epi_elem<INPASS, !EARLY_RES>(tv[e], bv[e], p.acc_scale, rv4[e], r4[e], b4v[e], alpha, one_m_alpha);
                    } else {                             // the loose expression: its contractions are hipcc's (see epi_elem)
                      v[0] = (t.x * cs4.x + b4.x) * p.acc_scale; v[1] = (t.y * cs4.y + b4.y) * p.acc_scale;
                      v[2] = (t.z * cs4.z + b4.z) * p.acc_scale; v[3] = (t.w * cs4.w + b4.w) * p.acc_scale;
                      const quad_t rq = rqv[k];
                      quad_t bq = rq;
                      if constexpr (FILM) {
                        const float4 f = ((gm >= sel_split) | ((gm & sel_odd) != 0)) ? film_hi : film_lo;     // branch-free (see gemm_w320.hip)
                        v[0] += f.x; v[1] += f.y; v[2] += f.z; v[3] += f.w;
                      }
                      if constexpr (INPASS) {
                        v[0] += rvv[k].x; v[1] += rvv[k].y; v[2] += rvv[k].z; v[3] += rvv[k].w;
                        bq = (p.blend && !blend_is_res) ? blv[k] : rq;
                      }
                      float r4[4], b4v[4];
                      quad_to_f32<Tag>(rq, r4);
                      quad_to_f32<Tag>(bq, b4v);
#pragma unroll
                      for (int e = 0; e < 4; ++e) v[e] = alpha * b4v[e] + one_m_alpha * (v[e] + r4[e]);
                    }
                    if constexpr (OUT8) st32(r_out, ok ? (int)((long)gm * p.ldo + gn) : kInv, pack4_fp8(v));
                    else {
                      const quad_t packed = f32_to_quad<Tag>(v);
                      if constexpr (ES == 2) st64(r_out, ok ? (int)(((long)(orow - o_org) * p.ldo + gn) * ES) : kInv, packed.x, packed.y);
                      else stq<Tag>(r_out, ok ? (int)(((long)(orow - o_org) * p.ldo + gn) * ES) : kInv, v);
                      if constexpr (STATS) {               // (rows >= m of a ragged last tile add nothing)
                        float sv[4];
                        quad_to_f32<Tag>(packed, sv);
                        const bool live = gm < p.m;
                        *(float4*)(ebuf + strip_off(r, qq, q_per_row)) = make_float4(live ? sv[0] : 0.f, live ? sv[1] : 0.f, live ? sv[2] : 0.f, live ? sv[3] : 0.f);
                      }
                    }
                  }
                }
              }
            }
            if constexpr (STATS) colstat_strip(ebuf, q_per_row, lane, sstage + jc * 32, sstage + WTN + jc * 32, i == 0);
          }
        }
      };
      const bool inpass = (p.blend && !blend_is_res) || (p.rowvec && p.rowvec_rows < 32 && !(p.rowvec_mod == 2 && p.rowvec_rows == 1)) ||
                          (!EARLY_RES && p.residual);
      const bool kstats = p.stats && p.splitk == 1;          // (a K slice leaves the sums to the reduction kernel)
      const bool phases = MODE == 1 && !PAD_BR && p.phases;  // phase-packed upsampling conv
      if constexpr (WIDE) {                                  // the wide variant: no row vector (tt_gemm refuses it), 16-bit or fp32 out
        static_assert(LN == 0, "the wide variant has no column scale");
        if (inpass) run(epi_arm::InPass{});
        else if (phases) { if constexpr (MODE == 1) run(epi_arm::Phase{}); }
        else { if (kstats) run(epi_arm::PlainStats{}); else run(epi_arm::Plain{}); }
      } else if (inpass) run(epi_arm::InPass{});             // (never with statistics: tt_gemm_stats_rows)
      else if (p.rowvec) { if (kstats) run(epi_arm::FilmStats{}); else run(epi_arm::Film{}); }
      else if (MODE == 0 && ES == 2 && p.out_fp8) {
        if constexpr (MODE == 0 && ES == 2) run(epi_arm::Out8{});
      } else if (phases) {
        if constexpr (MODE == 1 && !PAD_BR) run(epi_arm::Phase{});
      } else { if (kstats) run(epi_arm::PlainStats{}); else run(epi_arm::Plain{}); }
      if (kstats) {
        __syncthreads();
        // the tile-level step: one thread per column adds the waves' staging rows up in a fixed order
        const float* st0 = (const float*)(smem + STAT_OFF);
        if (p.stat_rows == BM) {                             // one statistics tile per output tile: the waves of one tile column, wave rows in order
          for (int c = tid; c < BN; c += NT) {
            const int wcc = c / WTN, col = c - wcc * WTN;
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < WGM; ++w) {
              const float* row = st0 + (w * WGN + wcc) * (2 * WTN);
              a += row[col]; b += row[WTN + col];
            }
            if (n0 + c < p.n) {
              p.stats[((long)tile_m * 2) * p.n + n0 + c] = a;
              p.stats[((long)tile_m * 2 + 1) * p.n + n0 + c] = b;
            }
          }
        } else {                                             // one per wave row (WTM rows; tt_gemm_stats_rows): segments that are no whole number of tiles
          for (int c = tid; c < BN * WGM; c += NT) {
            const int w = c / BN, cc = c - w * BN, wcc = cc / WTN, col = cc - wcc * WTN;
            const float* row = st0 + (w * WGN + wcc) * (2 * WTN);
            const long srow = (long)tile_m * WGM + w;
            if (n0 + cc < p.n && srow * WTM < p.m) {
              p.stats[(srow * 2) * p.n + n0 + cc] = row[col];
              p.stats[(srow * 2 + 1) * p.n + n0 + cc] = row[WTN + col];
            }
          }
        }
      }
    } else {
      // GEGLU: value/gate pairs are lane-local (regs g=0/2 value, g=1/3 gate); gelu in registers, then the 16
      // output columns of each fragment go through the strip: 2 fragments -> 32 output columns = 64 bytes per row.
      float4 bval[FN][2], bgate[FN][2];                  // bias of this lane's value / gate quads (row-independent)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int gnp = n0 + wc * WTN + j * 32 + tt * 16 + 4 * hi;      // packed column of the value quad
          bval[j][tt] = ld128f(r_bias, gnp < p.n ? gnp * 4 : kInv);
          bgate[j][tt] = ld128f(r_bias, gnp < p.n ? (gnp + 8) * 4 : kInv);
        }
      __syncthreads();                                 // all waves are done with the operand ring
      TL(4);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int mb = m0 + wr * WTM + i * 32;
#pragma unroll
        for (int jc = 0; jc < FN; jc += 2) {
          const int nfr = (jc + 1 < FN) ? 2 : 1;
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            if (jc + jj < FN) {
#pragma unroll
              for (int tt = 0; tt < 2; ++tt) {
                const float4 bv = bval[jc + jj][tt], bg = bgate[jc + jj][tt];
                const float bvv[4] = {bv.x, bv.y, bv.z, bv.w}, bgv[4] = {bg.x, bg.y, bg.z, bg.w};
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  v[e] = (acc[i][jc + jj][(2 * tt) * 4 + e] + bvv[e]) * gelu_erf_f(acc[i][jc + jj][(2 * tt + 1) * 4 + e] + bgv[e]);
                *(float4*)(ebuf + strip_off(l31, jj * 4 + tt * 2 + hi, nfr * 4)) = make_float4(v[0], v[1], v[2], v[3]);
              }
            }
          }
          const int q_per_row = nfr * 4;               // output quads per strip row (16 output columns per fragment)
          const int rows_per_pass = 64 / q_per_row;
          const int qq = lane % q_per_row, rr = lane / q_per_row;
          const int oc = ((n0 + wc * WTN + jc * 32) >> 1) + qq * 4;     // output column
#pragma unroll
          for (int pass = 0; pass < 4; ++pass) {
            if (pass * rows_per_pass < 32) {
              const int r = pass * rows_per_pass + rr;
              const float4 t = *(const float4*)(ebuf + strip_off(r, qq, q_per_row));
              const int gm = mb + r;
              const float t4[4] = {t.x, t.y, t.z, t.w};
              stq<Tag>(r_out, (gm < p.m && oc * 2 < p.n) ? (int)(((long)gm * p.ldo + oc) * ES) : kInv, t4);
            }
          }
        }
      }
    }
#ifdef TT_GEMM_TIMELINE
    __builtin_amdgcn_s_waitcnt(0);
    TL(5);
#endif
    return;
  }
  // direct path: fp32 output and the padded transposed output (never combined with split-K: see tt_gemm)
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int gm = m0 + wr * WTM + i * 32 + l31;
    if (gm >= p.m) continue;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int nb = n0 + wc * WTN + j * 32;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int gn = nb + 8 * g + 4 * hi;
        if (gn >= p.n) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][g * 4 + e];
        if constexpr (LN == 2) {
          const float4 c4 = *(const float4*)(colscale + j * 32 + 8 * g + 4 * hi);
          v[0] *= c4.x; v[1] *= c4.y; v[2] *= c4.z; v[3] *= c4.w;
        }
        epilogue_quad<Tag>(p, gm, gn, v);
      }
    }
  }
}

}  // namespace ttg
