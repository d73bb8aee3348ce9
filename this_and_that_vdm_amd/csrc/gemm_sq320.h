// gemm_sq320.h -- the streaming 320 x 320 kernel of tt_gemm (sq320_kernel) and its launcher; instantiated by gemm_inst_{bf16,f16}.hip,
// gemm.hip reads its shape constants.
#pragma once
#include "gemm_params.h"

namespace ttg {

// ---- (opt-in: tt_gemm_set_streaming_square / TT_GEMM_SQ320=1) square C = 320 linears of the finest UNet level (to_out /
// to_q / proj_in / proj_out at 32x56 latents: ~60 launches per step, M = 50176).  Measured: 31 us against 36 us for the
// tiled kernel in isolation, but 0.1-0.3 ms per step SLOWER inside the two-branch graph (one 160 KiB block per CU leaves
// no room for the other branch's kernels), hence off by default.  The tiled kernel above needs 1.5 rounds of lock-stepped blocks for them and re-reads W from L2
// for every tile (36-50 us against ~20 us for their 64-96 MB at HBM speed).  Here W never touches LDS: each of the 10
// waves of a block keeps its 32 output columns x 320 K of W in registers (20 MFMA operands = 80 VGPRs) for the whole
// launch, blocks are persistent over 32-row tiles of A, and LDS holds only a deep ring of A (and residual) tiles filled
// by LDS-DMA, so the launch streams A / residual / out at HBM speed with several tiles in flight per CU.
// Epilogue terms: bias, scale, residual, AlphaBlender with the residual as its source (the plain variant above).
constexpr int SQ_K = 320, SQ_N = 320, SQ_ROWS = 32, SQ_WAVES = SQ_N / 32, SQ_NT = 64 * SQ_WAVES;
constexpr int SQ_CPR = SQ_K / 8;                               // 16-byte chunks per tile row (40)
constexpr int SQ_TILE_BYTES = SQ_ROWS * SQ_K * 2;              // 20 KiB: one A (or residual) tile
constexpr int SQ_PASSES = SQ_ROWS * SQ_CPR / SQ_NT;            // DMA instructions per thread per tile (2)
static_assert(SQ_ROWS * SQ_CPR % SQ_NT == 0 && SQ_CPR % 8 == 0, "sq320 staging");
__device__ __forceinline__ int sq_swz(int row) { return (row >> 1) & 7; }     // 640-byte rows: see tile_swz
__device__ __forceinline__ int sq_off(int row, int chunk) { return (row * SQ_CPR + (chunk ^ sq_swz(row))) << 4; }

// HAS_RV (round 6): a row vector with at most TWO distinct rows over the launch -- the even / odd form (rowvec_rows = 1, rowvec_mod = 2: the temporal
// block's output projection) or two groups of rowvec_rows rows (a multiple of 32: the zero-context bias per CFG half) -- both rows are loaded ONCE
// before the tile loop (a load inside it would sit in the counted vmcnt stream of the DMA ring) and selected per row by arithmetic.
template <typename Tag, bool HAS_RES, bool HAS_RV = false>
__global__ __launch_bounds__(SQ_NT) void sq320_kernel(const GemmP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int G = HAS_RES ? 2 * SQ_PASSES : SQ_PASSES;       // DMA instructions per thread per ring slot
  constexpr int SLOT = HAS_RES ? 2 * SQ_TILE_BYTES : SQ_TILE_BYTES;
  constexpr int NST = HAS_RES ? 3 : 5;                         // ring depth: 120 / 100 KiB + 40 KiB of strips
  constexpr int KS = SQ_K / 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int ntiles = (p.m + SQ_ROWS - 1) / SQ_ROWS;
  const int my_tiles = blockIdx.x < ntiles ? (ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.a0, p.a0_bytes);
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(p.residual, p.res_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

  // ---- W operands of this wave's 32 columns: lane (column l31, k-half hi) holds k = ks*16 + hi*8 .. +8
  uint4 wf[KS];
  {
    const int voff = (int)(((long)(wid * 32 + l31) * p.ldw + hi * 8) * 2);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rw, voff, ks * 32, 0);
      wf[ks] = make_uint4(v.x, v.y, v.z, v.w);
    }
  }
  const int qq = lane & 7, rr_ = lane >> 3;                    // epilogue layout: 8 quads per 32-column row, 8 rows per pass
  const int gn = wid * 32 + qq * 4;
  const float4 b4 = ld128f(make_rsrc(p.bias, p.bias_bytes), gn * 4);
  float4 rv0 = make_float4(0.f, 0.f, 0.f, 0.f), rv1 = rv0;
  const bool rv_parity = HAS_RV && p.rowvec_mod == 2;           // row r takes rv[r & 1]; otherwise rv[r >= rowvec_rows]
  if constexpr (HAS_RV) {
    const __amdgpu_buffer_rsrc_t r_rv = make_rsrc(p.rowvec, p.rowvec_bytes);
    rv0 = ld128f(r_rv, gn * 4);
    rv1 = ld128f(r_rv, (int)((p.ld_rowvec + gn) * 4));           // (one group only: beyond the descriptor -> zeros, never selected)
  }
  const float alpha = p.blend ? p.alpha : 0.0f, one_m_alpha = 1.0f - alpha;
  const __amdgpu_buffer_rsrc_t r_out = make_rsrc(p.out, p.out_bytes);

  // per-thread source offsets inside a tile (the tile's first row is a scalar offset)
  int voa[SQ_PASSES], vor[SQ_PASSES], vrow[SQ_PASSES];
#pragma unroll
  for (int i = 0; i < SQ_PASSES; ++i) {
    const int c = i * SQ_NT + tid, row = c / SQ_CPR, ch = (c % SQ_CPR) ^ sq_swz(row);
    vrow[i] = row;
    voa[i] = (int)(((long)row * p.lda0 + ch * 8) * 2);
    vor[i] = (int)(((long)row * p.ld_res + ch * 8) * 2);
  }
  auto stage = [&](int j, int slot) {        // j-th tile of this block; beyond the end it still issues G (dropped) loads
    // straight-line on purpose: with a branch around the DMA hipcc loses count of the loads in flight and drains them
    // (vmcnt(0)) before every tile.  Past the last tile every row fails the bounds test, so nothing is fetched.
    const int m0 = ((int)blockIdx.x + j * (int)gridDim.x) * SQ_ROWS;
    char* la = smem + slot * SLOT + wid * 1024;
    const int soa = __builtin_amdgcn_readfirstlane((int)((long)m0 * p.lda0 * 2));
    const int sor = __builtin_amdgcn_readfirstlane((int)((long)m0 * p.ld_res * 2));
#pragma unroll
    for (int i = 0; i < SQ_PASSES; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)(la + i * (SQ_NT * 16)), 16,
                                               m0 + vrow[i] < p.m ? voa[i] : kInv, soa, 0, 0);
    if constexpr (HAS_RES) {
#pragma unroll
      for (int i = 0; i < SQ_PASSES; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (__attribute__((address_space(3))) void*)(la + SQ_TILE_BYTES + i * (SQ_NT * 16)), 16,
                                                 m0 + vrow[i] < p.m ? vor[i] : kInv, sor, 0, 0);
    }
  };
  const unsigned lds_base = lds_addr(smem);
  const unsigned strip = lds_base + NST * SLOT + wid * 4096;    // 32 rows x 128 bytes (fp32 x 32 columns), swizzled
  auto strip_off = [](int row, int quad) { return row * 128 + ((quad ^ (row & 7)) << 4); };

  // one tile: `after` = VMEM instructions this thread issued after the DMA of tile j (all of them may stay in flight)
  auto tile = [&](int j, int slot, int fill, auto after_tag) {
    constexpr int AFTER = decltype(after_tag)::value;
    wait_vmcnt<AFTER>();
    __builtin_amdgcn_s_barrier();            // tile j visible to all waves; every wave is done with tile j-1's slot
    asm volatile("" ::: "memory");
    stage(j + NST - 1, fill);
    const unsigned sa = lds_base + slot * SLOT;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // A fragments in batches of 2 (raw LDS reads, see lds_read16_raw): batch b+1 is in flight under batch b's MFMAs
    constexpr int FB = 2, NB = KS / FB;
    static_assert(KS % FB == 0, "fragment batches");
    raw_u32x4_t af[2][FB];
#pragma unroll
    for (int f = 0; f < FB; ++f) af[0][f] = lds_read16_raw(sa + sq_off(l31, f * 2 + hi));
#pragma unroll
    for (int bt = 0; bt < NB; ++bt) {
      if (bt + 1 < NB) {
#pragma unroll
        for (int f = 0; f < FB; ++f) af[(bt + 1) & 1][f] = lds_read16_raw(sa + sq_off(l31, ((bt + 1) * FB + f) * 2 + hi));
        lds_wait<FB>();
      } else {
        lds_wait<0>();
      }
#pragma unroll
      for (int f = 0; f < FB; ++f) {
        const raw_u32x4_t a4 = af[bt & 1][f];
        acc = Cvt<Tag>::mfma32(wf[bt * FB + f], make_uint4(a4.x, a4.y, a4.z, a4.w), acc);
      }
    }
    // epilogue of the wave's 32 x 32 block: transpose through the strip, 4 passes of 8 rows x 64 bytes.
    // The raw ds_write is invisible to hipcc's hazard recogniser: the MFMA results need their 18 wait states by hand.
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int g = 0; g < 4; ++g)
      lds_write16_raw(strip + strip_off(l31, 2 * g + hi), acc[g * 4], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]);
    const int m0 = ((int)blockIdx.x + j * (int)gridDim.x) * SQ_ROWS;
    raw_u32x4_t tq[4];
    raw_u32x2_t rq[4];
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int r = pass * 8 + rr_;
      tq[pass] = lds_read16_raw(strip + strip_off(r, qq));
      rq[pass] = (raw_u32x2_t){0u, 0u};
      if constexpr (HAS_RES) rq[pass] = lds_read8_raw(sa + SQ_TILE_BYTES + sq_off(r, gn >> 3) + (gn & 7) * 2);
    }
    lds_wait<0>();
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int r = pass * 8 + rr_;
      const float t4[4] = {__uint_as_float(tq[pass].x), __uint_as_float(tq[pass].y), __uint_as_float(tq[pass].z), __uint_as_float(tq[pass].w)};
      float v[4], r4[4];
      unpack4<Tag>(make_uint2(rq[pass].x, rq[pass].y), r4);
      const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
      const int gm = m0 + r;
      float rv[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (HAS_RV) {
        const bool second = rv_parity ? (gm & 1) != 0 : gm >= p.rowvec_rows;
        const float4 f = second ? rv1 : rv0;
        rv[0] = f.x; rv[1] = f.y; rv[2] = f.z; rv[3] = f.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = alpha * r4[e] + one_m_alpha * ((t4[e] + bb[e]) * p.acc_scale + rv[e] + r4[e]);
      st64(r_out, gm < p.m ? (int)(((long)gm * p.ldo + gn) * 2) : kInv, pack2<Tag>(v[0], v[1]), pack2<Tag>(v[2], v[3]));
    }
  };

  // ---- ring: tiles 0 .. NST-2 in flight before the loop; iteration j waits for tile j and issues tile j+NST-1.
  // VMEM instructions per iteration after its wait: G loads + 4 stores, hence the counts below.
#pragma unroll
  for (int s = 0; s < NST - 1; ++s) stage(s, s);
  int slot = 0, fill = NST - 1;
  auto advance = [&]() { slot = slot + 1 == NST ? 0 : slot + 1; fill = fill + 1 == NST ? 0 : fill + 1; };
  int j = 0;
  // first NST-1 iterations: fewer instructions separate a tile's DMA from its use
  if (j < my_tiles) { tile(j, slot, fill, std::integral_constant<int, (NST - 2) * G>{}); advance(); ++j; }
  if (j < my_tiles) { tile(j, slot, fill, std::integral_constant<int, (NST - 3 > 0 ? NST - 3 : 0) * G + (G + 4)>{}); advance(); ++j; }
  if constexpr (NST > 3) {
    if (j < my_tiles) { tile(j, slot, fill, std::integral_constant<int, (NST - 4 > 0 ? NST - 4 : 0) * G + 2 * (G + 4)>{}); advance(); ++j; }
    if (j < my_tiles) { tile(j, slot, fill, std::integral_constant<int, (NST - 5 > 0 ? NST - 5 : 0) * G + 3 * (G + 4)>{}); advance(); ++j; }
  }
  for (; j < my_tiles; ++j) { tile(j, slot, fill, std::integral_constant<int, 4 + (NST - 2) * (G + 4)>{}); advance(); }
}

template <typename Tag, bool HAS_RES, bool HAS_RV>
void launch_sq320(const GemmP& p, hipStream_t st) {
  constexpr size_t lds = (size_t)(HAS_RES ? 3 * 2 * SQ_TILE_BYTES : 5 * SQ_TILE_BYTES) + SQ_WAVES * 4096;
  static_assert(lds <= 160 * 1024, "sq320 LDS");
  static unsigned long long attr_done = 0;
  tt_lds_opt_in((const void*)sq320_kernel<Tag, HAS_RES, HAS_RV>, (int)lds, &attr_done);
  const int ntiles = (p.m + SQ_ROWS - 1) / SQ_ROWS;
  hipLaunchKernelGGL((sq320_kernel<Tag, HAS_RES, HAS_RV>), dim3(ntiles < 256 ? ntiles : 256), dim3(SQ_NT), lds, st, p);
}
template <typename Tag>
void launch_sq320_tag(const GemmP& p, hipStream_t st) {
  const Sq320Inst i = sq320_inst(p.residual, p.rowvec);
  if (i.has_rv) launch_sq320<Tag, true, true>(p, st);
  else if (i.has_res) launch_sq320<Tag, true, false>(p, st);
  else launch_sq320<Tag, false, false>(p, st);
}

}  // namespace ttg
