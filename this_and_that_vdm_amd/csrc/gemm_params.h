// gemm_params.h -- what every kernel family of tt_gemm shares: the launch-parameter struct GemmP, the bounds-checked buffer
// helpers of the epilogues, the per-quad epilogue (epi_load / epi_finish), the statistics strip, and each family's instance selector.
// Included by gemm.hip, gemm_pp.hip, gemm_w320.hip and conv_patch.hip directly and by the headers of the kernels (gemm_kernel.h:
// the tiled template, gemm_sq320.h, gemm_splitk.h).
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "common.h"

namespace ttg {



// Division by a launch-uniform divisor without the ~25-instruction software sequence (x2 for the remainder): the tiled template
// ran ~500 scalar instructions before its first load, most of them integer divisions, and the scalar unit is shared by all waves
// of a CU -- 16 waves x 500 instructions ~ 2.4 us of every launch (tools/gemm_timeline.py).
//   q = floor(n / d) = (n * mul) >> sh   for 0 <= n < 2^31, 1 <= d < 2^31,  mul = ceil(2^(31 + l) / d), sh = 31 + l, l = ceil(log2 d)
// (Granlund-Montgomery with N = 31: exact; mul <= 2^32 only for d = 1 ... handled: l = 0 -> mul = 2^31, sh = 31.)
struct FastDiv { unsigned mul, sh; };
static inline FastDiv make_fastdiv(long d_) {
  unsigned long long d = d_ < 1 ? 1 : (unsigned long long)d_;
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  FastDiv f;
  f.mul = (unsigned)(((1ull << (31 + l)) + d - 1) / d);
  f.sh = 31 + l;
  return f;
}
__device__ __forceinline__ int fdiv(int n, const FastDiv& f) { return (int)(((unsigned long long)(unsigned)n * f.mul) >> f.sh); }

struct GemmP {
  const char* a0; const char* a1;
  int k0, k1; long lda0, lda1;
  const char* w; long ldw;
  int m, n, mode;
  int nimg, hin, win, hout, wout, stride, upsample;
  int frames, hw;
  const float* bias; float acc_scale;
  const float* rowvec; int rowvec_rows; long ld_rowvec;
  int rowvec_mod;                   // > 0: row m takes rowvec[(m / rowvec_rows) % rowvec_mod] (TtGemmArgs.rowvec_mod)
  int geglu;
  const char* residual; long ld_res;
  const char* blend; long ld_blend; float alpha;
  char* out; long ldo; int out_f32;
  int out_col_hw, out_col_hwp;
  int nk0, nk1, taps, kt_total;     // derived: K steps per source, taps, total K steps
  int tiles_m, tiles_n;
  int group_m_override;             // > 0: host override (TT_GEMM_GROUP_M), else launch_cfg picks
  int group_m;                      // tile rows per group of the launch order (>= 1; see the tile mapping in gemm_kernel)
  unsigned a0_bytes, a1_bytes, w_bytes;   // extents for the buffer descriptors (< 2 GiB each)
  unsigned out_bytes, res_bytes, blend_bytes, bias_bytes, rowvec_bytes, ws_bytes;   // epilogue descriptors (0 = absent)
  int splitk;                       // > 1: block (tile, s) reduces K slice s and writes an fp32 slab to ws
  int slices;                       // blocks per tile, neighbours in the launch order: splitk, or the 4 phases of an upsample = 2 conv
  int phases;                       // 1: TtGemmArgs.upsample = 2 -- m / hout / wout describe the LOW-RES image (the tile domain); slice ph =
                                    // (py, px) walks taps 4 ph .. 4 ph + 3 of the phase-packed weight and owns output rows (2 y + py, 2 x + px)
  float* ws;                        // [splitk][m][n] fp32 partial sums
  int ln_fold; float ln_eps;        // fused LayerNorm of the A rows (1) / W rows (2): see gemm_kernel, MODE 3 / 4
  int out_fp8;                      // store e4m3 bytes (operands of the fp8 attention path) instead of 16-bit values
  float* stats;                     // != NULL: per (row tile, column) sum and sum of squares of the stored output (TtGemmArgs.stats_out)
  int stat_rows;                    // rows per statistics tile (tt_gemm_stats_rows); with gn_out: rows per GroupNorm segment
  char* gn_out; long ld_gn;         // != NULL: the split-K reduction also writes act(GroupNorm(out)) (TtGemmArgs.gn_out)
  const float* gn_gamma; const float* gn_beta; float gn_eps; int gn_silu;
  int f32_split;                    // TT_F32 only: products on the 16-bit matrix pipe as three split-fp16 terms (tt_gemm_set_f32_split)
  int presplit;                     // ... bit 0: a0 / a1, bit 1: w already hold the fp16 (h, l) pairs (TtGemmArgs.presplit)
  // launch-uniform divisors of the tiled template as multiply-shift pairs (fill_fastdivs, called by launch_cfg)
  FastDiv fd_splitk, fd_per_group, fd_group_m, fd_last_rows, fd_per_tap, fd_hwo, fd_wout, fd_hw, fd_frames, fd_rv_rows, fd_rv_mod;
};

// 4 floats -> 4 OCP e4m3 bytes (saturating at +-448: e4m3fn has no infinity, an overflow would become NaN)
__device__ __forceinline__ unsigned pack4_fp8(const float* v) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(v[0], -448.f, 448.f), __builtin_amdgcn_fmed3f(v[1], -448.f, 448.f), w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(v[2], -448.f, 448.f), __builtin_amdgcn_fmed3f(v[3], -448.f, 448.f), w, true);
  return (unsigned)w;
}
__device__ __forceinline__ void st32(__amdgpu_buffer_rsrc_t r, int off, unsigned a) {
  __builtin_amdgcn_raw_buffer_store_b32(a, r, off, 0, 0);
}

// ---- GroupNorm statistics of the OUTPUT, gathered beside the epilogue (GemmP.stats).  The epilogue passes a 32-row x 64 (32)
// column chunk through the wave's LDS strip; with statistics on, every lane writes the values it STORES (rounded to the storage type,
// as fp32) back into the strip slot it just read, and after the chunk's passes lane c adds up column c of the strip -- 32 rows, fixed
// order, two live registers (a version that kept 8 running sums per lane through the passes spilled 10-17 registers next to the 160
// accumulators of gemm_w320).  The wave's column sums go to its staging rows in LDS (plain store for the wave's first fragment row,
// read-add-store by the same lane for the following ones); the tile-level step then adds the waves of one tile column in a fixed order:
//   stats[(tile_m * 2 + 0) * n + col] = sum,  stats[(tile_m * 2 + 1) * n + col] = sum of squares     (fp32, one row tile = BM rows)
// No atomics: graph replays and eager launches stay bit-identical.
__device__ __forceinline__ void colstat_strip(const char* ebuf, int q_per_row, int lane, float* srow_sum, float* srow_sq, bool first) {
  if (lane < q_per_row * 4) {                                // one lane per column of the chunk
    const int quad = lane >> 2, e4 = (lane & 3) * 4;
    float a = 0.f, b = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      const float x = *(const float*)(ebuf + r * 256 + ((quad ^ (r & (q_per_row - 1))) << 4) + e4);      // strip_off(r, quad, q_per_row)
      a += x; b = fmaf(x, x, b);
    }
    if (!first) { a += srow_sum[lane]; b += srow_sq[lane]; }
    srow_sum[lane] = a; srow_sq[lane] = b;
  }
}

// ---- fused LayerNorm statistics: ln_stat (common.h) and its shifted form.
// fp32 storage (TT_F32, the mode that has to meet atol 1e-4 elementwise): sums of x - c with the pivot c = the row's first
// element, so E[(x-c)^2] - E[x-c]^2 does not cancel when |row mean| >> sigma (unshifted, the fp32 sums cost 6e-5 of the
// output at 5 sigma and 5e-3 at 50 sigma; shifted ~1e-6 at any mean).  The 16-bit types keep the packed dot products:
// their storage rounding (1e-3 / 8e-3) covers the one-pass error up to 50 sigma (tests/test_ops_gpu.py).
__device__ __forceinline__ void ln_stat_shifted(const raw_u32x4_t& f, float c, float& s, float& q) {
  const unsigned w[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
  for (int d = 0; d < 4; ++d) { const float x = __uint_as_float(w[d]) - c; s += x; q = fmaf(x, x, q); }
}


// ---- optional per-block timeline (make timeline): thread 0 of every block stamps the 100 MHz wall clock
#ifdef TT_GEMM_TIMELINE
static __device__ long long g_tl[8 * 8192];
#define TL(i) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_tl[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define TL(i) do { } while (0)
#endif

// ---- branch-free global access for the epilogue: 128-bit buffer descriptors with hardware bounds checking.  An
// offset of kInv (>= num_records) makes a load return 0 and drops a store, so ragged rows/columns and absent operands
// (null base, 0 records) need no exec-masked branch -- with branches hipcc serialises every pass behind
// `s_waitcnt vmcnt(0)` and the epilogue of one tile costs 4-8 us; straight-line it is ~1 us.
constexpr int kInv = (int)0x80000000;
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* ptr, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint2 ld64(__amdgpu_buffer_rsrc_t r, int off) {
  const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ float4 ld128f(__amdgpu_buffer_rsrc_t r, int off) {
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void st64(__amdgpu_buffer_rsrc_t r, int off, unsigned a, unsigned b) {
  __builtin_amdgcn_raw_buffer_store_b64((u32x2_t){a, b}, r, off, 0, 0);
}
__device__ __forceinline__ void st128f(__amdgpu_buffer_rsrc_t r, int off, float4 v) {
  __builtin_amdgcn_raw_buffer_store_b128((u32x4_t){__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}, r, off, 0, 0);
}
// 4 consecutive elements of the tag's storage type (8 bytes for the 16-bit tags, 16 for f32_tag)
template <typename Tag> __device__ __forceinline__ typename Elem<Tag>::quad_t ldq(__amdgpu_buffer_rsrc_t r, int off) { return ld64(r, off); }
template <> __device__ __forceinline__ uint4 ldq<f32_tag>(__amdgpu_buffer_rsrc_t r, int off) {
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}
template <typename Tag> __device__ __forceinline__ void stq(__amdgpu_buffer_rsrc_t r, int off, const float* v) {
  st64(r, off, pack2<Tag>(v[0], v[1]), pack2<Tag>(v[2], v[3]));
}
template <> __device__ __forceinline__ void stq<f32_tag>(__amdgpu_buffer_rsrc_t r, int off, const float* v) {
  st128f(r, off, make_float4(v[0], v[1], v[2], v[3]));
}
template <typename Tag> __device__ __forceinline__ typename Elem<Tag>::quad_t zero_quad();
template <> __device__ __forceinline__ uint2 zero_quad<bf16_tag>() { return make_uint2(0, 0); }
template <> __device__ __forceinline__ uint2 zero_quad<f16_tag>() { return make_uint2(0, 0); }
template <> __device__ __forceinline__ uint4 zero_quad<f32_tag>() { return make_uint4(0, 0, 0, 0); }

// ---- epilogue on 4 consecutive output columns (gn .. gn+3) of row gm, in two halves: epi_load requests the operands (bias, row vector,
// residual, blend), epi_finish does the arithmetic and stores.  The split-K reduction kernels request the operands of all their rows BEFORE
// they sum the slabs, so one memory round trip covers slabs and operands (epilogue_quad = both halves back to back: a round trip per operand).
template <typename Tag> struct EpiOps { float4 bias, rv; typename Elem<Tag>::quad_t res, bl; };
template <typename Tag>
__device__ __forceinline__ EpiOps<Tag> epi_load(const GemmP& p, int gm, int gn) {
  typedef typename Elem<Tag>::quad_t quad_t;
  constexpr int ES = Elem<Tag>::ES;
  EpiOps<Tag> o;
  o.bias = o.rv = make_float4(0.f, 0.f, 0.f, 0.f);
  o.res = o.bl = zero_quad<Tag>();
  if (p.bias) o.bias = *(const float4*)(p.bias + gn);
  if (p.rowvec) {
    int rg = gm / p.rowvec_rows;
    if (p.rowvec_mod > 0) rg %= p.rowvec_mod;
    o.rv = *(const float4*)(p.rowvec + (long)rg * p.ld_rowvec + gn);
  }
  if (p.residual) o.res = *(const quad_t*)(p.residual + ((long)gm * p.ld_res + gn) * ES);
  if (p.blend) o.bl = *(const quad_t*)(p.blend + ((long)gm * p.ld_blend + gn) * ES);
  return o;
}
template <typename Tag>
__device__ __forceinline__ void epi_finish(const GemmP& p, const EpiOps<Tag>& o, int gm, int gn, float (&v)[4]) {
  typedef typename Elem<Tag>::quad_t quad_t;
  constexpr int ES = Elem<Tag>::ES;
  if (p.bias) { v[0] += o.bias.x; v[1] += o.bias.y; v[2] += o.bias.z; v[3] += o.bias.w; }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= p.acc_scale;
  if (p.rowvec) { v[0] += o.rv.x; v[1] += o.rv.y; v[2] += o.rv.z; v[3] += o.rv.w; }
  if (p.residual) {
    float r4[4];
    quad_to_f32<Tag>(o.res, r4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += r4[e];
  }
  if (p.blend) {
    float r4[4];
    quad_to_f32<Tag>(o.bl, r4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = p.alpha * r4[e] + (1.0f - p.alpha) * v[e];
  }
  if (p.out_fp8) {
    if (p.out_col_hw > 0) {
      const unsigned w = pack4_fp8(v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = gn + e;
        const long oc = (long)(c / p.out_col_hw) * p.out_col_hwp + (c % p.out_col_hw);
        *(unsigned char*)(p.out + (long)gm * p.ldo + oc) = (unsigned char)(w >> (8 * e));
      }
    } else {
      *(unsigned*)(p.out + (long)gm * p.ldo + gn) = pack4_fp8(v);
    }
  } else if (p.out_f32) {
    *(float4*)(p.out + ((long)gm * p.ldo + gn) * 4) = make_float4(v[0], v[1], v[2], v[3]);
  } else if (p.out_col_hw > 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = gn + e;
      const long oc = (long)(c / p.out_col_hw) * p.out_col_hwp + (c % p.out_col_hw);
      store1<Tag>(p.out + ((long)gm * p.ldo + oc) * ES, v[e]);
    }
  } else {
    *(quad_t*)(p.out + ((long)gm * p.ldo + gn) * ES) = f32_to_quad<Tag>(v);
  }
}

template <typename Tag>
__device__ __forceinline__ void epilogue_quad(const GemmP& p, int gm, int gn, float (&v)[4]) {
  const EpiOps<Tag> o = epi_load<Tag>(p, gm, gn);
  epi_finish<Tag>(p, o, gm, gn, v);
}

template <int N> __device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// XCD-aware launch order: the dispatcher places block b on XCD b % 8; position `bid` of `n` is mapped so that every XCD gets a
// contiguous run of the n tiles (same A rows, neighbouring W columns: its private L2 sees the reuse; guide T1, bijective form).
__device__ __forceinline__ int xcd_remap(int bid, int n) {
  const int q = n >> 3, r = n & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// the instances of the streaming 320 x 320 kernel: a row vector only rides on the residual form (the output projections)
struct Sq320Inst { bool has_res, has_rv; };
inline Sq320Inst sq320_inst(const void* residual, const void* rowvec) { return Sq320Inst{residual || rowvec, rowvec != nullptr}; }
// ... of the persistent kernel (gemm_pp.hip) and of the two big-tile kernels (gemm_w320.hip: the fold only rides on the Linear gather)
struct PpInst { int lnrows, geglu; };
inline PpInst pp_inst(int ln_fold, int geglu) { return PpInst{ln_fold ? 1 : 0, geglu ? 1 : 0}; }
struct W320Inst { int mode, lnrows; };
inline W320Inst w320_inst(int mode, int ln_fold) { return mode == 1 || mode == 2 ? W320Inst{mode, 0} : W320Inst{0, ln_fold ? 1 : 0}; }

}  // namespace ttg
