// GroupNorm (statistics -> per-(image,channel) affine -> apply+SiLU) and LayerNorm for token-major tensors.
// All statistics in fp32 with fp64 block/group combination (inputs reach |x| ~ 1e2 after sigma scaling); a group whose mean lies far
// from zero against its spread is recomputed centred, in fp64 (the conditioning guard: GN_GUARD_RATIO below).
#include "common.h"
#include <type_traits>

namespace {

constexpr int GN_GROUPS = 32;
// rows of one image a partial-statistics block covers: 8 per thread row-lane (two rounds of 4 loads in flight).  With a
// fixed 128 rows the wide levels (C = 1280: one row-lane per block) walked 128 rows serially and launched 28 blocks:
// 12 us per call whatever the tensor size.
__host__ __device__ inline int gn_rows_per_chunk(int C) {
  int rpb = 256 / (C >> 3);
  if (rpb < 1) rpb = 1;
  const int rows = rpb * 8;
  return rows > 128 ? 128 : rows;
}

// ---- the conditioning guard of every statistics route.  var = E[x^2] - mean^2 is formed from UNCENTRED sums whose lowest level is fp32:
// a thread's running sums over its rows in the statistics-pass kernels (n <= 8 .. 16 additions each), the producers' tile sums in
// gn_tiles_kernel (colstat_strip chains the 32 rows of a strip, the strips of a wave and the waves of a tile: n <= 256;
// splitk_epilogue_stats_kernel n <= 35).  Each such sum is off by up to n u of itself (u = 2^-24), typically sqrt(n) u / 2, and the fp64
// combination of P of them averages that to about sqrt(n / P) u / 2 of E[x^2] -- harmless against var while E[x^2] / var = 1 + rho^2
// (rho = |mean| / sigma) is small, but it is an error of (1 + rho^2) sqrt(n / P) u / 2 RELATIVE TO var, against the u rho that the
// rounding of mean and rstd to fp32 costs anyway.  The two meet near rho = 2 sqrt(P / n): P / n is 16 for the coarsest use (28 rows
// x 40 channels, one row per thread; 7 tiles of 256 rows x 10 channels), so beyond rho = 8 -- E[x^2] > GN_GUARD_RATIO var -- the
// block recomputes that group's statistics CENTRED on the uncentred mean, in fp64, from the rows (gn_centred_group).  A constant
// group (var = 0 up to the rounding of its sums, which then decides rstd against eps and leaves mean off by n u / 2 of itself) is the
// limit of that case.  The tile sums carry 16 to 32 times longer chains per sum than the per-thread sums, so their guard sits a
// factor 16 lower (rho > 1.7): GN_GUARD_RATIO_TILES.  Below the guard nothing changes, bit for bit.
constexpr double GN_GUARD_RATIO = 64.0, GN_GUARD_RATIO_TILES = 4.0;

// ---- the pieces the GroupNorm kernels are built from (which also names the two sites that keep their own form).  The
// arithmetic is written once, here or in gn_group_stat (common.h); the kernels differ in who owns which rows and channels and in how the
// partial sums meet.

// channel `ch` of the token-major tensor (x0 | x1): the address of its element in row `row0` of its source, and that source's row stride in bytes
struct GnSource { const char* p; long rstride; };
template <typename Tag>
__device__ __forceinline__ GnSource gn_source(const char* x0, int c0, const char* x1, int c1, int ch, long row0) {
  constexpr int ES = Elem<Tag>::ES;
  const char* base; long ld; int coff;
  if (ch < c0) { base = x0; ld = c0; coff = ch; } else { base = x1; ld = c1; coff = ch - c0; }
  return {base + (row0 * ld + coff) * ES, ld * ES};
}

// a thread's fp32 sums of x and x^2 of one 8-channel vector over the rows r_begin, r_begin + step, .. < r_end, stored to psum[0..8) /
// psq[0..8).  8 independent row loads per round (the statistics pass streams from HBM / L2), then a tail of single rows: the rows are
// added in ascending order either way, so the unroll changes the loads in flight and nothing in the result.
template <typename Tag>
__device__ __forceinline__ void gn_row_sums(const char* pbase, long rstride, int r_begin, int r_end, int step, float* psum, float* psq) {
  constexpr int INFLIGHT = 8;
  float s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
  int r = r_begin;
  for (; r + (INFLIGHT - 1) * step < r_end; r += INFLIGHT * step) {
    float f[INFLIGHT][8];
#pragma unroll
    for (int k = 0; k < INFLIGHT; ++k) load8<Tag>(pbase + (long)(r + k * step) * rstride, f[k]);
#pragma unroll
    for (int k = 0; k < INFLIGHT; ++k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += f[k][e]; q[e] = fmaf(f[k][e], f[k][e], q[e]); }
    }
  }
  for (; r < r_end; r += step) {
    float f[8];
    load8<Tag>(pbase + (long)r * rstride, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] += f[e]; q[e] = fmaf(f[e], f[e], q[e]); }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { psum[e] = s[e]; psq[e] = q[e]; }
}

// group g of a block's LDS partials psum / psq [rows][ld] (its channels: g * cpg ..) is summed in fp64 by the 32 lanes sl = 0 .. 31 of a
// half wave -- slices of its rows * cpg values --, then combined by a wave-level fixed-order tree (xor shuffles: the same association on
// every run, bit-reproducible).  Every lane of the half wave returns the group's sums.
__device__ __forceinline__ void gn_combine_group32(const float* psum, const float* psq, int rows, int ld, int cpg, int g, int sl, double& a, double& b) {
  a = 0.0; b = 0.0;
  const int n = rows * cpg;
  for (int i = sl; i < n; i += 32) {
    const int r = i / cpg, c = g * cpg + (i - r * cpg);
    a += (double)psum[r * ld + c]; b += (double)psq[r * ld + c];
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
}

// y = x * sc + sh with sc = rstd * gamma, sh = beta - mean * sc for the 8 channels ch .. ch + 7 of a thread; channel ch + e belongs to
// the group (ch_in_block + e) / cpg of the block's shared statistics
__device__ __forceinline__ void gn_affine8(const float* s_mean, const float* s_rstd, const float* gamma, const float* beta, int ch, int ch_in_block,
                                           int cpg, float* sc, float* sh) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int gg = (ch_in_block + e) / cpg;
    sc[e] = s_rstd[gg] * gamma[ch + e];
    sh[e] = beta[ch + e] - s_mean[gg] * sc[e];
  }
}

__device__ __forceinline__ void gn_apply8(float* f, const float* sc, const float* sh, int silu) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = fmaf(f[e], sc[e], sh[e]);
    f[e] = silu ? silu_f(t) : t;
  }
}
// ... over the rows r_begin, r_begin + step, .. < r_end of a thread's 8-channel vector: INFLIGHT rows loaded per round, then single rows
template <typename Tag, int INFLIGHT>
__device__ __forceinline__ void gn_apply_rows(const char* pbase, long rstride, char* ybase, long ystride, int r_begin, int r_end, int step,
                                              const float* sc, const float* sh, int silu) {
  int r = r_begin;
  if constexpr (INFLIGHT > 1) {
    for (; r + (INFLIGHT - 1) * step < r_end; r += INFLIGHT * step) {
      float f[INFLIGHT][8];
#pragma unroll
      for (int k = 0; k < INFLIGHT; ++k) load8<Tag>(pbase + (long)(r + k * step) * rstride, f[k]);
#pragma unroll
      for (int k = 0; k < INFLIGHT; ++k) {
        gn_apply8(f[k], sc, sh, silu);
        store8<Tag>(ybase + (long)(r + k * step) * ystride, f[k]);
      }
    }
  }
  for (; r < r_end; r += step) {
    float f[8];
    load8<Tag>(pbase + (long)r * rstride, f);
    gn_apply8(f, sc, sh, silu);
    store8<Tag>(ybase + (long)r * ystride, f);
  }
}

// centred statistics of channels [c_lo, c_lo + cpg) over `rows` rows from row `row0` of the token-major tensor (x0 | x1), by ALL
// threads of the block (call under block-uniform control flow): sums of x - pivot and (x - pivot)^2 in fp64 -- thread t takes
// one channel of the group and every (blockDim.x / cpg)-th row, lanes meet by xor shuffles, waves through red[32] in a fixed order
// (bit-reproducible).  Every thread returns the same mean and variance.
template <typename Tag>
__device__ __forceinline__ void gn_centred_group(const char* x0, int c0, const char* x1, int c1, long row0, int rows, int c_lo, int cpg,
                                                 float pivot, double* red, double& mean, double& var) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long n = (long)rows * cpg;
  double a = 0.0, b = 0.0;
  // thread = (channel of the group, row lane): consecutive lanes read the consecutive channels of a row, so a wave's load touches a
  // handful of cache lines, not one per lane; the thread's channel -- and with it its source -- is fixed, and eight rows are in flight
  const double pv = (double)pivot;
  const int rl_n = nthr / cpg, cl = tid % cpg, rl = tid / cpg;       // (cpg <= 256 <= blockDim.x)
  if (rl < rl_n) {
    const GnSource sx = gn_source<Tag>(x0, c0, x1, c1, c_lo + cl, 0);
    const long ld = sx.rstride;
    const char* src = sx.p + row0 * ld;
    int r = rl;
    for (; r + 7 * rl_n < rows; r += 8 * rl_n) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = load1<Tag>(src + (long)(r + k * rl_n) * ld);
#pragma unroll
      for (int k = 0; k < 8; ++k) { const double d = (double)v[k] - pv; a += d; b += d * d; }
    }
    for (; r < rows; r += rl_n) { const double d = (double)load1<Tag>(src + (long)r * ld) - pv; a += d; b += d * d; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
  __syncthreads();                                          // the previous call's readers are done with red
  if ((tid & 63) == 0) { red[(tid >> 6) * 2] = a; red[(tid >> 6) * 2 + 1] = b; }
  __syncthreads();
  double sa = 0.0, sb = 0.0;
  for (int w = 0; w < ((nthr + 63) >> 6); ++w) { sa += red[w * 2]; sb += red[w * 2 + 1]; }
  const double dm = sa / (double)n;
  mean = (double)pivot + dm;
  var = sb / (double)n - dm * dm;
  if (var < 0.0) var = 0.0;
}
// ... for the groups [0, ng) of a block whose s_redo flag is set (s_mean / s_rstd / s_redo: the block's shared statistics, indexed by the
// block's own group number; channels of group g: c_base + g * cpg)
template <typename Tag>
__device__ __forceinline__ void gn_redo_groups(const char* x0, int c0, const char* x1, int c1, long row0, int rows, int c_base, int cpg, int ng,
                                               float eps, float* s_mean, float* s_rstd, const int* s_redo, double* red) {
  for (int g = 0; g < ng; ++g) {
    if (!s_redo[g]) continue;                                // (shared: the same answer in every thread)
    double mean, var;
    gn_centred_group<Tag>(x0, c0, x1, c1, row0, rows, c_base + g * cpg, cpg, s_mean[g], red, mean, var);
    if (threadIdx.x == 0) { s_mean[g] = (float)mean; s_rstd[g] = (float)(1.0 / sqrt(var + (double)eps)); }    // (every thread read its pivot two barriers ago)
  }
  __syncthreads();
}

// partial sums per (image, row-chunk, group): ws[((img*chunks + chunk)*32 + g)*2 + {0,1}] (double)
template <typename Tag>
__global__ void gn_partial_kernel(const char* x0, int c0, const char* x1, int c1, int hw, int chunks, double* ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // per-(row-lane, channel) partial sums, reduced in a fixed order: results are bit-reproducible
  const int C = c0 + c1, cv = C >> 3;    // 8-channel vectors per row
  const int img = blockIdx.y, chunk = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int rpb = nthr / cv;             // rows handled in parallel
  float* psum = (float*)smem;            // [rpb][C]
  float* psq = psum + rpb * C;           // [rpb][C]
  const int myv = tid % cv, myr = tid / cv;
  const int rows_per_chunk = gn_rows_per_chunk(C);
  const int r0 = chunk * rows_per_chunk, r1 = min(hw, r0 + rows_per_chunk);
  // (this kernel keeps its own source selection and row loop, 4 loads in flight: through gn_source / gn_row_sums the fp32 instance needs
  // 65 to 67 VGPRs instead of 64 and loses a wave -- DESIGN.md 6.P)
  if (myr < rpb) {
    float s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
    const int ch = myv * 8;
    const char* base; long ld; int coff;
    if (ch < c0) { base = x0; ld = c0; coff = ch; } else { base = x1; ld = c1; coff = ch - c0; }
    constexpr int ES = Elem<Tag>::ES;
    const char* pbase = base + (((long)img * hw) * ld + coff) * ES;
    const long rstride = ld * ES;
    int r = r0 + myr;
    for (; r + 3 * rpb < r1; r += 4 * rpb) {
      float f[4][8];                 // 4 independent row loads in flight per thread (the kernel is a pure HBM stream)
#pragma unroll
      for (int k = 0; k < 4; ++k) load8<Tag>(pbase + (long)(r + k * rpb) * rstride, f[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] += f[k][e]; q[e] = fmaf(f[k][e], f[k][e], q[e]); }
      }
    }
    for (; r < r1; r += rpb) {
      float f[8];
      load8<Tag>(pbase + (long)r * rstride, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += f[e]; q[e] = fmaf(f[e], f[e], q[e]); }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { psum[myr * C + ch + e] = s[e]; psq[myr * C + ch + e] = q[e]; }
  }
  __syncthreads();
  if (tid < GN_GROUPS) {
    const int cpg = C / GN_GROUPS;
    double a = 0.0, b = 0.0;
    for (int r = 0; r < rpb; ++r)
      for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { a += (double)psum[r * C + c]; b += (double)psq[r * C + c]; }
    double* o = ws + (((long)img * chunks + chunk) * GN_GROUPS + tid) * 2;
    o[0] = a; o[1] = b;
  }
}

// one block per statistics group-set: (image-group ig) -> images [ig*fpg, (ig+1)*fpg).
// 1024 threads = 32 groups x 32 slices; each slice sums a strided subset of the (frame, chunk) partials, then the
// 32 slices are combined in a fixed order (deterministic).  (The cross-frame statistics of the temporal ResBlocks reduce
// frames x chunks ~ 500 partials in 2 blocks: the slice count is what bounds this kernel's latency.)
constexpr int GN_SLICES = 32;
template <typename Tag>
__global__ __launch_bounds__(1024) void gn_finalize_kernel(const double* ws, int chunks, int hw, int C, int fpg,
                                                          const float* gamma, const float* beta, float eps,
                                                          float* scale, float* shift, const char* x0, int c0, const char* x1, int c1) {
  __shared__ double s_a[GN_SLICES][GN_GROUPS], s_b[GN_SLICES][GN_GROUPS];
  __shared__ float s_mean[GN_GROUPS], s_rstd[GN_GROUPS];
  __shared__ int s_redo[GN_GROUPS];
  const int ig = blockIdx.x, tid = threadIdx.x;
  const int g = tid & 31, slice = tid >> 5;
  {
    double a = 0.0, b = 0.0;
    const int total = fpg * chunks;
    const double* base = ws + ((long)ig * fpg * chunks) * GN_GROUPS * 2;
    // this kernel is two blocks of pure latency in front of every temporal GroupNorm's apply pass: keep 8 partials (16-byte loads)
    // in flight per thread instead of one dependent round trip per partial; the summation order is unchanged
    int i = slice;
    for (; i + 7 * GN_SLICES < total; i += 8 * GN_SLICES) {
      double2 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = *(const double2*)(base + ((long)(i + k * GN_SLICES) * GN_GROUPS + g) * 2);
#pragma unroll
      for (int k = 0; k < 8; ++k) { a += v[k].x; b += v[k].y; }
    }
    for (; i < total; i += GN_SLICES) {
      const double2 v = *(const double2*)(base + ((long)i * GN_GROUPS + g) * 2);
      a += v.x; b += v.y;
    }
    s_a[slice][g] = a; s_b[slice][g] = b;
  }
  __syncthreads();
  if (tid < GN_GROUPS) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int s = 0; s < GN_SLICES; ++s) { a += s_a[s][tid]; b += s_b[s][tid]; }
    s_redo[tid] = gn_group_stat(a, b, (double)fpg * hw * (C / GN_GROUPS), eps, GN_GUARD_RATIO, s_mean[tid], s_rstd[tid]);
  }
  __syncthreads();
  const int cpg = C / GN_GROUPS;
  gn_redo_groups<Tag>(x0, c0, x1, c1, (long)ig * fpg * hw, fpg * hw, 0, cpg, GN_GROUPS, eps, s_mean, s_rstd, s_redo, &s_a[0][0]);
  for (int c = tid; c < C; c += blockDim.x) {
    const int gg = c / cpg;
    const float sc = s_rstd[gg] * gamma[c];
    const float sh = beta[c] - s_mean[gg] * sc;
    for (int f = 0; f < fpg; ++f) {
      scale[((long)ig * fpg + f) * C + c] = sc;
      shift[((long)ig * fpg + f) * C + c] = sh;
    }
  }
}

// Small images (at most GN_ONE_BYTES per image, per-image statistics): ONE kernel, one 1024-thread block per image -- the
// partial + finalize pair costs two dependent launches (~5 us each in the step graph) for tensors a single CU streams in a
// few microseconds.  Thread = (row lane, 8-channel vector); fp32 sums per thread over its rows (8 loads in flight), combined
// per group in fp64 in a fixed order (bit-reproducible), then scale/shift for every channel of the image.
constexpr long GN_ONE_BYTES = 640 * 1024;
// With y != nullptr the kernel also APPLIES the norm (tt_groupnorm_small): gridDim.y = S blocks per image, every one of them
// computes the image's statistics (the same fixed-order arithmetic: identical results; the S-fold re-read is served by L2) and
// then normalises + activates its own 1/S of the rows -- one launch instead of three for tensors whose GroupNorm is launch-bound.
template <typename Tag>
__global__ __launch_bounds__(1024) void gn_stats_image_kernel(const char* x0, int c0, const char* x1, int c1, int hw, int rpb,
                                                              const float* gamma, const float* beta, float eps,
                                                              float* scale, float* shift, char* y, long ldy, int silu) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  kernarg_touch<104>();
  __shared__ float s_mean[GN_GROUPS], s_rstd[GN_GROUPS];
  __shared__ int s_redo[GN_GROUPS];
  __shared__ double s_red[32];
  const int C = c0 + c1, cv = C >> 3;
  const int img = blockIdx.x, tid = threadIdx.x;
  float* psum = (float*)smem;            // [rpb][C]
  float* psq = psum + rpb * C;           // [rpb][C]
  const int myv = tid % cv, myr = tid / cv;
  if (myr < rpb) {
    const int ch = myv * 8;
    const GnSource sx = gn_source<Tag>(x0, c0, x1, c1, ch, (long)img * hw);
    gn_row_sums<Tag>(sx.p, sx.rstride, myr, hw, rpb, psum + myr * C + ch, psq + myr * C + ch);
  }
  __syncthreads();
  const int cpg = C / GN_GROUPS;
  {
    // group g <- the 32 lanes tid = g*32 .. g*32+31
    const int g = tid >> 5, sl = tid & 31;
    double a, b;
    gn_combine_group32(psum, psq, rpb, C, cpg, g, sl, a, b);
    if (sl == 0) s_redo[g] = gn_group_stat(a, b, (double)hw * cpg, eps, GN_GUARD_RATIO, s_mean[g], s_rstd[g]);
  }
  __syncthreads();
  gn_redo_groups<Tag>(x0, c0, x1, c1, (long)img * hw, hw, 0, cpg, GN_GROUPS, eps, s_mean, s_rstd, s_redo, s_red);
  if (y == nullptr) {
    for (int c = tid; c < C; c += 1024) {
      const int gg = c / cpg;
      const float sc = s_rstd[gg] * gamma[c];
      scale[(long)img * C + c] = sc;
      shift[(long)img * C + c] = beta[c] - s_mean[gg] * sc;
    }
    return;
  }
  if (myr < rpb) {
    const int ch = myv * 8;
    float sc[8], sh[8];
    gn_affine8(s_mean, s_rstd, gamma, beta, ch, ch, cpg, sc, sh);
    constexpr int ES = Elem<Tag>::ES;
    const GnSource sx = gn_source<Tag>(x0, c0, x1, c1, ch, (long)img * hw);
    char* ybase = y + (((long)img * hw) * ldy + ch) * ES;
    const int S = gridDim.y, part = blockIdx.y;
    const int r_lo = (int)((long)hw * part / S), r_hi = (int)((long)hw * (part + 1) / S);
    gn_apply_rows<Tag, 1>(sx.p, sx.rstride, ybase, ldy * ES, r_lo + myr, r_hi, rpb, sc, sh, silu);
  }
}

template <typename Tag>
__global__ void gn_apply_kernel(const char* x0, int c0, const char* x1, int c1, int hw, long total_vec,
                                const float* scale, const float* shift, int silu, char* y, long ldy) {
  const int C = c0 + c1, cv = C >> 3;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < total_vec; v += (long)gridDim.x * blockDim.x) {
    const long row = v / cv;
    const int ch = (int)(v - row * cv) * 8;
    const int img = (int)(row / hw);
    constexpr int ES = Elem<Tag>::ES;
    // (per row, in this form: through gn_source the address set-up differs and the kernel measured 2 % slower at 7168 rows -- DESIGN.md 6.P)
    const char* src = ch < c0 ? x0 + (row * c0 + ch) * ES : x1 + (row * c1 + (ch - c0)) * ES;
    float f[8];
    load8<Tag>(src, f);
    const float4 s0 = *(const float4*)(scale + (long)img * C + ch), s1 = *(const float4*)(scale + (long)img * C + ch + 4);
    const float4 h0 = *(const float4*)(shift + (long)img * C + ch), h1 = *(const float4*)(shift + (long)img * C + ch + 4);
    const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    gn_apply8(f, sc, sh, silu);
    store8<Tag>(y + (row * ldy + ch) * ES, f);
  }
}

// LayerNorm: one wave per row, values kept in registers (C <= 64*8*MAXV)
template <typename Tag, int MAXV>
__global__ __launch_bounds__(256) void ln_kernel(const char* x, long ldx, int rows, int c, const float* gamma,
                                                 const float* beta, float eps, const float* rowvec, int rows_per_vec,
                                                 int nvec, char* xsum, char* y, long ldy) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int cv = c >> 3;
  float v[MAXV][8];
  float s = 0.f;
  const float* rv = rowvec ? rowvec + (long)((row / rows_per_vec) % nvec) * c : nullptr;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = lane + i * 64;
    if (vi < cv) {
      load8<Tag>(x + ((long)row * ldx + vi * 8) * Elem<Tag>::ES, v[i]);
      if (rv) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = round_store<Tag>(v[i][e] + rv[vi * 8 + e]);   // normalise what xsum stores
        store8<Tag>(xsum + ((long)row * ldx + vi * 8) * Elem<Tag>::ES, v[i]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[i][e];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / c;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = lane + i * 64;
    if (vi < cv) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; q = fmaf(d, d, q); }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = rsqrtf(q / c + eps);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int vi = lane + i * 64;
    if (vi < cv) {
      float o8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o8[e] = (v[i][e] - mean) * rstd * gamma[vi * 8 + e] + beta[vi * 8 + e];
      store8<Tag>(y + ((long)row * ldy + vi * 8) * Elem<Tag>::ES, o8);
    }
  }
}


// ---- per-image GroupNorm of ANY size in one launch, without any exchange between blocks: the statistics of a group need only
// that group's channels, so block (image, slice) owns `gpb` consecutive groups = `nv` 8-channel vectors of every row: it sums
// them (fp32 per thread and channel, fp64 per group in a fixed order: bit-reproducible), then re-reads its slice -- still in L2 --
// normalises, activates and stores it.  x crosses HBM once in each direction; statistics, finalize and apply are one launch.
// The slices of one image go to ONE XCD (linear block L: XCD L % 8 runs images L % 8 + 8 k), whose L2 then serves the sectors
// that neighbouring slices share (a 10-channel group is 20 bytes: slices are not sector-aligned).
template <typename Tag>
__global__ __launch_bounds__(512) void gn_group_kernel(const char* x0, int c0, const char* x1, int c1, int nimg, int hw, int gpb, int nslices,
                                                       int rlanes, const float* gamma, const float* beta, float eps, int silu,
                                                       char* y, long ldy) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float s_mean[GN_GROUPS], s_rstd[GN_GROUPS];
  __shared__ int s_redo[GN_GROUPS];
  __shared__ double s_red[16];
  kernarg_touch<88>();
  const int C = c0 + c1, cpg = C / GN_GROUPS;
  const int L = blockIdx.x, xcd = L & 7, t = L >> 3;
  const int slice = t % nslices, img = xcd + 8 * (t / nslices);
  if (img >= nimg) return;
  const int nch = gpb * cpg, nv = nch >> 3, ch_lo = slice * nch;
  const int tid = threadIdx.x;
  const int myv = tid % nv, myr = tid / nv;                 // vector of the slice, row lane
  float* psum = (float*)smem;                               // [rlanes][nch]
  float* psq = psum + rlanes * nch;
  constexpr int ES = Elem<Tag>::ES;
  const int ch = ch_lo + myv * 8;
  const GnSource sx = gn_source<Tag>(x0, c0, x1, c1, ch, (long)img * hw);
  const char* pbase = sx.p;
  const long rstride = sx.rstride;
  if (myr < rlanes) gn_row_sums<Tag>(pbase, rstride, myr, hw, rlanes, psum + myr * nch + myv * 8, psq + myr * nch + myv * 8);
  __syncthreads();
  {
    // group g of the slice <- the 32 lanes tid = g*32 .. g*32+31
    const int g = tid >> 5, sl = tid & 31;
    if (g < gpb) {
      double a, b;
      gn_combine_group32(psum, psq, rlanes, nch, cpg, g, sl, a, b);
      if (sl == 0) s_redo[g] = gn_group_stat(a, b, (double)hw * cpg, eps, GN_GUARD_RATIO, s_mean[g], s_rstd[g]);
    }
  }
  __syncthreads();
  gn_redo_groups<Tag>(x0, c0, x1, c1, (long)img * hw, hw, ch_lo, cpg, gpb, eps, s_mean, s_rstd, s_redo, s_red);
  if (myr < rlanes) {
    float sc[8], sh[8];
    gn_affine8(s_mean, s_rstd, gamma, beta, ch, myv * 8, cpg, sc, sh);
    char* ybase = y + (((long)img * hw) * ldy + ch) * ES;
    gn_apply_rows<Tag, 4>(pbase, rstride, ybase, ldy * ES, myr, hw, rlanes, sc, sh, silu);
  }
}
// ---- GroupNorm from the PRODUCER's tile sums (tt_gemm stats_out; round 5): the conv / Linear launch that wrote x also left, per tile
// of R rows and per channel, the sum and the sum of squares of what it stored.  A segment (one image, or the frames x hw rows of one
// video for the temporal ResBlock's cross-frame statistics) is a whole number of tiles, so its statistics are a sum over seg_rows / R
// tile rows -- a few KB instead of a pass over the tensor.  Block (row part of a segment, slice of gpb groups): adds the tile sums of its
// channels (fp64, fixed order: bit-reproducible), folds channels into groups, then streams ITS rows once: normalise, activate, store.
// x crosses HBM once in each direction and there is one launch per GroupNorm, for per-image and cross-frame statistics alike
// (before: two passes in one launch, or three launches).  Slices of one row part go to ONE XCD, as in gn_group_kernel.
template <typename Tag>
__global__ __launch_bounds__(512) void gn_tiles_kernel(const char* x, int C, const float* stats, int R, int seg_rows, int nunits, int parts,
                                                       int gpb, int nslices, int rlanes, const float* gamma, const float* beta, float eps,
                                                       int silu, char* y, long ldy) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float s_mean[GN_GROUPS], s_rstd[GN_GROUPS];
  __shared__ int s_redo[GN_GROUPS];
  __shared__ double s_red[16];
  kernarg_touch<96>();
  const int cpg = C / GN_GROUPS;
  const int L = blockIdx.x, xcd = L & 7, t = L >> 3;
  const int slice = t % nslices, unit = xcd + 8 * (t / nslices);
  if (unit >= nunits) return;
  const int seg = unit / parts, part = unit - seg * parts;
  const int nch = gpb * cpg, nv = nch >> 3, ch_lo = slice * nch;
  const int tid = threadIdx.x;
  constexpr int ES = Elem<Tag>::ES;
  // ---- statistics: tile rows of this segment, channels of this slice.  Thread (channel c, lane kl of KL) adds tiles kl, kl + KL, ..
  double* pd = (double*)smem;                                // [KL][nch][2], then the channel totals in row 0
  const int T = seg_rows / R, KL = 512 / nch;
  {
    const int c = tid % nch, kl = tid / nch;
    if (kl < KL) {
      double a = 0.0, b = 0.0;
      const float* base = stats + ((long)seg * T * 2) * C + ch_lo + c;
      for (int k = kl; k < T; k += KL) { a += (double)base[(long)k * 2 * C]; b += (double)base[(long)k * 2 * C + C]; }
      pd[(kl * nch + c) * 2] = a; pd[(kl * nch + c) * 2 + 1] = b;
    }
  }
  __syncthreads();
  if (tid < nch) {
    double a = 0.0, b = 0.0;
    for (int kl = 0; kl < KL; ++kl) { a += pd[(kl * nch + tid) * 2]; b += pd[(kl * nch + tid) * 2 + 1]; }
    pd[tid * 2] = a; pd[tid * 2 + 1] = b;                    // (row 0 of the table: only thread `tid` read these two entries)
  }
  __syncthreads();
  if (tid < gpb) {
    double a = 0.0, b = 0.0;
    for (int c = 0; c < cpg; ++c) { a += pd[(tid * cpg + c) * 2]; b += pd[(tid * cpg + c) * 2 + 1]; }
    s_redo[tid] = gn_group_stat(a, b, (double)seg_rows * cpg, eps, GN_GUARD_RATIO_TILES, s_mean[tid], s_rstd[tid]);
  }
  __syncthreads();
  // (every row part of the segment recomputes a guarded group over the WHOLE segment: the same numbers in each of them; one source:
  // no channel is >= C, the second pointer is never read)
  gn_redo_groups<Tag>(x, C, x, 0, (long)seg * seg_rows, seg_rows, ch_lo, cpg, gpb, eps, s_mean, s_rstd, s_redo, s_red);
  // ---- apply: rows [r_lo, r_hi) of the segment, this slice's channels
  const int myv = tid % nv, myr = tid / nv;
  if (myr >= rlanes) return;
  const int ch = ch_lo + myv * 8;
  float sc[8], sh[8];
  gn_affine8(s_mean, s_rstd, gamma, beta, ch, myv * 8, cpg, sc, sh);
  const int per = (seg_rows + parts - 1) / parts, r_lo = part * per, r_hi = min(seg_rows, r_lo + per);
  const char* pbase = x + (((long)seg * seg_rows) * C + ch) * ES;
  char* ybase = y + (((long)seg * seg_rows) * ldy + ch) * ES;
  gn_apply_rows<Tag, 4>(pbase, (long)C * ES, ybase, ldy * ES, r_lo + myr, r_hi, rlanes, sc, sh, silu);
}

// groups per block: the smallest count whose channels fill whole 8-channel vectors, doubled towards 128-byte row slices while an
// image keeps at least 8 slices (16 x 28 x 1280: 80-byte slices 47 us, 160-byte slices 26 us).  0: the channel counts do not allow it (a source boundary inside a vector cannot happen: c0 is a multiple of 8).
// Independent of the image count, so tt_groupnorm_small_supported can answer for the launch.
static int gn_group_gpb(int C, int es) {
  const int cpg = C / GN_GROUPS;
  int gpb = 1;
  while ((gpb * cpg) & 7) gpb *= 2;                          // <= 8
  while (gpb * 2 <= 4 && gpb * cpg * es < 128) gpb *= 2;
  if (gpb > 16 || (gpb * cpg) >> 3 > 512) return 0;          // 32 lanes per group in the combination; one thread per vector at least
  return gpb;
}
// rows: below, the per-group combination of the row lanes' sums dominates a block that owns three rows per lane (measured: 112 x 2560
// 41 us against 26 us for the one-block-per-image kernel, 28 x 2560 23 vs 11); above, an image's 32 / gpb blocks walk too many rows
// each and the multi-launch route with its thousands of blocks streams better (64 x 112 x 320: 112 us against 84 us; 32 x 56 x 320:
// 26 against 29 -- the slices' 80..240-byte row segments reach ~2.5 TB/s, full rows 3 to 4.5)
constexpr int GN_GROUPED_MIN_ROWS = 256, GN_GROUPED_MAX_ROWS = 4096;
static int g_gn_grouped = -1;          // TT_GN_GROUPED=0: the round-2 routes (A/B)
static bool gn_grouped_on() {
  if (g_gn_grouped < 0) { const char* e = getenv("TT_GN_GROUPED"); g_gn_grouped = e ? atoi(e) : 1; }
  return g_gn_grouped != 0;
}
// the route decisions of tt_groupnorm_small / tt_groupnorm_stats, taken here for the launchers and for tt_groupnorm_route alike
static int gn_grouped_gpb(int hw, int c, int es) {          // groups per block of gn_group_kernel; 0: not its problem
  return gn_grouped_on() && hw >= GN_GROUPED_MIN_ROWS && hw <= GN_GROUPED_MAX_ROWS ? gn_group_gpb(c, es) : 0;
}
static bool gn_one_block_ok(int hw, int c, int es) { return (c >> 3) <= 1024 && (long)hw * c * es <= GN_ONE_BYTES; }

// the per-image kernel keeps [rpb][C] x 2 fp32 partials in dynamic LDS (at most 96 KiB): ONE opt-in (per device) with that maximum
constexpr int GN_IMAGE_LDS_MAX = 96 * 1024;
template <typename Tag> static void gn_image_opt_in() {
  static unsigned long long done = 0;
  tt_lds_opt_in((const void*)gn_stats_image_kernel<Tag>, GN_IMAGE_LDS_MAX, &done);
}
// ... and its row lanes: one per 8-channel vector of 1024 threads, fewer while the partials exceed that LDS, at most the image's rows
static int gn_small_rpb(int C, int hw) {
  const int cv = C >> 3;
  int rpb = 1024 / cv;
  while (rpb > 1 && (size_t)2 * rpb * C * sizeof(float) > GN_IMAGE_LDS_MAX) --rpb;
  if (rpb > hw) rpb = hw;
  return rpb;
}

// ---- storage types of this file's entry points: validity, element size, and the one dispatch from the run-time code to a kernel's
// tag -- f(tag) is called with a value of bf16_tag / f16_tag / f32_tag (`dtype` has passed dtype_ok)
static bool dtype_ok(int dtype) { return dtype == TT_BF16 || dtype == TT_F16 || dtype == TT_F32; }
static int es(int dtype) { return dtype == TT_F32 ? 4 : 2; }
template <typename F> static void by_dtype(int dtype, F&& f) {
  if (dtype == TT_BF16) f(bf16_tag{}); else if (dtype == TT_F16) f(f16_tag{}); else f(f32_tag{});
}

}  // namespace

extern "C" size_t tt_groupnorm_ws_bytes(int32_t nimg, int32_t hw, int32_t c) {
  if (c < 8) c = 8;
  const int rows = gn_rows_per_chunk(c);
  const long chunks = (hw + rows - 1) / rows;
  return (size_t)nimg * chunks * GN_GROUPS * 2 * sizeof(double);
}

extern "C" int tt_groupnorm_stats(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg, int32_t hw,
                                  int32_t fpg, const float* gamma, const float* beta, float eps, float* scale, float* shift,
                                  void* ws, size_t ws_bytes, int32_t dtype, tt_stream_t stream) {
  const int C = c0 + c1;
  if (!x0 || !gamma || !beta || !scale || !shift || !ws) TT_FAIL(TT_EINVAL, "tt_groupnorm_stats: null operand");
  if (c1 && !x1) TT_FAIL(TT_EINVAL, "tt_groupnorm_stats: c1 without x1");
  if (nimg <= 0 || hw <= 0 || C <= 0 || (C % GN_GROUPS) || (c0 & 7) || (c1 & 7)) TT_FAIL(TT_EINVAL, "tt_groupnorm_stats: C=%d+%d must be a multiple of 32, sources of 8", c0, c1);
  if (fpg <= 0 || nimg % fpg) TT_FAIL(TT_EINVAL, "tt_groupnorm_stats: frames_per_group %d does not divide %d images", fpg, nimg);
  if (ws_bytes < tt_groupnorm_ws_bytes(nimg, hw, C)) TT_FAIL(TT_EINVAL, "tt_groupnorm_stats: workspace too small");
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_groupnorm_stats: bad dtype");
  const int cv = C >> 3;
  if (cv > 1024) TT_FAIL(TT_EUNSUPPORTED, "tt_groupnorm_stats: C=%d too wide", C);
  const int rows_per_chunk = gn_rows_per_chunk(C);
  const int chunks = (hw + rows_per_chunk - 1) / rows_per_chunk;
  int rpb = 256 / cv; if (rpb < 1) rpb = 1;
  int threads = cv * rpb; if (threads < GN_GROUPS) threads = GN_GROUPS;
  threads = (threads + 63) / 64 * 64;
  hipStream_t st = (hipStream_t)stream;
  if (fpg == 1 && gn_one_block_ok(hw, C, es(dtype))) {
    const int rpb1 = gn_small_rpb(C, hw);
    const size_t lds1 = (size_t)2 * rpb1 * C * sizeof(float);     // [rpb][C] x 2 fp32 in LDS
    by_dtype(dtype, [&](auto tag) {
      using Tag = decltype(tag);
      gn_image_opt_in<Tag>();
      hipLaunchKernelGGL(gn_stats_image_kernel<Tag>, dim3(nimg), dim3(1024), lds1, st, (const char*)x0, c0, (const char*)x1, c1, hw, rpb1, gamma, beta, eps,
                         scale, shift, (char*)nullptr, 0L, 0);
    });
    TT_CHECK_LAUNCH("tt_groupnorm_stats");
    return TT_OK;
  }
  const size_t lds = (size_t)2 * rpb * C * sizeof(float);
  by_dtype(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    hipLaunchKernelGGL(gn_partial_kernel<Tag>, dim3(chunks, nimg), dim3(threads), lds, st, (const char*)x0, c0, (const char*)x1, c1, hw, chunks, (double*)ws);
    hipLaunchKernelGGL(gn_finalize_kernel<Tag>, dim3(nimg / fpg), dim3(32 * GN_SLICES), 0, st, (const double*)ws, chunks, hw, C, fpg, gamma, beta, eps,
                       scale, shift, (const char*)x0, c0, (const char*)x1, c1);
  });
  TT_CHECK_LAUNCH("tt_groupnorm_stats");
  return TT_OK;
}

// ---- statistics + apply in one launch for small images (see gn_stats_image_kernel)
extern "C" int tt_groupnorm_small_supported(int32_t hw, int32_t c, int32_t dtype) {
  if (hw <= 0 || c <= 0 || (c % GN_GROUPS) || (c & 7)) return 0;
  if (gn_grouped_gpb(hw, c, es(dtype)) > 0) return 1;      // one block per (image, group slice)
  return gn_one_block_ok(hw, c, es(dtype));
}
extern "C" int tt_groupnorm_route(int32_t hw, int32_t c, int32_t dtype, int32_t frames_per_group, int32_t one_launch) {
  if (hw <= 0 || c <= 0 || frames_per_group <= 0 || (c % GN_GROUPS) || (c & 7)) return 0;
  if (one_launch) {
    if (frames_per_group != 1) return 0;
    if (gn_grouped_gpb(hw, c, es(dtype)) > 0) return TT_GN_ROUTE_GROUPED;
    return gn_one_block_ok(hw, c, es(dtype)) ? TT_GN_ROUTE_IMAGE : 0;
  }
  return frames_per_group == 1 && gn_one_block_ok(hw, c, es(dtype)) ? TT_GN_ROUTE_IMAGE : TT_GN_ROUTE_PARTIAL;
}
extern "C" int tt_groupnorm_small(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg, int32_t hw,
                                  const float* gamma, const float* beta, float eps, int32_t silu, void* y, int64_t ldy,
                                  int32_t dtype, tt_stream_t stream) {
  const int C = c0 + c1;
  if (!x0 || !gamma || !beta || !y) TT_FAIL(TT_EINVAL, "tt_groupnorm_small: null operand");
  if (c1 && !x1) TT_FAIL(TT_EINVAL, "tt_groupnorm_small: c1 without x1");
  if (nimg <= 0 || (c0 & 7) || (c1 & 7) || (ldy & 7) || ldy < C) TT_FAIL(TT_EINVAL, "tt_groupnorm_small: channel counts/stride must be multiples of 8");
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_groupnorm_small: bad dtype");
  if (!tt_groupnorm_small_supported(hw, C, dtype))
    TT_FAIL(TT_EUNSUPPORTED, "tt_groupnorm_small: %d x %d per image is served by tt_groupnorm_stats + tt_groupnorm_apply", hw, C);
  hipStream_t st = (hipStream_t)stream;
  if (const int gpb = gn_grouped_gpb(hw, C, es(dtype))) {
    const int nslices = GN_GROUPS / gpb, nv = (gpb * (C / GN_GROUPS)) >> 3;
    int rlanes = 512 / nv;
    if (rlanes > hw) rlanes = hw;
    const size_t ldsg = (size_t)2 * rlanes * nv * 8 * sizeof(float);
    const int blocks = ((nimg + 7) / 8) * 8 * nslices;
    by_dtype(dtype, [&](auto tag) {
      hipLaunchKernelGGL(gn_group_kernel<decltype(tag)>, dim3(blocks), dim3(512), ldsg, st, (const char*)x0, c0, (const char*)x1, c1, nimg, hw, gpb, nslices,
                         rlanes, gamma, beta, eps, (int)silu, (char*)y, (long)ldy);
    });
    TT_CHECK_LAUNCH("tt_groupnorm_small");
    return TT_OK;
  }
  const int rpb = gn_small_rpb(C, hw);
  const size_t lds = (size_t)2 * rpb * C * sizeof(float);
  // blocks per image: enough to put the apply phase on ~4 x 28..56 CUs without re-reading the image too often
  int parts = 4;
  if (hw < parts * rpb) parts = hw / rpb > 0 ? hw / rpb : 1;
  by_dtype(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    gn_image_opt_in<Tag>();
    hipLaunchKernelGGL(gn_stats_image_kernel<Tag>, dim3(nimg, parts), dim3(1024), lds, st, (const char*)x0, c0, (const char*)x1, c1, hw, rpb,
                       gamma, beta, eps, (float*)nullptr, (float*)nullptr, (char*)y, (long)ldy, (int)silu);
  });
  TT_CHECK_LAUNCH("tt_groupnorm_small");
  return TT_OK;
}

extern "C" int tt_groupnorm_tiles_supported(int32_t seg_rows, int32_t c, int32_t stat_rows, int32_t dtype) {
  if (seg_rows <= 0 || c <= 0 || stat_rows <= 0 || (c % GN_GROUPS) || (c & 7) || seg_rows % stat_rows) return 0;
  return gn_group_gpb(c, es(dtype)) > 0 ? 1 : 0;
}
extern "C" int tt_groupnorm_tiles(const void* x, int32_t c, const float* stats, int32_t stat_rows, int32_t nseg, int32_t seg_rows,
                                  const float* gamma, const float* beta, float eps, int32_t silu, void* y, int64_t ldy, int32_t dtype,
                                  tt_stream_t stream) {
  if (!x || !stats || !gamma || !beta || !y) TT_FAIL(TT_EINVAL, "tt_groupnorm_tiles: null operand");
  if (nseg <= 0 || (ldy & 7) || ldy < c) TT_FAIL(TT_EINVAL, "tt_groupnorm_tiles: segments / output stride");
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_groupnorm_tiles: bad dtype");
  if (!tt_groupnorm_tiles_supported(seg_rows, c, stat_rows, dtype))
    TT_FAIL(TT_EUNSUPPORTED, "tt_groupnorm_tiles: %d rows per segment must be a multiple of the %d statistics rows, C = %d a multiple of 32", seg_rows, stat_rows, c);
  const int gpb = gn_group_gpb(c, es(dtype)), nslices = GN_GROUPS / gpb, nch = gpb * (c / GN_GROUPS), nv = nch >> 3;
  // row parts per segment: ~2 blocks per CU over the launch, at least 128 rows each
  int parts = (512 + nseg * nslices - 1) / (nseg * nslices);
  if (parts > seg_rows / 128) parts = seg_rows / 128;
  if (parts < 1) parts = 1;
  const int per = (seg_rows + parts - 1) / parts;
  int rlanes = 512 / nv;
  if (rlanes > per) rlanes = per;
  const int nunits = nseg * parts, blocks = ((nunits + 7) / 8) * 8 * nslices;
  const size_t lds = (size_t)(512 / nch) * nch * 2 * sizeof(double);
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(gn_tiles_kernel<decltype(tag)>, dim3(blocks), dim3(512), lds, st, (const char*)x, (int)c, stats, (int)stat_rows, (int)seg_rows,
                       nunits, parts, gpb, nslices, rlanes, gamma, beta, eps, (int)silu, (char*)y, (long)ldy);
  });
  TT_CHECK_LAUNCH("tt_groupnorm_tiles");
  return TT_OK;
}

extern "C" int tt_groupnorm_apply(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg, int32_t hw,
                                  const float* scale, const float* shift, int32_t silu, void* y, int64_t ldy, int32_t dtype,
                                  tt_stream_t stream) {
  const int C = c0 + c1;
  if (!x0 || !scale || !shift || !y) TT_FAIL(TT_EINVAL, "tt_groupnorm_apply: null operand");
  if (c1 && !x1) TT_FAIL(TT_EINVAL, "tt_groupnorm_apply: c1 without x1");
  if ((c0 & 7) || (c1 & 7) || (ldy & 7) || ldy < C) TT_FAIL(TT_EINVAL, "tt_groupnorm_apply: channel counts/stride must be multiples of 8");
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_groupnorm_apply: bad dtype");
  const long total = (long)nimg * hw * (C >> 3);
  long blocks = (total + 255) / 256; if (blocks > 4096) blocks = 4096;
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(gn_apply_kernel<decltype(tag)>, dim3((unsigned)blocks), dim3(256), 0, st, (const char*)x0, c0, (const char*)x1, c1, hw, total, scale, shift,
                       silu, (char*)y, (long)ldy);
  });
  TT_CHECK_LAUNCH("tt_groupnorm_apply");
  return TT_OK;
}

extern "C" int tt_layernorm(const void* x, int64_t ldx, int32_t rows, int32_t c, const float* gamma, const float* beta,
                            float eps, const float* rowvec, int32_t rows_per_vec, int32_t nvec, void* xsum_out, void* y,
                            int64_t ldy, int32_t dtype, tt_stream_t stream) {
  if (!x || !gamma || !beta || !y) TT_FAIL(TT_EINVAL, "tt_layernorm: null operand");
  if (rows <= 0 || c <= 0 || (c & 7) || (ldx & 7) || (ldy & 7)) TT_FAIL(TT_EINVAL, "tt_layernorm: c and strides must be multiples of 8");
  if (rowvec && (!xsum_out || rows_per_vec <= 0 || nvec <= 0)) TT_FAIL(TT_EINVAL, "tt_layernorm: rowvec needs xsum_out, rows_per_vec, nvec");
  if (c > 64 * 8 * 4) TT_FAIL(TT_EUNSUPPORTED, "tt_layernorm: c=%d > 2048", c);
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_layernorm: bad dtype");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((rows + 3) / 4), block(256);
  const int mv = (c / 8 + 63) / 64;
  by_dtype(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    auto launch = [&](auto maxv) {
      hipLaunchKernelGGL((ln_kernel<Tag, decltype(maxv)::value>), grid, block, 0, st, (const char*)x, (long)ldx, rows, c, gamma, beta, eps, rowvec, rows_per_vec,
                         nvec, (char*)xsum_out, (char*)y, (long)ldy);
    };
    if (mv <= 1) launch(std::integral_constant<int, 1>{}); else if (mv <= 2) launch(std::integral_constant<int, 2>{}); else launch(std::integral_constant<int, 4>{});
  });
  TT_CHECK_LAUNCH("tt_layernorm");
  return TT_OK;
}
