// gemm_splitk.h -- the second pass of every split-K plan of tt_gemm (the tiled template's and gemm_w320h_kernel's): the fp32 slabs
// summed in a fixed order, then the full epilogue; with the GroupNorm tile sums, or with the GroupNorm itself.
#pragma once
#include "gemm_params.h"

namespace ttg {

// split-K second pass: sum the fp32 slabs in a fixed order (bit-reproducible) and run the normal epilogue
template <typename Tag>
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const GemmP p) {
  kernarg_touch<sizeof(GemmP)>();
  const long quads = (long)p.m * (p.n >> 2);
  const int nq = p.n >> 2;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
    const int gm = (int)(q / nq), gn = (int)(q - (long)gm * nq) * 4;
    const EpiOps<Tag> o = epi_load<Tag>(p, gm, gn);           // (requested with the slabs: one round trip)
    float4 a = *(const float4*)(p.ws + (long)gm * p.n + gn);
    for (int s2 = 1; s2 < p.splitk; ++s2) {
      const float4 b = *(const float4*)(p.ws + ((long)s2 * p.m + gm) * p.n + gn);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float v[4] = {a.x, a.y, a.z, a.w};
    epi_finish<Tag>(p, o, gm, gn, v);
  }
}

// ... the same with the GroupNorm tile sums of the output (GemmP.stats; the split-K routes of the two coarsest UNet levels): block (row tile of
// p.stat_rows rows, chunk of 32 columns), thread (column quad, one of 32 row lanes) walks its rows (one of a 28-row image, four of a 98- or
// 112-row tile), adds what it stores; the row lanes meet in LDS in a fixed order.  The caller picks the tile height (tt_gemm_stats_rows).
template <typename Tag>
__global__ __launch_bounds__(256) void splitk_epilogue_stats_kernel(const GemmP p) {
  __shared__ float red[32][8][8];
  kernarg_touch<sizeof(GemmP)>();
  const int R = p.stat_rows, rt = blockIdx.x, tid = threadIdx.x;
  const int qd = tid & 7, rl = tid >> 3;
  const int gn = (int)blockIdx.y * 32 + qd * 4;
  float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
  if (gn < p.n) {
    for (int r = rl; r < R; r += 32) {
      const int gm = rt * R + r;                              // < m: m is a multiple of R (tt_gemm_stats_rows)
      const EpiOps<Tag> o = epi_load<Tag>(p, gm, gn);
      float4 a = *(const float4*)(p.ws + (long)gm * p.n + gn);
      for (int s2 = 1; s2 < p.splitk; ++s2) {
        const float4 b = *(const float4*)(p.ws + ((long)s2 * p.m + gm) * p.n + gn);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      float v[4] = {a.x, a.y, a.z, a.w};
      epi_finish<Tag>(p, o, gm, gn, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float x = round_store<Tag>(v[e]); cs[e] += x; cq[e] = fmaf(x, x, cq[e]); }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[rl][qd][e] = cs[e]; red[rl][qd][4 + e] = cq[e]; }
  __syncthreads();
  if (tid < 64) {                                             // thread (column quad, one of its eight sums): the 32 row lanes in order
    const int q2 = tid >> 3, e = tid & 7, c = (int)blockIdx.y * 32 + q2 * 4 + (e & 3);
    if (c < p.n) {
      float t = red[0][q2][e];
#pragma unroll
      for (int l = 1; l < 32; ++l) t += red[l][q2][e];
      p.stats[((long)rt * 2 + (e >> 2)) * p.n + c] = t;
    }
  }
}
// ... and with the GroupNorm that reads the output (GemmP.gn_out; the coarsest UNet levels, where everything is bound by launches):
// block (segment of p.stat_rows rows = one image or the frames of a video, one of the 32 groups), thread (column quad of the group, row lane)
// finishes MAXR rows -- slabs summed in order, epilogue, `out` stored --, keeps the STORED values in registers, the block adds them up
// (fp64, fixed order: lanes by shuffle, waves through LDS), and every thread normalises what it holds.  One launch instead of the reduction
// and a GroupNorm launch; the normalised tensor is computed from the same rounded values and the same formula as tt_groupnorm_tiles
// (gn_group_stat, common.h -- without its conditioning guard: DESIGN.md 6.P).
// Row r of the segment belongs to lane r % rl_n, slot r / rl_n; the slab loads of all MAXR slots are issued before the first is used
// (slots beyond the segment re-read its last row and count for nothing: no branches around the loads).
template <typename Tag, int MAXR>
__global__ __launch_bounds__(1024) void splitk_epilogue_gn_kernel(const GemmP p, const int rl_n) {
  typedef typename Elem<Tag>::quad_t quad_t;
  constexpr int ES = Elem<Tag>::ES;
  __shared__ double wsum[16][2];
  __shared__ float s_stat[2];
  kernarg_touch<sizeof(GemmP)>();
  const int R = p.stat_rows, sg = blockIdx.x, grp = blockIdx.y, tid = threadIdx.x;
  const int cpg = p.n >> 5, nq = cpg >> 2;
  const int rl = tid / nq, qd = tid - rl * nq;
  const int gn = grp * cpg + qd * 4;
  const bool lane_ok = rl < rl_n;
  float x[MAXR][4];
  int gmr[MAXR];
  bool ok[MAXR];
  EpiOps<Tag> eo[MAXR];
  const float4 g4 = *(const float4*)(p.gn_gamma + gn), b4 = *(const float4*)(p.gn_beta + gn);
#pragma unroll
  for (int i = 0; i < MAXR; ++i) {
    const int r = rl + i * rl_n;
    ok[i] = lane_ok && r < R;
    gmr[i] = sg * R + (ok[i] ? r : R - 1);                    // < m: m is a multiple of R (tt_gemm_gn_fused)
    eo[i] = epi_load<Tag>(p, gmr[i], gn);
    const float4 a = *(const float4*)(p.ws + (long)gmr[i] * p.n + gn);
    x[i][0] = a.x; x[i][1] = a.y; x[i][2] = a.z; x[i][3] = a.w;
  }
  for (int s2 = 1; s2 < p.splitk; ++s2) {
#pragma unroll
    for (int i = 0; i < MAXR; ++i) {
      const float4 b = *(const float4*)(p.ws + ((long)s2 * p.m + gmr[i]) * p.n + gn);
      x[i][0] += b.x; x[i][1] += b.y; x[i][2] += b.z; x[i][3] += b.w;
    }
  }
  double cs = 0.0, cq = 0.0;
#pragma unroll
  for (int i = 0; i < MAXR; ++i) {
    if (ok[i]) {                                              // (the epilogue stores `out`)
      epi_finish<Tag>(p, eo[i], gmr[i], gn, x[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) { x[i][e] = round_store<Tag>(x[i][e]); cs += (double)x[i][e]; cq += (double)x[i][e] * (double)x[i][e]; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cs += __shfl_xor(cs, o); cq += __shfl_xor(cq, o); }
  if ((tid & 63) == 0) { wsum[tid >> 6][0] = cs; wsum[tid >> 6][1] = cq; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < (((int)blockDim.x + 63) >> 6); ++w) { a += wsum[w][0]; b += wsum[w][1]; }
    // (sums in fp64 from the first addition and no centred pass here: the guard's flag is not used, the ratio is a placeholder)
    (void)gn_group_stat(a, b, (double)R * cpg, p.gn_eps, 0.0, s_stat[0], s_stat[1]);
  }
  __syncthreads();
  const float mean = s_stat[0], rstd = s_stat[1];
  const float sc[4] = {rstd * g4.x, rstd * g4.y, rstd * g4.z, rstd * g4.w};
  const float sh[4] = {b4.x - mean * sc[0], b4.y - mean * sc[1], b4.z - mean * sc[2], b4.w - mean * sc[3]};
#pragma unroll
  for (int i = 0; i < MAXR; ++i) {
    if (ok[i]) {
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float t = fmaf(x[i][e], sc[e], sh[e]); y[e] = p.gn_silu ? silu_f(t) : t; }
      *(quad_t*)(p.gn_out + ((long)gmr[i] * p.ld_gn + gn) * ES) = f32_to_quad<Tag>(y);
    }
  }
}
// rows a thread of splitk_epilogue_gn_kernel holds for segments of `seg` rows: the smallest of 1, 2, 4, 8 with which (row lanes x column
// quads of a group) fit 1024 threads (0: the segment does not fit one block); *rl_n = row lanes
static inline int splitk_gn_rows(int seg, int n, int* rl_n) {
  const int nq = n / 128;                                   // column quads of one group (n / 32 channels)
  if (nq <= 0 || nq > 256 || seg <= 0) return 0;
  for (int mr = 1; mr <= 8; mr *= 2) {
    const int lanes = (seg + mr - 1) / mr;
    if ((long)lanes * nq <= 1024) { if (rl_n) *rl_n = lanes; return mr; }
  }
  return 0;
}
// second pass of a split-K launch (with or without the statistics)
template <typename Tag>
static inline void launch_splitk_epilogue(const GemmP& p, hipStream_t st) {
  if (p.gn_out) {
    int rl_n = 0;
    const int mr = splitk_gn_rows(p.stat_rows, p.n, &rl_n);
    const dim3 grid(p.m / p.stat_rows, 32), block((rl_n * (p.n / 128) + 63) / 64 * 64);
    if (mr == 1) hipLaunchKernelGGL((splitk_epilogue_gn_kernel<Tag, 1>), grid, block, 0, st, p, rl_n);
    else if (mr == 2) hipLaunchKernelGGL((splitk_epilogue_gn_kernel<Tag, 2>), grid, block, 0, st, p, rl_n);
    else if (mr == 4) hipLaunchKernelGGL((splitk_epilogue_gn_kernel<Tag, 4>), grid, block, 0, st, p, rl_n);
    else hipLaunchKernelGGL((splitk_epilogue_gn_kernel<Tag, 8>), grid, block, 0, st, p, rl_n);
    return;
  }
  if (p.stats) {
    hipLaunchKernelGGL(splitk_epilogue_stats_kernel<Tag>, dim3(p.m / p.stat_rows, (p.n + 31) / 32), dim3(256), 0, st, p);
    return;
  }
  long blocks = ((long)p.m * (p.n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(splitk_epilogue_kernel<Tag>, dim3((unsigned)blocks), dim3(256), 0, st, p);
}

}  // namespace ttg
