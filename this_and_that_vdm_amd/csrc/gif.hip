// libttvdm: the device half of the GIF export (include/ttvdm.h): tt_color_hist -- exact 15-bit colour histograms with channel sums of
// uint8 NHWC frames -- and tt_palette_map -- every pixel's nearest palette entry, the frames' squared-error sums and the per-entry
// sums of a Lloyd step.  Integer arithmetic and integer atomics only: adds commute, every call gives the same bits.
#include "common.h"
#include "block_scan.h"

namespace {

constexpr int BINS = TT_GIF_BINS, BLOCK = TT_GIF_BLOCK, WAVES = BLOCK / 64;
constexpr int SLOTS = TT_GIF_HIST_SLOTS, SLOT_BITS = 11;
constexpr int HIST_RUN = 8192;                     // pixels a histogram workgroup aims to own: its flush is amortised over them
constexpr int PIX = 4;                             // pixels a lane of the map kernel holds while it walks the palette
constexpr int MAP_TILE = BLOCK * PIX;
constexpr unsigned EMPTY = 0xffffffffu;
static_assert(SLOTS == 1 << SLOT_BITS, "the slot hash keeps SLOT_BITS bits");
static_assert(sizeof(TtColorBin) == 16, "TtColorBin layout (include/ttvdm.h)");
static_assert((long long)TT_GIF_MAX_PIXELS * 255 <= 0xffffffffLL, "a channel sum of TT_GIF_MAX_PIXELS pixels fits uint32");
// LDS of color_hist_kernel: SLOTS x (4 + 16) B = 40 KB of the CU's 160 KB: four workgroups (16 waves) per CU.

// one pixel into the workgroup's private table, or straight into the histogram when another bin holds its slot
__device__ __forceinline__ void hist_add(unsigned* tag_s, unsigned* rec_s, unsigned* __restrict__ hist, unsigned r, unsigned g, unsigned b) {
  const unsigned bin = ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3);
  const unsigned slot = (bin * 0x9E3779B1u) >> (32 - SLOT_BITS);
  unsigned seen = tag_s[slot];
  if (seen == EMPTY) seen = atomicCAS(&tag_s[slot], EMPTY, bin);
  if (seen == EMPTY || seen == bin) {
    unsigned* rec = rec_s + slot * 4;
    atomicAdd(rec + 0, 1u);
    atomicAdd(rec + 1, r);
    atomicAdd(rec + 2, g);
    atomicAdd(rec + 3, b);
  } else {
    unsigned* rec = hist + bin * 4;
    atomicAdd(rec + 0, 1u);
    atomicAdd(rec + 1, r);
    atomicAdd(rec + 2, g);
    atomicAdd(rec + 3, b);
  }
}

// grid (runs, nhist): workgroup x of histogram y owns pixels [x per, (x + 1) per) of the `pixels` that histogram y covers
__global__ __launch_bounds__(BLOCK) void color_hist_kernel(const unsigned char* __restrict__ src, long long pixels, unsigned* __restrict__ hist) {
  __shared__ unsigned tag_s[SLOTS];
  __shared__ unsigned rec_s[SLOTS * 4];
  const int tid = threadIdx.x;
  for (int i = tid; i < SLOTS; i += BLOCK) tag_s[i] = EMPTY;
  for (int i = tid; i < SLOTS * 4; i += BLOCK) rec_s[i] = 0u;
  __syncthreads();
  const unsigned char* p = src + (long long)blockIdx.y * pixels * 3;
  unsigned* hh = hist + (long long)blockIdx.y * BINS * 4;
  const long long per = (pixels + gridDim.x - 1) / gridDim.x;
  const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < pixels ? p0 + per : pixels;
  if (p0 < p1) {
    // the first pixel at or after p0 whose address is 16-byte aligned: 3 k = -a (mod 16), and 3 * 11 = 1 (mod 16)
    const unsigned a = (unsigned)((uintptr_t)(p + 3 * p0) & 15);
    const int head = (int)((((16u - a) & 15u) * 11u) & 15u);
    const long long pa = p0 + head < p1 ? p0 + head : p1;
    const long long groups = (p1 - pa) / 16, pt = pa + groups * 16;
    for (long long i = p0 + tid; i < pa; i += BLOCK) hist_add(tag_s, rec_s, hh, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    for (long long g = tid; g < groups; g += BLOCK) {
      const uint4* q = (const uint4*)(p + 3 * (pa + 16 * g));
      const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
      const unsigned wd[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int e = 3 * j;
        hist_add(tag_s, rec_s, hh, (wd[e >> 2] >> (8 * (e & 3))) & 0xffu, (wd[(e + 1) >> 2] >> (8 * ((e + 1) & 3))) & 0xffu,
                 (wd[(e + 2) >> 2] >> (8 * ((e + 2) & 3))) & 0xffu);
      }
    }
    for (long long i = pt + tid; i < p1; i += BLOCK) hist_add(tag_s, rec_s, hh, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
  }
  __syncthreads();
  for (int s = tid; s < SLOTS; s += BLOCK) {
    const unsigned bin = tag_s[s];
    if (bin != EMPTY) {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(hh + bin * 4 + j, rec_s[s * 4 + j]);
    }
  }
}

struct PalCounts { unsigned char minus1[TT_GIF_MAX_PALETTES]; };     // ncolors - 1 per palette, as kernel arguments

// grid (runs, n): workgroup x of frame y walks the frame's tiles of MAP_TILE pixels x, x + runs, ...; lane t of a tile holds its pixels
// t, t + BLOCK, ..: a wave's loads and its index stores are runs of consecutive bytes
template <bool STATS>
__global__ __launch_bounds__(BLOCK) void palette_map_kernel(const unsigned char* __restrict__ src, long long hw, const unsigned* __restrict__ pal,
                                                            int per_frame, PalCounts nc, unsigned char* __restrict__ idx,
                                                            unsigned long long* __restrict__ sse, unsigned* __restrict__ stats) {
  __shared__ unsigned stat_s[STATS ? 1024 : 4];
  __shared__ unsigned long long red_s[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frame = blockIdx.y, pi = per_frame ? frame : 0;
  const int ncol = (int)nc.minus1[pi] + 1;
  const unsigned* __restrict__ pw = pal + pi * 192;              // 256 entries x 3 bytes = 192 dwords: uniform over the workgroup
  const unsigned char* __restrict__ fp = src + (long long)frame * hw * 3;
  unsigned char* __restrict__ fi = idx + (long long)frame * hw;
  if constexpr (STATS) {
    for (int i = tid; i < 1024; i += BLOCK) stat_s[i] = 0u;
    __syncthreads();
  }
  unsigned long long err = 0ull;
  for (long long base = (long long)blockIdx.x * MAP_TILE; base < hw; base += (long long)gridDim.x * MAP_TILE) {
    int r[PIX], g[PIX], b[PIX], best[PIX], bi[PIX];
#pragma unroll
    for (int q = 0; q < PIX; ++q) {
      const long long p = base + q * BLOCK + tid;
      const bool in = p < hw;
      r[q] = in ? (int)fp[3 * p] : 0;
      g[q] = in ? (int)fp[3 * p + 1] : 0;
      b[q] = in ? (int)fp[3 * p + 2] : 0;
      best[q] = 0x7fffffff;
      bi[q] = 0;
    }
    for (int k4 = 0; k4 < ncol; k4 += 4) {
      const int d3 = 3 * (k4 >> 2);
      const unsigned w0 = pw[d3], w1 = pw[d3 + 1], w2 = pw[d3 + 2];
      const int er[4] = {(int)(w0 & 0xffu), (int)(w0 >> 24), (int)((w1 >> 16) & 0xffu), (int)((w2 >> 8) & 0xffu)};
      const int eg[4] = {(int)((w0 >> 8) & 0xffu), (int)(w1 & 0xffu), (int)(w1 >> 24), (int)((w2 >> 16) & 0xffu)};
      const int eb[4] = {(int)((w0 >> 16) & 0xffu), (int)((w1 >> 8) & 0xffu), (int)(w2 & 0xffu), (int)(w2 >> 24)};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k4 + j < ncol) {                                     // uniform
#pragma unroll
          for (int q = 0; q < PIX; ++q) {
            const int dr = r[q] - er[j], dg = g[q] - eg[j], db = b[q] - eb[j];
            const int d = __mul24(dr, dr) + __mul24(dg, dg) + __mul24(db, db);      // |differences| <= 255: exact in 24 bits; d <= 3 * 255^2
            if (d < best[q]) { best[q] = d; bi[q] = k4 + j; }     // strictly smaller, k ascending: the lowest index keeps a tie
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < PIX; ++q) {
      const long long p = base + q * BLOCK + tid;
      if (p < hw) {
        fi[p] = (unsigned char)bi[q];
        err += (unsigned long long)best[q];
        if constexpr (STATS) {
          atomicAdd(&stat_s[bi[q] * 4 + 0], 1u);
          atomicAdd(&stat_s[bi[q] * 4 + 1], (unsigned)r[q]);
          atomicAdd(&stat_s[bi[q] * 4 + 2], (unsigned)g[q]);
          atomicAdd(&stat_s[bi[q] * 4 + 3], (unsigned)b[q]);
        }
      }
    }
  }
  err = wave_sum(err);
  if (lane == 0) red_s[wave] = err;
  __syncthreads();
  if (tid == 0) {
    unsigned long long v = red_s[0];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) v += red_s[wv];
    if (v) atomicAdd(sse + frame, v);
  }
  if constexpr (STATS) {
    for (int i = tid; i < 1024; i += BLOCK) {
      const unsigned v = stat_s[i];
      if (v) atomicAdd(stats + (long long)pi * 1024 + i, v);
    }
  }
}

}  // namespace

extern "C" int tt_color_hist(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t nhist, TtColorBin* hist, tt_stream_t stream) {
  if (!frames || !hist) TT_FAIL(TT_EINVAL, "tt_color_hist: null %s", !frames ? "frames" : "hist");
  if (n <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "tt_color_hist: empty problem (n = %d, h = %d, w = %d)", n, h, w);
  if (ch != 3) TT_FAIL(TT_EINVAL, "tt_color_hist: %d channels (RGB frames: 3)", ch);
  if (nhist != n && nhist != 1) TT_FAIL(TT_EINVAL, "tt_color_hist: %d histograms for %d frames (one per frame, or 1 over all)", nhist, n);
  if ((uintptr_t)hist & 15) TT_FAIL(TT_EINVAL, "tt_color_hist: hist is not 16-byte aligned");
  const long long pixels = (long long)h * w * (nhist == 1 ? n : 1);
  if (pixels > TT_GIF_MAX_PIXELS)
    TT_FAIL(TT_EUNSUPPORTED, "tt_color_hist: %lld pixels per histogram, a uint32 channel sum holds %d (TT_GIF_MAX_PIXELS)", pixels, TT_GIF_MAX_PIXELS);
  if (nhist > 65535) TT_FAIL(TT_EUNSUPPORTED, "tt_color_hist: %d histograms: more than one grid covers (65535)", nhist);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, (size_t)nhist * BINS * sizeof(TtColorBin), st) != hipSuccess) TT_FAIL(TT_ELAUNCH, "tt_color_hist: hipMemsetAsync failed");
  long long runs = (pixels + HIST_RUN - 1) / HIST_RUN;
  const long long cap = nhist >= 1024 ? 1 : 1024 / nhist;
  if (runs > cap) runs = cap;
  hipLaunchKernelGGL(color_hist_kernel, dim3((unsigned)runs, (unsigned)nhist), dim3(BLOCK), 0, st, (const unsigned char*)frames, pixels, (unsigned*)hist);
  TT_CHECK_LAUNCH("tt_color_hist");
  return TT_OK;
}

extern "C" int tt_palette_map(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, const void* palettes, int32_t npal,
                              const int32_t* ncolors, uint8_t* indices, uint64_t* sse, TtColorBin* stats, tt_stream_t stream) {
  if (!frames || !palettes || !ncolors || !indices || !sse)
    TT_FAIL(TT_EINVAL, "tt_palette_map: null %s", !frames ? "frames" : (!palettes ? "palettes" : (!ncolors ? "ncolors" : (!indices ? "indices" : "sse"))));
  if (n <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "tt_palette_map: empty problem (n = %d, h = %d, w = %d)", n, h, w);
  if (ch != 3) TT_FAIL(TT_EINVAL, "tt_palette_map: %d channels (RGB frames: 3)", ch);
  if (npal != n && npal != 1) TT_FAIL(TT_EINVAL, "tt_palette_map: %d palettes for %d frames (one per frame, or 1 for all)", npal, n);
  if (npal > TT_GIF_MAX_PALETTES) TT_FAIL(TT_EUNSUPPORTED, "tt_palette_map: %d palettes in one call, at most %d (TT_GIF_MAX_PALETTES)", npal, TT_GIF_MAX_PALETTES);
  if (n > 65535) TT_FAIL(TT_EUNSUPPORTED, "tt_palette_map: %d frames: more than one grid covers (65535)", n);
  PalCounts nc;
  for (int i = 0; i < TT_GIF_MAX_PALETTES; ++i) nc.minus1[i] = 0;
  for (int i = 0; i < npal; ++i) {
    if (ncolors[i] < 1 || ncolors[i] > 256) TT_FAIL(TT_EINVAL, "tt_palette_map: ncolors[%d] = %d (1 to 256)", i, ncolors[i]);
    nc.minus1[i] = (unsigned char)(ncolors[i] - 1);
  }
  if ((uintptr_t)palettes & 3) TT_FAIL(TT_EINVAL, "tt_palette_map: palettes is not 4-byte aligned");
  if ((uintptr_t)sse & 7) TT_FAIL(TT_EINVAL, "tt_palette_map: sse is not 8-byte aligned");
  if ((uintptr_t)stats & 15) TT_FAIL(TT_EINVAL, "tt_palette_map: stats is not 16-byte aligned");
  const long long hw = (long long)h * w, per_pal = hw * (npal == 1 ? n : 1);
  if (stats && per_pal > TT_GIF_MAX_PIXELS)
    TT_FAIL(TT_EUNSUPPORTED, "tt_palette_map: %lld pixels per palette, a uint32 channel sum of stats holds %d (TT_GIF_MAX_PIXELS)", per_pal, TT_GIF_MAX_PIXELS);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sse, 0, (size_t)n * sizeof(uint64_t), st) != hipSuccess) TT_FAIL(TT_ELAUNCH, "tt_palette_map: hipMemsetAsync failed");
  if (stats && hipMemsetAsync(stats, 0, (size_t)npal * 256 * sizeof(TtColorBin), st) != hipSuccess)
    TT_FAIL(TT_ELAUNCH, "tt_palette_map: hipMemsetAsync failed");
  long long runs = (hw + MAP_TILE - 1) / MAP_TILE;
  if (stats) runs = (runs + 3) / 4;                              // a workgroup's 4 KB table is flushed once per four tiles at least
  const long long cap = n >= 2048 ? 1 : 2048 / n;
  if (runs > cap) runs = cap;
  const dim3 grid((unsigned)runs, (unsigned)n);
  if (stats)
    hipLaunchKernelGGL(palette_map_kernel<true>, grid, dim3(BLOCK), 0, st, (const unsigned char*)frames, hw, (const unsigned*)palettes, (int)(npal == n && n > 1),
                       nc, (unsigned char*)indices, (unsigned long long*)sse, (unsigned*)stats);
  else
    hipLaunchKernelGGL(palette_map_kernel<false>, grid, dim3(BLOCK), 0, st, (const unsigned char*)frames, hw, (const unsigned*)palettes,
                       (int)(npal == n && n > 1), nc, (unsigned char*)indices, (unsigned long long*)sse, (unsigned*)stats);
  TT_CHECK_LAUNCH("tt_palette_map");
  return TT_OK;
}
