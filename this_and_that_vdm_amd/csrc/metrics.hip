// libttvdm: tt_frame_metrics -- the sums behind MSE / PSNR / SSIM of two NHWC videos on the device -- and tt_frames_pool2, the 2 x 2 mean
// of the MS-SSIM pyramid (include/ttvdm.h).  frame_metrics_kernel: one workgroup per (frame, tile of TILE x TILE windows), all channels; the
// tile and its 10-pixel halo of both operands in LDS as fp32 (exact for both kinds), per channel a horizontal and a vertical pass in
// fp64, 12 partial sums per tile to the workspace.  frame_metrics_finalize_kernel (one workgroup per frame) adds them in tile order.
#include "common.h"
#include "block_scan.h"
#include <math.h>

// every fp64 operation below is rounded on its own: the header states the arithmetic operation by operation, and a == b must give
// ssim == 1.0 exactly (2 mab + C1 and (maa + mbb) + C1 are the same number only while neither is fused)
#pragma clang fp contract(off)

namespace {

constexpr int WIN = TT_METRICS_WIN, HALO = WIN - 1, TILE = TT_METRICS_TILE, BLOCK = TT_METRICS_BLOCK, WAVES = BLOCK / 64;
constexpr int REGION = TILE + HALO;                // rows / columns of pixels a tile's windows cover
constexpr int LW = REGION * 4;                     // fp32 per LDS row: REGION pixels of up to 4 channels, interleaved as in memory
constexpr int MOMENTS = 5;                         // a, b, a a, a b, b b
constexpr int PART = 12;                           // doubles per tile (and the first 12 words of a record): sse[4], ssim_sum[4], cs_sum[4]
constexpr int REC_WORDS = sizeof(TtFrameMetricsRecord) / 8;
static_assert(sizeof(TtFrameMetricsRecord) == 104 && REC_WORDS == PART + 1, "TtFrameMetricsRecord layout (include/ttvdm.h)");
static_assert(BLOCK == TILE * TILE, "the vertical pass gives every window of a tile its own lane");
// LDS: 2 operands x REGION x LW x 4 B = 21 632 B + MOMENTS x REGION x TILE x 8 B = 16 640 B + the reduction's 384 B: 38.7 KB of the
// CU's 160 KiB, so four workgroups (16 waves) stay resident per CU -- a 32 x 32 tile with fp64 rows would take 110 KB and leave one.

struct Window { double g[WIN]; };

// rows x cols pixels (ch channels, element size ES) whose first element is at p, row pitch `pitch` bytes -> s[r * LW + e] as fp32.
// Every aligned 16 bytes that lies inside a row's span is one vector load; what is left at the ends goes element by element.
template <int KIND>
__device__ __forceinline__ void load_region(const char* __restrict__ p, long long pitch, int rows, int cols, int ch, float* __restrict__ s) {
  constexpr int ES = KIND ? 1 : 4, EPV = 16 / ES;
  const int span = cols * ch * ES;                  // bytes of one row
  const int units = (span + 30) / 16;               // aligned 16-byte units a span can touch, whatever its alignment
  for (int i = threadIdx.x; i < rows * units; i += BLOCK) {
    const int r = i / units, u = i - r * units;
    const char* row = p + (long long)r * pitch;
    const long long first = -(long long)((uintptr_t)row & 15) + 16ll * u;        // byte offset of the unit within the span
    const int lo = (int)(first < 0 ? 0 : first), hi = (int)(first + 16 < span ? first + 16 : span);
    if (lo >= hi) continue;
    float* d = s + r * LW + lo / ES;
    if (hi - lo == 16) {
      const uint4 q = *(const uint4*)(row + lo);
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < EPV; ++j) {
        if constexpr (KIND) d[j] = (float)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
        else d[j] = __uint_as_float(w[j]);
      }
    } else {
      for (int b = lo; b < hi; b += ES) {
        if constexpr (KIND) d[b - lo] = (float)*(const unsigned char*)(row + b);
        else d[(b - lo) / 4] = *(const float*)(row + b);
      }
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(BLOCK) void frame_metrics_kernel(const char* __restrict__ a, const char* __restrict__ b, int h, int w, int ch, int ntx,
                                                              int nty, int sse_only, Window win, double c1, double c2, double* __restrict__ ws) {
  constexpr int ES = KIND ? 1 : 4;
  __shared__ float a_s[REGION * LW], b_s[REGION * LW];
  __shared__ double row_s[MOMENTS][REGION][TILE];
  __shared__ double part_s[WAVES][PART];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = ntx * nty;
  const long long frame = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)(frame * tiles), ty = tile / ntx, tx = tile - ty * ntx;
  const int y0 = ty * TILE, x0 = tx * TILE;
  const int rows = min(REGION, h - y0), cols = min(REGION, w - x0);            // pixels of the region that exist
  const long long pitch = (long long)w * ch * ES;
  const long long off = (frame * h + y0) * pitch + (long long)x0 * ch * ES;
  load_region<KIND>(a + off, pitch, rows, cols, ch, a_s);
  load_region<KIND>(b + off, pitch, rows, cols, ch, b_s);
  __syncthreads();

  double acc[PART];
#pragma unroll
  for (int i = 0; i < PART; ++i) acc[i] = 0.0;

  // ---- sse over the pixels this tile owns: its first TILE rows / columns, to the frame's edge for the last tile of an axis
  {
    const int orows = ty == nty - 1 ? rows : TILE, ocols = tx == ntx - 1 ? cols : TILE;
    unsigned isum[4] = {0u, 0u, 0u, 0u};
    for (int i = tid; i < orows * ocols; i += BLOCK) {
      const int r = i / ocols, x = i - r * ocols;
      const float* pa = a_s + r * LW + x * ch;
      const float* pb = b_s + r * LW + x * ch;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < ch) {
          if constexpr (KIND) {
            const int d = (int)pa[c] - (int)pb[c];
            isum[c] += (unsigned)(d * d);            // at most 3 pixels per lane: far below 2^32
          } else {
            const double d = (double)pa[c] - (double)pb[c];
            acc[c] += d * d;
          }
        }
      }
    }
    if constexpr (KIND) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = (double)isum[c];
    }
  }

  // ---- the windows: per channel, rows of the five moments (horizontal pass), then this lane's window (vertical pass)
  if (!sse_only) {
    const int nwy = min(TILE, h - HALO - y0), nwx = min(TILE, w - HALO - x0);  // windows of this tile
    const int vy = tid / TILE, vx = tid - vy * TILE;
    for (int c = 0; c < ch; ++c) {
      for (int i = tid; i < rows * TILE; i += BLOCK) {
        const int r = i / TILE, x = i - r * TILE;
        if (x < nwx) {
          const float* pa = a_s + r * LW + x * ch + c;
          const float* pb = b_s + r * LW + x * ch + c;
          double m[MOMENTS];
#pragma unroll
          for (int k = 0; k < WIN; ++k) {
            const double va = (double)pa[k * ch], vb = (double)pb[k * ch];
            const double v[MOMENTS] = {va, vb, va * va, va * vb, vb * vb};
#pragma unroll
            for (int j = 0; j < MOMENTS; ++j) {
              const double t = win.g[k] * v[j];
              m[j] = k == 0 ? t : m[j] + t;
            }
          }
#pragma unroll
          for (int j = 0; j < MOMENTS; ++j) row_s[j][r][x] = m[j];
        }
      }
      __syncthreads();
      if (vy < nwy && vx < nwx) {
        double m[MOMENTS];
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
#pragma unroll
          for (int j = 0; j < MOMENTS; ++j) {
            const double t = win.g[k] * row_s[j][vy + k][vx];
            m[j] = k == 0 ? t : m[j] + t;
          }
        }
        const double maa = m[0] * m[0], mbb = m[1] * m[1], mab = m[0] * m[1];
        const double saa = m[2] - maa, sbb = m[4] - mbb, sab = m[3] - mab;
        const double cs = (2.0 * sab + c2) / ((saa + sbb) + c2);
        const double ssim = ((2.0 * mab + c1) / ((maa + mbb) + c1)) * cs;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j == c) { acc[4 + j] += ssim; acc[8 + j] += cs; }
        }
      }
      __syncthreads();                               // row_s is the next channel's
    }
  }

  // ---- lanes -> wave (shuffles), waves -> workgroup (LDS, in wave order): a fixed shape
#pragma unroll
  for (int i = 0; i < PART; ++i) {
    const double v = wave_sum(acc[i]);
    if (lane == 0) part_s[wave][i] = v;
  }
  __syncthreads();
  if (tid < PART) {
    double v = part_s[0][tid];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) v += part_s[wv][tid];
    ws[(long long)blockIdx.x * PART + tid] = v;
  }
}

// one workgroup per frame: word i of the record = the tiles' words i added in tile order.  The partials travel through LDS a chunk at
// a time (all lanes load, coalesced); lanes 0 .. 11 add.
constexpr int FIN_CHUNK = 128;
__global__ __launch_bounds__(BLOCK) void frame_metrics_finalize_kernel(const double* __restrict__ ws, int tiles, long long count,
                                                                       double* __restrict__ rec) {
  __shared__ double chunk_s[FIN_CHUNK * PART];
  const int tid = threadIdx.x;
  const double* p = ws + (long long)blockIdx.x * tiles * PART;
  double v = 0.0;
  for (int t0 = 0; t0 < tiles; t0 += FIN_CHUNK) {
    const int nt = min(FIN_CHUNK, tiles - t0);
    for (int i = tid; i < nt * PART; i += BLOCK) chunk_s[i] = p[(long long)t0 * PART + i];
    __syncthreads();
    if (tid < PART)
      for (int t = 0; t < nt; ++t) v += chunk_s[t * PART + tid];
    __syncthreads();
  }
  double* r = rec + (long long)blockIdx.x * REC_WORDS;
  if (tid < PART) r[tid] = v;
  if (tid == PART) ((long long*)r)[PART] = count;
}

template <int KIND>
__global__ __launch_bounds__(256) void frames_pool2_kernel(const char* __restrict__ src, float* __restrict__ dst, long long total, int ho, int wo,
                                                           int ch) {
  const long long stride = (long long)gridDim.x * 256, wc = 2ll * wo * ch;     // wc: elements of one source row
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int c = (int)(i % ch);
    long long t = i / ch;
    const int x = (int)(t % wo);
    t /= wo;                                         // t = f * ho + y: source row 2 t
    const long long e = (2 * t * (2ll * wo) + 2 * x) * ch + c;
    float x00, x01, x10, x11;
    if constexpr (KIND) {
      const unsigned char* s = (const unsigned char*)src;
      x00 = (float)s[e]; x01 = (float)s[e + ch]; x10 = (float)s[e + wc]; x11 = (float)s[e + wc + ch];
    } else {
      const float* s = (const float*)src;
      x00 = s[e]; x01 = s[e + ch]; x10 = s[e + wc]; x11 = s[e + wc + ch];
    }
    dst[i] = 0.25f * ((x00 + x01) + (x10 + x11));
  }
}

void window(double* g) {
  double s = 0.0;
  for (int k = 0; k < WIN; ++k) {
    const double d = (double)(k - WIN / 2);
    g[k] = exp(-(d * d) / 4.5);
    s += g[k];
  }
  for (int k = 0; k < WIN; ++k) g[k] /= s;
}

// tiles along an axis of `len` pixels: its windows in runs of TILE; an axis without a window (SSE only) is one tile
long long tiles_of(int len) { return len > HALO ? ((long long)(len - HALO) + TILE - 1) / TILE : 1; }

}  // namespace

extern "C" int tt_frame_metrics_window(double* g) {
  if (!g) TT_FAIL(TT_EINVAL, "tt_frame_metrics_window: null output");
  window(g);
  return TT_OK;
}

extern "C" int tt_frame_metrics_launch(int32_t kind, int32_t* tile, int32_t* block, int32_t* elems_per_load) {
  if (kind != 0 && kind != 1) TT_FAIL(TT_EINVAL, "tt_frame_metrics_launch: kind %d (0 fp32, 1 uint8)", kind);
  if (!tile || !block || !elems_per_load) TT_FAIL(TT_EINVAL, "tt_frame_metrics_launch: null output");
  *tile = TILE;
  *block = BLOCK;
  *elems_per_load = kind ? 16 : 4;
  return TT_OK;
}

extern "C" int64_t tt_frame_metrics_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t flags) {
  if (n <= 0 || h <= 0 || w <= 0 || (flags & ~TT_METRICS_SSE_ONLY)) return 0;
  if (!(flags & TT_METRICS_SSE_ONLY) && (h < WIN || w < WIN)) return 0;
  const long long tiles = tiles_of(h) * tiles_of(w);
  if (tiles * n > 0x7fffffffLL) return 0;
  return tiles * n * PART * (long long)sizeof(double);
}

extern "C" int tt_frame_metrics(const void* a, const void* b, int32_t kind, int32_t n, int32_t h, int32_t w, int32_t ch, double data_range,
                                int32_t flags, TtFrameMetricsRecord* rec, void* ws, int64_t ws_bytes, tt_stream_t stream) {
  if (!a || !b || !rec) TT_FAIL(TT_EINVAL, "tt_frame_metrics: null %s", !a ? "a" : (!b ? "b" : "rec"));
  if (kind != 0 && kind != 1) TT_FAIL(TT_EINVAL, "tt_frame_metrics: kind %d (0 fp32, 1 uint8)", kind);
  if (n <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "tt_frame_metrics: empty problem (n = %d, h = %d, w = %d)", n, h, w);
  if (ch < 1 || ch > 4) TT_FAIL(TT_EINVAL, "tt_frame_metrics: %d channels (1 to 4)", ch);
  if (flags & ~TT_METRICS_SSE_ONLY) TT_FAIL(TT_EINVAL, "tt_frame_metrics: unknown flags 0x%x", (unsigned)flags);
  const int sse_only = flags & TT_METRICS_SSE_ONLY;
  if (!sse_only && (h < WIN || w < WIN))
    TT_FAIL(TT_EINVAL, "tt_frame_metrics: a %d x %d frame holds no %d x %d window (TT_METRICS_SSE_ONLY serves it)", h, w, WIN, WIN);
  if (!(data_range > 0.0) || !isfinite(data_range)) TT_FAIL(TT_EINVAL, "tt_frame_metrics: data_range = %g: positive and finite", data_range);
  if (!kind && (((uintptr_t)a | (uintptr_t)b) & 3)) TT_FAIL(TT_EINVAL, "tt_frame_metrics: a and b must be aligned to their 4-byte elements");
  if ((uintptr_t)rec & 7) TT_FAIL(TT_EINVAL, "tt_frame_metrics: rec is not 8-byte aligned");
  const long long ntx = tiles_of(w), nty = tiles_of(h), tiles = ntx * nty;
  if (tiles * n > 0x7fffffffLL) TT_FAIL(TT_EUNSUPPORTED, "tt_frame_metrics: %lld tiles x %d frames: more than one grid covers", tiles, n);
  const long long need = tiles * n * PART * (long long)sizeof(double);
  if (!ws || ws_bytes < need)
    TT_FAIL(TT_EINVAL, "tt_frame_metrics: workspace of %lld bytes, %lld needed (tt_frame_metrics_ws_bytes)", ws ? (long long)ws_bytes : 0ll, need);
  if ((uintptr_t)ws & 7) TT_FAIL(TT_EINVAL, "tt_frame_metrics: ws is not 8-byte aligned");
  Window win;
  window(win.g);
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  const long long count = sse_only ? 0 : (long long)(h - HALO) * (w - HALO);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(tiles * n));
  if (kind)
    hipLaunchKernelGGL(frame_metrics_kernel<1>, grid, dim3(BLOCK), 0, st, (const char*)a, (const char*)b, (int)h, (int)w, (int)ch, (int)ntx, (int)nty,
                       sse_only, win, c1, c2, (double*)ws);
  else
    hipLaunchKernelGGL(frame_metrics_kernel<0>, grid, dim3(BLOCK), 0, st, (const char*)a, (const char*)b, (int)h, (int)w, (int)ch, (int)ntx, (int)nty,
                       sse_only, win, c1, c2, (double*)ws);
  TT_CHECK_LAUNCH("tt_frame_metrics");
  hipLaunchKernelGGL(frame_metrics_finalize_kernel, dim3((unsigned)n), dim3(BLOCK), 0, st, (const double*)ws, (int)tiles, count, (double*)rec);
  TT_CHECK_LAUNCH("tt_frame_metrics");
  return TT_OK;
}

extern "C" int tt_frames_pool2(const void* src, int32_t kind, int32_t n, int32_t h, int32_t w, int32_t ch, float* dst, tt_stream_t stream) {
  if (!src || !dst) TT_FAIL(TT_EINVAL, "tt_frames_pool2: null %s", !src ? "src" : "dst");
  if (kind != 0 && kind != 1) TT_FAIL(TT_EINVAL, "tt_frames_pool2: kind %d (0 fp32, 1 uint8)", kind);
  if (n <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "tt_frames_pool2: empty problem (n = %d, h = %d, w = %d)", n, h, w);
  if ((h | w) & 1) TT_FAIL(TT_EINVAL, "tt_frames_pool2: a %d x %d frame: both sizes must be even", h, w);
  if (ch < 1 || ch > 4) TT_FAIL(TT_EINVAL, "tt_frames_pool2: %d channels (1 to 4)", ch);
  if (((uintptr_t)dst & 3) || (!kind && ((uintptr_t)src & 3))) TT_FAIL(TT_EINVAL, "tt_frames_pool2: fp32 operands must be 4-byte aligned");
  const int ho = h / 2, wo = w / 2;
  const long long total = (long long)n * ho * wo * ch;
  long long blocks = (total + 255) / 256;
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipStream_t st = (hipStream_t)stream;
  if (kind) hipLaunchKernelGGL(frames_pool2_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, (const char*)src, dst, total, ho, wo, (int)ch);
  else hipLaunchKernelGGL(frames_pool2_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, (const char*)src, dst, total, ho, wo, (int)ch);
  TT_CHECK_LAUNCH("tt_frames_pool2");
  return TT_OK;
}
