// The request path around the models: CLIP image preprocessing (tt_clip_image), the context LayerNorm of use_text requests
// (tt_layernorm_block), the export of decoded frames (tt_frames_out), the gesture maps from their points (tt_gesture_maps) and the request
// image itself: PIL's 8-bit resize and the VAE input (tt_resize_u8 / tt_vae_image).  None of it is in the denoise step; all of it is
// arithmetic on a few hundred thousand elements, written for being on the stream (no host round trip, no vendor conv library).
#include <math.h>

#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ tt_clip_image
constexpr int CLIP_MAX_TAPS = 63;
// Gaussian taps of one axis, normalised on the host in fp64 and rounded once to fp32; a kernel ARGUMENT (256 bytes by value): no
// device table to allocate or keep between calls, and a captured graph holds its own copy.
struct ClipTaps { float w[CLIP_MAX_TAPS + 1]; };

// what pipeline_utils.resize_with_antialiasing derives from one axis: f = in / out, sigma = max((f - 1) / 2, 1e-3),
// k = int(max(4 sigma, 3)) made odd -- the same double arithmetic as the Python
struct ClipAxis { int k; double sigma; };
ClipAxis clip_axis(int in, int out) {
  const double f = (double)in / (double)out;
  const double sigma = fmax((f - 1.0) / 2.0, 0.001);
  int k = (int)fmax(4.0 * sigma, 3.0);
  k += 1 - k % 2;
  return {k, sigma};
}
void clip_taps(const ClipAxis& ax, ClipTaps* t) {
  double e[CLIP_MAX_TAPS], s = 0.0;
  for (int i = 0; i < ax.k; ++i) { const double d = i - ax.k / 2; e[i] = exp(-d * d / (2.0 * ax.sigma * ax.sigma)); s += e[i]; }
  for (int i = 0; i <= CLIP_MAX_TAPS; ++i) t->w[i] = i < ax.k ? (float)(e[i] / s) : 0.f;
}

// index of a reflect-padded axis (no edge repeat): valid for -n < i < 2 n - 1, which the entry point guarantees (pad < n)
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// One blur pass over fp32 planes [planes, h, w]: out[p][y][x] = sum_t w[t] in[p][reflect(pos + t - k / 2)], pos along x (HORIZONTAL)
// or y.  The horizontal pass is the first one and reads the caller's image: SRC 0 uint8 [nimg, h, w, 3] (v = 2 (u / 255) - 1),
// SRC 1 fp32 [nimg, 3, h, w] in [0, 1] (v = 2 x - 1), SRC 2 the other pass's fp32 planes as they are.
template <int SRC, bool HORIZONTAL>
__global__ __launch_bounds__(256) void clip_blur_kernel(const void* src, int h, int w, long total, int k, ClipTaps taps, float* dst) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % w), y = (int)((idx / w) % h);
  const long plane = idx / ((long)w * h);
  const int front = k / 2;
  float acc = 0.f;
  for (int t = 0; t < k; ++t) {
    const int xx = HORIZONTAL ? reflect(x + t - front, w) : x, yy = HORIZONTAL ? y : reflect(y + t - front, h);
    float v;
    if constexpr (SRC == 0) {
      const long n = plane / 3;
      const int c = (int)(plane - n * 3);
      v = 2.0f * ((float)((const unsigned char*)src)[((n * h + yy) * w + xx) * 3 + c] / 255.0f) - 1.0f;
    } else {
      v = ((const float*)src)[(plane * h + yy) * w + xx];
      if constexpr (SRC == 1) v = 2.0f * v - 1.0f;
    }
    acc = fmaf(taps.w[t], v, acc);
  }
  dst[idx] = acc;
}

// torch's cubic convolution coefficients (A = -0.75) of the four taps around a sample at fraction t of the way from tap 1 to tap 2.
// The outer two are written in their factored form, A (x - 1) (x - 2)^2 at x = 1 + t and x = 2 - t, which has no cancellation.
__device__ __forceinline__ void cubic_coeffs(float t, float* c) {
  constexpr float A = -0.75f;
  const float s = 1.0f - t;
  c[0] = A * t * (s * s);
  c[1] = fmaf(fmaf(A + 2.0f, t, -(A + 3.0f)) * t, t, 1.0f);
  c[2] = fmaf(fmaf(A + 2.0f, s, -(A + 3.0f)) * s, s, 1.0f);
  c[3] = A * s * (t * t);
}

// Bicubic resample with align_corners = True (sample position o (in - 1) / (out - 1), formed exactly as an integer quotient and
// remainder), border indices clamped, then (v + 1) / 2 and the per-channel (. - mean) / std; one lane per output element.
struct ClipNorm { float mean[3], std[3]; };
template <typename Tag>
__global__ __launch_bounds__(256) void clip_resample_kernel(const float* src, int h, int w, int oh, int ow, long total, ClipNorm nm, char* dst) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % ow), oy = (int)((idx / ow) % oh);
  const long plane = idx / ((long)ow * oh);
  const int c = (int)(plane % 3);
  const long py = (long)oy * (h - 1), px = (long)ox * (w - 1);
  const int iy = (int)(py / (oh - 1)), ix = (int)(px / (ow - 1));
  float cy[4], cx[4];
  cubic_coeffs((float)(int)(py - (long)iy * (oh - 1)) / (float)(oh - 1), cy);
  cubic_coeffs((float)(int)(px - (long)ix * (ow - 1)) / (float)(ow - 1), cx);
  const float* p = src + plane * h * w;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* row = p + (long)min(max(iy - 1 + i, 0), h - 1) * w;
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) r = fmaf(cx[j], row[min(max(ix - 1 + j, 0), w - 1)], r);
    acc = fmaf(cy[i], r, acc);
  }
  const float v = ((acc + 1.0f) * 0.5f - nm.mean[c]) / nm.std[c];
  store1<Tag>(dst + idx * Elem<Tag>::ES, v);
}

// ------------------------------------------------------------------------------------------------ tt_layernorm_block
// sum of one double per thread over a 256-thread block, the same value returned to every thread (fixed order: bit-reproducible)
__device__ __forceinline__ double block_sum256(double v, double* s4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                                    // the previous call's readers are done with s4
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// One block per batch element: all rows * c elements are one normalisation group.  Three sweeps over the block (the second and third
// come from L2): (1) the mean, as pivot + mean of (x - pivot) with the block's first element as pivot, so the fp32 partial sums hold
// deviations, not a large common offset; (2) the sum of squares centred on that mean; (3) y = (x - mean) rstd.  fp32 per thread,
// fp64 across threads.  In place is safe: no element is written before both statistics sweeps have ended (the block-wide sums are
// barriers), and each element is read and written by the same thread.
template <typename Tag>
__global__ __launch_bounds__(256) void ln_block_kernel(const char* x, long ldx, int rows, int c, float eps, char* y) {
  __shared__ double s4[4];
  constexpr int ES = Elem<Tag>::ES;
  const int cv = c >> 3, total = rows * cv;
  const char* xb = x + (long)blockIdx.x * rows * ldx * ES;
  char* yb = y + (long)blockIdx.x * rows * ldx * ES;
  const float pivot = load1<Tag>(xb);
  const double n = (double)rows * c;
  float s = 0.f;
  for (int v = threadIdx.x; v < total; v += 256) {
    const int r = v / cv;
    float f[8];
    load8<Tag>(xb + ((long)r * ldx + (v - r * cv) * 8) * ES, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += f[e] - pivot;
  }
  const float mean = (float)((double)pivot + block_sum256((double)s, s4) / n);
  float q = 0.f;
  for (int v = threadIdx.x; v < total; v += 256) {
    const int r = v / cv;
    float f[8];
    load8<Tag>(xb + ((long)r * ldx + (v - r * cv) * 8) * ES, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = f[e] - mean; q = fmaf(d, d, q); }
  }
  const float rstd = (float)(1.0 / sqrt(block_sum256((double)q, s4) / n + (double)eps));
  for (int v = threadIdx.x; v < total; v += 256) {
    const int r = v / cv;
    const long off = ((long)r * ldx + (v - r * cv) * 8) * ES;
    float f[8];
    load8<Tag>(xb + off, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (f[e] - mean) * rstd;
    store8<Tag>(yb + off, f);
  }
}

// ------------------------------------------------------------------------------------------------ tt_frames_out
// clamp(x / 2 + 0.5, 0, 1): x / 2 is exact, the addition rounds once (a fused multiply-add rounds the same sum).  Written with
// comparisons, not fmin / fmax, so that what a NaN becomes is defined: 0.
__device__ __forceinline__ float frame_value(float x) {
  float f = x * 0.5f + 0.5f;
  f = f > 0.f ? f : 0.f;
  return f < 1.f ? f : 1.f;
}
// rint(f * 255): one fp32 product, round-half-to-even (v_rndne_f32), as numpy.round on the fp32 product
__device__ __forceinline__ unsigned frame_byte(float f) { return (unsigned)(int)__builtin_rintf(f * 255.0f); }

// [n, ch, hw] -> [n, hw, ch], one lane per pixel: channel reads are coalesced across lanes, the pixel's ch values leave together
template <typename Tag, int KIND>
__global__ __launch_bounds__(256) void frames_out_kernel(const char* src, int ch, int hw, long total, char* dst) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long n = idx / hw;
  const int p = (int)(idx - n * hw);
  for (int c = 0; c < ch; ++c) {
    const float f = frame_value(load1<Tag>(src + ((n * ch + c) * hw + p) * Elem<Tag>::ES));
    if constexpr (KIND == 0) ((float*)dst)[idx * ch + c] = f;
    else ((unsigned char*)dst)[idx * ch + c] = (unsigned char)frame_byte(f);
  }
}

// the same for four consecutive pixels of one image per lane (hw % 4 == 0, 16-byte aligned operands): one 8- or 16-byte load per
// channel, and the 4 CH outputs -- contiguous in NHWC -- leave as CH float4 (kind 0) or CH dwords (kind 1)
template <typename Tag, int KIND, int CH>
__global__ __launch_bounds__(256) void frames_out4_kernel(const char* src, int hw, long total4, char* dst) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int q = hw >> 2;
  const long n = idx / q;
  const int p = (int)(idx - n * q) * 4;
  float f[4 * CH];                                   // [pixel][channel]: memory order of the output
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    float v[4];
    quad_to_f32<Tag>(*(const typename Elem<Tag>::quad_t*)(src + ((n * CH + c) * hw + p) * Elem<Tag>::ES), v);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i * CH + c] = frame_value(v[i]);
  }
  const long base = (n * hw + p) * CH;               // a multiple of 4 elements
#pragma unroll
  for (int g = 0; g < CH; ++g) {
    if constexpr (KIND == 0) ((float4*)(dst + base * 4))[g] = make_float4(f[4 * g], f[4 * g + 1], f[4 * g + 2], f[4 * g + 3]);
    else ((unsigned*)(dst + base))[g] = frame_byte(f[4 * g]) | frame_byte(f[4 * g + 1]) << 8 | frame_byte(f[4 * g + 2]) << 16 | frame_byte(f[4 * g + 3]) << 24;
  }
}

// ------------------------------------------------------------------------------------------------ tt_gesture_maps
// The gesture frames of get_thisthat_sam (data_loader/video_this_that_dataset.py:28-130; the blur kernel is
// utils/optical_flow_utils.py:197-219) without the canvas: every frame is 1 - d_c ry[y] rx[x] (include/ttvdm.h).
constexpr int GESTURE_TAPS = 99, GESTURE_DOT = 10;
// Kernel ARGUMENTS, like ClipTaps: the fp64 Gaussian taps (792 bytes), the clipped box of every live point (1 KiB) and which frame
// each live point decides (772 bytes).  "Live": no later record names the same (map, frame) -- the host drops the others, so a
// frame has at most one live point and the kernels never see the order of the list.
struct GestureTaps { double k[GESTURE_TAPS]; };
struct GestureBoxes { int lo[TT_GESTURE_MAX_POINTS][2], hi[TT_GESTURE_MAX_POINTS][2]; };      // [point][axis: 0 vertical, 1 horizontal]
struct GestureLive { int n, slab[TT_GESTURE_MAX_POINTS], first[TT_GESTURE_MAX_POINTS]; };   // slab = map * frames + frame

// BORDER_REFLECT_101 as index arithmetic: any number of bounces (the blur radius 49 may exceed the axis)
__device__ __forceinline__ int reflect101(int j, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  j = (j < 0 ? -j : j) % p;
  return j >= n ? p - j : j;
}

// Keys cubic weights (A = -0.75) exactly as gesture_map._cubic_weights writes them, in fp64
__device__ __forceinline__ double keys_near(double x) { return ((-0.75 + 2.0) * x - (-0.75 + 3.0)) * x * x + 1.0; }
__device__ __forceinline__ double keys_far(double x) { return ((-0.75 * x - 5.0 * -0.75) * x + 8.0 * -0.75) * x - 4.0 * -0.75; }

// Launch 1: the resized profile of one axis of one point, one lane per output position: prof[point][0 .. out_h) = ry,
// prof[point][out_h .. out_h + out_w) = rx (mirrored when `flip`).  The blurred box is evaluated only at the four source positions the
// resize reads -- 4 x 99 indicator tests per lane, nothing as long as the original axis is ever stored, so its length costs nothing.
__global__ __launch_bounds__(256) void gesture_profile_kernel(GestureTaps taps, GestureBoxes boxes, int ntaps, int org_h, int org_w,
                                                              int out_h, int out_w, int flip, double* prof) {
  const int axis = blockIdx.y, pt = blockIdx.z;
  const int n = axis ? org_w : org_h, n_out = axis ? out_w : out_h;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n_out) return;
  const int lo = boxes.lo[pt][axis], hi = boxes.hi[pt][axis];
  const double scale = (double)n / (double)n_out;
  const double s = ((double)o + 0.5) * scale - 0.5, fl = floor(s), t = s - fl;
  const int base = (int)fl;                                                     // in [-1, n - 1]
  const double w[4] = {keys_far(t + 1.0), keys_near(t), keys_near(1.0 - t), keys_far(2.0 - t)};
  double r = 0.0;
#pragma unroll
  for (int tap = 0; tap < 4; ++tap) {
    const int i = min(max(base - 1 + tap, 0), n - 1);
    double g = 0.0;
    for (int k = 0; k < ntaps; ++k) {
      const int j = reflect101(i + k - ntaps / 2, n);
      if (j >= lo && j < hi) g += taps.k[k];
    }
    r += w[tap] * g;
  }
  const int at = axis ? out_h + (flip ? out_w - 1 - o : o) : o;
  prof[(long)pt * (out_h + out_w) + at] = r;
}

// the value of one output element: plane c of a frame decided by live point `rec` (-1: no point names the frame)
__device__ __forceinline__ bool gesture_plane_on(int first, int c) { return c == 0 || (c == 1) == (first != 0); }   // d = (1,1,0) / (1,0,1)
__device__ __forceinline__ float gesture_value(double ry, double rx) { return 1.0f - (float)(ry * rx); }

// Launch 2: the store stream.  The output is one flat array of 16-byte chunks, one chunk per lane; a chunk that lies inside one row
// (every chunk when out_w is a multiple of the chunk) takes one frame lookup and one ry, the others walk their elements across the
// row / plane / frame boundary.  The block's first element is split into (frame slab, offset) once, on the scalar unit.
template <typename Tag>
__global__ __launch_bounds__(256) void gesture_store_kernel(const double* __restrict__ prof, GestureLive live, int out_h, int out_w,
                                                            long total, char* __restrict__ dst) {
  constexpr int EPC = Elem<Tag>::EPC, ES = Elem<Tag>::ES;
  const unsigned hw = (unsigned)out_h * out_w, slab = 3u * hw, np = out_h + out_w;
  const long e_blk = (long)blockIdx.x * (256 * EPC);
  const long slab_blk = e_blk / slab;
  const long e0 = e_blk + threadIdx.x * EPC;
  if (e0 >= total) return;
  unsigned rem = (unsigned)(e_blk - slab_blk * slab) + threadIdx.x * EPC;       // < slab + 256 EPC: the entry point keeps it in 32 bits
  const unsigned q = rem / slab;
  rem -= q * slab;
  int mf = (int)(slab_blk + q), c = rem / hw;
  rem -= c * hw;
  int y = rem / out_w, x = rem - y * out_w;
  // the live point of a frame slab (-1: none) and its colour; the loop bound and the argument reads are wave-uniform
  const auto lookup = [&](int frame, int& first) {
    int rec = -1;
    for (int i = 0; i < live.n; ++i)
      if (live.slab[i] == frame) { rec = i; first = live.first[i]; }
    return rec;
  };
  int first = 0;
  float f[EPC];
  if (x + EPC <= out_w) {                                                       // (then e0 + EPC <= total as well)
    const int rec = lookup(mf, first);
    if (rec < 0 || !gesture_plane_on(first, c)) {
      const float v = rec < 0 ? 0.f : 1.f;
#pragma unroll
      for (int i = 0; i < EPC; ++i) f[i] = v;
    } else {
      const double* p = prof + (long)rec * np;
      const double ry = p[y];
#pragma unroll
      for (int i = 0; i < EPC; ++i) f[i] = gesture_value(ry, p[out_h + x + i]);
    }
    *(uint4*)(dst + e0 * ES) = pack_chunk<Tag>(f);
    return;
  }
  const int valid = (int)min((long)EPC, total - e0);
#pragma unroll
  for (int i = 0; i < EPC; ++i) {
    f[i] = 0.f;
    if (i < valid) {
      const int rec = lookup(mf, first);
      if (rec >= 0) f[i] = gesture_plane_on(first, c) ? gesture_value(prof[(long)rec * np + y], prof[(long)rec * np + out_h + x]) : 1.f;
      if (++x == out_w) { x = 0; if (++y == out_h) { y = 0; if (++c == 3) { c = 0; ++mf; } } }
    }
  }
  if (valid == EPC) { *(uint4*)(dst + e0 * ES) = pack_chunk<Tag>(f); return; }
#pragma unroll
  for (int i = 0; i < EPC; ++i)                                                 // the last, partial chunk of the whole output
    if (i < valid) store1<Tag>(dst + (e0 + i) * ES, f[i]);
}

// ------------------------------------------------------------------------------------------------ tt_resize_u8 / tt_vae_image
// PIL's 8-bit resize as two integer passes over tables the host formed (tt_resample_coeffs, lib.cpp), and the VAE input computed in
// the epilogue of the last pass (include/ttvdm.h).  One axis: the device table ([out] xmin, [out] n, [ksize][out]
// kk -- tap-major, so the lanes of neighbouring outputs read neighbouring words) and the sizes it maps.
struct ResampleAxis { const int* tab; int in, out, ksize; };

// (first source index, taps) of output o, clamped to the source and to the table whatever the table holds
__device__ __forceinline__ void resample_bounds(const ResampleAxis& ax, int o, int& first, int& n) {
  first = min(max(ax.tab[o], 0), ax.in - 1);
  n = min(max(ax.tab[ax.out + o], 0), min(ax.ksize, ax.in - first));
}
// Pillow's accumulation of one output byte of output o: n source bytes `step` apart from p, int32 from 1 << 21, >> 22, clip8
__device__ __forceinline__ unsigned clip8(int acc) { return (unsigned)min(max(acc >> 22, 0), 255); }
__device__ __forceinline__ unsigned resample_byte(const unsigned char* p, long step, const ResampleAxis& ax, int o, int n) {
  const int* kk = ax.tab + 2 * ax.out + o;
  int acc = 1 << 21;
  for (int t = 0; t < n; ++t) acc += (int)p[t * step] * kk[t * ax.out];
  return clip8(acc);
}
// one output byte of a pass: HORIZONTAL src [rows, ax.in, 3] at (row, ox, c); vertical src [nimg, ax.in, rb] at (img, oy, byte xb)
__device__ __forceinline__ unsigned resample_h(const unsigned char* src, const ResampleAxis& ax, long row, int ox, int c) {
  int first, n;
  resample_bounds(ax, ox, first, n);
  return resample_byte(src + (row * ax.in + first) * 3 + c, 3, ax, ox, n);
}
__device__ __forceinline__ unsigned resample_v(const unsigned char* src, const ResampleAxis& ax, long rb, long img, int oy, long xb) {
  int first, n;
  resample_bounds(ax, oy, first, n);
  return resample_byte(src + (img * ax.in + first) * rb + xb, rb, ax, oy, n);
}

// One pass, uint8 to uint8.  The output is one flat array of bytes, four per lane, stored as a dword (the last total % 4 bytes leave
// one by one); rb = 3 x (pixels per row) is the byte length of a row, the same on both sides of the vertical pass, which therefore
// never looks at pixels: a row of coefficients is shared by every lane that works on the row, and with DWORDS (rb % 4 == 0 and an
// aligned source: no dword crosses a row) each tap is one dword load of four source bytes.
template <bool HORIZONTAL, bool DWORDS>
__global__ __launch_bounds__(256) void resample_u8_kernel(const unsigned char* __restrict__ src, ResampleAxis ax, long rb, long total,
                                                          unsigned char* __restrict__ dst) {
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  unsigned b[4] = {0, 0, 0, 0};
  if constexpr (HORIZONTAL) {
    long pix = e0 / 3, row = pix / ax.out;
    int c = (int)(e0 - pix * 3), ox = (int)(pix - row * ax.out);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (e0 + i < total) b[i] = resample_h(src, ax, row, ox, c);
      if (++c == 3) { c = 0; if (++ox == ax.out) { ox = 0; ++row; } }
    }
  } else {
    long line = e0 / rb, xb = e0 - line * rb, img = line / ax.out;
    int oy = (int)(line - img * ax.out);
    if constexpr (DWORDS) {
      int first, n;
      resample_bounds(ax, oy, first, n);
      const unsigned char* p = src + (img * ax.in + first) * rb + xb;
      const int* kk = ax.tab + 2 * ax.out + oy;
      int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      for (int t = 0; t < n; ++t) {
        const unsigned v = *(const unsigned*)(p + t * rb);
        const int k = kk[t * ax.out];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += (int)((v >> (8 * i)) & 255u) * k;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = clip8(acc[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (e0 + i < total) b[i] = resample_v(src, ax, rb, img, oy, xb);
        if (++xb == rb) { xb = 0; if (++oy == ax.out) { oy = 0; ++img; } }
      }
    }
  }
  if (e0 + 4 <= total) { *(unsigned*)(dst + e0) = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24; return; }
  for (int i = 0; i < 4 && e0 + i < total; ++i) dst[e0 + i] = (unsigned char)b[i];
}

// image_processor.preprocess and the noise augmentation on one byte: u / 255, 2 x - 1, + na * noise, each rounded to fp32 on its own
// as the torch statements round them (contraction off: a fused na * noise + v would round once)
__device__ __forceinline__ float vae_value(unsigned u, float na, float nz, bool noised) {
#pragma clang fp contract(off)
  const float x = (float)u / 255.0f;
  const float v = 2.0f * x - 1.0f;
  const float s = na * nz;
  return noised ? v + s : v;
}

// The last pass with the VAE input as its epilogue, laid out by the OUTPUT: one lane per four consecutive x of one (image, channel,
// row) of the NCHW result, so that the stores -- and the noise loads, the largest stream of the stage: 4 bytes per element against
// the source's 1 -- are whole 8- / 16-byte vectors along x (VEC: out_w % 4 == 0 and aligned operands; otherwise element by element).
// The source bytes of a channel are 3 apart; a wave reads all of a 768-byte span of each tap row and the other two channels' waves
// find it in L2.  MODE 0: no resampling (src [nimg, oh, ow, 3]); 1: horizontal (src [nimg, oh, ax.in, 3]); 2: vertical
// (src [nimg, ax.in, ow, 3]).  Image i serves requests i nvid .. i nvid + nvid - 1, each with its own noise.
template <typename Tag, int MODE, bool VEC>
__global__ __launch_bounds__(256) void vae_image_kernel(const unsigned char* __restrict__ src, ResampleAxis ax, int oh, int ow, long total,
                                                        const float* __restrict__ noise, float na, int nvid, char* __restrict__ dst) {
  constexpr int ES = Elem<Tag>::ES;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int q = (ow + 3) >> 2;
  const long line = idx / q, plane = line / oh, img = plane / 3;
  const int x0 = (int)(idx - line * q) * 4, oy = (int)(line - plane * oh), c = (int)(plane - img * 3);
  const int valid = VEC ? 4 : min(4, ow - x0);
  unsigned u[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= valid) continue;
    if constexpr (MODE == 0) u[i] = src[((img * oh + oy) * ow + x0 + i) * 3 + c];
    else if constexpr (MODE == 1) u[i] = resample_h(src, ax, img * oh + oy, x0 + i, c);
    else u[i] = resample_v(src, ax, 3L * ow, img, oy, 3L * (x0 + i) + c);
  }
  for (int j = 0; j < nvid; ++j) {
    const long off = (((img * nvid + j) * 3 + c) * oh + oy) * ow + x0;
    float nz[4] = {0.f, 0.f, 0.f, 0.f}, f[4];
    if (noise) {
      if constexpr (VEC) { const float4 v = *(const float4*)(noise + off); nz[0] = v.x; nz[1] = v.y; nz[2] = v.z; nz[3] = v.w; }
      else for (int i = 0; i < valid; ++i) nz[i] = noise[off + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = vae_value(u[i], na, nz[i], noise != nullptr);
    if constexpr (VEC) *(typename Elem<Tag>::quad_t*)(dst + off * ES) = f32_to_quad<Tag>(f);
    else for (int i = 0; i < valid; ++i) store1<Tag>(dst + (off + i) * ES, f[i]);
  }
}

bool dtype_ok(int32_t d) { return d == TT_BF16 || d == TT_F16 || d == TT_F32; }

}  // namespace

extern "C" size_t tt_clip_image_ws_bytes(int32_t nimg, int32_t h, int32_t w) {
  if (nimg <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)2 * nimg * 3 * h * w * sizeof(float);                 // the two blur passes' fp32 planes
}

extern "C" int tt_clip_image(const void* src, int32_t src_kind, int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w,
                             float mean0, float mean1, float mean2, float std0, float std1, float std2, void* dst, int32_t dtype,
                             void* ws, size_t ws_bytes, tt_stream_t stream) {
  if (!src || !dst || !ws) TT_FAIL(TT_EINVAL, "tt_clip_image: null operand");
  if (src_kind != 0 && src_kind != 1) TT_FAIL(TT_EINVAL, "tt_clip_image: src_kind %d (0 uint8 NHWC, 1 fp32 NCHW)", src_kind);
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_clip_image: bad dtype");
  if (nimg <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "tt_clip_image: empty image");
  if (out_h < 2 || out_w < 2) TT_FAIL(TT_EINVAL, "tt_clip_image: output %d x %d, each side must be at least 2 (align_corners)", out_h, out_w);
  if (!(std0 > 0.f && std1 > 0.f && std2 > 0.f)) TT_FAIL(TT_EINVAL, "tt_clip_image: std must be positive");
  const ClipAxis ay = clip_axis(h, out_h), ax = clip_axis(w, out_w);
  if (ay.k > CLIP_MAX_TAPS || ax.k > CLIP_MAX_TAPS)
    TT_FAIL(TT_EUNSUPPORTED, "tt_clip_image: %d x %d -> %d x %d needs %d x %d taps, built for at most %d", h, w, out_h, out_w, ay.k, ax.k, CLIP_MAX_TAPS);
  if (ay.k / 2 >= h || ax.k / 2 >= w)
    TT_FAIL(TT_EINVAL, "tt_clip_image: reflect pad %d x %d reaches the image size %d x %d", ay.k / 2, ax.k / 2, h, w);
  const long planes = (long)nimg * 3, total = planes * h * w, total_out = planes * out_h * out_w;
  if (total > 0x7fffffffL * 256 || total_out > 0x7fffffffL * 256) TT_FAIL(TT_EUNSUPPORTED, "tt_clip_image: more elements than one grid covers");
  if (ws_bytes < tt_clip_image_ws_bytes(nimg, h, w)) TT_FAIL(TT_EINVAL, "tt_clip_image: workspace too small");
  if (((size_t)ws & 15) || ((size_t)dst & (dtype == TT_F32 ? 3 : 1)) || (src_kind == 1 && ((size_t)src & 3))) TT_FAIL(TT_EINVAL, "tt_clip_image: ws must start on a 16-byte boundary, fp32 src and dst on their element size");
  ClipTaps ty, tx;
  clip_taps(ay, &ty);
  clip_taps(ax, &tx);
  const ClipNorm nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
  float* a = (float*)ws;
  float* b = a + total;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((total + 255) / 256)), grid_out((unsigned)((total_out + 255) / 256)), block(256);
  if (src_kind == 0) hipLaunchKernelGGL((clip_blur_kernel<0, true>), grid, block, 0, st, src, h, w, total, ax.k, tx, a);
  else hipLaunchKernelGGL((clip_blur_kernel<1, true>), grid, block, 0, st, src, h, w, total, ax.k, tx, a);
  hipLaunchKernelGGL((clip_blur_kernel<2, false>), grid, block, 0, st, (const void*)a, h, w, total, ay.k, ty, b);
#define TT_RS(TAG) hipLaunchKernelGGL(clip_resample_kernel<TAG>, grid_out, block, 0, st, (const float*)b, h, w, out_h, out_w, total_out, nm, (char*)dst)
  if (dtype == TT_BF16) TT_RS(bf16_tag); else if (dtype == TT_F16) TT_RS(f16_tag); else TT_RS(f32_tag);
#undef TT_RS
  TT_CHECK_LAUNCH("tt_clip_image");
  return TT_OK;
}

extern "C" int tt_layernorm_block(const void* x, int64_t ldx, int32_t nb, int32_t rows, int32_t c, float eps, void* y, int32_t dtype,
                                  tt_stream_t stream) {
  if (!x || !y) TT_FAIL(TT_EINVAL, "tt_layernorm_block: null operand");
  if (nb <= 0 || rows <= 0 || c <= 0) TT_FAIL(TT_EINVAL, "tt_layernorm_block: empty problem");
  if ((c & 7) || (ldx & 7) || ldx < c) TT_FAIL(TT_EINVAL, "tt_layernorm_block: c and the row stride must be multiples of 8, stride >= c");
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_layernorm_block: bad dtype");
  if (!(eps >= 0.f)) TT_FAIL(TT_EINVAL, "tt_layernorm_block: eps must not be negative");
  if ((((size_t)x | (size_t)y) & 15)) TT_FAIL(TT_EINVAL, "tt_layernorm_block: x and y must start on 16-byte boundaries");
  if ((long)rows * (c >> 3) > 0x7fff0000L) TT_FAIL(TT_EUNSUPPORTED, "tt_layernorm_block: %d x %d elements per block", rows, c);
  hipStream_t st = (hipStream_t)stream;
#define TT_LNB(TAG) hipLaunchKernelGGL(ln_block_kernel<TAG>, dim3(nb), dim3(256), 0, st, (const char*)x, (long)ldx, (int)rows, (int)c, eps, (char*)y)
  if (dtype == TT_BF16) TT_LNB(bf16_tag); else if (dtype == TT_F16) TT_LNB(f16_tag); else TT_LNB(f32_tag);
#undef TT_LNB
  TT_CHECK_LAUNCH("tt_layernorm_block");
  return TT_OK;
}

extern "C" int tt_frames_out(const void* src, int32_t src_dtype, int32_t n, int32_t ch, int32_t h, int32_t w, int32_t kind, void* dst,
                             tt_stream_t stream) {
  if (!src || !dst) TT_FAIL(TT_EINVAL, "tt_frames_out: null operand");
  if (!dtype_ok(src_dtype)) TT_FAIL(TT_EINVAL, "tt_frames_out: bad dtype");
  if (kind != 0 && kind != 1) TT_FAIL(TT_EINVAL, "tt_frames_out: kind %d (0 fp32, 1 uint8)", kind);
  if (n <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "tt_frames_out: empty problem");
  if (ch < 1 || ch > 4) TT_FAIL(TT_EUNSUPPORTED, "tt_frames_out: %d channels (1 to 4)", ch);
  const long hw = (long)h * w, total = (long)n * hw;
  if (hw > 0x7fffffffL || total > 0x7fffffffL * 256) TT_FAIL(TT_EUNSUPPORTED, "tt_frames_out: more pixels than one grid covers");
  const int es = src_dtype == TT_F32 ? 4 : 2;
  if (((size_t)src & (es - 1)) || (kind == 0 && ((size_t)dst & 3))) TT_FAIL(TT_EINVAL, "tt_frames_out: src and dst must be aligned to their element size");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (hw & 3) == 0 && !(((size_t)src | (size_t)dst) & 15);
  const long work = vec ? total / 4 : total;
  const dim3 grid((unsigned)((work + 255) / 256)), block(256);
#define TT_FO4(TAG, KIND, CH) hipLaunchKernelGGL((frames_out4_kernel<TAG, KIND, CH>), grid, block, 0, st, (const char*)src, (int)hw, work, (char*)dst)
#define TT_FO(TAG, KIND) do { \
    if (!vec) hipLaunchKernelGGL((frames_out_kernel<TAG, KIND>), grid, block, 0, st, (const char*)src, (int)ch, (int)hw, work, (char*)dst); \
    else if (ch == 1) TT_FO4(TAG, KIND, 1); else if (ch == 2) TT_FO4(TAG, KIND, 2); else if (ch == 3) TT_FO4(TAG, KIND, 3); else TT_FO4(TAG, KIND, 4); } while (0)
#define TT_FOK(TAG) do { if (kind == 0) TT_FO(TAG, 0); else TT_FO(TAG, 1); } while (0)
  if (src_dtype == TT_BF16) TT_FOK(bf16_tag); else if (src_dtype == TT_F16) TT_FOK(f16_tag); else TT_FOK(f32_tag);
#undef TT_FOK
#undef TT_FO
#undef TT_FO4
  TT_CHECK_LAUNCH("tt_frames_out");
  return TT_OK;
}

extern "C" size_t tt_gesture_maps_ws_bytes(int32_t npoints, int32_t out_h, int32_t out_w) {
  if (npoints <= 0 || out_h <= 0 || out_w <= 0) return 0;
  return (size_t)npoints * ((size_t)out_h + (size_t)out_w) * sizeof(double);      // ry and rx of every point
}

extern "C" int tt_gesture_maps(const TtGesturePoint* points, int32_t npoints, int32_t nmaps, int32_t frames, int32_t org_h,
                               int32_t org_w, int32_t out_h, int32_t out_w, int32_t dilate, int32_t flip, void* dst, int32_t dtype,
                               void* ws, size_t ws_bytes, tt_stream_t stream) {
  if (!dst) TT_FAIL(TT_EINVAL, "tt_gesture_maps: null dst");
  if (npoints < 0) TT_FAIL(TT_EINVAL, "tt_gesture_maps: npoints %d", npoints);
  if (npoints > 0 && !points) TT_FAIL(TT_EINVAL, "tt_gesture_maps: null points with npoints %d", npoints);
  if (nmaps <= 0 || frames <= 0) TT_FAIL(TT_EINVAL, "tt_gesture_maps: %d map(s) of %d frame(s)", nmaps, frames);
  if (out_h <= 0 || out_w <= 0) TT_FAIL(TT_EINVAL, "tt_gesture_maps: output size %d x %d", out_h, out_w);
  if (org_h <= 0 || org_w <= 0) TT_FAIL(TT_EINVAL, "tt_gesture_maps: original size %d x %d", org_h, org_w);
  if ((dilate != 0 && dilate != 1) || (flip != 0 && flip != 1)) TT_FAIL(TT_EINVAL, "tt_gesture_maps: dilate %d, flip %d (0 or 1)", dilate, flip);
  if (!dtype_ok(dtype)) TT_FAIL(TT_EINVAL, "tt_gesture_maps: bad dtype");
  if ((size_t)dst & 15) TT_FAIL(TT_EINVAL, "tt_gesture_maps: dst must start on a 16-byte boundary");
  if (npoints > TT_GESTURE_MAX_POINTS) TT_FAIL(TT_EUNSUPPORTED, "tt_gesture_maps: %d points, built for at most %d", npoints, TT_GESTURE_MAX_POINTS);
  for (int i = 0; i < npoints; ++i) {
    const TtGesturePoint& p = points[i];
    if (p.map < 0 || p.map >= nmaps || p.frame < 0 || p.frame >= frames)
      TT_FAIL(TT_EINVAL, "tt_gesture_maps: point %d names map %d, frame %d of %d map(s) x %d frame(s)", i, p.map, p.frame, nmaps, frames);
    if (p.first != 0 && p.first != 1) TT_FAIL(TT_EINVAL, "tt_gesture_maps: point %d has first %d (0 or 1)", i, p.first);
  }
  if (org_h > TT_GESTURE_MAX_AXIS || org_w > TT_GESTURE_MAX_AXIS)
    TT_FAIL(TT_EUNSUPPORTED, "tt_gesture_maps: original size %d x %d, an axis may be at most %d", org_h, org_w, TT_GESTURE_MAX_AXIS);
  const int epc = dtype == TT_F32 ? 4 : 8;
  const long slab = 3L * out_h * out_w, nslab = (long)nmaps * frames, total = slab * nslab;
  const long blocks = (total + 256L * epc - 1) / (256L * epc);
  if (slab > 0x7fffffffL - 4096 || nslab > 0x7fffffffL || blocks > 0x7fffffffL)
    TT_FAIL(TT_EUNSUPPORTED, "tt_gesture_maps: %d x %d frames of 3 x %d x %d are beyond the kernel's 32-bit frame indices", nmaps, frames, out_h, out_w);
  if (npoints > 0 && (!ws || ((size_t)ws & 15) || ws_bytes < tt_gesture_maps_ws_bytes(npoints, out_h, out_w)))
    TT_FAIL(TT_EINVAL, "tt_gesture_maps: the workspace must hold tt_gesture_maps_ws_bytes() = %zu bytes on a 16-byte boundary",
            tt_gesture_maps_ws_bytes(npoints, out_h, out_w));
  // live points: the last record of every (map, frame), in list order
  GestureBoxes boxes;
  GestureLive live;
  live.n = 0;
  for (int i = 0; i < npoints; ++i) {
    bool later = false;
    for (int j = i + 1; j < npoints && !later; ++j) later = points[j].map == points[i].map && points[j].frame == points[i].frame;
    if (later) continue;
    const int r = live.n++;
    live.slab[r] = points[i].map * frames + points[i].frame;
    live.first[r] = points[i].first;
    const long c[2] = {points[i].y, points[i].x}, n[2] = {org_h, org_w};
    for (int a = 0; a < 2; ++a) {                                             // 64-bit: a centre may be anywhere in int32
      boxes.lo[r][a] = (int)(c[a] - GESTURE_DOT > 0 ? (c[a] - GESTURE_DOT < n[a] ? c[a] - GESTURE_DOT : n[a]) : 0);
      boxes.hi[r][a] = (int)(c[a] + GESTURE_DOT + 1 < n[a] ? (c[a] + GESTURE_DOT + 1 > 0 ? c[a] + GESTURE_DOT + 1 : 0) : n[a]);
    }
  }
  for (int r = live.n; r < TT_GESTURE_MAX_POINTS; ++r) {
    live.slab[r] = -1; live.first[r] = 0;
    boxes.lo[r][0] = boxes.lo[r][1] = boxes.hi[r][0] = boxes.hi[r][1] = 0;
  }
  // gesture_map.gaussian_taps: exp(-x^2 / (2 sigma^2)), sigma = 10, on x = -49 .. 49, normalised to sum 1; T = 1 without dilate
  GestureTaps taps;
  const int ntaps = dilate ? GESTURE_TAPS : 1;
  double sum = 0.0;
  for (int t = 0; t < GESTURE_TAPS; ++t) { const double x = (t - GESTURE_TAPS / 2) / 10.0; taps.k[t] = exp(-0.5 * x * x); sum += taps.k[t]; }
  for (int t = 0; t < GESTURE_TAPS; ++t) taps.k[t] = dilate ? taps.k[t] / sum : (t == 0 ? 1.0 : 0.0);
  hipStream_t st = (hipStream_t)stream;
  if (live.n > 0) {
    const int longest = out_h > out_w ? out_h : out_w;
    hipLaunchKernelGGL(gesture_profile_kernel, dim3((unsigned)((longest + 255) / 256), 2, (unsigned)live.n), dim3(256), 0, st, taps, boxes, ntaps,
                       (int)org_h, (int)org_w, (int)out_h, (int)out_w, (int)flip, (double*)ws);
  }
#define TT_GS(TAG) hipLaunchKernelGGL(gesture_store_kernel<TAG>, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)ws, live, (int)out_h, (int)out_w, total, (char*)dst)
  if (dtype == TT_BF16) TT_GS(bf16_tag); else if (dtype == TT_F16) TT_GS(f16_tag); else TT_GS(f32_tag);
#undef TT_GS
  TT_CHECK_LAUNCH("tt_gesture_maps");
  return TT_OK;
}

// ------------------------------------------------------------------------------------------------ tt_resize_u8 / tt_vae_image
namespace {
size_t resample_ws_bytes(int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w) {
  if (nimg <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0 || out_w == w || out_h == h) return 0;
  return (size_t)nimg * h * out_w * 3;                                 // the uint8 image between the two passes
}

struct VaeEpilogue { const float* noise; float na; int nvid; void* dst; int dtype; };      // null: the uint8 result of tt_resize_u8

// what the two entry points share: every refusal, then at most two launches
int resample_run(const char* name, const void* src, int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w, const int32_t* tab_x,
                 int32_t ksize_x, const int32_t* tab_y, int32_t ksize_y, void* dst_u8, const VaeEpilogue* ep, void* ws, size_t ws_bytes,
                 tt_stream_t stream) {
  void* dst = ep ? ep->dst : dst_u8;
  if (!src || !dst) TT_FAIL(TT_EINVAL, "%s: null operand", name);
  if (nimg <= 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0)
    TT_FAIL(TT_EINVAL, "%s: %d image(s) of %d x %d -> %d x %d, every size must be positive", name, nimg, h, w, out_h, out_w);
  if (h > TT_RESAMPLE_MAX_AXIS || w > TT_RESAMPLE_MAX_AXIS || out_h > TT_RESAMPLE_MAX_AXIS || out_w > TT_RESAMPLE_MAX_AXIS)
    TT_FAIL(TT_EUNSUPPORTED, "%s: %d x %d -> %d x %d, an axis may be at most %d", name, h, w, out_h, out_w, TT_RESAMPLE_MAX_AXIS);
  const bool need_x = out_w != w, need_y = out_h != h;
  if (need_x != (tab_x != nullptr) || need_y != (tab_y != nullptr))
    TT_FAIL(TT_EINVAL, "%s: %d x %d -> %d x %d takes a table for exactly the axes that change", name, h, w, out_h, out_w);
  if ((need_x && ksize_x < 1) || (need_y && ksize_y < 1)) TT_FAIL(TT_EINVAL, "%s: ksize %d x %d", name, ksize_y, ksize_x);
  if ((need_x && (long)(2 + (long)ksize_x) * out_w > 0x7fffffffL) || (need_y && (long)(2 + (long)ksize_y) * out_h > 0x7fffffffL))
    TT_FAIL(TT_EUNSUPPORTED, "%s: a table of more than 2^31 words", name);
  if (((size_t)tab_x | (size_t)tab_y) & 3) TT_FAIL(TT_EINVAL, "%s: the tables must start on 4-byte boundaries", name);
  if (ep) {
    if (!dtype_ok(ep->dtype)) TT_FAIL(TT_EINVAL, "%s: bad dtype", name);
    if (ep->nvid <= 0) TT_FAIL(TT_EINVAL, "%s: %d videos per image", name, ep->nvid);
    if (((size_t)dst & (ep->dtype == TT_F32 ? 3 : 1)) || ((size_t)ep->noise & 3)) TT_FAIL(TT_EINVAL, "%s: dst and noise must be aligned to their element size", name);
  } else if ((size_t)dst & 3) TT_FAIL(TT_EINVAL, "%s: dst must start on a 4-byte boundary", name);
  const long mid = 3L * nimg * h * out_w, total_u8 = 3L * nimg * out_h * out_w;                 // bytes after the horizontal / the last pass
  const long lanes = ep ? 3L * nimg * out_h * ((out_w + 3) / 4) : (total_u8 + 3) / 4;           // of the last launch
  if (mid > 0x7fffffffL * 1024 || lanes > 0x7fffffffL * 256 || (ep && total_u8 > 0x7fffffffffffL / ep->nvid))
    TT_FAIL(TT_EUNSUPPORTED, "%s: more elements than one grid covers", name);
  const size_t need = resample_ws_bytes(nimg, h, w, out_h, out_w);
  if (need && (!ws || ((size_t)ws & 15) || ws_bytes < need))
    TT_FAIL(TT_EINVAL, "%s: the workspace must hold %zu bytes on a 16-byte boundary", name, need);
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(256);
  const ResampleAxis ax = {tab_x, w, out_w, ksize_x}, ay = {tab_y, h, out_h, ksize_y}, none = {nullptr, 1, 1, 0};
  const unsigned char* in = (const unsigned char*)src;
  const auto pass_u8 = [&](bool horizontal, const unsigned char* from, long total, unsigned char* to) {
    const dim3 grid((unsigned)((total + 1023) / 1024));
    const long rb = 3L * out_w;                                  // the vertical pass runs after the horizontal one: rows are out_w pixels
    if (horizontal) hipLaunchKernelGGL((resample_u8_kernel<true, false>), grid, block, 0, st, from, ax, rb, total, to);
    else if ((rb & 3) == 0 && ((size_t)from & 3) == 0) hipLaunchKernelGGL((resample_u8_kernel<false, true>), grid, block, 0, st, from, ay, rb, total, to);
    else hipLaunchKernelGGL((resample_u8_kernel<false, false>), grid, block, 0, st, from, ay, rb, total, to);
  };
  if (need_x && need_y) { pass_u8(true, in, mid, (unsigned char*)ws); in = (const unsigned char*)ws; }
  if (!ep) {
    if (need_y) pass_u8(false, in, total_u8, (unsigned char*)dst);
    else if (need_x) pass_u8(true, in, total_u8, (unsigned char*)dst);
    else {
      const hipError_t e = hipMemcpyAsync(dst, src, (size_t)total_u8, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) TT_FAIL(TT_ELAUNCH, "%s: %s", name, hipGetErrorString(e));
    }
  } else {
    const int mode = need_y ? 2 : need_x ? 1 : 0;
    const ResampleAxis& a = need_y ? ay : need_x ? ax : none;
    const int es = ep->dtype == TT_F32 ? 4 : 2;
    const bool vec = (out_w & 3) == 0 && !((size_t)dst & (4 * es - 1)) && !((size_t)ep->noise & 15);
    const dim3 grid((unsigned)((lanes + 255) / 256));
#define TT_VI(TAG, MODE, VEC) hipLaunchKernelGGL((vae_image_kernel<TAG, MODE, VEC>), grid, block, 0, st, in, a, (int)out_h, (int)out_w, lanes, \
                                                ep->noise, ep->na, ep->nvid, (char*)dst)
#define TT_VIM(TAG, VEC) do { if (mode == 0) TT_VI(TAG, 0, VEC); else if (mode == 1) TT_VI(TAG, 1, VEC); else TT_VI(TAG, 2, VEC); } while (0)
#define TT_VIV(TAG) do { if (vec) TT_VIM(TAG, true); else TT_VIM(TAG, false); } while (0)
    if (ep->dtype == TT_BF16) TT_VIV(bf16_tag); else if (ep->dtype == TT_F16) TT_VIV(f16_tag); else TT_VIV(f32_tag);
#undef TT_VIV
#undef TT_VIM
#undef TT_VI
  }
  TT_CHECK_LAUNCH(name);
  return TT_OK;
}
}  // namespace

extern "C" size_t tt_resize_u8_ws_bytes(int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w) {
  return resample_ws_bytes(nimg, h, w, out_h, out_w);
}
extern "C" size_t tt_vae_image_ws_bytes(int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w) {
  return resample_ws_bytes(nimg, h, w, out_h, out_w);
}

extern "C" int tt_resize_u8(const void* src, int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w, const int32_t* tab_x,
                            int32_t ksize_x, const int32_t* tab_y, int32_t ksize_y, void* dst, void* ws, size_t ws_bytes, tt_stream_t stream) {
  return resample_run("tt_resize_u8", src, nimg, h, w, out_h, out_w, tab_x, ksize_x, tab_y, ksize_y, dst, nullptr, ws, ws_bytes, stream);
}

extern "C" int tt_vae_image(const void* src, int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w, const int32_t* tab_x,
                            int32_t ksize_x, const int32_t* tab_y, int32_t ksize_y, const float* noise, float na, int32_t nvid, void* dst,
                            int32_t dtype, void* ws, size_t ws_bytes, tt_stream_t stream) {
  const VaeEpilogue ep = {noise, na, nvid, dst, dtype};
  return resample_run("tt_vae_image", src, nimg, h, w, out_h, out_w, tab_x, ksize_x, tab_y, ksize_y, nullptr, &ep, ws, ws_bytes, stream);
}
