// The request path around the models: CLIP image preprocessing (tt_clip_image), the context LayerNorm of use_text requests
// (tt_layernorm_block) and the export of decoded frames (tt_frames_out).  None of it is in the denoise step; all of it is fp32
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
