// libttvdm: version / error plumbing and the resampling tables of tt_resize_u8 / tt_vae_image (host only).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "ttvdm.h"
#include "host_common.h"

static thread_local char g_err[512] = "";

void tt_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

int tt_put_name(const char* who, char* name, int32_t cap, const char* fmt, ...) {
  char buf[128];
  va_list ap;
  va_start(ap, fmt);
  const int len = vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (!name || len < 0 || len >= (int)sizeof buf || len >= cap) {
    tt_set_error("%s: the name takes %d bytes with its terminator, the buffer holds %d", who, len + 1, name ? cap : 0);
    return TT_EINVAL;
  }
  memcpy(name, buf, (size_t)len + 1);
  return TT_OK;
}

extern "C" int tt_abi_version(void) { return 11; }   // 2: TtGemmArgs.ln_fold / ln_eps, TT_F32; 3: out_fp8, TtAttnArgs.fp8, tt_add_rowvec, tt_conv3x3; 4: tt_groupnorm_small; 5: tt_softmax_rows; 6: TtAttnArgs fused query projection (qx, wq, bq, qc, ln_eps), tt_gemm_set_big_tile; 7: TtGemmArgs.rowvec_mod; 8: TtGemmArgs.stats_out / stats_seg, tt_gemm_stats_rows, tt_groupnorm_tiles; 9: TtGemmArgs.gn_out (GroupNorm in the split-K reduction), tt_gemm_gn_fused; 10: TtAttnArgs.v_rows (row-major V); 11: tt_gemm_set_f32_split (split-fp16 products in TT_F32)
extern "C" const char* tt_target_arch(void) { return "gfx950"; }
extern "C" const char* tt_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------ tt_resample_coeffs
// Pillow's 8-bit resampling tables (precompute_coeffs + normalize_coeffs_8bpc) of one axis, restated in fp64 with libm in the order
// include/ttvdm.h gives: the kernels of tt_resize_u8 / tt_vae_image (image.hip) only do integer arithmetic on what this writes.
namespace {
const double PI = 3.14159265358979323846;
double sinc_pi(double x) { if (x == 0.0) return 1.0; x *= PI; return sin(x) / x; }
double f_box(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }
double f_bilinear(double x) { x = fabs(x); return x < 1.0 ? 1.0 - x : 0.0; }
double f_hamming(double x) {
  x = fabs(x);
  if (x == 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  x *= PI;
  return sin(x) / x * (0.54f + 0.46f * cos(x));              // Pillow's constants are float literals, widened to double
}
double f_bicubic(double x) {
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double f_lanczos(double x) { return -3.0 <= x && x < 3.0 ? sinc_pi(x) * sinc_pi(x / 3) : 0.0; }
}  // namespace

extern "C" int tt_resample_coeffs(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds, int32_t* kk) {
  if (!ksize) TT_FAIL(TT_EINVAL, "tt_resample_coeffs: null ksize");
  if (!bounds != !kk) TT_FAIL(TT_EINVAL, "tt_resample_coeffs: bounds and kk are given together or not at all");
  if (in_size <= 0 || out_size <= 0) TT_FAIL(TT_EINVAL, "tt_resample_coeffs: %d -> %d, sizes must be positive", in_size, out_size);
  double (*f)(double);
  double support;
  switch (filter) {
    case TT_RESAMPLE_BOX: f = f_box; support = 0.5; break;
    case TT_RESAMPLE_BILINEAR: f = f_bilinear; support = 1.0; break;
    case TT_RESAMPLE_HAMMING: f = f_hamming; support = 1.0; break;
    case TT_RESAMPLE_BICUBIC: f = f_bicubic; support = 2.0; break;
    case TT_RESAMPLE_LANCZOS: f = f_lanczos; support = 3.0; break;
    default: TT_FAIL(TT_EINVAL, "tt_resample_coeffs: filter %d (PIL's codes: 1 lanczos, 2 bilinear, 3 bicubic, 4 box, 5 hamming)", filter);
  }
  if (in_size > TT_RESAMPLE_MAX_AXIS || out_size > TT_RESAMPLE_MAX_AXIS)
    TT_FAIL(TT_EUNSUPPORTED, "tt_resample_coeffs: %d -> %d, an axis may be at most %d", in_size, out_size, TT_RESAMPLE_MAX_AXIS);
  const double scale = (double)in_size / (double)out_size, fs = scale < 1.0 ? 1.0 : scale, ss = 1.0 / fs;
  support *= fs;
  const int ks = (int)ceil(support) * 2 + 1;                  // <= 6 2^20 + 3: out ks stays inside int32 (ks > 7 only when out < in)
  *ksize = ks;
  if (!kk) return TT_OK;
  std::vector<double> wbuf((size_t)ks);
  double* wp = wbuf.data();
  for (int o = 0; o < out_size; ++o) {
    const double c = (o + 0.5) * scale;
    int xmin = (int)(c - support + 0.5);
    if (xmin < 0) xmin = 0;
    int n = (int)(c + support + 0.5);
    if (n > in_size) n = in_size;
    n -= xmin;
    if (n < 0) n = 0;
    if (n > ks) n = ks;                                       // (never: n <= 2 support + 1 <= ks)
    double ww = 0.0;
    for (int x = 0; x < n; ++x) { wp[x] = f((x + xmin - c + 0.5) * ss); ww += wp[x]; }
    int32_t* k = kk + (size_t)o * ks;
    for (int x = 0; x < ks; ++x) {
      if (x >= n) { k[x] = 0; continue; }
      const double v = ww != 0.0 ? wp[x] / ww : wp[x];
      k[x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
    }
    bounds[2 * o] = xmin;
    bounds[2 * o + 1] = n;
  }
  return TT_OK;
}
