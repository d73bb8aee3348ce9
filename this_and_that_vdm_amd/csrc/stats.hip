// libttvdm: tt_tensor_stats -- one bandwidth-bound pass that classifies every element of a row-strided tensor (include/ttvdm.h).
// Two launches, no hand-off inside either: stats_kernel leaves one partial record per workgroup in the workspace, stats_finalize_kernel
// (one workgroup) merges them in a fixed, index-ordered shape into the caller's record.  A tensor one workgroup covers does both in stats_kernel.
#include "common.h"
#include "block_scan.h"

namespace {

constexpr int BLOCK = TT_STATS_BLOCK, WAVES = BLOCK / 64, MAX_GRID = TT_STATS_MAX_GRID;
constexpr int UNITS_PER_LANE = 4;                  // a workgroup is added per BLOCK * UNITS_PER_LANE loads, up to MAX_GRID
constexpr int WORDS = sizeof(TtTensorStats) / 8;   // the record as 8-byte words: 73 counters, 2 doubles, 2 float pairs
constexpr int W_COUNT = 0, W_NAN = 1, W_PINF = 2, W_NINF = 3, W_ZERO = 4, W_GE = 5, W_HIST = 9, W_SUM = 73, W_SQ = 74, W_ABS = 75, W_VAL = 76;
constexpr int HIST_COPIES = 8;                     // per-wave histogram, each bin 8 times: lanes of one wave that hit the same bin spread out
static_assert(sizeof(TtTensorStats) == 616 && WORDS == 77, "TtTensorStats layout (include/ttvdm.h)");

constexpr unsigned INF_BITS = 0x7f800000u;
// fp32 bit pattern -> unsigned key with the order of the values (-0 below +0), and back
__device__ __forceinline__ unsigned order_key(unsigned u) { return (u >> 31) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned key_bits(unsigned k) { return (k >> 31) ? (k & 0x7fffffffu) : ~k; }
constexpr unsigned KEY_NINF = ~0xff800000u, KEY_PINF = 0x7f800000u | 0x80000000u;      // the empty set: max = -inf, min = +inf

struct LaneAcc {
  unsigned n_nan = 0, n_pinf = 0, n_ninf = 0, n_zero = 0, n_ge[4] = {0, 0, 0, 0};
  unsigned max_a = 0, min_a = INF_BITS, max_k = KEY_NINF, min_k = KEY_PINF;
  double sum = 0.0, sq = 0.0;
};

__device__ __forceinline__ void acc1(LaneAcc& s, unsigned* hist, unsigned u, const uint4& thr) {
  const unsigned a = u & 0x7fffffffu;
  if (a >= INF_BITS) {
    if (a > INF_BITS) ++s.n_nan;
    else if (u >> 31) ++s.n_ninf;
    else ++s.n_pinf;
    return;
  }
  const unsigned k = order_key(u);
  s.max_k = max(s.max_k, k);
  s.min_k = min(s.min_k, k);
  const double d = (double)__uint_as_float(u);
  s.sum += d;
  s.sq += d * d;
  if (a == 0) { ++s.n_zero; return; }
  s.max_a = max(s.max_a, a);
  s.min_a = min(s.min_a, a);
  s.n_ge[0] += a >= thr.x;
  s.n_ge[1] += a >= thr.y;
  s.n_ge[2] += a >= thr.z;
  s.n_ge[3] += a >= thr.w;
  const int bin = min(max((int)(a >> 23) - 87, 0), 63);
  atomicAdd(&hist[bin * HIST_COPIES], 1u);           // LDS, this wave's copy (the caller offsets `hist` by wave and lane)
}

// OCP e4m3 byte -> fp32 bits (exact; S.1111.111 is NaN, there is no infinity; subnormals m 2^-9)
__device__ __forceinline__ unsigned e4m3_bits(unsigned b) {
  const unsigned s = (b & 0x80u) << 24, e = (b >> 3) & 15u, m = b & 7u;
  if (e == 0) return s | __float_as_uint((float)m * 0.001953125f);
  if (e == 15u && m == 7u) return s | 0x7fc00000u;
  return s | ((e + 120u) << 23) | (m << 20);
}

template <int DT> struct Dt;
template <> struct Dt<TT_BF16> { static constexpr int ES = 2; };
template <> struct Dt<TT_F16> { static constexpr int ES = 2; };
template <> struct Dt<TT_F32> { static constexpr int ES = 4; };
template <> struct Dt<TT_FP8_E4M3> { static constexpr int ES = 1; };

template <int DT> __device__ __forceinline__ unsigned load_bits(const char* p) {
  if constexpr (DT == TT_F32) return *(const unsigned*)p;
  else if constexpr (DT == TT_BF16) return ((unsigned)*(const unsigned short*)p) << 16;
  else if constexpr (DT == TT_F16) return __float_as_uint((float)__builtin_bit_cast(_Float16, *(const unsigned short*)p));
  else return e4m3_bits(*(const unsigned char*)p);
}

template <int DT> __device__ __forceinline__ void acc_vec(LaneAcc& s, unsigned* hist, const uint4& q, const uint4& thr) {
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (DT == TT_F32) {
      acc1(s, hist, w[i], thr);
    } else if constexpr (DT == TT_BF16) {
      acc1(s, hist, w[i] << 16, thr);
      acc1(s, hist, w[i] & 0xffff0000u, thr);
    } else if constexpr (DT == TT_F16) {
      acc1(s, hist, __float_as_uint((float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] & 0xffffu))), thr);
      acc1(s, hist, __float_as_uint((float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] >> 16))), thr);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc1(s, hist, e4m3_bits((w[i] >> (8 * j)) & 0xffu), thr);
    }
  }
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_down(v, o, 64));
  return v;
}

__device__ __forceinline__ unsigned long long pack_f2(unsigned lo, unsigned hi) { return (unsigned long long)lo | ((unsigned long long)hi << 32); }

// word `w` of a record: `part` merged into `cur` (counters and sums add, the float pairs combine)
__device__ __forceinline__ unsigned long long merge_word(int w, unsigned long long cur, unsigned long long part) {
  if (w < W_SUM) return cur + part;
  if (w < W_ABS) return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)cur) + __longlong_as_double((long long)part));
  const unsigned c0 = (unsigned)cur, c1 = (unsigned)(cur >> 32), p0 = (unsigned)part, p1 = (unsigned)(part >> 32);
  if (w == W_ABS) return pack_f2(max(c0, p0), min(c1, p1));                     // magnitudes of finite values: the bits order like the values
  return pack_f2(key_bits(max(order_key(c0), order_key(p0))), key_bits(min(order_key(c1), order_key(p1))));
}
__device__ __forceinline__ unsigned long long empty_word(int w) {
  if (w < W_ABS) return 0ull;                                                    // counters 0, sums +0.0
  if (w == W_ABS) return pack_f2(0u, INF_BITS);
  return pack_f2(0xff800000u, INF_BITS);
}

// x: the tensor; flat != 0: `nunits` 16-byte loads from x, then `tail` single elements; flat == 0 and vpr > 0: rows of vpr 16-byte loads, row
// stride ldx elements; vpr == 0: nunits single elements in rows of `cols`.  nparts == 1 (one workgroup): the result goes to rec.
template <int DT>
__global__ __launch_bounds__(BLOCK) void stats_kernel(const char* __restrict__ x, long long ldx, int cols, unsigned vpr, int flat,
                                                      unsigned long long nunits, int tail, uint4 thr, unsigned long long total,
                                                      unsigned long long* __restrict__ ws, unsigned long long* __restrict__ rec,
                                                      int accumulate) {
  constexpr int ES = Dt<DT>::ES;
  __shared__ unsigned hist_s[WAVES * 64 * HIST_COPIES];
  __shared__ unsigned long long wave_s[WAVES][W_HIST + 4];        // per wave: words 0..8 (counters), then sum, sq, abs pair, val pair
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < WAVES * 64 * HIST_COPIES; i += BLOCK) hist_s[i] = 0;
  __syncthreads();
  unsigned* hist = hist_s + wave * 64 * HIST_COPIES + (lane & (HIST_COPIES - 1));
  LaneAcc s;
  const unsigned long long stride = (unsigned long long)gridDim.x * BLOCK;
  unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + tid;
  if (flat) {
    for (; i < nunits; i += stride) acc_vec<DT>(s, hist, *(const uint4*)(x + i * 16ull), thr);
    if (blockIdx.x == 0 && tid < tail) acc1(s, hist, load_bits<DT>(x + nunits * 16ull + (unsigned long long)tid * ES), thr);
  } else if (vpr) {
    for (; i < nunits; i += stride) {
      const unsigned long long r = i / vpr, c = i - r * vpr;
      acc_vec<DT>(s, hist, *(const uint4*)(x + (long long)r * ldx * ES + c * 16ull), thr);
    }
  } else {
    for (; i < nunits; i += stride) {
      const unsigned long long r = i / (unsigned)cols, c = i - r * (unsigned)cols;
      acc1(s, hist, load_bits<DT>(x + ((long long)r * ldx + (long long)c) * ES), thr);
    }
  }
  // ---- lanes -> wave (shuffles), waves -> workgroup (LDS, in wave order)
  const unsigned cnt[8] = {wave_sum(s.n_nan), wave_sum(s.n_pinf), wave_sum(s.n_ninf), wave_sum(s.n_zero),
                           wave_sum(s.n_ge[0]), wave_sum(s.n_ge[1]), wave_sum(s.n_ge[2]), wave_sum(s.n_ge[3])};
  const unsigned max_a = wave_max(s.max_a), min_a = wave_min(s.min_a), max_k = wave_max(s.max_k), min_k = wave_min(s.min_k);
  const double sum = wave_sum(s.sum), sq = wave_sum(s.sq);
  if (lane == 0) {
    wave_s[wave][0] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) wave_s[wave][1 + j] = cnt[j];
    wave_s[wave][W_HIST + 0] = (unsigned long long)__double_as_longlong(sum);
    wave_s[wave][W_HIST + 1] = (unsigned long long)__double_as_longlong(sq);
    wave_s[wave][W_HIST + 2] = pack_f2(max_a, min_a);
    wave_s[wave][W_HIST + 3] = pack_f2(key_bits(max_k), key_bits(min_k));
  }
  __syncthreads();
  if (tid < WORDS) {
    unsigned long long v;
    if (tid >= W_HIST && tid < W_SUM) {                           // histogram bin: the waves' copies
      const int bin = tid - W_HIST;
      v = 0;
      for (int w = 0; w < WAVES; ++w)
#pragma unroll
        for (int c = 0; c < HIST_COPIES; ++c) v += hist_s[(w * 64 + bin) * HIST_COPIES + c];
    } else {
      const int src = tid < W_HIST ? tid : tid - W_SUM + W_HIST;
      v = wave_s[0][src];
      for (int w = 1; w < WAVES; ++w) v = merge_word(tid, v, wave_s[w][src]);
    }
    if (gridDim.x > 1) {
      ws[(unsigned long long)blockIdx.x * WORDS + tid] = v;
    } else {
      if (tid == W_COUNT) v = total;
      rec[tid] = accumulate ? merge_word(tid, rec[tid], v) : v;
    }
  }
}

// one workgroup: word w of the record = the partials' words w merged in a FIXED shape -- FIN_GROUPS runs of consecutive partials, each in
// index order, then the runs in order -- so the fp64 sums come out the same every time (nparts == 0: the empty record).  A lane
// fetches eight partials at a time: the loads of a run are independent, only the merge is ordered.
constexpr int FIN_GROUPS = 8, FIN_STRIDE = 80, FIN_THREADS = FIN_GROUPS * FIN_STRIDE;
static_assert(FIN_STRIDE >= WORDS, "one lane per word of the record");
__global__ __launch_bounds__(FIN_THREADS) void stats_finalize_kernel(const unsigned long long* __restrict__ ws, int nparts, unsigned long long total,
                                                                     unsigned long long* __restrict__ rec, int accumulate) {
  __shared__ unsigned long long run_s[FIN_GROUPS][FIN_STRIDE];
  const int g = threadIdx.x / FIN_STRIDE, w = threadIdx.x % FIN_STRIDE;
  if (w < WORDS) {
    const int per = (nparts + FIN_GROUPS - 1) / FIN_GROUPS;
    const int p0 = min(g * per, nparts), p1 = min(p0 + per, nparts);
    unsigned long long v = empty_word(w);
    int p = p0;
    for (; p + 8 <= p1; p += 8) {
      unsigned long long t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = ws[(long long)(p + j) * WORDS + w];
#pragma unroll
      for (int j = 0; j < 8; ++j) v = merge_word(w, v, t[j]);
    }
    for (; p < p1; ++p) v = merge_word(w, v, ws[(long long)p * WORDS + w]);
    run_s[g][w] = v;
  }
  __syncthreads();
  if (threadIdx.x < WORDS) {
    const int ww = threadIdx.x;
    unsigned long long v = run_s[0][ww];
    for (int r = 1; r < FIN_GROUPS; ++r) v = merge_word(ww, v, run_s[r][ww]);
    if (ww == W_COUNT) v = total;
    rec[ww] = accumulate ? merge_word(ww, rec[ww], v) : v;
  }
}

int elem_size(int dtype) {
  switch (dtype) {
    case TT_BF16: case TT_F16: return 2;
    case TT_F32: return 4;
    case TT_FP8_E4M3: return 1;
    default: return 0;
  }
}
long long grid_for(unsigned long long units) {
  const unsigned long long per = (unsigned long long)BLOCK * UNITS_PER_LANE;
  unsigned long long g = (units + per - 1) / per;
  return g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : (long long)g);
}

}  // namespace

extern "C" int tt_tensor_stats_launch(int32_t dtype, int32_t* max_grid, int32_t* block, int32_t* elems_per_load) {
  const int es = elem_size(dtype);
  if (!es) TT_FAIL(TT_EINVAL, "tt_tensor_stats_launch: bad dtype %d", dtype);
  if (!max_grid || !block || !elems_per_load) TT_FAIL(TT_EINVAL, "tt_tensor_stats_launch: null output");
  *max_grid = MAX_GRID;
  *block = BLOCK;
  *elems_per_load = 16 / es;
  return TT_OK;
}

extern "C" int64_t tt_tensor_stats_ws_bytes(int64_t rows, int32_t cols, int32_t dtype) {
  if (rows <= 0 || cols <= 0 || !elem_size(dtype)) return 0;
  // the scalar route has the most units (one per element): its grid bounds every route's
  const long long g = grid_for((unsigned long long)rows * (unsigned long long)cols);
  return g > 1 ? g * (long long)sizeof(TtTensorStats) : 0;
}

extern "C" int tt_tensor_stats(const void* x, int64_t ldx, int64_t rows, int32_t cols, int32_t dtype, const float* thr, TtTensorStats* rec,
                               void* ws, int64_t ws_bytes, int32_t accumulate, tt_stream_t stream) {
  const int es = elem_size(dtype);
  if (!es) TT_FAIL(TT_EINVAL, "tt_tensor_stats: bad dtype %d (TT_BF16, TT_F16, TT_F32 or TT_FP8_E4M3)", dtype);
  if (!rec || !thr) TT_FAIL(TT_EINVAL, "tt_tensor_stats: null %s", !rec ? "rec" : "thr");
  if ((uintptr_t)rec & 7) TT_FAIL(TT_EINVAL, "tt_tensor_stats: rec is not 8-byte aligned");
  if (rows < 0 || cols < 0) TT_FAIL(TT_EINVAL, "tt_tensor_stats: rows = %lld, cols = %d: neither may be negative", (long long)rows, cols);
  unsigned tb[4];
  for (int i = 0; i < 4; ++i) {
    if (!(thr[i] >= 0.0f)) TT_FAIL(TT_EINVAL, "tt_tensor_stats: thr[%d] = %g: a threshold is >= 0 and not NaN", i, (double)thr[i]);
    const float t = thr[i] + 0.0f;                                 // (-0 -> +0)
    tb[i] = __builtin_bit_cast(unsigned, t);
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* recw = (unsigned long long*)rec;
  if (rows == 0 || cols == 0) {
    if (!accumulate) {
      hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, st, (const unsigned long long*)nullptr, 0, 0ull, recw, 0);
      TT_CHECK_LAUNCH("tt_tensor_stats");
    }
    return TT_OK;
  }
  if (!x) TT_FAIL(TT_EINVAL, "tt_tensor_stats: null x");
  if ((uintptr_t)x % es) TT_FAIL(TT_EINVAL, "tt_tensor_stats: x is not aligned to its %d-byte elements", es);
  if (rows > 1 && ldx < cols) TT_FAIL(TT_EINVAL, "tt_tensor_stats: row stride %lld < cols %d", (long long)ldx, cols);
  if ((unsigned long long)rows > (1ull << 62) / (unsigned long long)cols)
    TT_FAIL(TT_EINVAL, "tt_tensor_stats: rows * cols = %lld * %d overflows", (long long)rows, cols);
  const unsigned long long total = (unsigned long long)rows * (unsigned long long)cols;
  const int epc = 16 / es;
  const bool aligned = ((uintptr_t)x & 15) == 0;
  int flat = 0, tail = 0;
  unsigned vpr = 0;
  unsigned long long nunits = total;                               // scalar route: one element per unit
  if (aligned && (rows == 1 || ldx == cols)) {
    flat = 1; nunits = total / epc; tail = (int)(total % epc);
  } else if (aligned && cols % epc == 0 && (ldx * es) % 16 == 0) {
    vpr = (unsigned)(cols / epc); nunits = (unsigned long long)rows * vpr;
  }
  const long long grid = grid_for(nunits);
  if (grid > 1) {
    if (!ws || ws_bytes < grid * (long long)sizeof(TtTensorStats))
      TT_FAIL(TT_EINVAL, "tt_tensor_stats: workspace of %lld bytes, %lld needed (tt_tensor_stats_ws_bytes)", ws ? (long long)ws_bytes : 0ll,
              grid * (long long)sizeof(TtTensorStats));
    if ((uintptr_t)ws & 7) TT_FAIL(TT_EINVAL, "tt_tensor_stats: ws is not 8-byte aligned");
  }
  const uint4 t4 = make_uint4(tb[0], tb[1], tb[2], tb[3]);
#define TT_STATS(DT) hipLaunchKernelGGL(stats_kernel<DT>, dim3((unsigned)grid), dim3(BLOCK), 0, st, (const char*)x, (long long)ldx, (int)cols, vpr, flat, \
                                        nunits, tail, t4, total, (unsigned long long*)ws, recw, (int)(accumulate != 0))
  switch (dtype) {
    case TT_BF16: TT_STATS(TT_BF16); break;
    case TT_F16: TT_STATS(TT_F16); break;
    case TT_F32: TT_STATS(TT_F32); break;
    default: TT_STATS(TT_FP8_E4M3); break;
  }
#undef TT_STATS
  TT_CHECK_LAUNCH("tt_tensor_stats");
  if (grid > 1) {
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, st, (const unsigned long long*)ws, (int)grid, total, recw,
                       (int)(accumulate != 0));
    TT_CHECK_LAUNCH("tt_tensor_stats");
  }
  return TT_OK;
}
