// libttvdm: the device half of the PNG export (include/ttvdm.h): tt_png_filter -- the row filters of uint8 NHWC frames, fixed or chosen
// per row --, tt_png_tokens -- the run tokens of every 32 KiB stripe of the filtered streams, counted per symbol, with the stripe's
// Adler-32 pair -- and tt_png_emit -- the stripes' DEFLATE blocks, bit for bit, from the code tables the host made of those counts.
// Integer arithmetic only; LDS atomics are adds and ORs, which commute: every call gives the same bytes.
#include "common.h"
#include "block_scan.h"
#include "png_host.h"

namespace {

constexpr int STRIPE = TT_PNG_STRIPE, BLOCK = TT_PNG_BLOCK, WAVES = BLOCK / 64, PER = STRIPE / BLOCK;
constexpr int FBLOCK = TT_PNG_FILTER_BLOCK, FWAVES = FBLOCK / 64;
constexpr int CHUNK_WORDS = TT_PNG_CHUNK / 4, CHUNK_BITS = TT_PNG_CHUNK * 8;
constexpr int HEADER_BITS_MAX = (TT_PNG_HEADER_WORDS - 1) * 32;
constexpr unsigned ADLER = 65521u;
static_assert(PER == 32, "a lane's run starts are the bits of one 32-bit mask");
static_assert(CHUNK_WORDS == 4 * BLOCK, "a lane stores one 16-byte unit of a chunk");
static_assert(TT_PNG_RECORD_WORDS == TT_PNG_SYMS + 2 && TT_PNG_TABLE_WORDS == TT_PNG_SYMS + 2, "286 symbols and two more words");
static_assert(TT_PNG_RECORD_WORDS <= BLOCK, "one lane per record word");

// ---------------------------------------------------------------- the filter
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ unsigned filtered_byte(int type, int x, int a, int b, int c) {
  const int pred = type == 0 ? 0 : (type == 1 ? a : (type == 2 ? b : (type == 3 ? (a + b) >> 1 : paeth(a, b, c))));
  return (unsigned)(x - pred) & 0xffu;
}

// grid (n h): one workgroup per row
__global__ __launch_bounds__(FBLOCK) void png_filter_kernel(const unsigned char* __restrict__ src, int h, int rowbytes, int bpp, int filter,
                                                            unsigned char* __restrict__ dst, long long stride) {
  __shared__ unsigned long long cost_s[FWAVES][5];
  __shared__ int type_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row = blockIdx.x;
  const int y = (int)(row % h);
  const unsigned char* __restrict__ cur = src + row * rowbytes;
  const unsigned char* __restrict__ up = cur - rowbytes;            // read for y > 0 only
  unsigned char* __restrict__ out = dst + (row / h) * stride + (long long)y * (1 + rowbytes);
  int type = filter;
  if (filter == TT_PNG_ADAPTIVE) {                                  // uniform
    unsigned long long cost[5] = {0, 0, 0, 0, 0};
    for (int x = tid; x < rowbytes; x += FBLOCK) {
      const bool left = x >= bpp;
      const int v = cur[x], a = left ? cur[x - bpp] : 0, b = y ? up[x] : 0, c = left && y ? up[x - bpp] : 0;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const unsigned r = filtered_byte(t, v, a, b, c);
        cost[t] += r < 128u ? r : 256u - r;
      }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const unsigned long long s = wave_sum(cost[t]);
      if (lane == 0) cost_s[wave][t] = s;
    }
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      unsigned long long least = 0;
      for (int t = 0; t < 5; ++t) {
        unsigned long long s = 0;
        for (int wv = 0; wv < FWAVES; ++wv) s += cost_s[wv][t];
        if (t == 0 || s < least) { least = s; best = t; }           // strictly smaller, t ascending: the lowest type keeps a tie
      }
      type_s = best;
    }
    __syncthreads();
    type = type_s;
  }
  if (tid == 0) out[0] = (unsigned char)type;
  for (int x = tid; x < rowbytes; x += FBLOCK) {
    const bool left = x >= bpp;
    const int v = cur[x], a = left ? cur[x - bpp] : 0, b = y ? up[x] : 0, c = left && y ? up[x - bpp] : 0;
    out[1 + x] = (unsigned char)filtered_byte(type, v, a, b, c);
  }
}

// ---------------------------------------------------------------- a lane's share of a stripe: shared by tokens and emit
struct Lane {
  unsigned w[8];           // positions base .. base + 31 of the stripe: position base + j is byte j & 3 of w[j >> 2]; zeros from len on
  unsigned starts;         // bit j: a run starts at base + j (position len starts the run of what lies behind the stripe)
  int s_in;                // where the run through position base starts, when bit 0 of starts is clear
  int e_out;               // where the run through position base + 31 ends
};

__device__ __forceinline__ unsigned lane_byte(const Lane& L, int j) { return (L.w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// loads the lane's bytes and finds the runs (two workgroup scans).  wmax_s / wmin_s: WAVES ints each.  Holds one __syncthreads.
__device__ __forceinline__ void lane_load(Lane& L, const unsigned char* __restrict__ p, int len, int* wmax_s, int* wmin_s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, base = tid * PER;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  const uint4 q0 = base < len ? *(const uint4*)(p + base) : zero;                  // a 16-byte unit that starts inside the stream ends inside
  const uint4 q1 = base + 16 < len ? *(const uint4*)(p + base + 16) : zero;        // the frame's region (tt_png_frame_stride)
  const unsigned raw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  unsigned prev = base > 0 && base <= len ? p[base - 1] : 0u;
  unsigned starts = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) L.w[k] = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = base + j;
    const unsigned b = i < len ? (raw[j >> 2] >> (8 * (j & 3))) & 0xffu : 0u;
    const bool st = i == 0 || (i < len ? b != prev : i == len);
    starts |= (unsigned)st << j;
    L.w[j >> 2] |= b << (8 * (j & 3));
    prev = b;
  }
  L.starts = starts;
  int mx = starts ? base + 31 - __clz((int)starts) : -1;                // the last run start of this lane
  int mn = starts ? base + __ffs((int)starts) - 1 : STRIPE;             // ... and the first
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(mx, o, 64), b = __shfl_down(mn, o, 64);
    if (lane >= o) mx = max(mx, a);
    if (lane + o < 64) mn = min(mn, b);
  }
  if (lane == 63) wmax_s[wave] = mx;
  if (lane == 0) wmin_s[wave] = mn;
  __syncthreads();
  int ex = __shfl_up(mx, 1, 64), en = __shfl_down(mn, 1, 64);
  if (lane == 0) ex = -1;
  if (lane == 63) en = STRIPE;
  for (int wv = 0; wv < WAVES; ++wv) {
    if (wv < wave) ex = max(ex, wmax_s[wv]);
    if (wv > wave) en = min(en, wmin_s[wv]);
  }
  L.s_in = ex;
  L.e_out = en;
}

// rule 3: the token that starts at position base + j: -1 none, 0 .. 255 that literal, 256 + m a match of length m
__device__ __forceinline__ int token_at(const Lane& L, int base, int j, int len) {
  const int i = base + j;
  if (i >= len) return -1;
  const unsigned lower = L.starts & ((2u << j) - 1u);                   // run starts at or before j
  const int s = lower ? base + 31 - __clz((int)lower) : L.s_in;
  const int v = (int)lane_byte(L, j);
  if (i == s) return v;
  const unsigned upper = j < 31 ? L.starts >> (j + 1) : 0u;              // run starts after j
  const int e = upper ? i + __ffs((int)upper) : L.e_out;
  const int run = e - s, q = i - s - 1;
  const int full = (run - 1) / 258, r = (run - 1) - full * 258;
  const int k = q / 258, at = q - k * 258;
  if (k < full) return at == 0 ? 256 + 258 : -1;
  if (r >= 3) return at == 0 ? 256 + r : -1;
  return v;
}

__device__ __forceinline__ void length_symbol(int m, int& sym, int& nextra, unsigned& extra) {
  nextra = 0;
  extra = 0u;
  if (m <= 10) sym = 254 + m;
  else if (m == 258) sym = 285;
  else {
    const unsigned l = (unsigned)(m - 3);
    const int k = 29 - __clz((int)l);
    sym = 265 + 4 * (k - 1) + (int)((l >> k) & 3u);
    nextra = k;
    extra = l & ((1u << k) - 1u);
  }
}

// where stripe g of the launch lies: its bytes and its length
__device__ __forceinline__ const unsigned char* stripe_of(const unsigned char* filtered, long long g, int stripes, long long stream, long long stride, int& len) {
  const long long f = g / stripes, k = g % stripes, left = stream - k * STRIPE;
  len = left < STRIPE ? (int)left : STRIPE;
  return filtered + f * stride + k * STRIPE;
}

// grid (n stripes): one workgroup per stripe
__global__ __launch_bounds__(BLOCK) void png_tokens_kernel(const unsigned char* __restrict__ filtered, long long stream, long long stride, int stripes,
                                                           unsigned* __restrict__ records) {
  __shared__ unsigned cnt_s[TT_PNG_RECORD_WORDS];
  __shared__ int wmax_s[WAVES], wmin_s[WAVES];
  __shared__ unsigned red_s[WAVES][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, base = tid * PER;
  int len;
  const unsigned char* p = stripe_of(filtered, blockIdx.x, stripes, stream, stride, len);
  if (tid < TT_PNG_RECORD_WORDS) cnt_s[tid] = 0u;
  Lane L;
  lane_load(L, p, len, wmax_s, wmin_s);                              // its barrier also orders the zeroing above
  unsigned s1 = 0u, s2 = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int t = token_at(L, base, j, len);
    if (t >= 0) {
      int sym = t, nextra;
      unsigned extra;
      if (t >= 256) length_symbol(t - 256, sym, nextra, extra);
      atomicAdd(&cnt_s[sym], 1u);
    }
    const unsigned b = lane_byte(L, j);                               // zero from len on
    s1 += b;
    s2 += b * (unsigned)max(len - (base + j), 0);                     // 32 terms of at most 255 x 32768: below 2^29
  }
  s1 = wave_sum(s1);                                                  // at most 255 x 32768 in all
  s2 = wave_sum(s2 % ADLER);                                          // at most 1024 x 65520 in all
  if (lane == 0) { red_s[wave][0] = s1; red_s[wave][1] = s2; }
  __syncthreads();
  unsigned* rec = records + (long long)blockIdx.x * TT_PNG_RECORD_WORDS;
  if (tid < TT_PNG_SYMS) rec[tid] = tid == 256 ? 1u : cnt_s[tid];
  else if (tid < TT_PNG_RECORD_WORDS) {
    const int which = tid - TT_PNG_SYMS;
    unsigned v = which ? (unsigned)len : 1u;
    for (int wv = 0; wv < WAVES; ++wv) v += red_s[wv][which];
    rec[tid] = v % ADLER;
  }
}

// ---------------------------------------------------------------- emit
// ORs the low `nbits` <= 32 bits of v in at bit `pos` of the stripe's 16-byte-aligned window, where they fall into chunk c
__device__ __forceinline__ void or_word(unsigned* chunk_s, int c, int word, unsigned v) {
  const int k = word - c * CHUNK_WORDS;
  if (v && k >= 0 && k < CHUNK_WORDS) atomicOr(&chunk_s[k], v);
}
__device__ __forceinline__ void or_bits(unsigned* chunk_s, int c, int pos, unsigned v) {
  const unsigned long long x = (unsigned long long)v << (pos & 31);
  or_word(chunk_s, c, pos >> 5, (unsigned)x);
  or_word(chunk_s, c, (pos >> 5) + 1, (unsigned)(x >> 32));
}

__device__ __forceinline__ void token_bits(const unsigned* tab_s, int t, unsigned& code, int& nbits) {
  if (t < 256) {
    const unsigned e = tab_s[t];
    code = e & 0xffffu;
    nbits = (int)min(e >> 16, 15u);
  } else {
    int sym, nextra;
    unsigned extra;
    length_symbol(t - 256, sym, nextra, extra);
    const unsigned e = tab_s[sym];
    const int cl = (int)min(e >> 16, 15u);
    code = (e & 0xffffu) | (extra << cl);
    nbits = cl + nextra + 1;                                          // + 1: the distance code, the bit 0
  }
}

__global__ __launch_bounds__(BLOCK) void png_emit_kernel(const unsigned char* __restrict__ filtered, long long stream, long long stride, int stripes,
                                                         const unsigned* __restrict__ tables, const unsigned* __restrict__ headers,
                                                         unsigned char* __restrict__ out, long long out_bytes) {
  __shared__ __attribute__((aligned(16))) unsigned chunk_s[CHUNK_WORDS];
  __shared__ unsigned tab_s[TT_PNG_TABLE_WORDS];
  __shared__ int wmax_s[WAVES], wmin_s[WAVES];
  __shared__ unsigned wsum_s[WAVES];
  const int tid = threadIdx.x, base = tid * PER;
  int len;
  const unsigned char* p = stripe_of(filtered, blockIdx.x, stripes, stream, stride, len);
  if (tid < TT_PNG_TABLE_WORDS) tab_s[tid] = tables[(long long)blockIdx.x * TT_PNG_TABLE_WORDS + tid];
  const unsigned* __restrict__ hdr = headers + (long long)blockIdx.x * TT_PNG_HEADER_WORDS;
  const int hbits = (int)min(hdr[0], (unsigned)HEADER_BITS_MAX);
  Lane L;
  lane_load(L, p, len, wmax_s, wmin_s);                              // its barrier also orders tab_s
  // the lane's bits, and where they start
  unsigned mine = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int t = token_at(L, base, j, len);
    if (t >= 0) {
      unsigned code;
      int nbits;
      token_bits(tab_s, t, code, nbits);
      mine += (unsigned)nbits;
    }
  }
  unsigned total;
  const unsigned before = block_scan_excl<WAVES>(mine, wsum_s, total);
  const long long off = (long long)(((unsigned long long)tab_s[287] << 32) | tab_s[286]);
  const long long window = off & ~15ll;                               // the 16-byte unit of `out` the stripe starts in
  const int first = (int)(off & 15);                                  // the stripe's first byte in the window
  const int tok0 = first * 8 + hbits;                                 // bit positions in the window: the tokens, ...
  const int start = tok0 + (int)before;
  const unsigned eob = tab_s[256];
  const int eob_at = tok0 + (int)total, eob_bits = (int)min(eob >> 16, 15u);                    // ... the end-of-block code, ...
  const int tail = (eob_at + eob_bits + 3 + 7) >> 3;                  // ... and the byte at which the stored block's 00 00 FF FF starts
  const int last = tail + 4;                                          // the stripe's bytes in the window: first .. last - 1
  const int chunks = (last + TT_PNG_CHUNK - 1) / TT_PNG_CHUNK;
  for (int c = 0; c < chunks; ++c) {
    *(uint4*)&chunk_s[4 * tid] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (tid < ((hbits + 31) >> 5)) or_bits(chunk_s, c, first * 8 + 32 * tid, hdr[1 + tid]);
    if (tid == BLOCK - 1) {
      or_bits(chunk_s, c, eob_at, eob & 0xffffu);
      or_bits(chunk_s, c, tail * 8 + 16, 0xffffu);
    }
    if (mine && start < (c + 1) * CHUNK_BITS && start + (int)mine > c * CHUNK_BITS) {
      unsigned long long acc = 0ull;
      int nb = start & 31, word = start >> 5;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int t = token_at(L, base, j, len);
        if (t >= 0) {
          unsigned code;
          int nbits;
          token_bits(tab_s, t, code, nbits);
          acc |= (unsigned long long)code << nb;
          nb += nbits;
          if (nb >= 32) {
            or_word(chunk_s, c, word, (unsigned)acc);
            acc >>= 32;
            nb -= 32;
            ++word;
          }
        }
      }
      if (nb > 0) or_word(chunk_s, c, word, (unsigned)acc);
    }
    __syncthreads();
    const int lo = c * TT_PNG_CHUNK + 16 * tid;                       // this lane's 16-byte unit of the window
    const long long at = window + lo;
    if (lo + 16 > first && lo < last && at >= 0) {                   // (an offset the host never makes writes nothing)
      if (lo >= first && lo + 16 <= last && at + 16 <= out_bytes) {
        *(uint4*)(out + at) = *(const uint4*)&chunk_s[4 * tid];
      } else {                                                        // a unit shared with a neighbouring stripe: this stripe's bytes only
        for (int b = 0; b < 16; ++b)
          if (lo + b >= first && lo + b < last && at + b < out_bytes) out[at + b] = (unsigned char)(chunk_s[4 * tid + (b >> 2)] >> (8 * (b & 3)));
      }
    }
    __syncthreads();
  }
}

int refuse_shape(const char* who, int32_t n, int32_t h, int32_t w, int32_t ch) {
  if (n <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "%s: empty problem (n = %d, h = %d, w = %d)", who, n, h, w);
  if (ch < 1 || ch > 4) TT_FAIL(TT_EINVAL, "%s: %d channels (1 to 4)", who, ch);
  const long long stream = (long long)h * (1 + (long long)w * ch);
  if (stream >= (1ll << 31)) TT_FAIL(TT_EUNSUPPORTED, "%s: a filtered stream of %lld bytes per frame (below 2^31)", who, stream);
  if ((long long)n * h > 0x7fffffffll || (long long)n * tt_png_stripes(h, w, ch) > 0x7fffffffll)
    TT_FAIL(TT_EUNSUPPORTED, "%s: %lld rows: more than one grid covers (2^31 - 1)", who, (long long)n * h);
  return TT_OK;
}

}  // namespace

extern "C" int tt_png_filter(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t filter, uint8_t* filtered, tt_stream_t stream) {
  if (!frames || !filtered) TT_FAIL(TT_EINVAL, "tt_png_filter: null %s", !frames ? "frames" : "filtered");
  const int rc = refuse_shape("tt_png_filter", n, h, w, ch);
  if (rc != TT_OK) return rc;
  if (filter < 0 || filter > TT_PNG_ADAPTIVE) TT_FAIL(TT_EINVAL, "tt_png_filter: filter = %d (0 to 4, or 5: adaptive)", filter);
  if ((uintptr_t)filtered & 15) TT_FAIL(TT_EINVAL, "tt_png_filter: filtered is not 16-byte aligned");
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((long long)n * h)), dim3(FBLOCK), 0, (hipStream_t)stream, (const unsigned char*)frames, (int)h,
                     (int)(w * ch), (int)ch, (int)filter, (unsigned char*)filtered, (long long)tt_png_frame_stride(h, w, ch));
  TT_CHECK_LAUNCH("tt_png_filter");
  return TT_OK;
}

extern "C" int tt_png_tokens(const uint8_t* filtered, int32_t n, int32_t h, int32_t w, int32_t ch, uint32_t* records, tt_stream_t stream) {
  if (!filtered || !records) TT_FAIL(TT_EINVAL, "tt_png_tokens: null %s", !filtered ? "filtered" : "records");
  const int rc = refuse_shape("tt_png_tokens", n, h, w, ch);
  if (rc != TT_OK) return rc;
  if ((uintptr_t)filtered & 15) TT_FAIL(TT_EINVAL, "tt_png_tokens: filtered is not 16-byte aligned");
  if ((uintptr_t)records & 15) TT_FAIL(TT_EINVAL, "tt_png_tokens: records is not 16-byte aligned");
  const long long stripes = tt_png_stripes(h, w, ch);
  hipLaunchKernelGGL(png_tokens_kernel, dim3((unsigned)(n * stripes)), dim3(BLOCK), 0, (hipStream_t)stream, (const unsigned char*)filtered,
                     (long long)tt_png_stream_bytes(h, w, ch), (long long)tt_png_frame_stride(h, w, ch), (int)stripes, (unsigned*)records);
  TT_CHECK_LAUNCH("tt_png_tokens");
  return TT_OK;
}

extern "C" int tt_png_emit(const uint8_t* filtered, int32_t n, int32_t h, int32_t w, int32_t ch, const uint32_t* tables, const uint32_t* headers,
                           uint8_t* out, int64_t out_bytes, int64_t cap, tt_stream_t stream) {
  if (!filtered || !tables || !headers || !out)
    TT_FAIL(TT_EINVAL, "tt_png_emit: null %s", !filtered ? "filtered" : (!tables ? "tables" : (!headers ? "headers" : "out")));
  const int rc = refuse_shape("tt_png_emit", n, h, w, ch);
  if (rc != TT_OK) return rc;
  if ((uintptr_t)filtered & 15) TT_FAIL(TT_EINVAL, "tt_png_emit: filtered is not 16-byte aligned");
  if ((uintptr_t)tables & 15) TT_FAIL(TT_EINVAL, "tt_png_emit: tables is not 16-byte aligned");
  if ((uintptr_t)headers & 15) TT_FAIL(TT_EINVAL, "tt_png_emit: headers is not 16-byte aligned");
  if ((uintptr_t)out & 15) TT_FAIL(TT_EINVAL, "tt_png_emit: out is not 16-byte aligned");
  if (out_bytes <= 0) TT_FAIL(TT_EINVAL, "tt_png_emit: out_bytes = %lld", (long long)out_bytes);
  if (cap < out_bytes) TT_FAIL(TT_EINVAL, "tt_png_emit: cap too small: %lld bytes for out_bytes = %lld", (long long)cap, (long long)out_bytes);
  const long long stripes = tt_png_stripes(h, w, ch);
  hipLaunchKernelGGL(png_emit_kernel, dim3((unsigned)(n * stripes)), dim3(BLOCK), 0, (hipStream_t)stream, (const unsigned char*)filtered,
                     (long long)tt_png_stream_bytes(h, w, ch), (long long)tt_png_frame_stride(h, w, ch), (int)stripes, (const unsigned*)tables,
                     (const unsigned*)headers, (unsigned char*)out, (long long)out_bytes);
  TT_CHECK_LAUNCH("tt_png_emit");
  return TT_OK;
}
