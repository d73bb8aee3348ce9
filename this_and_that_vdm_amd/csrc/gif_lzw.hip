// libttvdm: the GIF export's LZW stage on the device (include/ttvdm.h, "GIF LZW on the device", rules 1 - 8): tt_gif_lzw_frames codes
// every frame's indices in independent segments, each with a dictionary of its own behind a clear code, and leaves the finished image
// data -- min-code-size byte, sub-blocks, terminator -- of every frame at its stride.  Four launches on the stream, no readback between
// them, no workgroup that waits on another: codes (one wave per segment) -> a scan of the segments' bit lengths per frame -> the
// frame's zeroed span with its closed-form framing bytes -> the codes ORed into place.  Integers only: the same bytes every call.
#include "common.h"
#include "block_scan.h"
#include "gif_host.h"

namespace {

constexpr int SLOTS = 2 * TT_LZW_MAX_CODES, SLOT_BITS = 13;      // the string table: never more than half full (at most 3838 entries)
constexpr unsigned EMPTY = 0xffffffffu;                          // no entry has prefix 4095: the word (key << 12 | code) never equals it
constexpr int CHUNK = 4096;                                      // indices of a segment staged in LDS at a time
constexpr int SCAN_BLOCK = 256, SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int FILL_BLOCK = 256, FILL_SPAN = FILL_BLOCK * 16 * 16;     // bytes of a frame's span one workgroup of the fill kernel owns
constexpr int PACK_BLOCK = 256, PACK_PER = 8, PACK_TILE = PACK_BLOCK * PACK_PER;      // codes a workgroup of the pack kernel places
constexpr int PACK_WORDS = PACK_TILE * TT_LZW_MAX_BITS / 32 + 4;      // their bits, the tile's bit phase, the frame's first clear code
static_assert(SLOTS == 1 << SLOT_BITS, "the slot hash keeps SLOT_BITS bits");
static_assert(TT_LZW_MAX_BITS == 12 && TT_LZW_MAX_CODES == 4096, "a table word is key (20 bits) << 12 | code (12 bits)");
static_assert(TT_LZW_SEGMENT >= 1 && TT_LZW_SEGMENT <= TT_LZW_SEGMENT_MAX && TT_LZW_SEGMENT_MAX >= 9216, "the built default segment");
// LDS of lzw_codes_kernel: 32 KiB of table + 4 KiB of indices: four workgroups (four waves) a CU in 160 KiB.

__host__ __device__ inline int clamp_mcs(int m) { return m < 2 ? 2 : (m > 8 ? 8 : m); }
// codes between two clear codes that a full table forces, the clear code included: entry 4095 is made by code 4093 - 2^m, one more
// code follows, then the clear code
__host__ __device__ inline unsigned period(int m) { return 4096u - (1u << m); }
// the width of the code at place r behind a clear code (rule 3 and 4: one bit more from the code after entry 2^width was made, the
// code that made it being r - 1; a closing clear or end code at place r follows the same rule)
__host__ __device__ inline unsigned width_at(int m, unsigned r) {
  const unsigned v = (1u << m) + 1u + r;
  const unsigned w = 32u - (unsigned)__builtin_clz(v);
  return w > (unsigned)TT_LZW_MAX_BITS ? (unsigned)TT_LZW_MAX_BITS : w;
}
// the bits of places 0 .. r - 1 behind a clear code, r <= period: at most ten terms
__host__ __device__ inline unsigned bits_before(int m, unsigned r) {
  const unsigned base = (1u << m) + 1u;
  unsigned total = 0, at = 0;
  for (int w = m + 1; w < TT_LZW_MAX_BITS; ++w) {
    const unsigned end = (1u << w) - base;                       // places below this one are at most w bits wide
    const unsigned hi = end < r ? end : r;
    if (hi > at) { total += (hi - at) * (unsigned)w; at = hi; }
  }
  return total + (r - at) * (unsigned)TT_LZW_MAX_BITS;
}
// the bits of a segment's codes 0 .. j - 1 (a code's width depends only on its place behind the last clear code)
__host__ __device__ inline unsigned seg_bits_before(int m, unsigned j) {
  const unsigned p = period(m);
  return (j / p) * bits_before(m, p) + bits_before(m, j % p);
}

struct Geo {                                       // one call's geometry, the same in every kernel
  unsigned npix, segment, nseg, cstride;           // cstride: uint16 codes a segment's slot of the workspace holds
  long long stride;                                // bytes of a frame in out
  int nmcs;
};

__device__ __forceinline__ unsigned uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

// grid (nseg, n), one wave per segment.  All lanes stage the segment's pixels and clear the string table; the walk through the pixels
// is one dependent chain, so every lane runs it alike on wave-uniform values (what LDS returns goes through readfirstlane): the
// state lives in scalar registers and every branch is a scalar one.  Lane 0 stores the codes.
__global__ __launch_bounds__(64) void lzw_codes_kernel(const unsigned char* __restrict__ indices, const int* __restrict__ mcs, Geo g,
                                                       unsigned short* __restrict__ codes, unsigned* __restrict__ ncodes,
                                                       unsigned* __restrict__ status) {
  __shared__ unsigned tab_s[SLOTS];
  __shared__ unsigned pix_s[CHUNK / 4 + 1];                      // four pixels a word; the walk reads one word ahead
  const int lane = threadIdx.x;
  const unsigned seg = blockIdx.x, frame = blockIdx.y;
  const int m_raw = mcs[g.nmcs == 1 ? 0 : frame], m = clamp_mcs(m_raw);
  const unsigned clear = 1u << m, first = clear + 2u, mask = clear - 1u;
  const unsigned p0 = seg * g.segment, len = g.npix - p0 < g.segment ? g.npix - p0 : g.segment;
  const unsigned char* __restrict__ src = indices + (long long)frame * g.npix + p0;
  unsigned short* __restrict__ out = codes + ((long long)frame * g.nseg + seg) * g.cstride;
  unsigned char* pix_b = (unsigned char*)pix_s;
  unsigned bad = m_raw != m ? (unsigned)TT_GIF_LZW_STATUS_MCS : 0u;
  for (int i = lane; i < SLOTS; i += 64) tab_s[i] = EMPTY;
  unsigned prefix = 0, next = first, j = 0;                      // uniform: the open string's code, the next entry, codes written
  for (unsigned c0 = 0; c0 < len; c0 += CHUNK) {
    const unsigned cl = len - c0 < (unsigned)CHUNK ? len - c0 : (unsigned)CHUNK;
    __syncthreads();                                             // the chunk before is walked
    for (unsigned i = lane; i < cl; i += 64) {
      const unsigned v = src[c0 + i];
      if (v > mask) bad |= (unsigned)TT_GIF_LZW_STATUS_INDEX;
      pix_b[i] = (unsigned char)(v & mask);                      // clamped: a code never exceeds the table
    }
    __syncthreads();
    unsigned i = 0;
    if (c0 == 0) { prefix = uniform(pix_s[0]) & 0xffu; i = 1; }
    // a table fills after 3838 codes at the least, so a chunk of 4096 pixels meets at most two full tables: three walks end it
    for (int round = 0; round < CHUNK / 3838 + 2; ++round) {
      bool full = false;
      unsigned pw = uniform(pix_s[i >> 2]);
      while (i < cl) {                                           // i grows in every trip
        const unsigned c = (pw >> (8u * (i & 3u))) & 0xffu;
        ++i;
        if ((i & 3u) == 0u) pw = uniform(pix_s[i >> 2]);
        const unsigned k = (prefix << 8) | c, key = k << 12;
        unsigned slot = (k * 0x9E3779B1u) >> (32 - SLOT_BITS);
        unsigned w = EMPTY, diff = EMPTY;                        // diff: the slot's word against the key, its code when the key matches
        for (int probe = 0; probe < SLOTS; ++probe) {            // ends at an empty slot: the table is never more than half full
          w = uniform(tab_s[slot]);
          diff = w ^ key;
          if (w == EMPTY || diff < (unsigned)TT_LZW_MAX_CODES) break;
          slot = (slot + 1) & (SLOTS - 1);
        }
        if (w != EMPTY && diff < (unsigned)TT_LZW_MAX_CODES) { prefix = diff; continue; }
        if (lane == 0 && j < g.cstride) out[j] = (unsigned short)prefix;
        ++j;
        prefix = c;
        if (next < (unsigned)TT_LZW_MAX_CODES) {
          tab_s[slot] = key | next;                               // every lane the same word: each reads back what it wrote
          ++next;
        } else {                                                 // the table is full: a clear code, and the table starts over
          if (lane == 0 && j < g.cstride) out[j] = (unsigned short)clear;
          ++j;
          next = first;
          full = true;
          break;
        }
      }
      if (!full) break;                                          // uniform: the chunk is walked
      __syncthreads();
      for (int t = lane; t < SLOTS; t += 64) tab_s[t] = EMPTY;
      __syncthreads();
    }
  }
  if (lane == 0) {
    if (j < g.cstride) out[j] = (unsigned short)prefix;
    ++j;
    ncodes[(long long)frame * g.nseg + seg] = j < g.cstride ? j : g.cstride;
  }
  if (bad) atomicOr(status + frame, bad);
}

// grid (n): a frame's segments' bit lengths (their codes and the code that closes them) scanned into bit offsets; its data bytes and length
__global__ __launch_bounds__(SCAN_BLOCK) void lzw_offsets_kernel(const int* __restrict__ mcs, Geo g, const unsigned* __restrict__ ncodes,
                                                                 unsigned* __restrict__ segoff, unsigned* __restrict__ nbytes,
                                                                 unsigned* __restrict__ lengths) {
  __shared__ unsigned red_s[SCAN_WAVES];
  const unsigned frame = blockIdx.x;
  const int m = clamp_mcs(mcs[g.nmcs == 1 ? 0 : frame]);
  const unsigned* __restrict__ nc = ncodes + (long long)frame * g.nseg;
  unsigned* __restrict__ off = segoff + (long long)frame * g.nseg;
  for (unsigned s = threadIdx.x; s < g.nseg; s += SCAN_BLOCK) off[s] = seg_bits_before(m, nc[s] + 1u);
  __syncthreads();
  const unsigned bits = scan_in_place<SCAN_WAVES>(off, (long long)g.nseg, red_s) + (unsigned)(m + 1);      // the frame's first clear code
  if (threadIdx.x == 0) {
    const unsigned data = (bits + 7u) >> 3;
    nbytes[frame] = data;
    lengths[frame] = 2u + data + (data + 254u) / 255u;
  }
}

// grid (spans of a frame, n): the frame's bytes 0 .. length - 1 zeroed, with the min-code-size byte, the sub-blocks' length bytes and the
// terminator, which are closed forms of the frame's data bytes
__global__ __launch_bounds__(FILL_BLOCK) void lzw_fill_kernel(const int* __restrict__ mcs, Geo g, const unsigned* __restrict__ nbytes,
                                                              unsigned char* __restrict__ out) {
  const unsigned frame = blockIdx.y;
  const unsigned m = (unsigned)clamp_mcs(mcs[g.nmcs == 1 ? 0 : frame]);
  const unsigned data = nbytes[frame];
  const long long length = 2ll + data + (data + 254u) / 255u;
  unsigned char* __restrict__ of = out + (long long)frame * g.stride;
  const long long span0 = (long long)blockIdx.x * FILL_SPAN;
  for (int it = 0; it < FILL_SPAN / (FILL_BLOCK * 16); ++it) {
    const long long q0 = span0 + ((long long)it * FILL_BLOCK + threadIdx.x) * 16;
    if (q0 >= length || q0 + 16 > g.stride) continue;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long q = q0 + i;
      unsigned v = 0u;
      if (q == 0) v = m;
      else if (q < length - 1 && ((q - 1) & 255) == 0) {         // the length byte of sub-block (q - 1) / 256
        const unsigned left = data - 255u * (unsigned)((q - 1) >> 8);
        v = left < 255u ? left : 255u;
      }
      w[i >> 2] |= v << (8 * (i & 3));
    }
    if (q0 + 16 <= length) *(uint4*)(of + q0) = make_uint4(w[0], w[1], w[2], w[3]);
    else
      for (int i = 0; i < 16 && q0 + i < length; ++i) of[q0 + i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
  }
}

// grid (nseg * tiles of a segment, n): a tile's codes ORed into LDS at their bit offsets, then its bytes ORed into the frame at their
// framed places, data byte k at 2 + k + k / 255.  Tiles share bytes at their ends, so every store is an atomic OR onto the zeroed span.
__global__ __launch_bounds__(PACK_BLOCK) void lzw_pack_kernel(const int* __restrict__ mcs, Geo g, unsigned tiles,
                                                              const unsigned short* __restrict__ codes, const unsigned* __restrict__ ncodes,
                                                              const unsigned* __restrict__ segoff, unsigned char* __restrict__ out) {
  __shared__ unsigned bits_s[PACK_WORDS];
  const int tid = threadIdx.x;
  const unsigned seg = blockIdx.x / tiles, tile = blockIdx.x % tiles, frame = blockIdx.y;
  const long long slot = (long long)frame * g.nseg + seg;
  const unsigned count = ncodes[slot] + 1u;                      // the segment's codes and the one that closes it
  const unsigned j0 = tile * PACK_TILE;
  if (j0 >= count) return;                                       // uniform
  const unsigned j1 = count - j0 < (unsigned)PACK_TILE ? count : j0 + PACK_TILE;
  const int m = clamp_mcs(mcs[g.nmcs == 1 ? 0 : frame]);
  const unsigned clear = 1u << m, p = period(m);
  const unsigned base = (unsigned)(m + 1) + segoff[slot];        // the segment's first bit in the frame
  const bool head = seg == 0 && tile == 0;                       // this tile holds the frame's first clear code
  const unsigned b0 = head ? 0u : base + seg_bits_before(m, j0);
  const unsigned b1 = base + seg_bits_before(m, j1);
  const unsigned k0 = b0 >> 3, k1 = (b1 - 1u) >> 3;              // the tile's first and last data byte
  for (int i = tid; i < PACK_WORDS; i += PACK_BLOCK) bits_s[i] = 0u;
  __syncthreads();
  const unsigned short* __restrict__ cs = codes + slot * g.cstride;
  if (head && tid == 0) atomicOr(&bits_s[0], clear);
  unsigned j = j0 + tid * PACK_PER;
  if (j < j1) {
    unsigned bit = base + seg_bits_before(m, j) - 8u * k0;
    for (int e = 0; e < PACK_PER && j < j1; ++e, ++j) {
      const unsigned w = width_at(m, j % p);
      const unsigned v = j + 1u < count ? (unsigned)cs[j] : (seg + 1u == g.nseg ? clear + 1u : clear);
      const unsigned long long sh = (unsigned long long)(v & ((1u << w) - 1u)) << (bit & 31u);
      const unsigned word = bit >> 5;
      if (word + 1u < (unsigned)PACK_WORDS) {
        atomicOr(&bits_s[word], (unsigned)sh);
        if (sh >> 32) atomicOr(&bits_s[word + 1], (unsigned)(sh >> 32));
      }
      bit += w;
    }
  }
  __syncthreads();
  const unsigned char* bytes = (const unsigned char*)bits_s;
  const unsigned q0 = 2u + k0 + k0 / 255u, q1 = 2u + k1 + k1 / 255u;
  unsigned char* __restrict__ of = out + (long long)frame * g.stride;
  const unsigned d0 = q0 >> 2, nd = (q1 >> 2) - d0 + 1u;
  for (unsigned d = tid; d < nd; d += PACK_BLOCK) {
    const unsigned q = (d0 + d) << 2;
    unsigned word = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned qi = q + i;
      if (qi < q0 || qi > q1 || ((qi - 1u) & 255u) == 0u) continue;      // outside the tile, or a length byte
      const unsigned k = ((qi - 1u) >> 8) * 255u + ((qi - 1u) & 255u) - 1u;
      if (k - k0 < (unsigned)(PACK_WORDS * 4)) word |= (unsigned)bytes[k - k0] << (8 * i);
    }
    if (word && (long long)q + 4 <= g.stride) atomicOr((unsigned*)(of + q), word);
  }
}

struct Plan {                                      // what the three host functions agree on; ok = 0: refused arguments
  int ok;
  long long nseg, cstride, stride, tiles;          // tiles: workgroups of the pack kernel a segment takes
  long long ncodes_at, segoff_at, nbytes_at, codes_at, total;      // the workspace, each part at a multiple of 16
};

long long up16(long long v) { return (v + 15) / 16 * 16; }

Plan plan(long long n, long long npix, int segment) {
  Plan pl = {};
  if (n <= 0 || npix <= 0 || segment < 0 || segment > TT_LZW_SEGMENT_MAX) return pl;
  const long long seg = segment ? segment : TT_LZW_SEGMENT;
  pl.nseg = (npix + seg - 1) / seg;
  const long long per = seg < npix ? seg : npix;
  pl.cstride = (per + per / 2048 + 2 + 7) / 8 * 8;               // one code per pixel at most, the clear codes of full tables, slack
  // every pixel a code of 12 bits at most, a clear code per 3838 codes at the least, a closing code per segment, the first clear code
  const long long bits = (npix + npix / 2048 + pl.nseg + 1) * TT_LZW_MAX_BITS;
  const long long data = (bits + 7) / 8;
  pl.stride = up16(2 + data + (data + 254) / 255);
  pl.ncodes_at = 0;
  pl.segoff_at = up16(pl.ncodes_at + n * pl.nseg * 4);
  pl.nbytes_at = up16(pl.segoff_at + n * pl.nseg * 4);
  pl.codes_at = up16(pl.nbytes_at + n * 4);
  pl.total = up16(pl.codes_at + n * pl.nseg * pl.cstride * 2);
  pl.tiles = (pl.cstride + 1 + PACK_TILE - 1) / PACK_TILE;
  pl.ok = 1;
  return pl;
}

constexpr long long NPIX_MAX = 1ll << 40;          // keeps plan()'s products inside 64 bits; far beyond what the limits below admit
// the kernels' limits: bit offsets inside a frame are 32-bit, so 8 * stride stays below 2^32; code offsets are 32-bit; one grid's y
bool stride_fits(const Plan& pl) { return pl.stride < (1ll << 29); }
bool codes_fit(const Plan& pl, long long n) { return pl.nseg * pl.tiles <= 0x7fffffffll && n * pl.nseg * pl.cstride <= 0x7fffffffll; }

}  // namespace

extern "C" int64_t tt_gif_lzw_frames_bound(int64_t npix, int32_t segment) {
  if (npix > NPIX_MAX) return 0;
  const Plan pl = plan(1, npix, segment);
  return pl.ok && stride_fits(pl) && codes_fit(pl, 1) ? pl.stride : 0;
}

extern "C" int64_t tt_gif_lzw_frames_ws_bytes(int32_t n, int64_t npix, int32_t segment) {
  if (npix > NPIX_MAX || n > 65535) return 0;
  const Plan pl = plan(n, npix, segment);
  return pl.ok && stride_fits(pl) && codes_fit(pl, n) ? pl.total : 0;
}

extern "C" int tt_gif_lzw_frames(const uint8_t* indices, int32_t n, int64_t npix, const int32_t* min_code_size, int32_t nmcs, int32_t segment,
                                 uint8_t* out, int64_t cap, uint32_t* lengths, uint32_t* status, void* ws, int64_t ws_bytes, tt_stream_t stream) {
  if (!indices || !min_code_size || !out || !lengths || !status || !ws)
    TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: null %s",
            !indices ? "indices" : (!min_code_size ? "min_code_size" : (!out ? "out" : (!lengths ? "lengths" : (!status ? "status" : "ws")))));
  if (n <= 0 || npix <= 0) TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: empty problem (n = %d, npix = %lld)", n, (long long)npix);
  if (nmcs != 1 && nmcs != n) TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: nmcs = %d (1, or one min_code_size per frame: %d)", nmcs, n);
  if (segment < 0 || segment > TT_LZW_SEGMENT_MAX)
    TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: segment = %d (1 to %d, or 0 for the default %d)", segment, TT_LZW_SEGMENT_MAX, TT_LZW_SEGMENT);
  if ((uintptr_t)out & 15) TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: out is not 16-byte aligned");
  if ((uintptr_t)ws & 15) TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: ws is not 16-byte aligned");
  if ((uintptr_t)lengths & 3) TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: lengths is not 4-byte aligned");
  if ((uintptr_t)status & 3) TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: status is not 4-byte aligned");
  if ((uintptr_t)min_code_size & 3) TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: min_code_size is not 4-byte aligned");
  if (n > 65535) TT_FAIL(TT_EUNSUPPORTED, "tt_gif_lzw_frames: %d frames: more than one grid covers (65535)", n);
  if (npix > NPIX_MAX) TT_FAIL(TT_EUNSUPPORTED, "tt_gif_lzw_frames: npix = %lld: a frame's stride is beyond 2^29 bytes", (long long)npix);
  const Plan pl = plan(n, npix, segment);
  // bit offsets inside a frame are 32-bit: 8 * stride must stay below 2^32
  if (!stride_fits(pl))
    TT_FAIL(TT_EUNSUPPORTED, "tt_gif_lzw_frames: a frame's stride of %lld bytes: the kernels' 32-bit bit offsets address fewer than 2^29 = 536870912", pl.stride);
  const long long tiles = pl.tiles;
  if (!codes_fit(pl, n))
    TT_FAIL(TT_EUNSUPPORTED, "tt_gif_lzw_frames: %lld segments of %lld codes in %d frames: the kernels' 32-bit offsets address fewer than 2^31 = 2147483648 codes",
            pl.nseg, pl.cstride, n);
  if (cap < n * pl.stride)
    TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: cap too small: %lld bytes, %d frames at tt_gif_lzw_frames_bound = %lld take %lld", (long long)cap, n, pl.stride,
            n * pl.stride);
  if (ws_bytes < pl.total)
    TT_FAIL(TT_EINVAL, "tt_gif_lzw_frames: ws too small: %lld bytes, tt_gif_lzw_frames_ws_bytes = %lld", (long long)ws_bytes, pl.total);
  hipStream_t st = (hipStream_t)stream;
  const long long seg = segment ? segment : TT_LZW_SEGMENT;
  Geo g;
  g.npix = (unsigned)npix;
  g.segment = (unsigned)seg;
  g.nseg = (unsigned)pl.nseg;
  g.cstride = (unsigned)pl.cstride;
  g.stride = pl.stride;
  g.nmcs = nmcs;
  char* w = (char*)ws;
  unsigned* ncodes = (unsigned*)(w + pl.ncodes_at);
  unsigned* segoff = (unsigned*)(w + pl.segoff_at);
  unsigned* nbytes = (unsigned*)(w + pl.nbytes_at);
  unsigned short* codes = (unsigned short*)(w + pl.codes_at);
  if (hipMemsetAsync(status, 0, (size_t)n * sizeof(uint32_t), st) != hipSuccess) TT_FAIL(TT_ELAUNCH, "tt_gif_lzw_frames: hipMemsetAsync failed");
  hipLaunchKernelGGL(lzw_codes_kernel, dim3(g.nseg, (unsigned)n), dim3(64), 0, st, (const unsigned char*)indices, (const int*)min_code_size, g, codes, ncodes,
                     (unsigned*)status);
  hipLaunchKernelGGL(lzw_offsets_kernel, dim3((unsigned)n), dim3(SCAN_BLOCK), 0, st, (const int*)min_code_size, g, (const unsigned*)ncodes, segoff, nbytes,
                     (unsigned*)lengths);
  hipLaunchKernelGGL(lzw_fill_kernel, dim3((unsigned)((pl.stride + FILL_SPAN - 1) / FILL_SPAN), (unsigned)n), dim3(FILL_BLOCK), 0, st,
                     (const int*)min_code_size, g, (const unsigned*)nbytes, (unsigned char*)out);
  hipLaunchKernelGGL(lzw_pack_kernel, dim3((unsigned)(pl.nseg * tiles), (unsigned)n), dim3(PACK_BLOCK), 0, st, (const int*)min_code_size, g, (unsigned)tiles,
                     (const unsigned short*)codes, (const unsigned*)ncodes, (const unsigned*)segoff, (unsigned char*)out);
  TT_CHECK_LAUNCH("tt_gif_lzw_frames");
  return TT_OK;
}
