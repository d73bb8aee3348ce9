// The device pieces the JPEG import's units share (jpeg_decode.hip: baseline scans; jpeg_progressive.hip: progressive scans): the
// launch shapes, rule 3's three unstuffing kernels over ITEMS (frames, restart spans or the scans of progressive frames), the 32-bit
// window read and the table lookup of rule 4.  Device only; every unit that includes it gets its own copies of the kernels.
#pragma once
#include "common.h"
#include "block_scan.h"
#include "jpeg_host.h"

namespace {

constexpr int UBLOCK = 256;                         // lanes of an unstuffing chunk: 16 bytes a lane
constexpr int CHUNK = TT_JPEG_CHUNK;
static_assert(CHUNK == 16 * UBLOCK, "a lane holds one 16-byte unit of an unstuffing chunk");
constexpr int SCAN_BLOCK = 1024, SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int ELANES = TT_JPEG_DECODE_LANES, EWAVES = ELANES / 64;
constexpr int SUBSEQ = TT_JPEG_SUBSEQ_BITS;
constexpr unsigned SEQ_BITS = (unsigned)SUBSEQ * ELANES, SEQ_WORDS = SEQ_BITS / 32;
static_assert(SUBSEQ % 32 == 0 && SUBSEQ >= 64, "a subsequence is whole dwords and longer than any symbol (16 + 15 bits)");

// ---------------------------------------------------------------- rule 3: unstuffing
// frame f's stuffed scan: its first byte and its length, both held inside `scans`; a span that is not gives an empty frame
__device__ __forceinline__ long long span_of(long long scans_bytes, const long long* __restrict__ offsets, const unsigned* __restrict__ lengths,
                                             long long max_bytes, int f, unsigned& len, bool& bad) {
  const long long off = offsets[f], l = (long long)lengths[f];
  bad = off < 0 || l > max_bytes || off > scans_bytes || l > scans_bytes - off;
  len = bad ? 0u : (unsigned)l;
  return bad ? 0 : off;
}
__device__ __forceinline__ const unsigned char* frame_span(const unsigned char* __restrict__ scans, long long scans_bytes, const long long* __restrict__ offsets,
                                                           const unsigned* __restrict__ lengths, long long max_bytes, int f, unsigned& len, bool& bad) {
  return scans + span_of(scans_bytes, offsets, lengths, max_bytes, f, len, bad);
}

// the chunk's bytes (and the one before them) into LDS, then per lane: the 0x00 bytes behind an 0xFF among its 16, as a bit mask
__device__ __forceinline__ unsigned chunk_drops(const unsigned char* __restrict__ src, unsigned len, unsigned char* raw_s, bool& marker) {
  const unsigned c0 = blockIdx.x * (unsigned)CHUNK;
  for (int i = threadIdx.x; i < CHUNK + 1; i += UBLOCK) {
    const long long g = (long long)c0 + i - 1;
    raw_s[i] = (g >= 0 && g < (long long)len) ? src[g] : (unsigned char)0;
  }
  __syncthreads();
  unsigned mask = 0u;
  marker = false;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned at = c0 + 16 * threadIdx.x + j;
    if (at < len) {
      const unsigned b = raw_s[1 + 16 * threadIdx.x + j], before = raw_s[16 * threadIdx.x + j];
      if (before == 0xffu && b == 0u) mask |= 1u << j;
      marker = marker || (before == 0xffu && b != 0u) || (at == len - 1 && b == 0xffu);
    }
  }
  return mask;
}

// grid (chunks, items); span_frame NULL: item i is frame i, else the frame an item's status bits go to (held inside the call's frames)
__global__ __launch_bounds__(UBLOCK) void jpeg_unstuff_count_kernel(const unsigned char* __restrict__ scans, long long scans_bytes, const long long* __restrict__ offsets,
                                                                   const unsigned* __restrict__ lengths, long long max_bytes, unsigned* __restrict__ chunk_drop,
                                                                   int chunks, unsigned* __restrict__ status, const int* __restrict__ span_frame, int nframes) {
  __shared__ unsigned char raw_s[CHUNK + 16];
  __shared__ unsigned red_s[UBLOCK / 64];
  unsigned len;
  bool bad, marker;
  const unsigned char* src = frame_span(scans, scans_bytes, offsets, lengths, max_bytes, blockIdx.y, len, bad);
  const unsigned drops = __popc(chunk_drops(src, len, raw_s, marker));
  const unsigned flags = (marker ? TT_JPEG_STATUS_MARKER : 0u) | ((bad && blockIdx.x == 0 && threadIdx.x == 0) ? TT_JPEG_STATUS_SPAN : 0u);
  if (flags) atomicOr(&status[span_frame ? min(max(span_frame[blockIdx.y], 0), nframes - 1) : (int)blockIdx.y], flags);
  const unsigned all = block_sum<UBLOCK / 64>(drops, red_s);
  if (threadIdx.x == 0) chunk_drop[(long long)blockIdx.y * chunks + blockIdx.x] = all;
}

// grid (items): the dropped bytes before every chunk, and the item's plain (unstuffed) length
__global__ __launch_bounds__(SCAN_BLOCK) void jpeg_unstuff_scan_kernel(unsigned* __restrict__ chunk_drop, int chunks, const long long* __restrict__ offsets,
                                                                      const unsigned* __restrict__ lengths, long long scans_bytes, long long max_bytes,
                                                                      unsigned* __restrict__ plain_bytes) {
  __shared__ unsigned red_s[SCAN_WAVES];
  const unsigned total = scan_in_place<SCAN_WAVES>(chunk_drop + (long long)blockIdx.x * chunks, (long long)chunks, red_s);
  if (threadIdx.x == 0) {
    unsigned len;
    bool bad;
    span_of(scans_bytes, offsets, lengths, max_bytes, blockIdx.x, len, bad);
    plain_bytes[blockIdx.x] = len - min(total, len);
  }
}

// grid (chunks, items): every byte that stays moves down by the drops before it
__global__ __launch_bounds__(UBLOCK) void jpeg_unstuff_gather_kernel(const unsigned char* __restrict__ scans, long long scans_bytes, const long long* __restrict__ offsets,
                                                                    const unsigned* __restrict__ lengths, long long max_bytes, const unsigned* __restrict__ chunk_drop,
                                                                    int chunks, unsigned char* __restrict__ plain, long long plain_stride) {
  __shared__ unsigned char raw_s[CHUNK + 16];
  __shared__ unsigned red_s[UBLOCK / 64];
  unsigned len, all;
  bool bad, marker;
  const unsigned char* src = frame_span(scans, scans_bytes, offsets, lengths, max_bytes, blockIdx.y, len, bad);
  const unsigned mask = chunk_drops(src, len, raw_s, marker);
  const unsigned before = chunk_drop[(long long)blockIdx.y * chunks + blockIdx.x] + block_scan_excl<UBLOCK / 64>((unsigned)__popc(mask), red_s, all);
  const unsigned at0 = blockIdx.x * (unsigned)CHUNK + 16 * threadIdx.x;
  unsigned char* __restrict__ dst = plain + (long long)blockIdx.y * plain_stride;
  long long pos = (long long)at0 - before;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (at0 + j < len && !((mask >> j) & 1u)) {
      if (pos >= 0 && pos < plain_stride) dst[pos] = raw_s[1 + 16 * threadIdx.x + j];
      ++pos;
    }
  }
}

// ---------------------------------------------------------------- rule 4: the pieces of a symbol
struct DecState { unsigned p, mz; };                 // bit position; block within the MCU << 6 | zig-zag index
__device__ __forceinline__ bool same(const DecState& a, const DecState& b) { return a.p == b.p && a.mz == b.mz; }

// the 32 bits at bit p of a window of big-endian dwords whose bit 0 of word 0 is bit `win0` of the stream; word (p - win0) / 32 + 1 is read
__device__ __forceinline__ unsigned window_bits(const unsigned* win_s, unsigned win0, unsigned p) {
  const unsigned rel = p - win0, wi = rel >> 5;
  const unsigned long long two = ((unsigned long long)win_s[wi] << 32) | win_s[wi + 1];
  return (unsigned)((two << (rel & 31u)) >> 32);
}

// the code that heads the 32 bits v, by the decode table t (rule 2): its length -- 0: no code -- and its symbol; every index is masked
__device__ __forceinline__ void huff_lookup(const unsigned* t, unsigned v, unsigned& len, unsigned& sym) {
  const unsigned pair = t[v >> 25];
  const unsigned e = ((v >> 24) & 1u) ? pair >> 16 : pair & 0xffffu;
  len = e >> 8;
  sym = e & 0xffu;
  if (len == 0u) {
#pragma unroll
    for (unsigned l = 9; l <= 16; ++l) {
      const unsigned code = v >> (32 - l);
      if (len == 0u && (int)code <= (int)t[128 + l]) {
        len = l;
        const unsigned at = (code + t[145 + l]) & 255u;
        sym = (t[192 + (at >> 2)] >> (8u * (at & 3u))) & 0xffu;
      }
    }
  }
}

// a magnitude of n bits (1 .. 15) as T.81 F.2.2.1 extends it
__device__ __forceinline__ int huff_extend(unsigned raw, unsigned n) { return (raw >> (n - 1u)) ? (int)raw : (int)raw - (int)((1u << n) - 1u); }

}  // namespace
