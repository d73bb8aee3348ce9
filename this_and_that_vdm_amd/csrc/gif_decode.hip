// libttvdm: the GIF import's device half (include/ttvdm.h, "GIF import", rules 2 - 5).  tt_gif_decode_indices turns every frame's LZW
// bytes into its index map: clears (one workgroup per frame follows the chain of clear codes; a code's place behind a clear code fixes
// its bit position, so a batch of codes is extracted per round) -> lengths (per segment the string length of every code, by binary
// lifting over the parent pointers code - E0) -> offsets (a scan over a frame's segments; chunks of pixels for the last launch) ->
// pixels (a lane per pixel: its code by a binary search, its index by at most 12 lookups up the tree).  tt_gif_compose draws the frames
// onto the canvas, one lane per canvas pixel.  No workgroup waits on another; integers only: the same bytes every call.
#include "common.h"
#include "block_scan.h"
#include "gif_host.h"

namespace {

constexpr int CLR_BLOCK = 256, CLR_WAVES = CLR_BLOCK / 64;        // the clears and the offsets kernel
constexpr int DEC_BLOCK = 1024, DEC_WAVES = DEC_BLOCK / 64;       // the lengths and the pixels kernel
constexpr int LEVELS = TT_LZW_MAX_BITS, PLACES = TT_LZW_MAX_CODES; // places whose codes can be named by an entry: fewer than 4096
constexpr int TILE = DEC_BLOCK, TILE_STEPS = 10;                  // codes of a segment scanned at a time; 2^10 = TILE
constexpr unsigned short NONE = 0xffffu;                          // no parent: a pixel code (or an invalid one, read as pixel 0)
constexpr unsigned NOSTOP = 0xffffffffu;
constexpr int CMP_BLOCK = 256;
constexpr unsigned CHUNK = TT_GIF_DEC_CHUNK;
static_assert(TILE == 1 << TILE_STEPS && LEVELS == 12 && PLACES == 4096, "the lifting table is 12 levels of 4096 places");
// LDS of the lengths and the pixels kernel: 96 KiB lifting table + 8 KiB lengths + 4 KiB first + 4 KiB tail pixels (+ 6 KiB of a tile in
// the pixels kernel): one workgroup of 16 waves a CU, inside the 160 KiB a single workgroup may declare on gfx950.

__host__ __device__ inline int clamp_mcs(int m) { return m < 2 ? 2 : (m > 8 ? 8 : m); }
// rule 2a: the width of the code at place r behind a clear code, 12 once the table is full
__host__ __device__ inline unsigned width_at(int m, unsigned long long r) {
  const unsigned long long v = (1ull << m) + 1ull + r;
  if (v >= (1ull << TT_LZW_MAX_BITS)) return (unsigned)TT_LZW_MAX_BITS;
  return 32u - (unsigned)__builtin_clz((unsigned)v);
}
// the bits of places 0 .. r - 1 behind a clear code, for any r (deferred clear: 12 bits each behind the full table): at most ten terms
__host__ __device__ inline unsigned long long bits_before(int m, unsigned long long r) {
  const unsigned long long base = (1ull << m) + 1ull;
  unsigned long long total = 0, at = 0;
  for (int w = m + 1; w < TT_LZW_MAX_BITS; ++w) {
    const unsigned long long end = (1ull << w) - base;            // places below this one are at most w bits wide
    const unsigned long long hi = end < r ? end : r;
    if (hi > at) { total += (hi - at) * (unsigned long long)w; at = hi; }
  }
  return total + (r - at) * (unsigned long long)TT_LZW_MAX_BITS;
}

struct FrameRec {                                  // what the clears kernel leaves per frame (32 bytes)
  unsigned long long segbase;                      // the frame's first segment record
  unsigned segcap, nseg, nchunk, ok, len, npix;    // ok = 0: rule 3's SPAN, the frame is empty
};

struct Dec {                                       // one call's arguments, the same in every kernel
  const unsigned char* data;
  long long data_bytes;
  const long long* offsets;
  const unsigned* lengths;
  const unsigned* npix;
  const int* mcs;
  const int* rows;
  const long long* map_offsets;
  int n;
  unsigned char* maps;
  long long maps_bytes;
  unsigned* status;
  FrameRec* rec;
  unsigned long long segtotal;                     // segment records in the workspace
  unsigned *bitoff, *count, *segpix, *pixoff, *chunkoff;
};

// a frame's validated data length: 0 when its span leaves the uploaded bytes
__device__ __forceinline__ unsigned valid_len(const Dec& d, unsigned f, bool* ok) {
  const long long off = d.offsets[f];
  const unsigned len = d.lengths[f];
  *ok = off >= 0 && (long long)len <= d.data_bytes && off <= d.data_bytes - (long long)len && len < (1u << 29);
  return *ok ? len : 0u;
}
// the most segments that hold a code in `len` bytes: such a segment and its closing code take 6 bits or more; the last needs no closing code
__host__ __device__ inline unsigned long long seg_cap(unsigned long long len) { return 8ull * len / 6ull + 1ull; }

// the code of `w` bits at bit `pos` of src[0, len): bytes behind the data read as zero (the callers only ask for codes that lie inside)
__device__ __forceinline__ unsigned extract(const unsigned char* __restrict__ src, unsigned len, unsigned long long pos, unsigned w) {
  const unsigned i = (unsigned)(pos >> 3);
  unsigned v = 0;
  if (i < len) v = src[i];
  if (i + 1u < len) v |= (unsigned)src[i + 1u] << 8;
  if (i + 2u < len) v |= (unsigned)src[i + 2u] << 16;
  return (v >> (unsigned)(pos & 7u)) & ((1u << w) - 1u);
}

// rule 2b: a node is the place a code names (its parent in the tree of strings), or NONE with the pixel it stands for
struct Node { unsigned short par; unsigned char lit; bool bad; };
__device__ __forceinline__ Node node_of(unsigned code, unsigned long long r, unsigned clear) {
  const unsigned e0 = clear + 2u;
  if (code < clear) return {NONE, (unsigned char)code, false};
  if (code >= e0 && r >= 1) {
    const unsigned k = code - e0, most = (unsigned)TT_LZW_MAX_CODES - 1u - e0;
    if ((unsigned long long)k <= r - 1 && k <= most) return {(unsigned short)k, 0, false};
  }
  return {NONE, 0, true};
}

// grid (n), one workgroup per frame: the frame's record and its segments
__global__ __launch_bounds__(CLR_BLOCK) void gif_clears_kernel(Dec d) {
  __shared__ unsigned long long red_s[CLR_WAVES];
  __shared__ unsigned first_s[CLR_WAVES];
  __shared__ unsigned long long next_s;
  __shared__ unsigned kind_s;
  const unsigned f = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  unsigned long long mine = 0;
  for (unsigned g = tid; g < f; g += CLR_BLOCK) {                // bounded by n
    bool ok;
    mine += seg_cap(valid_len(d, g, &ok));
  }
  const unsigned long long base = block_sum<CLR_WAVES>(mine, red_s);
  bool ok;
  const unsigned len = valid_len(d, f, &ok);
  const unsigned npix = d.npix[f];
  const long long moff = d.map_offsets[f];
  const int rows = d.rows[f];
  ok = ok && moff >= 0 && (long long)npix <= d.maps_bytes && moff <= d.maps_bytes - (long long)npix && rows >= 0 && (unsigned)rows <= npix;
  unsigned long long cap = seg_cap(len);
  if (base >= d.segtotal) { cap = 0; ok = false; }
  else if (base + cap > d.segtotal) cap = d.segtotal - base;
  if (cap > 0xffffffffull) cap = 0xffffffffull;
  const int m = clamp_mcs(d.mcs[f]);
  const unsigned clear = 1u << m;
  const unsigned char* __restrict__ src = d.data + (ok ? d.offsets[f] : 0);
  const unsigned long long total_bits = ok ? 8ull * len : 0ull;
  const unsigned long long rounds = total_bits / 3ull + 2ull;    // a round passes a code (3 bits or more) at the least, or ends the walk
  unsigned long long b = 0, r0 = 0;                              // uniform: the segment's first bit, the batch's first place
  unsigned nseg = 0;
  for (unsigned long long round = 0; round < rounds && nseg < cap; ++round) {
    const unsigned long long r = r0 + tid, pos = b + bits_before(m, r);
    const unsigned w = width_at(m, r);
    const bool fits = pos + w <= total_bits;
    const unsigned code = fits ? extract(src, len, pos, w) : 0u;
    const bool stop = !fits || code == clear || code == clear + 1u;
    const unsigned long long mask = __ballot(stop);
    if (lane == 0) first_s[wave] = mask ? (wave << 6) + (unsigned)__ffsll((long long)mask) - 1u : NOSTOP;
    __syncthreads();
    unsigned first = NOSTOP;
    for (int wv = 0; wv < CLR_WAVES; ++wv) first = first_s[wv] < first ? first_s[wv] : first;
    if (tid == first) { next_s = pos + w; kind_s = fits && code == clear ? 1u : 0u; }
    __syncthreads();
    if (first == NOSTOP) { r0 += CLR_BLOCK; continue; }
    const unsigned long long count = r0 + first;
    if (count > 0) {                                             // a segment that holds a code
      if (tid == 0) {
        d.bitoff[base + nseg] = (unsigned)b;
        d.count[base + nseg] = (unsigned)(count > 0xffffffffull ? 0xffffffffull : count);
      }
      ++nseg;
    }
    if (kind_s == 0u) break;                                     // the end code or the end of the data
    b = next_s;
    r0 = 0;
  }
  if (tid == 0) {
    FrameRec rc;
    rc.segbase = base;
    rc.segcap = (unsigned)cap;
    rc.nseg = ok ? nseg : 0u;
    rc.nchunk = 0;
    rc.ok = ok ? 1u : 0u;
    rc.len = len;
    rc.npix = npix;
    d.rec[f] = rc;
    if (!ok) atomicOr(d.status + f, (unsigned)TT_GIF_DEC_STATUS_SPAN);
  }
}

// the tables of one segment, by every lane of a DEC_BLOCK workgroup: up_s[j][x] the 2^j-th ancestor of place x, len_s[x] the length of
// the string of the code at place x, first_s[x] its first pixel, tail_s[x] its last.  Ends with a barrier.
__device__ __forceinline__ void build_tables(const unsigned char* __restrict__ src, unsigned len, unsigned long long b0, unsigned count, int m,
                                             unsigned short (*up_s)[PLACES], unsigned short* len_s, unsigned char* first_s, unsigned char* tail_s) {
  const unsigned clear = 1u << m;
  for (unsigned x = threadIdx.x; x < (unsigned)PLACES; x += DEC_BLOCK) {
    Node nd = {NONE, 0, false};
    if (x < count) nd = node_of(extract(src, len, b0 + bits_before(m, x), width_at(m, x)), x, clear);
    up_s[0][x] = nd.par;
    tail_s[x] = nd.lit;
  }
  __syncthreads();
  for (int j = 1; j < LEVELS; ++j) {
    for (unsigned x = threadIdx.x; x < (unsigned)PLACES; x += DEC_BLOCK) {
      const unsigned short p = up_s[j - 1][x];
      up_s[j][x] = p == NONE ? NONE : up_s[j - 1][p & (PLACES - 1)];
    }
    __syncthreads();
  }
  for (unsigned x = threadIdx.x; x < (unsigned)PLACES; x += DEC_BLOCK) {
    unsigned y = x, depth = 0;
    for (int j = LEVELS - 1; j >= 0; --j) {                      // a place has a 2^j-th ancestor exactly when it lies 2^j deep or deeper
      const unsigned short p = up_s[j][y];
      if (p != NONE) { y = p & (PLACES - 1); depth += 1u << j; }
    }
    len_s[x] = (unsigned short)(depth + 1u);
    first_s[x] = tail_s[y];                                      // the root's pixel
  }
  __syncthreads();
  for (unsigned x = threadIdx.x; x < (unsigned)PLACES; x += DEC_BLOCK) {
    const unsigned short p = up_s[0][x];
    if (p != NONE) tail_s[x] = first_s[(p + 1u) & (PLACES - 1)]; // rule 2c: the string at place p plus the first pixel of the one at p + 1
  }
  __syncthreads();
}

// grid (workgroups, n): the pixels of every segment of a frame
__global__ __launch_bounds__(DEC_BLOCK) void gif_lengths_kernel(Dec d) {
  __shared__ unsigned short up_s[LEVELS][PLACES];
  __shared__ unsigned short len_s[PLACES];
  __shared__ unsigned char first_s[PLACES], tail_s[PLACES];
  __shared__ unsigned long long red_s[DEC_WAVES];
  const unsigned f = blockIdx.y;
  const FrameRec rc = d.rec[f];
  if (!rc.ok) return;
  const unsigned nseg = rc.nseg < rc.segcap ? rc.nseg : rc.segcap;
  const int m = clamp_mcs(d.mcs[f]);
  const unsigned clear = 1u << m;
  const unsigned char* __restrict__ src = d.data + d.offsets[f];
  for (unsigned s = blockIdx.x; s < nseg; s += gridDim.x) {
    const unsigned long long b0 = d.bitoff[rc.segbase + s];
    const unsigned count = d.count[rc.segbase + s];
    build_tables(src, rc.len, b0, count, m, up_s, len_s, first_s, tail_s);
    unsigned long long sum = 0;
    for (unsigned long long r = threadIdx.x; r < count; r += DEC_BLOCK) {
      if (r < (unsigned)PLACES) { sum += len_s[r]; continue; }
      const Node nd = node_of(extract(src, rc.len, b0 + bits_before(m, r), width_at(m, r)), r, clear);
      sum += nd.par == NONE ? 1u : (unsigned)len_s[nd.par & (PLACES - 1)] + 1u;
    }
    const unsigned long long total = block_sum<DEC_WAVES>(sum, red_s);
    if (threadIdx.x == 0) d.segpix[rc.segbase + s] = (unsigned)(total < rc.npix ? total : rc.npix);
    __syncthreads();
  }
}

// grid (n): every segment's first pixel, clipped to w h; SHORT; the chunks of the pixels kernel
__global__ __launch_bounds__(CLR_BLOCK) void gif_offsets_kernel(Dec d) {
  __shared__ unsigned long long red_s[CLR_WAVES];
  const unsigned f = blockIdx.x, tid = threadIdx.x;
  const FrameRec rc = d.rec[f];
  if (!rc.ok) return;
  const unsigned nseg = rc.nseg < rc.segcap ? rc.nseg : rc.segcap;
  unsigned long long carry = 0, chunks = 0;
  for (unsigned at = 0; at < nseg; at += CLR_BLOCK) {
    const unsigned i = at + tid;
    unsigned long long all;
    const unsigned long long v = i < nseg ? d.segpix[rc.segbase + i] : 0u;
    const unsigned long long before = carry + block_scan_excl<CLR_WAVES>(v, red_s, all);
    if (i < nseg) d.pixoff[rc.segbase + i] = (unsigned)(before < rc.npix ? before : rc.npix);
    carry += all;
    __syncthreads();
  }
  for (unsigned at = 0; at < nseg; at += CLR_BLOCK) {
    const unsigned i = at + tid;
    unsigned long long c = 0, all;
    if (i < nseg) {
      const unsigned long long lo = d.pixoff[rc.segbase + i], end = lo + d.segpix[rc.segbase + i], hi = end < rc.npix ? end : rc.npix;
      c = (hi - lo + CHUNK - 1u) / CHUNK;
    }
    const unsigned long long before = chunks + block_scan_excl<CLR_WAVES>(c, red_s, all);
    if (i < nseg) d.chunkoff[rc.segbase + i] = (unsigned)before;
    chunks += all;
    __syncthreads();
  }
  if (tid == 0) {
    d.rec[f].nchunk = (unsigned)(chunks > 0xffffffffull ? 0xffffffffull : chunks);
    if (carry < rc.npix) atomicOr(d.status + f, (unsigned)TT_GIF_DEC_STATUS_SHORT);
  }
}

// rule 4: the real row of the row-th row an interlaced image of h rows sends
__device__ __forceinline__ unsigned real_row(unsigned row, unsigned h) {
  const unsigned n0 = (h + 7u) / 8u, n1 = (h + 3u) / 8u, n2 = (h + 1u) / 4u;
  if (row < n0) return 8u * row;
  row -= n0;
  if (row < n1) return 8u * row + 4u;
  row -= n1;
  if (row < n2) return 4u * row + 2u;
  return 2u * (row - n2) + 1u;
}

// grid (workgroups, n): the indices of every chunk of a frame
__global__ __launch_bounds__(DEC_BLOCK) void gif_pixels_kernel(Dec d) {
  __shared__ unsigned short up_s[LEVELS][PLACES];
  __shared__ unsigned short len_s[PLACES];
  __shared__ unsigned char first_s[PLACES], tail_s[PLACES];
  __shared__ unsigned red_s[DEC_WAVES];
  __shared__ unsigned off_s[TILE];
  __shared__ unsigned short node_s[TILE];                        // a code's parent, or 0x8000 | the pixel it stands for
  const unsigned f = blockIdx.y, tid = threadIdx.x;
  const FrameRec rc = d.rec[f];
  if (!rc.ok) return;
  const unsigned nseg = rc.nseg < rc.segcap ? rc.nseg : rc.segcap;
  const int m = clamp_mcs(d.mcs[f]);
  const unsigned clear = 1u << m;
  const unsigned char* __restrict__ src = d.data + d.offsets[f];
  unsigned char* __restrict__ map = d.maps + d.map_offsets[f];
  const unsigned rows = (unsigned)d.rows[f], width = rows ? rc.npix / rows : 0u;
  for (unsigned item = blockIdx.x; item < rc.nchunk; item += gridDim.x) {
    unsigned lo = 0, hi = nseg ? nseg - 1u : 0u;                 // the last segment whose first chunk is not behind the item
    for (int step = 0; step < 32 && lo < hi; ++step) {
      const unsigned mid = lo + (hi - lo + 1u) / 2u;
      if (d.chunkoff[rc.segbase + mid] <= item) lo = mid;
      else hi = mid - 1u;
    }
    const unsigned s = lo;
    const unsigned long long b0 = d.bitoff[rc.segbase + s];
    const unsigned count = d.count[rc.segbase + s];
    const unsigned long long first = d.pixoff[rc.segbase + s], seg_end = first + d.segpix[rc.segbase + s];
    const unsigned long long p0 = first + (unsigned long long)(item - d.chunkoff[rc.segbase + s]) * CHUNK;
    unsigned long long p1 = p0 + CHUNK;
    p1 = p1 < seg_end ? p1 : seg_end;
    p1 = p1 < rc.npix ? p1 : rc.npix;
    build_tables(src, rc.len, b0, count, m, up_s, len_s, first_s, tail_s);
    unsigned long long base = first;                             // the first pixel of the tile's first code
    const unsigned ntiles = (unsigned)(((unsigned long long)count + TILE - 1) / TILE);
    for (unsigned t = 0; t < ntiles && base < p1; ++t) {
      const unsigned long long r = (unsigned long long)t * TILE + tid;
      unsigned length = 0;
      unsigned short packed = 0x8000u;
      bool bad = false;
      if (r < count) {
        const Node nd = node_of(extract(src, rc.len, b0 + bits_before(m, r), width_at(m, r)), r, clear);
        bad = nd.bad;
        packed = nd.par == NONE ? (unsigned short)(0x8000u | nd.lit) : (unsigned short)(nd.par & (PLACES - 1));
        length = nd.par == NONE ? 1u : (unsigned)len_s[nd.par & (PLACES - 1)] + 1u;
      }
      unsigned all;
      const unsigned before = block_scan_excl<DEC_WAVES>(length, red_s, all);
      off_s[tid] = before;
      node_s[tid] = packed;
      if (bad && base + before >= p0 && base + before < p1) atomicOr(d.status + f, (unsigned)TT_GIF_DEC_STATUS_CODE);
      __syncthreads();
      const unsigned have = count - (unsigned long long)t * TILE < (unsigned long long)TILE ? (unsigned)(count - t * TILE) : (unsigned)TILE;
      const unsigned long long from = base > p0 ? base : p0, tile_end = base + all, to = tile_end < p1 ? tile_end : p1;
      for (unsigned long long p = from + tid; p < to; p += DEC_BLOCK) {      // at most CHUNK / DEC_BLOCK trips
        const unsigned q = (unsigned)(p - base);
        unsigned j = 0;
        for (int bit = TILE_STEPS - 1; bit >= 0; --bit) {         // the last code of the tile that starts at or before q
          const unsigned c = j | (1u << bit);
          if (c < have && off_s[c] <= q) j = c;
        }
        const unsigned short nd = node_s[j];
        unsigned px;
        if (nd & 0x8000u) px = nd & 0xffu;
        else {
          const unsigned deep = (unsigned)len_s[nd] - (q - off_s[j]);      // ancestors to climb from the code's own place: length - 1 - i
          if (deep == 0u) px = first_s[(nd + 1u) & (PLACES - 1)];
          else {
            unsigned y = nd, left = deep - 1u;
            for (int lv = 0; lv < LEVELS; ++lv)
              if ((left >> lv) & 1u) y = up_s[lv][y] & (PLACES - 1);
            px = tail_s[y];
          }
        }
        unsigned long long at = p;
        if (rows) {
          const unsigned row = (unsigned)(p / width), col = (unsigned)(p - (unsigned long long)row * width);
          if (row >= rows) continue;
          at = (unsigned long long)real_row(row, rows) * width + col;
        }
        if (at < rc.npix) map[at] = (unsigned char)px;
      }
      base = tile_end;
      __syncthreads();
    }
    __syncthreads();
  }
}

struct Cmp {
  const unsigned char* maps;
  long long maps_bytes;
  const TtGifComposeFrame* table;
  const unsigned char* palettes;
  int n, height, width;
  unsigned initial;
  unsigned char* out;
};

// one lane per canvas pixel (rule 5)
__global__ __launch_bounds__(CMP_BLOCK) void gif_compose_kernel(Cmp c) {
  const long long pixels = (long long)c.height * c.width;
  const long long p = (long long)blockIdx.x * CMP_BLOCK + threadIdx.x;
  if (p >= pixels) return;
  const int y = (int)(p / c.width), x = (int)(p - (long long)y * c.width);
  unsigned cur = c.initial & 0xffffffu, saved = cur;
  bool was_in = false;                                           // the pixel lies in the rectangle of the frame before
  int was_disposal = 0;
  unsigned was_fill = 0;
  for (int f = 0; f < c.n; ++f) {
    if (was_in) {
      if (was_disposal == 2) cur = was_fill;
      else if (was_disposal == 3) cur = saved;
    }
    const TtGifComposeFrame t = c.table[f];
    const bool valid = t.w > 0 && t.h > 0 && t.left >= 0 && t.top >= 0 && (long long)t.left + t.w <= c.width && (long long)t.top + t.h <= c.height &&
                       t.map_offset >= 0 && (long long)t.w * t.h <= c.maps_bytes && t.map_offset <= c.maps_bytes - (long long)t.w * t.h;
    const bool in = valid && x >= t.left && x < t.left + t.w && y >= t.top && y < t.top + t.h;
    saved = cur;
    if (in) {
      const unsigned idx = c.maps[t.map_offset + (long long)(y - t.top) * t.w + (x - t.left)];
      if ((int)idx != t.transparent) {
        const unsigned char* e = c.palettes + ((long long)f * 256 + idx) * 3;
        cur = (unsigned)e[0] | ((unsigned)e[1] << 8) | ((unsigned)e[2] << 16);
      }
    }
    was_in = in;
    was_disposal = t.disposal;
    was_fill = t.fill & 0xffffffu;
    unsigned char* o = c.out + ((long long)f * pixels + p) * 3;
    o[0] = (unsigned char)cur;
    o[1] = (unsigned char)(cur >> 8);
    o[2] = (unsigned char)(cur >> 16);
  }
}

struct Plan {                                      // the workspace, each part at a multiple of 16; ok = 0: refused arguments
  int ok;
  long long segtotal, rec_at, bitoff_at, count_at, segpix_at, pixoff_at, chunkoff_at, total;
};

long long up16(long long v) { return (v + 15) / 16 * 16; }

Plan plan(long long n, long long data_bytes) {
  Plan pl = {};
  if (n <= 0 || n > TT_GIF_MAX_FRAMES || data_bytes <= 0 || data_bytes >= (1ll << 29)) return pl;
  pl.segtotal = 8 * data_bytes / 6 + n;
  const long long part = up16(pl.segtotal * 4);
  pl.rec_at = 0;
  pl.bitoff_at = up16(n * (long long)sizeof(FrameRec));
  pl.count_at = pl.bitoff_at + part;
  pl.segpix_at = pl.count_at + part;
  pl.pixoff_at = pl.segpix_at + part;
  pl.chunkoff_at = pl.pixoff_at + part;
  pl.total = pl.chunkoff_at + part;
  pl.ok = 1;
  return pl;
}

}  // namespace

extern "C" int64_t tt_gif_decode_ws_bytes(int32_t n, int64_t data_bytes) {
  const Plan pl = plan(n, data_bytes);
  return pl.ok ? pl.total : 0;
}

extern "C" int tt_gif_decode_indices(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const uint32_t* lengths, const uint32_t* npix,
                                     const int32_t* min_code_size, const int32_t* rows, const int64_t* map_offsets, int32_t n, uint8_t* maps,
                                     int64_t maps_bytes, uint32_t* status, void* ws, int64_t ws_bytes, tt_stream_t stream) {
  const char* who = "tt_gif_decode_indices";
  const void* ptrs[] = {data, offsets, lengths, npix, min_code_size, rows, map_offsets, maps, status, ws};
  const char* names[] = {"data", "offsets", "lengths", "npix", "min_code_size", "rows", "map_offsets", "maps", "status", "ws"};
  for (int i = 0; i < 10; ++i)
    if (!ptrs[i]) TT_FAIL(TT_EINVAL, "%s: null %s", who, names[i]);
  if (n <= 0 || data_bytes <= 0 || maps_bytes <= 0)
    TT_FAIL(TT_EINVAL, "%s: empty problem (n = %d, data_bytes = %lld, maps_bytes = %lld)", who, n, (long long)data_bytes, (long long)maps_bytes);
  if ((uintptr_t)offsets & 7) TT_FAIL(TT_EINVAL, "%s: offsets is not 8-byte aligned", who);
  if ((uintptr_t)map_offsets & 7) TT_FAIL(TT_EINVAL, "%s: map_offsets is not 8-byte aligned", who);
  for (int i = 2; i <= 5; ++i)
    if ((uintptr_t)ptrs[i] & 3) TT_FAIL(TT_EINVAL, "%s: %s is not 4-byte aligned", who, names[i]);
  if ((uintptr_t)status & 3) TT_FAIL(TT_EINVAL, "%s: status is not 4-byte aligned", who);
  if ((uintptr_t)ws & 15) TT_FAIL(TT_EINVAL, "%s: ws is not 16-byte aligned", who);
  if (n > TT_GIF_MAX_FRAMES) TT_FAIL(TT_EUNSUPPORTED, "%s: %d frames: more than one grid covers (%d)", who, n, TT_GIF_MAX_FRAMES);
  if (data_bytes >= (1ll << 29))
    TT_FAIL(TT_EUNSUPPORTED, "%s: data_bytes = %lld: the kernels' 32-bit bit offsets address fewer than 2^29 = 536870912", who, (long long)data_bytes);
  if (maps_bytes >= (1ll << 31)) TT_FAIL(TT_EUNSUPPORTED, "%s: maps_bytes = %lld (fewer than 2^31 = 2147483648)", who, (long long)maps_bytes);
  const Plan pl = plan(n, data_bytes);
  if (!pl.ok || ws_bytes < pl.total)
    TT_FAIL(TT_EINVAL, "%s: ws too small: %lld bytes, tt_gif_decode_ws_bytes = %lld", who, (long long)ws_bytes, pl.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  Dec d;
  d.data = data;
  d.data_bytes = data_bytes;
  d.offsets = (const long long*)offsets;
  d.lengths = lengths;
  d.npix = npix;
  d.mcs = min_code_size;
  d.rows = rows;
  d.map_offsets = (const long long*)map_offsets;
  d.n = n;
  d.maps = maps;
  d.maps_bytes = maps_bytes;
  d.status = status;
  d.rec = (FrameRec*)(w + pl.rec_at);
  d.segtotal = (unsigned long long)pl.segtotal;
  d.bitoff = (unsigned*)(w + pl.bitoff_at);
  d.count = (unsigned*)(w + pl.count_at);
  d.segpix = (unsigned*)(w + pl.segpix_at);
  d.pixoff = (unsigned*)(w + pl.pixoff_at);
  d.chunkoff = (unsigned*)(w + pl.chunkoff_at);
  if (hipMemsetAsync(status, 0, (size_t)n * sizeof(uint32_t), st) != hipSuccess || hipMemsetAsync(maps, 0, (size_t)maps_bytes, st) != hipSuccess)
    TT_FAIL(TT_ELAUNCH, "%s: hipMemsetAsync failed", who);
  // workgroups that stride over a frame's segments and chunks: about 2048 in all, never more than there can be segments
  long long per = 2048 / n < 1 ? 1 : 2048 / n;
  per = per > 1024 ? 1024 : per;
  const long long seg_groups = per < pl.segtotal ? per : pl.segtotal;
  hipLaunchKernelGGL(gif_clears_kernel, dim3((unsigned)n), dim3(CLR_BLOCK), 0, st, d);
  hipLaunchKernelGGL(gif_lengths_kernel, dim3((unsigned)seg_groups, (unsigned)n), dim3(DEC_BLOCK), 0, st, d);
  hipLaunchKernelGGL(gif_offsets_kernel, dim3((unsigned)n), dim3(CLR_BLOCK), 0, st, d);
  hipLaunchKernelGGL(gif_pixels_kernel, dim3((unsigned)per, (unsigned)n), dim3(DEC_BLOCK), 0, st, d);
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}

extern "C" int tt_gif_compose(const uint8_t* maps, int64_t maps_bytes, const TtGifComposeFrame* table, const uint8_t* palettes, int32_t n, int32_t height,
                              int32_t width, uint32_t initial, uint8_t* out, tt_stream_t stream) {
  const char* who = "tt_gif_compose";
  if (!maps || !table || !palettes || !out) TT_FAIL(TT_EINVAL, "%s: null %s", who, !maps ? "maps" : (!table ? "table" : (!palettes ? "palettes" : "out")));
  if (n <= 0 || height <= 0 || width <= 0 || maps_bytes <= 0)
    TT_FAIL(TT_EINVAL, "%s: empty problem (n = %d, %d x %d, maps_bytes = %lld)", who, n, height, width, (long long)maps_bytes);
  if ((uintptr_t)table & 7) TT_FAIL(TT_EINVAL, "%s: table is not 8-byte aligned", who);
  if (n > TT_GIF_MAX_FRAMES) TT_FAIL(TT_EUNSUPPORTED, "%s: %d frames (at most %d)", who, n, TT_GIF_MAX_FRAMES);
  if ((long long)height * width > TT_GIF_MAX_PIXELS)
    TT_FAIL(TT_EUNSUPPORTED, "%s: a canvas of %d x %d pixels (at most TT_GIF_MAX_PIXELS = %d)", who, height, width, TT_GIF_MAX_PIXELS);
  Cmp c;
  c.maps = maps;
  c.maps_bytes = maps_bytes;
  c.table = table;
  c.palettes = palettes;
  c.n = n;
  c.height = height;
  c.width = width;
  c.initial = initial;
  c.out = out;
  const long long pixels = (long long)height * width;
  hipLaunchKernelGGL(gif_compose_kernel, dim3((unsigned)((pixels + CMP_BLOCK - 1) / CMP_BLOCK)), dim3(CMP_BLOCK), 0, (hipStream_t)stream, c);
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}
