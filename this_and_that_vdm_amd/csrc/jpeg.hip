// libttvdm: the device half of the JPEG export (include/ttvdm.h): tt_jpeg_coeffs -- colour conversion, 4:2:0 cell sums, the 8 x 8 integer
// DCT, the quantiser and the zig-zag of every block of uint8 NHWC frames, in scan order, with the frames' symbol counts -- and
// tt_jpeg_scan -- the Huffman-coded, byte-stuffed scan of every frame from those coefficients and a code table; tt_jpeg_scan_restart and
// tt_jpeg_counts_restart -- the same with restart intervals (rule 6a), of which tt_jpeg_scan is the interval 0.
// Integer arithmetic only; atomics are integer adds and ORs, which commute: every call gives the same bytes.
#include "common.h"
#include "block_scan.h"
#include "jpeg_host.h"

namespace {

constexpr int CBLOCK = 256;                         // lanes of a coefficient tile: TILE_W pixels across, one MCU row down
constexpr int TILE_W = 256;
constexpr int SBLOCK = 256;                         // lanes of the per-block kernels (bits, counts, emit) and of a stuffing chunk
constexpr int SCAN_BLOCK = 1024, SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int CHUNK = TT_JPEG_CHUNK;
static_assert(CHUNK == 16 * SBLOCK, "a lane holds one 16-byte unit of a stuffing chunk");
static_assert(TT_JPEG_COUNT_WORDS == 4 * TT_JPEG_TABLE_WORDS && TT_JPEG_TABLE_WORDS == 256, "four tables of 256 symbols");

// ZZ[k]: the natural (row-major) index of the k-th coefficient of the zig-zag scan
__device__ constexpr int ZZ[64] = TT_JPEG_ZIGZAG;

// ---------------------------------------------------------------- rule 2: colour
__device__ __forceinline__ int to_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int to_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int to_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// ---------------------------------------------------------------- rule 4: jfdctint's pass over eight values
template <bool FIRST> __device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
template <bool FIRST> __device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int N = FIRST ? 13 - 2 : 13 + 2;
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) { d0 = (t10 + t11) << 2; d4 = (t10 - t11) << 2; }
  else { d0 = descale<FIRST>(t10 + t11, 2); d4 = descale<FIRST>(t10 - t11, 2); }
  const int z1 = (t12 + t13) * 4433;
  d2 = descale<FIRST>(z1 + t13 * 6270, N);
  d6 = descale<FIRST>(z1 - t12 * 15137, N);
  const int y1 = t4 + t7, y2 = t5 + t6, y3 = t4 + t6, y4 = t5 + t7, z5 = (y3 + y4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  const int b1 = -y1 * 7373, b2 = -y2 * 20995, b3 = -y3 * 16069 + z5, b4 = -y4 * 3196 + z5;
  d7 = descale<FIRST>(a4 + b1 + b3, N);
  d5 = descale<FIRST>(a5 + b2 + b4, N);
  d3 = descale<FIRST>(a6 + b2 + b3, N);
  d1 = descale<FIRST>(a7 + b1 + b4, N);
}

// one pixel of frame `src` (h x w x ch) with both coordinates held inside the frame: edge replication
__device__ __forceinline__ void pixel(const unsigned char* __restrict__ src, int h, int w, int ch, int y, int x, int& r, int& g, int& b) {
  const unsigned char* p = src + ((long long)min(y, h - 1) * w + min(x, w - 1)) * ch;
  r = p[0];
  if (ch == 3) { g = p[1]; b = p[2]; } else { g = r; b = r; }
}

// grid (tiles per MCU row x MCU rows, n): a tile is one MCU row down and TILE_W pixels across.  SUB: 4:2:0 (16 x 16 MCUs of 6 blocks).
// The tile's samples go to LDS once, converted (and, SUB, the chroma cells summed); then one lane per block transforms it.
template <bool SUB> __global__ __launch_bounds__(CBLOCK) void jpeg_coeffs_kernel(const unsigned char* __restrict__ frames, int h, int w, int ch,
                                                                                TtJpegGeometry geo, int tiles_x, TtJpegQuant quant,
                                                                                short* __restrict__ coeffs, long long blocks) {
  constexpr int MCU = SUB ? 16 : 8, ROWS = MCU, CW = SUB ? TILE_W / 2 : TILE_W, MCUS = TILE_W / MCU;
  __shared__ __attribute__((aligned(16))) unsigned char y_s[ROWS][TILE_W];
  __shared__ __attribute__((aligned(16))) unsigned char c_s[2][8][CW];
  __shared__ int dc_s[MCUS][4];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % tiles_x, mcu_y = blockIdx.x / tiles_x;
  const int x0 = tile * TILE_W, y0 = mcu_y * MCU;
  const unsigned char* __restrict__ src = frames + (long long)blockIdx.y * h * w * ch;
  if (SUB) {
    const int hc = (h + 1) >> 1;
    for (int cell = tid; cell < 8 * CW; cell += CBLOCK) {
      const int cy = cell / CW, cx = cell % CW;                      // the chroma sample of this tile; its 2 x 2 luminance samples
      int sb = 0, sr = 0;
      int r, g, b;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pixel(src, h, w, ch, y0 + 2 * cy + (k >> 1), x0 + 2 * cx + (k & 1), r, g, b);
        y_s[2 * cy + (k >> 1)][2 * cx + (k & 1)] = (unsigned char)to_y(r, g, b);
        sb += to_cb(r, g, b);
        sr += to_cr(r, g, b);
      }
      const int gy = (y0 >> 1) + cy;
      if (gy >= hc) {                                                // below the chroma plane: its LAST ROW again, not the source's
        sb = 0;
        sr = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pixel(src, h, w, ch, 2 * (hc - 1) + (k >> 1), x0 + 2 * cx + (k & 1), r, g, b);
          sb += to_cb(r, g, b);
          sr += to_cr(r, g, b);
        }
      }
      const int bias = 1 + (cx & 1);                                 // x0 / 2 is even: the tile's parity is the plane's
      c_s[0][cy][cx] = (unsigned char)((sb + bias) >> 2);
      c_s[1][cy][cx] = (unsigned char)((sr + bias) >> 2);
    }
  } else {
    for (int i = tid; i < 8 * TILE_W; i += CBLOCK) {
      const int yy = i / TILE_W, xx = i % TILE_W;
      int r, g, b;
      pixel(src, h, w, ch, y0 + yy, x0 + xx, r, g, b);
      if (ch == 3) {
        y_s[yy][xx] = (unsigned char)to_y(r, g, b);
        c_s[0][yy][xx] = (unsigned char)to_cb(r, g, b);
        c_s[1][yy][xx] = (unsigned char)to_cr(r, g, b);
      } else {
        y_s[yy][xx] = (unsigned char)r;
      }
    }
  }
  __syncthreads();
  // lane -> (MCU of the tile, block of the MCU)
  const int bpm = geo.blocks_per_mcu;
  const int m = tid / bpm, k = tid % bpm;
  const int mcu_x = tile * MCUS + m;
  const bool active = m < MCUS && mcu_x < geo.mcus_x;
  bool real = active;
  int comp = 0;
  const unsigned char* base = &y_s[0][0];
  int pitch = TILE_W;
  if (SUB) {
    if (k < 4) {
      const int by = 2 * mcu_y + (k >> 1), bx = 2 * mcu_x + (k & 1);
      real = active && by < (h + 7) / 8 && bx < (w + 7) / 8;
      base = &y_s[(k >> 1) * 8][m * 16 + (k & 1) * 8];
    } else {
      comp = k - 3;
      base = &c_s[k - 4][0][m * 8];
      pitch = CW;
    }
  } else {
    comp = k;
    base = k == 0 ? &y_s[0][m * 8] : &c_s[k - 1][0][m * 8];
  }
  if (!active) base = &y_s[0][0];
  short* __restrict__ out = coeffs + ((long long)blockIdx.y * blocks + ((long long)mcu_y * geo.mcus_x + mcu_x) * bpm + k) * 64;
  if (real) {
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint2 v = *(const uint2*)(base + r * pitch);
#pragma unroll
      for (int c = 0; c < 8; ++c) d[r * 8 + c] = (int)(((c < 4 ? v.x : v.y) >> (8 * (c & 3))) & 0xffu) - 128;
      fdct8<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
#pragma unroll
    for (int i = 0; i < 64; ++i) {                                   // rule 5
      const int q = 8 * (int)(comp ? quant.q[1][i] : quant.q[0][i]);
      const int v = d[i], mag = (int)((unsigned)(abs(v) + (q >> 1)) / (unsigned)q);
      d[i] = v < 0 ? -mag : mag;
    }
    if (SUB && k < 4) dc_s[m][k] = d[0];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      unsigned wd[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) wd[j] = ((unsigned)d[ZZ[8 * u + 2 * j]] & 0xffffu) | ((unsigned)d[ZZ[8 * u + 2 * j + 1]] << 16);
      *(uint4*)(out + 8 * u) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
  }
  if (SUB) {
    __syncthreads();
    if (active && !real) {                                           // a dummy block: the DC of the block coded before it in this MCU
      int dc = dc_s[m][0];                                           // (block 0 of an MCU is never a dummy)
      for (int j = 1; j < k; ++j) {
        const int by = 2 * mcu_y + (j >> 1), bx = 2 * mcu_x + (j & 1);
        if (by < (h + 7) / 8 && bx < (w + 7) / 8) dc = dc_s[m][j];
      }
      *(uint4*)out = make_uint4((unsigned)dc & 0xffffu, 0u, 0u, 0u);
#pragma unroll
      for (int u = 1; u < 8; ++u) *(uint4*)(out + 8 * u) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// ---------------------------------------------------------------- rule 6: a block's symbols
// which component block b of a frame's scan belongs to (0 Y, else chroma), and the block whose DC it is coded against (-1: none).
// ri_blocks: the blocks of a restart interval (0: none): the first MCU of an interval is coded against no block, like the frame's first
__device__ __forceinline__ void block_place(long long b, int bpm, long long ri_blocks, int& chroma, long long& pred) {
  const int k = (int)(b % bpm);
  chroma = bpm == 6 ? k >= 4 : k > 0;
  const long long back = bpm == 6 ? (k >= 4 ? 6 : (k == 0 ? 3 : 1)) : bpm;
  const bool fresh = b < bpm || (ri_blocks > 0 && b % ri_blocks < bpm);
  pred = (bpm == 6 && k > 0 && k < 4) ? b - 1 : (fresh ? -1 : b - back);
}
__device__ __forceinline__ int category(int v) { return 32 - __clz(abs(v)); }
__device__ __forceinline__ unsigned magnitude(int v, int n) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

// calls f(table: 0 DC / 1 AC, symbol, magnitude bits, how many of them) for every symbol of the block at `c` in order
template <typename F> __device__ __forceinline__ void walk_block(const short* __restrict__ c, int pred_dc, F&& f) {
  unsigned wd[32];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const uint4 v = *(const uint4*)(c + 8 * u);
    wd[4 * u] = v.x; wd[4 * u + 1] = v.y; wd[4 * u + 2] = v.z; wd[4 * u + 3] = v.w;
  }
  const int diff = (int)(short)(wd[0] & 0xffffu) - pred_dc;
  int n = category(diff);
  f(0, n, magnitude(diff, n), n);
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int v = (int)(short)((wd[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    if (v == 0) { ++run; continue; }
    while (run > 15) { f(1, 0xF0, 0u, 0); run -= 16; }
    n = category(v);
    f(1, (run << 4) | n, magnitude(v, n), n);
    run = 0;
  }
  if (run > 0) f(1, 0x00, 0u, 0);
}

__device__ __forceinline__ int pred_of(const short* __restrict__ frame_coeffs, long long pred) { return pred < 0 ? 0 : (int)frame_coeffs[pred * 64]; }

// grid (ceil(blocks / SBLOCK), n): one lane per block; the frame's counts are summed in LDS first
__global__ __launch_bounds__(SBLOCK) void jpeg_counts_kernel(const short* __restrict__ coeffs, long long blocks, int bpm, long long ri_blocks,
                                                             unsigned* __restrict__ counts) {
  __shared__ unsigned cnt_s[TT_JPEG_COUNT_WORDS];
  for (int i = threadIdx.x; i < TT_JPEG_COUNT_WORDS; i += SBLOCK) cnt_s[i] = 0u;
  __syncthreads();
  const long long b = (long long)blockIdx.x * SBLOCK + threadIdx.x;
  const short* __restrict__ fc = coeffs + (long long)blockIdx.y * blocks * 64;
  if (b < blocks) {
    int chroma;
    long long pred;
    block_place(b, bpm, ri_blocks, chroma, pred);
    unsigned* t = cnt_s + (chroma ? 2 * TT_JPEG_TABLE_WORDS : 0);
    walk_block(fc + b * 64, pred_of(fc, pred), [&](int ac, int sym, unsigned, int) { atomicAdd(&t[ac * TT_JPEG_TABLE_WORDS + (sym & 0xff)], 1u); });
  }
  __syncthreads();
  unsigned* __restrict__ dst = counts + (long long)blockIdx.y * TT_JPEG_COUNT_WORDS;
  for (int i = threadIdx.x; i < TT_JPEG_COUNT_WORDS; i += SBLOCK)
    if (cnt_s[i]) atomicAdd(&dst[i], cnt_s[i]);
}

__device__ __forceinline__ void load_tables(unsigned* tab_s, const unsigned* __restrict__ tables, int ntables) {
  const unsigned* __restrict__ t = tables + (ntables > 1 ? (long long)blockIdx.y * TT_JPEG_COUNT_WORDS : 0);
  for (int i = threadIdx.x; i < TT_JPEG_COUNT_WORDS; i += SBLOCK) tab_s[i] = t[i];
  __syncthreads();
}
// a symbol's code and its length; whatever the table holds, a code with its magnitude bits stays within 16 + 11 bits
__device__ __forceinline__ void code_of(const unsigned* t, int ac, int sym, unsigned& code, int& len) {
  const unsigned e = t[ac * TT_JPEG_TABLE_WORDS + (sym & 0xff)];
  len = (int)min(e >> 16, 16u);
  code = e & ((1u << len) - 1u);
}

// the bits of every block: grid as jpeg_counts_kernel
__global__ __launch_bounds__(SBLOCK) void jpeg_bits_kernel(const short* __restrict__ coeffs, long long blocks, int bpm, long long ri_blocks,
                                                           const unsigned* __restrict__ tables, int ntables, unsigned* __restrict__ bits) {
  __shared__ unsigned tab_s[TT_JPEG_COUNT_WORDS];
  load_tables(tab_s, tables, ntables);
  const long long b = (long long)blockIdx.x * SBLOCK + threadIdx.x;
  if (b >= blocks) return;
  const short* __restrict__ fc = coeffs + (long long)blockIdx.y * blocks * 64;
  int chroma;
  long long pred;
  block_place(b, bpm, ri_blocks, chroma, pred);
  const unsigned* t = tab_s + (chroma ? 2 * TT_JPEG_TABLE_WORDS : 0);
  unsigned total = 0u;
  walk_block(fc + b * 64, pred_of(fc, pred), [&](int ac, int sym, unsigned, int n) {
    unsigned code;
    int len;
    code_of(t, ac, sym, code, len);
    total += (unsigned)(len + min(n, 11));
  });
  bits[(long long)blockIdx.y * blocks + b] = total;
}

// grid (n): the blocks' bit offsets inside their frame, and the frame's unstuffed bytes
// With restart intervals of ri_blocks blocks (0: none) every interval but the last is filled to a whole byte and followed by a marker of
// 16 bits: extra[i] gets the bits that adds before interval i, so block b of interval i starts at bit bits[b] + extra[i].
__global__ __launch_bounds__(SCAN_BLOCK) void jpeg_offsets_kernel(unsigned* __restrict__ bits, long long blocks, unsigned* __restrict__ plain_bytes,
                                                                  long long ri_blocks, long long intervals, unsigned* __restrict__ extra) {
  __shared__ unsigned red_s[SCAN_WAVES + 1];
  unsigned* __restrict__ fb = bits + (long long)blockIdx.x * blocks;
  const unsigned total = scan_in_place<SCAN_WAVES>(fb, blocks, red_s);
  unsigned carry = 0u;
  if (ri_blocks > 0) {                                               // uniform; scan_in_place ended on a barrier: fb is final
    unsigned* __restrict__ fx = extra + (long long)blockIdx.x * intervals;
    for (long long at = 0; at < intervals; at += SCAN_BLOCK) {
      const long long i = at + threadIdx.x;
      unsigned mine = 0u;
      if (i < intervals - 1 && (i + 1) * ri_blocks < blocks) mine =((0u - (fb[(i + 1) * ri_blocks] - fb[i * ri_blocks])) & 7u) + 16u;       // (i + 1) ri_blocks < blocks
      unsigned all;
      const unsigned before = carry + block_scan_excl<SCAN_WAVES>(mine, red_s, all);
      if (i < intervals) fx[i] = before;
      carry += all;
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) plain_bytes[blockIdx.x] = (total + carry + 7u) >> 3;
}

// the bits themselves, MSB first, into 32-bit words whose most significant byte is the stream's first: one lane per block.  A lane's
// first and last word are shared with its neighbours (OR); the words between are its own.  `words` is zeroed before.
struct BitWriter {
  unsigned* __restrict__ words;
  long long limit;             // words of the frame's region
  unsigned long long acc;
  int nacc;
  long long word;
  bool first;
  __device__ __forceinline__ void put(unsigned v, int len) {
    acc = (acc << len) | v;
    nacc += len;
    if (nacc >= 32) {
      nacc -= 32;
      const unsigned out = (unsigned)(acc >> nacc);
      if (word < limit) {
        if (first) atomicOr(&words[word], out); else words[word] = out;
      }
      first = false;
      ++word;
    }
  }
  __device__ __forceinline__ void flush() {
    if (nacc > 0 && word < limit) atomicOr(&words[word], (unsigned)(acc << (32 - nacc)));
  }
};

// With restart intervals (ri_blocks > 0) the lane of an interval's last block fills the byte with one-bits like the frame's last lane, writes
// the marker FF D0 + (interval mod 8) behind it unless the frame ends there, and sets the bit of the marker's FF byte in the frame's
// bitmap `marks` (zeroed before): the stuffing passes tell it from a data FF by that position, never by its value.
__global__ __launch_bounds__(SBLOCK) void jpeg_emit_kernel(const short* __restrict__ coeffs, long long blocks, int bpm, long long ri_blocks,
                                                           const unsigned* __restrict__ tables, int ntables, const unsigned* __restrict__ offsets,
                                                           const unsigned* __restrict__ extra, long long intervals, unsigned* __restrict__ plain,
                                                           long long plain_stride, unsigned* __restrict__ marks, long long mark_words) {
  __shared__ unsigned tab_s[TT_JPEG_COUNT_WORDS];
  load_tables(tab_s, tables, ntables);
  const long long b = (long long)blockIdx.x * SBLOCK + threadIdx.x;
  if (b >= blocks) return;
  const short* __restrict__ fc = coeffs + (long long)blockIdx.y * blocks * 64;
  int chroma;
  long long pred;
  block_place(b, bpm, ri_blocks, chroma, pred);
  const unsigned* t = tab_s + (chroma ? 2 * TT_JPEG_TABLE_WORDS : 0);
  const long long interval = ri_blocks > 0 ? min(b / ri_blocks, intervals - 1) : 0;
  const unsigned at = offsets[(long long)blockIdx.y * blocks + b] + (ri_blocks > 0 ? extra[(long long)blockIdx.y * intervals + interval] : 0u);
  BitWriter bw{plain + (long long)blockIdx.y * (plain_stride / 4), plain_stride / 4, 0ull, (int)(at & 31u), (long long)(at >> 5), true};
  unsigned pos = at;
  walk_block(fc + b * 64, pred_of(fc, pred), [&](int ac, int sym, unsigned mag, int n) {
    unsigned code;
    int len;
    code_of(t, ac, sym, code, len);
    n = min(n, 11);
    bw.put((code << n) | (mag & ((1u << n) - 1u)), len + n);
    pos += (unsigned)(len + n);
  });
  const bool closes = ri_blocks > 0 && b != blocks - 1 && (b + 1) % ri_blocks == 0;
  if ((b == blocks - 1 || closes) && (pos & 7u)) {                   // the frame's (the interval's) last byte is filled with one-bits
    const int pad = 8 - (int)(pos & 7u);
    bw.put((1u << pad) - 1u, pad);
    pos += (unsigned)pad;
  }
  if (closes) {
    bw.put(0xffd0u + (unsigned)(interval & 7), 16);
    const long long byte = (long long)(pos >> 3);
    if (byte < plain_stride && (byte >> 5) < mark_words) atomicOr(&marks[(long long)blockIdx.y * mark_words + (byte >> 5)], 1u << (byte & 31));
  }
  bw.flush();
}

// ---------------------------------------------------------------- byte stuffing: count the FF bytes per chunk, scan, scatter
// the lane's 16 bytes of its frame's unstuffed stream, in stream order; `have`: how many of them are inside the stream
__device__ __forceinline__ void chunk_bytes(const unsigned* __restrict__ plain, long long plain_stride, const unsigned* __restrict__ plain_bytes,
                                            unsigned by[4], int& have, long long& at) {
  at = (long long)blockIdx.x * CHUNK + 16 * threadIdx.x;
  const long long total = min((long long)plain_bytes[blockIdx.y], plain_stride);
  have = (int)max(0ll, min(16ll, total - at));
  by[0] = by[1] = by[2] = by[3] = 0u;
  if (have > 0) {
    const uint4 v = *(const uint4*)((const unsigned char*)plain + (long long)blockIdx.y * plain_stride + at);
    by[0] = v.x; by[1] = v.y; by[2] = v.z; by[3] = v.w;
  }
}
__device__ __forceinline__ unsigned byte_at(const unsigned by[4], int j) { return (by[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu; }
// bit j: byte j of the lane's 16 is a restart marker's FF and is not stuffed (marks NULL: no restart intervals, none is)
__device__ __forceinline__ unsigned chunk_marks(const unsigned* __restrict__ marks, long long mark_words, long long at, int have) {
  if (!marks || have <= 0 || (at >> 5) >= mark_words) return 0u;
  return (marks[(long long)blockIdx.y * mark_words + (at >> 5)] >> (at & 16)) & 0xffffu;
}

// grid (chunks, n)
__global__ __launch_bounds__(SBLOCK) void jpeg_ff_count_kernel(const unsigned* __restrict__ plain, long long plain_stride, const unsigned* __restrict__ plain_bytes,
                                                               unsigned* __restrict__ chunk_ff, int chunks, const unsigned* __restrict__ marks,
                                                               long long mark_words) {
  __shared__ unsigned red_s[SBLOCK / 64];
  unsigned by[4];
  int have;
  long long at;
  chunk_bytes(plain, plain_stride, plain_bytes, by, have, at);
  const unsigned mk = chunk_marks(marks, mark_words, at, have);
  unsigned ff = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) ff += j < have && byte_at(by, j) == 0xffu && !((mk >> j) & 1u);
  const unsigned all = block_sum<SBLOCK / 64>(ff, red_s);
  if (threadIdx.x == 0) chunk_ff[(long long)blockIdx.y * chunks + blockIdx.x] = all;
}

// grid (n): the FF bytes before every chunk, and the frame's stuffed length
__global__ __launch_bounds__(SCAN_BLOCK) void jpeg_ff_scan_kernel(unsigned* __restrict__ chunk_ff, int chunks, const unsigned* __restrict__ plain_bytes,
                                                                  unsigned* __restrict__ lengths) {
  __shared__ unsigned red_s[SCAN_WAVES + 1];
  const unsigned total = scan_in_place<SCAN_WAVES>(chunk_ff + (long long)blockIdx.x * chunks, (long long)chunks, red_s);
  if (threadIdx.x == 0) lengths[blockIdx.x] = plain_bytes[blockIdx.x] + total;
}

// grid (chunks, n)
__global__ __launch_bounds__(SBLOCK) void jpeg_stuff_kernel(const unsigned* __restrict__ plain, long long plain_stride, const unsigned* __restrict__ plain_bytes,
                                                            const unsigned* __restrict__ chunk_ff, int chunks, unsigned char* __restrict__ out, long long stride,
                                                            const unsigned* __restrict__ marks, long long mark_words) {
  __shared__ unsigned red_s[SBLOCK / 64];
  unsigned by[4];
  int have;
  long long at;
  chunk_bytes(plain, plain_stride, plain_bytes, by, have, at);
  const unsigned mk = chunk_marks(marks, mark_words, at, have);
  unsigned ff = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) ff += j < have && byte_at(by, j) == 0xffu && !((mk >> j) & 1u);
  unsigned all;
  const unsigned before = block_scan_excl<SBLOCK / 64>(ff, red_s, all);
  long long pos = at + chunk_ff[(long long)blockIdx.y * chunks + blockIdx.x] + before;
  unsigned char* __restrict__ dst = out + (long long)blockIdx.y * stride;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < have) {
      const unsigned v = byte_at(by, j);
      if (pos < stride) dst[pos] = (unsigned char)v;
      ++pos;
      if (v == 0xffu && !((mk >> j) & 1u)) {
        if (pos < stride) dst[pos] = 0;
        ++pos;
      }
    }
  }
}

}  // namespace

extern "C" int tt_jpeg_coeffs(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t quality, int32_t subsampling, int16_t* coeffs,
                              uint32_t* counts, tt_stream_t stream) {
  if (!frames || !coeffs) TT_FAIL(TT_EINVAL, "tt_jpeg_coeffs: null %s", !frames ? "frames" : "coeffs");
  const int rc = tt_jpeg_refuse_shape("tt_jpeg_coeffs", n, h, w, ch, subsampling, "; JPEG has no alpha");
  if (rc != TT_OK) return rc;
  if (quality < 1 || quality > 100) TT_FAIL(TT_EINVAL, "tt_jpeg_coeffs: quality = %d (1 to 100)", quality);
  if ((uintptr_t)coeffs & 15) TT_FAIL(TT_EINVAL, "tt_jpeg_coeffs: coeffs is not 16-byte aligned");
  if ((uintptr_t)counts & 15) TT_FAIL(TT_EINVAL, "tt_jpeg_coeffs: counts is not 16-byte aligned");
  const TtJpegGeometry geo = tt_jpeg_geometry(h, w, ch, subsampling);
  const long long blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  TtJpegQuant quant;
  tt_jpeg_fill_quant(quality, &quant);
  const bool sub = geo.blocks_per_mcu == 6;
  const int tiles_x = (geo.mcus_x * (sub ? 16 : 8) + TILE_W - 1) / TILE_W;
  const dim3 grid((unsigned)(tiles_x * geo.mcus_y), (unsigned)n);
  if (sub)
    hipLaunchKernelGGL(jpeg_coeffs_kernel<true>, grid, dim3(CBLOCK), 0, (hipStream_t)stream, (const unsigned char*)frames, (int)h, (int)w, (int)ch, geo,
                       tiles_x, quant, (short*)coeffs, blocks);
  else
    hipLaunchKernelGGL(jpeg_coeffs_kernel<false>, grid, dim3(CBLOCK), 0, (hipStream_t)stream, (const unsigned char*)frames, (int)h, (int)w, (int)ch, geo,
                       tiles_x, quant, (short*)coeffs, blocks);
  if (counts) {
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * TT_JPEG_COUNT_WORDS * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) TT_FAIL(TT_ELAUNCH, "tt_jpeg_coeffs: zeroing counts: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(jpeg_counts_kernel, dim3((unsigned)((blocks + SBLOCK - 1) / SBLOCK), (unsigned)n), dim3(SBLOCK), 0, (hipStream_t)stream,
                       (const short*)coeffs, blocks, (int)geo.blocks_per_mcu, 0ll, (unsigned*)counts);
  }
  TT_CHECK_LAUNCH("tt_jpeg_coeffs");
  return TT_OK;
}

extern "C" int tt_jpeg_counts_restart(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval,
                                      uint32_t* counts, tt_stream_t stream) {
  if (!coeffs || !counts) TT_FAIL(TT_EINVAL, "tt_jpeg_counts_restart: null %s", !coeffs ? "coeffs" : "counts");
  const int rc = tt_jpeg_refuse_shape("tt_jpeg_counts_restart", n, h, w, ch, subsampling, "; JPEG has no alpha");
  if (rc != TT_OK) return rc;
  if (restart_interval < 0 || restart_interval > 65535) TT_FAIL(TT_EINVAL, "tt_jpeg_counts_restart: restart_interval = %d (0: none, to 65535 MCUs)", restart_interval);
  if ((uintptr_t)coeffs & 15) TT_FAIL(TT_EINVAL, "tt_jpeg_counts_restart: coeffs is not 16-byte aligned");
  if ((uintptr_t)counts & 15) TT_FAIL(TT_EINVAL, "tt_jpeg_counts_restart: counts is not 16-byte aligned");
  const TtJpegGeometry geo = tt_jpeg_geometry(h, w, ch, subsampling);
  const long long blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * TT_JPEG_COUNT_WORDS * sizeof(uint32_t), (hipStream_t)stream);
  if (e != hipSuccess) TT_FAIL(TT_ELAUNCH, "tt_jpeg_counts_restart: zeroing counts: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(jpeg_counts_kernel, dim3((unsigned)((blocks + SBLOCK - 1) / SBLOCK), (unsigned)n), dim3(SBLOCK), 0, (hipStream_t)stream, (const short*)coeffs,
                     blocks, (int)geo.blocks_per_mcu, (long long)restart_interval * geo.blocks_per_mcu, (unsigned*)counts);
  TT_CHECK_LAUNCH("tt_jpeg_counts_restart");
  return TT_OK;
}

// tt_jpeg_scan is the restart interval 0 of tt_jpeg_scan_restart: the same kernels, with no interval to close and no bitmap to read
static int scan_frames(const char* who, const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t ri,
                       const uint32_t* tables, int32_t ntables, uint8_t* out, int64_t cap, uint32_t* lengths, void* ws, int64_t ws_bytes, tt_stream_t stream) {
  if (!coeffs || !tables || !out || !lengths || !ws)
    TT_FAIL(TT_EINVAL, "%s: null %s", who, !coeffs ? "coeffs" : (!tables ? "tables" : (!out ? "out" : (!lengths ? "lengths" : "ws"))));
  const int rc = tt_jpeg_refuse_shape(who, n, h, w, ch, subsampling, "; JPEG has no alpha");
  if (rc != TT_OK) return rc;
  if (ntables != 1 && ntables != n) TT_FAIL(TT_EINVAL, "%s: ntables = %d (1, or one set per frame: %d)", who, ntables, n);
  if ((uintptr_t)coeffs & 15) TT_FAIL(TT_EINVAL, "%s: coeffs is not 16-byte aligned", who);
  if ((uintptr_t)tables & 15) TT_FAIL(TT_EINVAL, "%s: tables is not 16-byte aligned", who);
  if ((uintptr_t)out & 15) TT_FAIL(TT_EINVAL, "%s: out is not 16-byte aligned", who);
  if ((uintptr_t)lengths & 3) TT_FAIL(TT_EINVAL, "%s: lengths is not 4-byte aligned", who);
  if ((uintptr_t)ws & 15) TT_FAIL(TT_EINVAL, "%s: ws is not 16-byte aligned", who);
  if (ri < 0 || ri > 65535) TT_FAIL(TT_EINVAL, "%s: restart_interval = %d (0: none, to 65535 MCUs)", who, ri);
  const long long stride = tt_jpeg_scan_bound_restart(h, w, ch, subsampling, ri);
  if (stride >= (1ll << 31)) TT_FAIL(TT_EUNSUPPORTED, "%s: a scan bound of %lld bytes per frame (below 2^31)", who, stride);
  if (cap < (long long)n * stride)
    TT_FAIL(TT_EINVAL, "%s: cap too small: %lld bytes, %d frames at the scan bound = %lld take %lld", who, (long long)cap, n, stride, (long long)n * stride);
  const TtJpegScanWs lay(n, h, w, ch, subsampling, ri);
  if (ws_bytes < lay.total)
    TT_FAIL(TT_EINVAL, "%s: ws too small: %lld bytes, the size query gives %lld", who, (long long)ws_bytes, (long long)lay.total);
  const TtJpegGeometry geo = tt_jpeg_geometry(h, w, ch, subsampling);
  const long long blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  const long long plain_stride = lay.plain_stride;
  const int chunks = (int)lay.chunks;
  unsigned* bits = (unsigned*)((char*)ws + lay.bits);
  unsigned* plain_bytes = (unsigned*)((char*)ws + lay.plain_bytes);
  unsigned* chunk_ff = (unsigned*)((char*)ws + lay.chunk_ff);
  unsigned* plain = (unsigned*)((char*)ws + lay.plain);
  unsigned* extra = ri ? (unsigned*)((char*)ws + lay.extra) : nullptr;
  unsigned* marks = ri ? (unsigned*)((char*)ws + lay.marks) : nullptr;
  const long long ri_blocks = (long long)ri * geo.blocks_per_mcu, intervals = lay.intervals, mark_words = lay.mark_words;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 per_block((unsigned)((blocks + SBLOCK - 1) / SBLOCK), (unsigned)n), per_chunk((unsigned)chunks, (unsigned)n);
  hipError_t e = hipMemsetAsync(plain, 0, (size_t)(n * plain_stride), s);
  if (e == hipSuccess && ri) e = hipMemsetAsync(marks, 0, (size_t)(n * mark_words) * sizeof(unsigned), s);
  if (e != hipSuccess) TT_FAIL(TT_ELAUNCH, "%s: zeroing ws: %s", who, hipGetErrorString(e));
  hipLaunchKernelGGL(jpeg_bits_kernel, per_block, dim3(SBLOCK), 0, s, (const short*)coeffs, blocks, (int)geo.blocks_per_mcu, ri_blocks,
                     (const unsigned*)tables, (int)ntables, bits);
  hipLaunchKernelGGL(jpeg_offsets_kernel, dim3((unsigned)n), dim3(SCAN_BLOCK), 0, s, bits, blocks, plain_bytes, ri_blocks, intervals, extra);
  hipLaunchKernelGGL(jpeg_emit_kernel, per_block, dim3(SBLOCK), 0, s, (const short*)coeffs, blocks, (int)geo.blocks_per_mcu, ri_blocks,
                     (const unsigned*)tables, (int)ntables, (const unsigned*)bits, (const unsigned*)extra, intervals, plain, plain_stride, marks, mark_words);
  hipLaunchKernelGGL(jpeg_ff_count_kernel, per_chunk, dim3(SBLOCK), 0, s, (const unsigned*)plain, plain_stride, (const unsigned*)plain_bytes, chunk_ff, chunks, (const unsigned*)marks, mark_words);
  hipLaunchKernelGGL(jpeg_ff_scan_kernel, dim3((unsigned)n), dim3(SCAN_BLOCK), 0, s, chunk_ff, chunks, (const unsigned*)plain_bytes, (unsigned*)lengths);
  hipLaunchKernelGGL(jpeg_stuff_kernel, per_chunk, dim3(SBLOCK), 0, s, (const unsigned*)plain, plain_stride, (const unsigned*)plain_bytes,
                     (const unsigned*)chunk_ff, chunks, (unsigned char*)out, stride, (const unsigned*)marks, mark_words);
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}

extern "C" int tt_jpeg_scan(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, const uint32_t* tables,
                            int32_t ntables, uint8_t* out, int64_t cap, uint32_t* lengths, void* ws, int64_t ws_bytes, tt_stream_t stream) {
  return scan_frames("tt_jpeg_scan", coeffs, n, h, w, ch, subsampling, 0, tables, ntables, out, cap, lengths, ws, ws_bytes, stream);
}

extern "C" int tt_jpeg_scan_restart(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval,
                                    const uint32_t* tables, int32_t ntables, uint8_t* out, int64_t cap, uint32_t* lengths, void* ws, int64_t ws_bytes,
                                    tt_stream_t stream) {
  return scan_frames("tt_jpeg_scan_restart", coeffs, n, h, w, ch, subsampling, restart_interval, tables, ntables, out, cap, lengths, ws, ws_bytes, stream);
}
