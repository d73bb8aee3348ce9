// libttvdm: the device half of the JPEG import (include/ttvdm.h, "JPEG import"): tt_jpeg_entropy -- byte unstuffing, the
// self-synchronising Huffman decode of every frame's scan into tt_jpeg_coeffs' coefficient layout, the DC prefix sums --,
// tt_jpeg_entropy_spans -- the same per span between restart markers (rule 4a), of which tt_jpeg_entropy is "one span a frame" -- and
// tt_jpeg_pixels -- dequantiser, the jidctint inverse DCT, fancy 4:2:0 chroma upsampling and the colour conversion in one launch.
// Integer arithmetic only; the one atomic is an OR into a frame's status word: every call gives the same bytes.
#include "jpeg_device.h"

namespace {

constexpr int PBLOCK = 256, TILE_W = 256;           // the reconstruction's tile: one MCU row down, TILE_W pixels across

// ZZ[k]: the natural (row-major) index of the k-th coefficient of the zig-zag scan
__device__ constexpr int ZZ[64] = TT_JPEG_ZIGZAG;

// Items.  tt_jpeg_entropy's items are frames; tt_jpeg_entropy_spans' are the spans between restart markers, each with its frame, its
// first block there and its block count (device arrays).  A span whose place is not inside its frame is taken as empty (`bad`), and its
// frame index is held inside the call's frames.  span_frame NULL: item i is frame i, whole.
struct ItemPlace { int frame; unsigned first, count; bool bad; };
__device__ __forceinline__ ItemPlace item_place(const int* __restrict__ span_frame, const unsigned* __restrict__ span_first, const unsigned* __restrict__ span_blocks,
                                                int item, int nframes, unsigned blocks) {
  if (!span_frame) return {item, 0u, blocks, false};
  const int f = span_frame[item];
  const unsigned first = span_first[item], count = span_blocks[item];
  const bool bad = f < 0 || f >= nframes || first > blocks || count > blocks - first;
  return {min(max(f, 0), nframes - 1), bad ? 0u : first, bad ? 0u : count, bad};
}

// ---------------------------------------------------------------- rule 4: the entropy decoder
// a frame's constants, uniform over the workgroup
struct DecFrame {
  unsigned L;                                        // bits of the plain stream
  unsigned map;                                      // bit 2 c: component c's DC table, bit 2 c + 1: its AC table
  int bpm;
  unsigned blocks;                                   // tt_jpeg_blocks
};

// f_i: the whole symbols that start in [max(st.p, start), end) of the window `win_s` (big-endian dwords, bit 0 of word 0 is bit `win0` of
// the stream); st becomes the exit state; returns the blocks completed.  WRITE: the values go to `out` (the frame's coefficients), the
// first block touched is `block`, and what a valid stream never holds is ORed into `err`.  At most SUBSEQ iterations: every one takes a
// bit or more, and end - start <= SUBSEQ.
template <bool WRITE>
__device__ __forceinline__ unsigned decode_span(const unsigned* win_s, unsigned win0, const unsigned* tab_s, const DecFrame& fr, unsigned start, unsigned end,
                                                DecState& st, short* __restrict__ out, unsigned block, unsigned& err) {
  unsigned p = st.p, m = st.mz >> 6, z = st.mz & 63u, done = 0u;
  if (p < start) return 0u;                          // a lane before this one stopped at the end of the stream: pass the state on
  for (int it = 0; it < SUBSEQ && p < end; ++it) {
    const unsigned v = window_bits(win_s, win0, p);                     // the 32 bits at p
    const unsigned avail = fr.L - p;
    const unsigned comp = fr.bpm == 6 ? (m < 4u ? 0u : m - 3u) : m;
    const unsigned id = (fr.map >> (2u * comp + (z ? 1u : 0u))) & 1u;
    const unsigned* t = tab_s + (id * 2u + (z ? 1u : 0u)) * TT_JPEG_DECODE_WORDS;
    unsigned len, sym;
    huff_lookup(t, v, len, sym);
    if (len == 0u) {
      if (avail < 16u) break;                        // no code within the bits left: the lane stops
      if (WRITE) err |= TT_JPEG_STATUS_CODE;
      p += 1u;                                       // no code at all: skip one bit
      continue;
    }
    const unsigned n = sym & 15u;
    if (len + n > avail) break;                      // the symbol would read beyond L: the lane stops
    const unsigned raw = n ? (v << len) >> (32u - n) : 0u;
    const int value = n ? ((raw >> (n - 1u)) ? (int)raw : (int)raw - (int)((1u << n) - 1u)) : 0;
    p += len + n;
    bool ends = false;
    if (z == 0u) {
      if (WRITE) {
        if (sym > 11u) err |= TT_JPEG_STATUS_CODE;
        if (block + done < fr.blocks) out[(long long)(block + done) * 64] = (short)value;
      }
      z = 1u;
    } else if (n == 0u) {
      if ((sym >> 4) == 15u) { z += 16u; ends = z > 63u; }
      else ends = true;                              // EOB
    } else {
      z += sym >> 4;
      if (z > 63u) {
        ends = true;                                 // a run that passes index 63: the block ends
        if (WRITE) err |= TT_JPEG_STATUS_CODE;
      } else {
        if (WRITE && block + done < fr.blocks) out[(long long)(block + done) * 64 + z] = (short)value;
        ++z;
        ends = z > 63u;
      }
    }
    if (ends) {
      z = 0u;
      m = (int)m + 1 == fr.bpm ? 0u : m + 1u;
      ++done;
    }
  }
  st.p = p;
  st.mz = m << 6 | z;
  return done;
}

// grid (items), ELANES lanes: ONE workgroup walks its item's sequences in order, from the true state (0, 0, 0): a frame's scan, or the span
// behind a restart marker, where the stream is at a byte, an MCU begins and the DC predictors are zero.  Nothing another workgroup writes is read.
__global__ __launch_bounds__(ELANES) void jpeg_entropy_kernel(const unsigned char* __restrict__ plain, long long plain_stride, const unsigned* __restrict__ plain_bytes,
                                                            long long max_bytes, const unsigned* __restrict__ tables, int ntables, int bpm, unsigned blocks,
                                                            short* __restrict__ coeffs, unsigned* __restrict__ status, const int* __restrict__ span_frame,
                                                            const unsigned* __restrict__ span_first, const unsigned* __restrict__ span_blocks, int nframes) {
  __shared__ unsigned win_s[SEQ_WORDS + 2];
  __shared__ unsigned tab_s[TT_JPEG_DECODE_SET_WORDS];
  __shared__ unsigned ex_p[ELANES], ex_mz[ELANES];
  __shared__ unsigned red_s[EWAVES];
  const int tid = threadIdx.x;
  const ItemPlace it = item_place(span_frame, span_first, span_blocks, (int)blockIdx.x, nframes, blocks);
  const unsigned* __restrict__ tset = tables + (ntables > 1 ? (long long)it.frame * TT_JPEG_DECODE_SET_WORDS : 0);
  for (int i = tid; i < TT_JPEG_DECODE_SET_WORDS; i += ELANES) tab_s[i] = tset[i];
  const unsigned nbytes = (unsigned)min((long long)plain_bytes[blockIdx.x], max_bytes);
  const unsigned char* __restrict__ stream = plain + (long long)blockIdx.x * plain_stride;
  const unsigned* __restrict__ words = (const unsigned*)stream;
  const long long stride_words = plain_stride / 4;
  short* __restrict__ out = coeffs + ((long long)it.frame * blocks + it.first) * 64;
  __syncthreads();
  DecFrame fr;
  fr.L = nbytes * 8u;                                // max_bytes < 2^28: below 2^31
  fr.map = tab_s[4 * TT_JPEG_DECODE_WORDS];
  fr.bpm = bpm;
  fr.blocks = it.count;
  DecState carried = {0u, 0u};                       // the true state at the head of the sequence
  unsigned base = 0u, err = (it.bad && tid == 0) ? TT_JPEG_STATUS_SPAN : 0u;       // blocks completed before the sequence
  const unsigned nseq = (fr.L + SEQ_BITS - 1u) / SEQ_BITS;
  for (unsigned q = 0; q < nseq; ++q) {
    const unsigned win0 = q * SEQ_BITS;
    __syncthreads();                                 // the window and the states of the sequence before are done with
    // The last words of the window may hold workspace bytes behind the stream's L bits that nothing wrote.  No result depends on them:
    // a code of at most `avail` bits is decided by bits before L alone (the table is a prefix code, the shortest match is taken), and it
    // and its magnitude bits are used only when len + n <= avail; every other outcome with avail < 16 is the same `break`, and "no code:
    // skip a bit" needs avail >= 16, i.e. 16 real bits.  (The CPU emulation reads zeros there and gives the same states.)
    for (unsigned i = tid; i < SEQ_WORDS + 2u; i += ELANES) {
      const long long gw = (long long)q * SEQ_WORDS + i;
      win_s[i] = gw < stride_words ? __builtin_bswap32(words[gw]) : 0u;
    }
    __syncthreads();
    const unsigned start = win0 + (unsigned)tid * SUBSEQ, end = min(start + (unsigned)SUBSEQ, fr.L);
    const bool active = start < fr.L;                // a lane behind the end of the stream decodes nothing and never asks for a pass
    const int last = (int)min((unsigned)ELANES - 1u, (fr.L - win0 - 1u) / (unsigned)SUBSEQ);       // the last lane with bits of the stream
    unsigned none = 0u;
    DecState used = carried, x;
    if (tid) { used.p = start; used.mz = 0u; }
    x = used;
    unsigned done = decode_span<false>(win_s, win0, tab_s, fr, start, end, x, out, 0u, none);
    ex_p[tid] = x.p;
    ex_mz[tid] = x.mz;
    for (int pass = 1; pass < ELANES; ++pass) {       // after k passes the first k + 1 lanes are exact
      __syncthreads();
      DecState entry = carried;
      if (tid) { entry.p = ex_p[tid - 1]; entry.mz = ex_mz[tid - 1]; }
      const bool changed = active && !same(entry, used);
      if (!__syncthreads_or(changed)) break;         // uniform: nobody's entry moved, the states are final
      if (changed) {
        used = entry;
        x = used;
        done = decode_span<false>(win_s, win0, tab_s, fr, start, end, x, out, 0u, none);
        ex_p[tid] = x.p;
        ex_mz[tid] = x.mz;
      }
    }
    // every lane's first block: an exclusive scan of the blocks completed.  Its barrier also: every ex_p / ex_mz of the last pass is stored
    unsigned all;
    const unsigned first = base + block_scan_excl<EWAVES>(done, red_s, all);
    x = used;
    decode_span<true>(win_s, win0, tab_s, fr, start, end, x, out, first, err);
    carried.p = ex_p[last];
    carried.mz = ex_mz[last];
    base += all;
  }
  if (tid == 0) {
    if (base != it.count) err |= TT_JPEG_STATUS_BLOCKS;
    const unsigned left = fr.L - min(carried.p, fr.L);
    const unsigned ones = left ? (1u << min(left, 8u)) - 1u : 0u;
    if (left >= 8u || (left && ((unsigned)stream[nbytes - 1] & ones) != ones)) err |= TT_JPEG_STATUS_TAIL;
  }
  if (err) atomicOr(&status[it.frame], err);
}

// grid (items), SCAN_BLOCK lanes: one lane per MCU, a prefix sum per component over the DC differences (int32), stored as int16; it
// starts from zero at every item: a frame, or the span behind a restart marker
__global__ __launch_bounds__(SCAN_BLOCK) void jpeg_dc_kernel(short* __restrict__ coeffs, long long blocks, int bpm, const int* __restrict__ span_frame,
                                                             const unsigned* __restrict__ span_first, const unsigned* __restrict__ span_blocks, int nframes) {
  __shared__ int red_s[SCAN_WAVES];
  const int tid = threadIdx.x;
  const ItemPlace it = item_place(span_frame, span_first, span_blocks, (int)blockIdx.x, nframes, (unsigned)blocks);
  short* __restrict__ fc = coeffs + ((long long)it.frame * blocks + it.first) * 64;
  const long long mcus = it.count / bpm;
  const int ncomp = bpm == 1 ? 1 : 3, ny = bpm == 6 ? 4 : 1;
  int carry[3] = {0, 0, 0};
  for (long long at = 0; at < mcus; at += SCAN_BLOCK) {
    const long long u = at + tid;
    for (int c = 0; c < ncomp; ++c) {
      const int k0 = c == 0 ? 0 : ny + c - 1, nk = c == 0 ? ny : 1;
      int d[4] = {0, 0, 0, 0}, mine = 0;
      if (u < mcus)
        for (int k = 0; k < nk; ++k) { d[k] = fc[(u * bpm + k0 + k) * 64]; mine += d[k]; }
      int all;
      int before = carry[c] + block_scan_excl<SCAN_WAVES>(mine, red_s, all);
      if (u < mcus)
        for (int k = 0; k < nk; ++k) { before += d[k]; fc[(u * bpm + k0 + k) * 64] = (short)before; }
      carry[c] += all;
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- rule 5: reconstruction
// jidctint's arithmetic in 32-bit two's complement: sums and products are formed in unsigned, so crafted coefficients wrap instead of
// overflowing a signed int; the descale is an arithmetic shift of the wrapped value
template <int N> __device__ __forceinline__ int descale(unsigned x) { return (int)(x + (1u << (N - 1))) >> N; }
// jidctint's pass over eight values; N: the descale
template <int N> __device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  const unsigned i0 = (unsigned)d0, i1 = (unsigned)d1, i2 = (unsigned)d2, i3 = (unsigned)d3, i4 = (unsigned)d4, i5 = (unsigned)d5, i6 = (unsigned)d6,
                 i7 = (unsigned)d7;
  const unsigned z1 = (i2 + i6) * 4433u;
  const unsigned e2 = z1 - i6 * 15137u, e3 = z1 + i2 * 6270u;
  const unsigned e0 = (i0 + i4) << 13, e1 = (i0 - i4) << 13;
  const unsigned t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  const unsigned y1 = i7 + i1, y2 = i5 + i3, y3 = i7 + i3, y4 = i5 + i1, z5 = (y3 + y4) * 9633u;
  const unsigned a0 = i7 * 2446u, a1 = i5 * 16819u, a2 = i3 * 25172u, a3 = i1 * 12299u;
  const unsigned b1 = 0u - y1 * 7373u, b2 = 0u - y2 * 20995u, b3 = z5 - y3 * 16069u, b4 = z5 - y4 * 3196u;
  const unsigned o0 = a0 + b1 + b3, o1 = a1 + b2 + b4, o2 = a2 + b2 + b3, o3 = a3 + b1 + b4;
  d0 = descale<N>(t10 + o3); d7 = descale<N>(t10 - o3);
  d1 = descale<N>(t11 + o2); d6 = descale<N>(t11 - o2);
  d2 = descale<N>(t12 + o1); d5 = descale<N>(t12 - o1);
  d3 = descale<N>(t13 + o0); d4 = descale<N>(t13 - o0);
}
__device__ __forceinline__ unsigned clamp8(int v) { return (unsigned)min(max(v, 0), 255); }

// the block at `c` (zig-zag int16) dequantised by q (natural order), inverted, as 8 rows of 8 samples at dst (8-byte aligned rows)
__device__ __forceinline__ void block_samples(const short* __restrict__ c, const unsigned char* q, unsigned char* dst, int pitch) {
  int d[64];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const uint4 v = *(const uint4*)(c + 8 * u);
    const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * u + j;
      d[ZZ[k]] = (int)(short)((wd[j >> 1] >> (16 * (j & 1))) & 0xffffu) * (int)q[ZZ[k]];
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) idct8<11>(d[col], d[8 + col], d[16 + col], d[24 + col], d[32 + col], d[40 + col], d[48 + col], d[56 + col]);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    idct8<18>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
    unsigned lo = 0u, hi = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo |= clamp8(d[r * 8 + j] + 128) << (8 * j);
      hi |= clamp8(d[r * 8 + 4 + j] + 128) << (8 * j);
    }
    *(uint2*)(dst + r * pitch) = make_uint2(lo, hi);
  }
}

__device__ __forceinline__ void store_rgb(unsigned char* __restrict__ p, int y, int cb, int cr) {
  cb -= 128;
  cr -= 128;
  p[0] = (unsigned char)clamp8(y + ((91881 * cr + 32768) >> 16));
  p[1] = (unsigned char)clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  p[2] = (unsigned char)clamp8(y + ((116130 * cb + 32768) >> 16));
}

// grid (tiles per MCU row x MCU rows, n): a tile is one MCU row down and TILE_W pixels across.  One lane per block inverts it into LDS;
// then every lane converts the tile's pixels.  SUB (4:2:0): the chroma blocks of the MCU rows above and below and of one MCU to either
// side are inverted as well -- the upsampler's neighbours -- into a plane of 3 x CBW blocks per component.
constexpr int CBW = TILE_W / 16 + 2, CPITCH = 8 * CBW;
template <bool SUB> __global__ __launch_bounds__(PBLOCK) void jpeg_pixels_kernel(const short* __restrict__ coeffs, long long blocks, int h, int w, int ch,
                                                                               TtJpegGeometry geo, int tiles_x, const unsigned char* __restrict__ quant,
                                                                               int ntables, unsigned char* __restrict__ frames) {
  constexpr int MCU = SUB ? 16 : 8, MCUS = TILE_W / MCU;
  __shared__ __attribute__((aligned(16))) unsigned char y_s[MCU][TILE_W];
  __shared__ __attribute__((aligned(16))) unsigned char c_s[SUB ? 2 * 24 * CPITCH : 2 * 8 * TILE_W];
  __shared__ unsigned char q_s[3 * 64];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % tiles_x, mcu_y = blockIdx.x / tiles_x;
  const int x0 = tile * TILE_W, y0 = mcu_y * MCU;
  if (tid < 192) q_s[tid] = quant[(ntables > 1 ? (long long)blockIdx.y * 192 : 0) + tid];
  __syncthreads();
  const short* __restrict__ fc = coeffs + (long long)blockIdx.y * blocks * 64;
  const int bpm = geo.blocks_per_mcu;
  if (SUB) {
    if (tid < 4 * MCUS) {                            // the tile's Y blocks
      const int m = tid >> 2, k = tid & 3, mcu_x = tile * MCUS + m;
      if (mcu_x < geo.mcus_x && 2 * mcu_y + (k >> 1) < (h + 7) / 8 && 2 * mcu_x + (k & 1) < (w + 7) / 8)       // dummy blocks are dropped
        block_samples(fc + (((long long)mcu_y * geo.mcus_x + mcu_x) * 6 + k) * 64, q_s, &y_s[(k >> 1) * 8][m * 16 + (k & 1) * 8], TILE_W);
    } else if (tid < 4 * MCUS + 2 * 3 * CBW) {       // chroma: 3 block rows of CBW blocks per component
      const int i = tid - 4 * MCUS, comp = i / (3 * CBW), brow = (i % (3 * CBW)) / CBW, bcol = i % CBW;
      const int my = mcu_y - 1 + brow, mx = tile * MCUS - 1 + bcol;
      if (my >= 0 && my < geo.mcus_y && mx >= 0 && mx < geo.mcus_x)
        block_samples(fc + (((long long)my * geo.mcus_x + mx) * 6 + 4 + comp) * 64, q_s + 64 * (1 + comp), c_s + (comp * 24 + brow * 8) * CPITCH + bcol * 8, CPITCH);
    }
  } else {
    const int m = tid / bpm, k = tid % bpm, mcu_x = tile * MCUS + m;
    if (m < MCUS && mcu_x < geo.mcus_x)
      block_samples(fc + (((long long)mcu_y * geo.mcus_x + mcu_x) * bpm + k) * 64, q_s + 64 * k, k == 0 ? &y_s[0][m * 8] : c_s + (k - 1) * 8 * TILE_W + m * 8,
                    TILE_W);
  }
  __syncthreads();
  unsigned char* __restrict__ dst = frames + (long long)blockIdx.y * h * w * ch;
  const int hc = (h + 1) >> 1, wc = (w + 1) >> 1;
  const bool fancy = wc > 2;
  for (int i = tid; i < MCU * TILE_W; i += PBLOCK) {
    const int yy = i / TILE_W, xx = i % TILE_W, gy = y0 + yy, gx = x0 + xx;
    if (gy >= h || gx >= w) continue;
    unsigned char* __restrict__ p = dst + ((long long)gy * w + gx) * ch;
    const int y = y_s[yy][xx];
    if (ch == 1) { p[0] = (unsigned char)y; continue; }
    if (!SUB) { store_rgb(p, y, c_s[yy * TILE_W + xx], c_s[(8 + yy) * TILE_W + xx]); continue; }
    // the chroma sample (r, c) of the plane sits at row r - (8 mcu_y - 8), column c - (x0 / 2 - 8) of the component's LDS plane
    const int r = gy >> 1, c = gx >> 1, rb = 8 * mcu_y - 8, cbase = (x0 >> 1) - 8;
    int cc[2];
#pragma unroll
    for (int comp = 0; comp < 2; ++comp) {
      const unsigned char* s = c_s + comp * 24 * CPITCH;
      if (!fancy) { cc[comp] = s[(r - rb) * CPITCH + c - cbase]; continue; }
      const int r2 = (gy & 1) ? min(r + 1, hc - 1) : max(r - 1, 0), c2 = (gx & 1) ? min(c + 1, wc - 1) : max(c - 1, 0);
      const int va = 3 * s[(r - rb) * CPITCH + c - cbase] + s[(r2 - rb) * CPITCH + c - cbase];
      const int vb = 3 * s[(r - rb) * CPITCH + c2 - cbase] + s[(r2 - rb) * CPITCH + c2 - cbase];
      cc[comp] = (3 * va + vb + ((gx & 1) ? 7 : 8)) >> 4;
    }
    store_rgb(p, y, cc[0], cc[1]);
  }
}

}  // namespace

// tt_jpeg_entropy (items = n frames, span_frame NULL) and tt_jpeg_entropy_spans (items = the spans of n frames) are the same launches
static int entropy_items(const char* who, const uint8_t* scans, int64_t scans_bytes, const int64_t* offsets, const uint32_t* lengths, const int32_t* span_frame,
                         const uint32_t* span_first, const uint32_t* span_blocks, int64_t max_bytes, int32_t items, int32_t n, int32_t h, int32_t w, int32_t ch,
                         int32_t subsampling, const uint32_t* tables, int32_t ntables, int16_t* coeffs, uint32_t* status, void* ws, int64_t ws_bytes,
                         tt_stream_t stream) {
  if (!scans || !offsets || !lengths || !tables || !coeffs || !status || !ws)
    TT_FAIL(TT_EINVAL, "%s: null %s", who,
            !scans ? "scans" : (!offsets ? "offsets" : (!lengths ? "lengths" : (!tables ? "tables" : (!coeffs ? "coeffs" : (!status ? "status" : "ws"))))));
  const int rc = tt_jpeg_refuse_shape(who, n, h, w, ch, subsampling, "");
  if (rc != TT_OK) return rc;
  if (scans_bytes <= 0 || max_bytes <= 0) TT_FAIL(TT_EINVAL, "%s: empty scans (scans_bytes = %lld, max_bytes = %lld)", who, (long long)scans_bytes, (long long)max_bytes);
  if (max_bytes >= (1ll << 28)) TT_FAIL(TT_EUNSUPPORTED, "%s: max_bytes = %lld (a scan below 2^28 bytes)", who, (long long)max_bytes);
  if (ntables != 1 && ntables != n) TT_FAIL(TT_EINVAL, "%s: ntables = %d (1, or one set per frame: %d)", who, ntables, n);
  if ((uintptr_t)offsets & 7) TT_FAIL(TT_EINVAL, "%s: offsets is not 8-byte aligned", who);
  if ((uintptr_t)lengths & 3) TT_FAIL(TT_EINVAL, "%s: lengths is not 4-byte aligned", who);
  if ((uintptr_t)tables & 15) TT_FAIL(TT_EINVAL, "%s: tables is not 16-byte aligned", who);
  if ((uintptr_t)coeffs & 15) TT_FAIL(TT_EINVAL, "%s: coeffs is not 16-byte aligned", who);
  if ((uintptr_t)status & 3) TT_FAIL(TT_EINVAL, "%s: status is not 4-byte aligned", who);
  if ((uintptr_t)ws & 15) TT_FAIL(TT_EINVAL, "%s: ws is not 16-byte aligned", who);
  const TtJpegEntropyWs lay(items, max_bytes);
  if (ws_bytes < lay.total)
    TT_FAIL(TT_EINVAL, "%s: ws too small: %lld bytes, tt_jpeg_entropy_ws_bytes = %lld", who, (long long)ws_bytes, (long long)lay.total);
  const TtJpegGeometry geo = tt_jpeg_geometry(h, w, ch, subsampling);
  const long long blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  const int chunks = (int)lay.chunks;
  const long long plain_stride = lay.plain_stride;
  unsigned* plain_bytes = (unsigned*)((char*)ws + lay.plain_bytes);
  unsigned* chunk_drop = (unsigned*)((char*)ws + lay.chunk_drop);
  unsigned char* plain = (unsigned char*)ws + lay.plain;
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t) * (size_t)n, s);
  if (e == hipSuccess) e = hipMemsetAsync(coeffs, 0, (size_t)n * (size_t)blocks * 128, s);
  if (e != hipSuccess) TT_FAIL(TT_ELAUNCH, "%s: zeroing coeffs and status: %s", who, hipGetErrorString(e));
  const dim3 per_chunk((unsigned)chunks, (unsigned)items);
  hipLaunchKernelGGL(jpeg_unstuff_count_kernel, per_chunk, dim3(UBLOCK), 0, s, (const unsigned char*)scans, (long long)scans_bytes, (const long long*)offsets,
                     (const unsigned*)lengths, (long long)max_bytes, chunk_drop, chunks, (unsigned*)status, (const int*)span_frame, (int)n);
  hipLaunchKernelGGL(jpeg_unstuff_scan_kernel, dim3((unsigned)items), dim3(SCAN_BLOCK), 0, s, chunk_drop, chunks, (const long long*)offsets, (const unsigned*)lengths,
                     (long long)scans_bytes, (long long)max_bytes, plain_bytes);
  hipLaunchKernelGGL(jpeg_unstuff_gather_kernel, per_chunk, dim3(UBLOCK), 0, s, (const unsigned char*)scans, (long long)scans_bytes, (const long long*)offsets,
                     (const unsigned*)lengths, (long long)max_bytes, (const unsigned*)chunk_drop, chunks, plain, plain_stride);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)items), dim3(ELANES), 0, s, (const unsigned char*)plain, plain_stride, (const unsigned*)plain_bytes,
                     (long long)max_bytes, (const unsigned*)tables, (int)ntables, (int)geo.blocks_per_mcu, (unsigned)blocks, (short*)coeffs, (unsigned*)status,
                     (const int*)span_frame, (const unsigned*)span_first, (const unsigned*)span_blocks, (int)n);
  hipLaunchKernelGGL(jpeg_dc_kernel, dim3((unsigned)items), dim3(SCAN_BLOCK), 0, s, (short*)coeffs, blocks, (int)geo.blocks_per_mcu, (const int*)span_frame,
                     (const unsigned*)span_first, (const unsigned*)span_blocks, (int)n);
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}

extern "C" int tt_jpeg_entropy(const uint8_t* scans, int64_t scans_bytes, const int64_t* offsets, const uint32_t* lengths, int64_t max_bytes, int32_t n,
                               int32_t h, int32_t w, int32_t ch, int32_t subsampling, const uint32_t* tables, int32_t ntables, int16_t* coeffs,
                               uint32_t* status, void* ws, int64_t ws_bytes, tt_stream_t stream) {
  return entropy_items("tt_jpeg_entropy", scans, scans_bytes, offsets, lengths, nullptr, nullptr, nullptr, max_bytes, n, n, h, w, ch, subsampling, tables, ntables,
                       coeffs, status, ws, ws_bytes, stream);
}

extern "C" int tt_jpeg_entropy_spans(const uint8_t* scans, int64_t scans_bytes, const int64_t* offsets, const uint32_t* lengths, const int32_t* span_frame,
                                     const uint32_t* span_first, const uint32_t* span_blocks, int64_t max_bytes, int32_t nspans, int32_t n, int32_t h, int32_t w,
                                     int32_t ch, int32_t subsampling, const uint32_t* tables, int32_t ntables, int16_t* coeffs, uint32_t* status, void* ws,
                                     int64_t ws_bytes, tt_stream_t stream) {
  if (!span_frame || !span_first || !span_blocks)
    TT_FAIL(TT_EINVAL, "tt_jpeg_entropy_spans: null %s", !span_frame ? "span_frame" : (!span_first ? "span_first" : "span_blocks"));
  if (nspans <= 0) TT_FAIL(TT_EINVAL, "tt_jpeg_entropy_spans: nspans = %d", nspans);
  if (nspans > TT_JPEG_MAX_SPANS) TT_FAIL(TT_EUNSUPPORTED, "tt_jpeg_entropy_spans: %d spans: more than one grid covers (%d)", nspans, TT_JPEG_MAX_SPANS);
  if (((uintptr_t)span_frame | (uintptr_t)span_first | (uintptr_t)span_blocks) & 3)
    TT_FAIL(TT_EINVAL, "tt_jpeg_entropy_spans: span_frame, span_first or span_blocks is not 4-byte aligned");
  return entropy_items("tt_jpeg_entropy_spans", scans, scans_bytes, offsets, lengths, span_frame, span_first, span_blocks, max_bytes, nspans, n, h, w, ch, subsampling,
                       tables, ntables, coeffs, status, ws, ws_bytes, stream);
}

extern "C" int tt_jpeg_pixels(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, const uint8_t* quant, int32_t ntables,
                              void* frames, tt_stream_t stream) {
  if (!coeffs || !quant || !frames) TT_FAIL(TT_EINVAL, "tt_jpeg_pixels: null %s", !coeffs ? "coeffs" : (!quant ? "quant" : "frames"));
  const int rc = tt_jpeg_refuse_shape("tt_jpeg_pixels", n, h, w, ch, subsampling, "");
  if (rc != TT_OK) return rc;
  if (ntables != 1 && ntables != n) TT_FAIL(TT_EINVAL, "tt_jpeg_pixels: ntables = %d (1, or one set per frame: %d)", ntables, n);
  if ((uintptr_t)coeffs & 15) TT_FAIL(TT_EINVAL, "tt_jpeg_pixels: coeffs is not 16-byte aligned");
  const TtJpegGeometry geo = tt_jpeg_geometry(h, w, ch, subsampling);
  const long long blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  const bool sub = geo.blocks_per_mcu == 6;
  const int tiles_x = (geo.mcus_x * (sub ? 16 : 8) + TILE_W - 1) / TILE_W;
  const dim3 grid((unsigned)(tiles_x * geo.mcus_y), (unsigned)n);
  if (sub)
    hipLaunchKernelGGL(jpeg_pixels_kernel<true>, grid, dim3(PBLOCK), 0, (hipStream_t)stream, (const short*)coeffs, blocks, (int)h, (int)w, (int)ch, geo, tiles_x,
                       (const unsigned char*)quant, (int)ntables, (unsigned char*)frames);
  else
    hipLaunchKernelGGL(jpeg_pixels_kernel<false>, grid, dim3(PBLOCK), 0, (hipStream_t)stream, (const short*)coeffs, blocks, (int)h, (int)w, (int)ch, geo, tiles_x,
                       (const unsigned char*)quant, (int)ntables, (unsigned char*)frames);
  TT_CHECK_LAUNCH("tt_jpeg_pixels");
  return TT_OK;
}
