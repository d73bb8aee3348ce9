// libttvdm: the PNG import's device half (include/ttvdm.h, "PNG import").  tt_png_inflate is a general zlib inflate that knows nothing of
// PNG: tokens (one workgroup per stream walks its blocks; a block's symbols are decoded window by window, every lane from a bit offset
// of its own until the lanes agree) -> jumps (every output byte is a literal or names an earlier byte: src <- src[src], a launch per
// round, ceil(log2(max_out)) of them) -> bytes (the literals leave as bytes, with an Adler-32 pair per chunk) -> adler (the pairs
// combined and compared with the stream's trailer).  tt_png_unfilter undoes the five row filters along anti-diagonals, a lane per row of
// a band.  No workgroup waits on another; integers only: the same bytes every call.
#include "common.h"
#include "block_scan.h"
#include "png_host.h"

namespace {

constexpr int INF_BLOCK = 1024, INF_WAVES = INF_BLOCK / 64;      // the tokens kernel
constexpr unsigned SUB_BITS = 128;                               // a lane's sub-window: longer than any token (48 bits)
constexpr unsigned WIN_BITS = INF_BLOCK * SUB_BITS;              // 16 KiB of compressed bits a window
constexpr unsigned WIN_WORDS = WIN_BITS / 32 + 8;                // ... and what a token that starts in its last bits reads
constexpr unsigned LIT = 0x80000000u;                            // a source word that is a literal (its byte in the low bits), not an index
constexpr int JMP_BLOCK = 256;
constexpr int BYT_BLOCK = 256, BYT_WAVES = BYT_BLOCK / 64, BYT_PER = 16;
constexpr unsigned CHUNK = TT_INFLATE_CHUNK;
constexpr unsigned long long ADLER = 65521ull;
constexpr int UNF_BLOCK = TT_PNG_UNFILTER_BAND;
static_assert(BYT_BLOCK * BYT_PER == (int)CHUNK && SUB_BITS > 48 && INF_WAVES == 16, "a chunk is a lane's 16 bytes times 256 lanes");

__device__ const unsigned short LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const unsigned short DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                                 8193, 12289, 16385, 24577};
__device__ const unsigned char CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Code {                                      // a canonical code: how many symbols have each length, and the symbols by ascending code
  unsigned short count[16];
  unsigned short symbol[288];
};

struct StreamRec {                                 // what the tokens kernel leaves per stream (32 bytes)
  long long out_off;
  unsigned ok, expected, trailer, checked;         // checked: the stream ended cleanly with `expected` bytes and a whole trailer
  unsigned pad[2];
};

struct Inf {                                       // one call's arguments, the same in every kernel
  const unsigned char* data;
  long long data_bytes;
  const long long* offsets;
  const unsigned* lengths;
  const unsigned* expected;
  const long long* out_offsets;
  int n;
  unsigned char* out;
  long long out_bytes;
  unsigned max_out, chunks_per;
  unsigned* status;
  StreamRec* rec;
  unsigned* src;                                   // out_bytes words: per output byte a literal or the index of the byte it copies
  unsigned* pairs;                                 // n chunks_per pairs
};

// 25 bits or more of src[0, len) from bit `pos`; bytes behind the data read as zero
__device__ __forceinline__ unsigned peek_g(const unsigned char* __restrict__ src, unsigned len, unsigned long long pos) {
  const unsigned i = (unsigned)(pos >> 3);
  unsigned v = 0;
#pragma unroll
  for (unsigned k = 0; k < 4; ++k)
    if (i + k < len && i + k >= i) v |= (unsigned)src[i + k] << (8 * k);
  return v >> (unsigned)(pos & 7u);
}

// 64 bits of the staged window from bit `rel`
__device__ __forceinline__ unsigned long long peek_w(const unsigned* win_s, unsigned rel) {
  const unsigned k = rel >> 5, s = rel & 31u;
  const unsigned long long lo = (unsigned long long)win_s[k] | ((unsigned long long)win_s[k + 1] << 32);
  return s ? (lo >> s) | ((unsigned long long)win_s[k + 2] << (64u - s)) : lo;
}

// one symbol of a canonical code from the low bits of `bits` (15 of them are enough); -1: no code of the set starts with these bits
__device__ __forceinline__ int decode_sym(const Code& c, unsigned long long bits, unsigned& used) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; ++len) {
    code |= (int)(bits & 1ull);
    bits >>= 1;
    const int cnt = c.count[len];
    if (code - cnt < first) { used = (unsigned)len; return c.symbol[index + (code - first)]; }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  used = 15;
  return -1;
}

// lengths -> the code; returns what is left of the code space (negative: over-subscribed, positive: incomplete) and the longest length
__device__ int build_code(Code& c, const unsigned char* lens, int n, int* longest) {
  unsigned short offs[16];
  for (int l = 0; l < 16; ++l) c.count[l] = 0;
  for (int s = 0; s < n; ++s) ++c.count[lens[s] & 15];
  int left = 1, most = 0;
  for (int l = 1; l <= 15; ++l) {
    left = (left << 1) - (int)c.count[l];
    if (left < 0) return left;
    if (c.count[l]) most = l;
  }
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (unsigned short)(offs[l] + c.count[l]);
  for (int s = 0; s < n; ++s)
    if (lens[s] & 15) c.symbol[offs[lens[s] & 15]++] = (unsigned short)s;
  *longest = most;
  return left;
}

struct Reader {                                    // lane 0's bit reader over the stream itself, for a block's header
  const unsigned char* src;
  unsigned len;
  unsigned long long pos, total;
  bool cut;                                        // asked for bits behind the data
  __device__ unsigned get(unsigned n) {
    if (pos + n > total) { cut = true; return 0; }
    const unsigned v = peek_g(src, len, pos) & ((1u << n) - 1u);
    pos += n;
    return v;
  }
  __device__ int sym(const Code& c) {
    unsigned used;
    const int s = decode_sym(c, peek_g(src, len, pos), used);
    if (pos + used > total) { cut = true; return -1; }                                    // a code, or the 15 bits that are none, behind the data
    if (s >= 0) pos += used;
    return s;
  }
};

// lane 0: a dynamic block's two codes from its header, or the fixed block's.  0: built; else the status bit (0x8000: the data ended)
__device__ unsigned block_codes(Reader& r, bool fixed, Code& lit, Code& dist, unsigned char* lens) {
  int nlit = 288, ndist = 32, longest = 0;                                               // the fixed codes name 288 and 32 symbols; the last two of each are refused when met
  if (fixed) {
    for (int s = 0; s < 288; ++s) lens[s] = s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
    for (int s = 0; s < 32; ++s) lens[288 + s] = 5;
  } else {
    nlit = (int)r.get(5) + 257;
    ndist = (int)r.get(5) + 1;
    const int ncl = (int)r.get(4) + 4;
    if (r.cut) return 0x8000u;
    if (nlit > 286 || ndist > 30) return TT_INFLATE_STATUS_CODE;
    for (int i = 0; i < 19; ++i) lens[CL_ORDER[i]] = i < ncl ? (unsigned char)r.get(3) : 0;
    if (r.cut) return 0x8000u;
    if (build_code(lit, lens, 19, &longest) != 0) return TT_INFLATE_STATUS_CODE;        // the code-length code: complete, or refused
    int at = 0;
    const int all = nlit + ndist;
    for (int trip = 0; trip < 320 && at < all; ++trip) {                                  // a symbol fills one length at the least
      const int s = r.sym(lit);
      if (r.cut) return 0x8000u;
      if (s < 0) return TT_INFLATE_STATUS_CODE;
      if (s < 16) { lens[20 + at++] = (unsigned char)s; continue; }
      int rep, val = 0;
      if (s == 16) {
        if (at == 0) return TT_INFLATE_STATUS_CODE;
        val = lens[20 + at - 1];
        rep = 3 + (int)r.get(2);
      } else if (s == 17) rep = 3 + (int)r.get(3);
      else rep = 11 + (int)r.get(7);
      if (r.cut) return 0x8000u;
      if (at + rep > all) return TT_INFLATE_STATUS_CODE;
      for (int k = 0; k < rep; ++k) lens[20 + at++] = (unsigned char)val;
    }
    if (lens[20 + 256] == 0) return TT_INFLATE_STATUS_CODE;                               // no end-of-block code
    for (int s = 0; s < all; ++s) lens[s] = lens[20 + s];                                 // forward, onto lower addresses: no overlap trouble
    for (int s = 0; s < ndist; ++s) lens[288 + 32 + s] = lens[nlit + s];
    for (int s = 0; s < ndist; ++s) lens[288 + s] = lens[288 + 32 + s];
  }
  int left = build_code(lit, lens, nlit, &longest);
  if (left < 0 || (left > 0 && longest > 1)) return TT_INFLATE_STATUS_CODE;
  left = build_code(dist, lens + 288, ndist, &longest);
  if (left < 0 || (left > 0 && longest > 1)) return TT_INFLATE_STATUS_CODE;
  return 0;
}

struct Sub { unsigned exit, cnt, stop, err; };     // stop: 0 the lane ran to its sub-window's end, 1 end of block, 2 the stream ends here

// the tokens that start in [start, end) of the staged window, from `start`; WRITE: their source words go to src[abs0 + p ...]
template <bool WRITE> __device__ __forceinline__ Sub decode_sub(const unsigned* win_s, const Code& lit, const Code& dist, unsigned start, unsigned end,
                                                                unsigned limit, unsigned* __restrict__ src, unsigned abs0, unsigned long long p,
                                                                unsigned expected, unsigned* status) {
  Sub r = {start, 0u, 0u, 0u};
  unsigned pos = start;
  for (unsigned trip = 0; trip <= SUB_BITS && pos < end; ++trip) {                        // a token takes a bit at the least
    if (pos >= limit) { r.stop = 2; break; }
    unsigned long long bits = peek_w(win_s, pos);
    unsigned used, at = pos;
    const int s = decode_sym(lit, bits, used);
    if (s < 0 || s > 285) { r.stop = 2; r.err = at + used <= limit ? TT_INFLATE_STATUS_CODE : 0u; break; }
    at += used;
    bits >>= used;
    if (at > limit) { r.stop = 2; break; }
    if (s < 256) {
      if (WRITE && p < expected) src[abs0 + (unsigned)p] = LIT | (unsigned)s;
      ++p;
      ++r.cnt;
      pos = at;
      continue;
    }
    if (s == 256) { r.stop = 1; pos = at; break; }
    const int ls = s - 257;
    const unsigned lx = s < 265 || s == 285 ? 0u : (unsigned)(s - 261) >> 2;
    const unsigned length = LEN_BASE[ls] + ((unsigned)bits & ((1u << lx) - 1u));
    at += lx;
    bits >>= lx;
    const int ds = decode_sym(dist, bits, used);
    if (ds < 0 || ds > 29) { r.stop = 2; r.err = at + used <= limit ? TT_INFLATE_STATUS_CODE : 0u; break; }
    at += used;
    bits >>= used;
    const unsigned dx = ds < 4 ? 0u : (unsigned)(ds - 2) >> 1;
    const unsigned d = DIST_BASE[ds] + ((unsigned)bits & ((1u << dx) - 1u));
    at += dx;
    if (at > limit) { r.stop = 2; break; }
    if (WRITE) {
      if ((unsigned long long)d > p) atomicOr(status, (unsigned)TT_INFLATE_STATUS_DIST);
      for (unsigned j = 0; j < length; ++j) {                                             // at most 258
        const unsigned long long q = p + j;
        if (q < expected) src[abs0 + (unsigned)q] = q >= d ? abs0 + (unsigned)(q - d) : LIT;
      }
    }
    p += length;
    r.cnt += length;
    pos = at;
  }
  r.exit = pos;
  return r;
}

// grid (n), one workgroup per stream: its blocks in order, its source words, its record
__global__ __launch_bounds__(INF_BLOCK) void inflate_tokens_kernel(Inf d) {
  __shared__ unsigned win_s[WIN_WORDS];
  __shared__ unsigned exit_s[INF_BLOCK];
  __shared__ Code lit_s, dist_s;
  __shared__ unsigned char lens_s[288 + 64];
  __shared__ unsigned long long red_s[INF_WAVES];
  __shared__ unsigned long long hdr_pos_s;
  __shared__ unsigned hdr_err_s, first_s, stop_exit_s, stop_kind_s, stop_err_s;
  const unsigned f = blockIdx.x, tid = threadIdx.x;
  const long long off = d.offsets[f], out_off = d.out_offsets[f];
  const unsigned len = d.lengths[f], expected = d.expected[f];
  const bool ok = off >= 0 && (long long)len <= d.data_bytes && off <= d.data_bytes - (long long)len && len < (1u << 29) && out_off >= 0 &&
                  expected <= d.max_out && (long long)expected <= d.out_bytes && out_off <= d.out_bytes - (long long)expected;
  if (!ok) {
    if (tid == 0) {
      StreamRec rc = {};
      d.rec[f] = rc;
      atomicOr(d.status + f, (unsigned)TT_INFLATE_STATUS_SPAN);
    }
    return;
  }
  const unsigned char* __restrict__ src = d.data + off;
  const unsigned abs0 = (unsigned)out_off;
  unsigned* status = d.status + f;
  const unsigned long long total = 8ull * len;
  unsigned long long pos = 16, produced = 0;
  bool clean = false;
  unsigned err = 0;
  // the zlib header: method 8, a window of 32 KiB at the most, no preset dictionary, the check bits
  const unsigned head = len >= 2 ? peek_g(src, len, 0) & 0xffffu : 0u;
  const unsigned cmf = head & 0xffu, flg = head >> 8;
  bool going = len >= 2;
  if (going && ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u) || ((cmf << 8) + flg) % 31u)) { err |= TT_INFLATE_STATUS_BLOCK; going = false; }
  const unsigned long long blocks = total / 3ull + 1ull;                                  // a block takes three bits at the least
  for (unsigned long long blk = 0; blk < blocks && going; ++blk) {
    if (pos + 3 > total) break;
    const unsigned h3 = peek_g(src, len, pos) & 7u;
    const bool last = h3 & 1u;
    const unsigned type = h3 >> 1;
    pos += 3;
    if (type == 3u) { err |= TT_INFLATE_STATUS_BLOCK; break; }
    if (type == 0u) {                                                                     // stored: a byte-aligned copy
      pos = (pos + 7ull) & ~7ull;
      if (pos + 32 > total) break;
      const unsigned at = (unsigned)(pos >> 3);
      const unsigned n16 = (unsigned)src[at] | ((unsigned)src[at + 1] << 8), c16 = (unsigned)src[at + 2] | ((unsigned)src[at + 3] << 8);
      if ((n16 ^ c16) != 0xffffu) { err |= TT_INFLATE_STATUS_BLOCK; break; }
      const unsigned have = len - (at + 4u), take = n16 < have ? n16 : have;
      for (unsigned j = tid; j < take; j += INF_BLOCK) {                                  // at most 65 535 bytes
        const unsigned long long q = produced + j;
        if (q < expected) d.src[abs0 + (unsigned)q] = LIT | (unsigned)src[at + 4u + j];
      }
      produced += take;
      pos += 32ull + 8ull * take;
      if (take < n16) break;
      if (last) { clean = true; break; }
      continue;
    }
    __syncthreads();                                                                      // the codes of the block before are done with
    if (tid == 0) {
      Reader r = {src, len, pos, total, false};
      hdr_err_s = block_codes(r, type == 1u, lit_s, dist_s, lens_s);
      hdr_pos_s = r.pos;
    }
    __syncthreads();
    if (hdr_err_s) { err |= hdr_err_s & 0x7fffu; break; }
    pos = hdr_pos_s;
    bool ended = false, fatal = false;
    const unsigned long long windows = (total - pos) / WIN_BITS + 2ull;                   // a window without an end passes WIN_BITS bits or more
    for (unsigned long long wi = 0; wi < windows; ++wi) {
      const unsigned base = (unsigned)(pos >> 3), rel0 = (unsigned)(pos & 7u);
      for (unsigned k = tid; k < WIN_WORDS; k += INF_BLOCK) {
        unsigned v = 0;
#pragma unroll
        for (unsigned b = 0; b < 4; ++b) {
          const unsigned long long i = (unsigned long long)base + 4ull * k + b;
          if (i < len) v |= (unsigned)src[i] << (8 * b);
        }
        win_s[k] = v;
      }
      if (tid == 0) { first_s = INF_BLOCK; stop_kind_s = 0; }
      __syncthreads();
      const unsigned long long left = total - 8ull * base;
      const unsigned limit = left > 0xffff0000ull ? 0xffff0000u : (unsigned)left;
      const unsigned end = rel0 + (tid + 1u) * SUB_BITS;
      unsigned start = rel0 + tid * SUB_BITS, used_start = 0xffffffffu;
      Sub mine = {start, 0u, 0u, 0u};
      for (int round = 0; round <= INF_BLOCK; ++round) {                                  // lane k starts right from round k on
        const int changed = start != used_start;
        if (changed) {
          mine = decode_sub<false>(win_s, lit_s, dist_s, start, end, limit, nullptr, 0u, 0ull, 0u, nullptr);
          used_start = start;
          exit_s[tid] = mine.stop ? end : mine.exit;                                      // behind a stop nothing counts: the neighbour keeps its guess
        }
        if (!__syncthreads_or(changed)) break;
        if (tid > 0) start = exit_s[tid - 1];
        __syncthreads();
      }
      if (mine.stop) atomicMin(&first_s, tid);
      __syncthreads();
      const unsigned first = first_s;
      const bool live = tid <= first;
      if (tid == first) { stop_exit_s = mine.exit; stop_kind_s = mine.stop; stop_err_s = mine.err; }
      unsigned long long all;
      const unsigned long long before = block_scan_excl<INF_WAVES>((unsigned long long)(live ? mine.cnt : 0u), red_s, all);
      if (live && mine.cnt) decode_sub<true>(win_s, lit_s, dist_s, start, end, limit, d.src, abs0, produced + before, expected, status);
      produced += all;
      const unsigned kind = stop_kind_s, stop_exit = stop_exit_s, stop_err = stop_err_s, last_exit = exit_s[INF_BLOCK - 1];
      __syncthreads();
      if (kind) {
        pos = 8ull * base + stop_exit;
        if (kind == 1u) ended = true;
        else { fatal = true; err |= stop_err; }
        break;
      }
      pos = 8ull * base + last_exit;
    }
    if (fatal || !ended) break;
    if (last) { clean = true; break; }
  }
  // the trailer, SHORT and LONG, and the bytes the stream did not reach
  const unsigned long long made = produced < expected ? produced : expected;
  for (unsigned long long q = made + tid; q < expected; q += INF_BLOCK) d.src[abs0 + (unsigned)q] = LIT;
  if (tid == 0) {
    StreamRec rc = {};
    rc.out_off = out_off;
    rc.ok = 1u;
    rc.expected = expected;
    if (produced < expected) err |= TT_INFLATE_STATUS_SHORT;
    if (produced > expected) err |= TT_INFLATE_STATUS_LONG;
    if (clean && produced == expected) {
      const unsigned long long at = (pos + 7ull) >> 3;
      if (at + 4ull <= len) {
        rc.trailer = ((unsigned)src[at] << 24) | ((unsigned)src[at + 1] << 16) | ((unsigned)src[at + 2] << 8) | (unsigned)src[at + 3];
        rc.checked = 1u;
      } else err |= TT_INFLATE_STATUS_ADLER;                                               // no whole trailer
    }
    d.rec[f] = rc;
    if (err) atomicOr(status, err);
  }
}

// grid (ceil(max_out / JMP_BLOCK), n): one round of src <- src[src].  A word read while another lane replaces it is the old or the new
// one, each an ancestor further up or the literal: after round k every word is a literal or names a byte 2^k copies back or more
__global__ __launch_bounds__(JMP_BLOCK) void inflate_jump_kernel(Inf d) {
  const StreamRec rc = d.rec[blockIdx.y];
  const unsigned long long p = (unsigned long long)blockIdx.x * JMP_BLOCK + threadIdx.x;
  if (!rc.ok || p >= rc.expected) return;
  const unsigned long long i = (unsigned long long)rc.out_off + p;
  const unsigned v = d.src[i];
  if (!(v & LIT) && (long long)v < d.out_bytes) d.src[i] = d.src[v];
}

// grid (chunks_per, n): a chunk's bytes, and its Adler-32 pair started from (0, 0): sum b, sum (L - i) b over the chunk's L bytes
__global__ __launch_bounds__(BYT_BLOCK) void inflate_bytes_kernel(Inf d) {
  __shared__ unsigned long long red_s[BYT_WAVES];
  const unsigned f = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const StreamRec rc = d.rec[f];
  if (!rc.ok) return;
  const unsigned long long c0 = (unsigned long long)c * CHUNK;
  if (c0 >= rc.expected) return;
  const unsigned chunk_len = rc.expected - c0 < CHUNK ? (unsigned)(rc.expected - c0) : CHUNK;
  const unsigned s = tid * BYT_PER, mine = s >= chunk_len ? 0u : (chunk_len - s < (unsigned)BYT_PER ? chunk_len - s : (unsigned)BYT_PER);
  unsigned long long a = 0, b = 0;
  for (unsigned j = 0; j < mine; ++j) {
    const unsigned long long i = (unsigned long long)rc.out_off + c0 + s + j;
    const unsigned v = d.src[i];
    const unsigned byte = v & LIT ? v & 0xffu : 0u;
    d.out[i] = (unsigned char)byte;
    a += byte;
    b += (unsigned long long)(mine - j) * byte;
  }
  if (mine) b += (unsigned long long)(chunk_len - s - mine) * a;
  const unsigned long long sa = block_sum<BYT_WAVES>(a, red_s);
  __syncthreads();
  const unsigned long long sb = block_sum<BYT_WAVES>(b, red_s);
  if (tid == 0) {
    d.pairs[2ull * ((unsigned long long)f * d.chunks_per + c)] = (unsigned)(sa % ADLER);
    d.pairs[2ull * ((unsigned long long)f * d.chunks_per + c) + 1ull] = (unsigned)(sb % ADLER);
  }
}

// grid (n): the chunks' pairs combined into the stream's Adler-32 and compared with its trailer
__global__ __launch_bounds__(BYT_BLOCK) void inflate_adler_kernel(Inf d) {
  __shared__ unsigned long long red_s[BYT_WAVES];
  const unsigned f = blockIdx.x, tid = threadIdx.x;
  const StreamRec rc = d.rec[f];
  if (!rc.ok || !rc.checked) return;
  const unsigned chunks = (unsigned)(((unsigned long long)rc.expected + CHUNK - 1ull) / CHUNK);
  unsigned long long a = 0, b = 0;
  for (unsigned c = tid; c < chunks && c < d.chunks_per; c += BYT_BLOCK) {
    const unsigned long long c0 = (unsigned long long)c * CHUNK, chunk_len = rc.expected - c0 < CHUNK ? rc.expected - c0 : CHUNK;
    const unsigned long long pa = d.pairs[2ull * ((unsigned long long)f * d.chunks_per + c)], pb = d.pairs[2ull * ((unsigned long long)f * d.chunks_per + c) + 1ull];
    a += pa;                                                                              // 2^20 chunks of 65 520 at the most: far from 2^64
    b += pb + ((rc.expected - c0 - chunk_len) % ADLER) * pa;
  }
  const unsigned long long sa = block_sum<BYT_WAVES>(a, red_s);
  __syncthreads();
  const unsigned long long sb = block_sum<BYT_WAVES>(b % ADLER, red_s);
  if (tid == 0) {
    const unsigned s1 = (unsigned)((1ull + sa) % ADLER), s2 = (unsigned)((rc.expected % ADLER + sb) % ADLER);
    if (((s2 << 16) | s1) != rc.trailer) atomicOr(d.status + f, (unsigned)TT_INFLATE_STATUS_ADLER);
  }
}

struct Unf {
  const unsigned char* filtered;
  long long stride;
  int n, h, w, ch;
  unsigned char* out;
  unsigned* status;
};

__device__ __forceinline__ unsigned paeth(unsigned a, unsigned b, unsigned c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
  return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

// grid (bands, n).  A band is UNF_BLOCK rows, a lane per row; step t handles the pixels x = t - row of the band's anti-diagonal, whose
// left, upper and upper-left neighbours were made one and two steps before.  A band whose first row is of type 0 or 1 needs nothing of
// the row above: its workgroup starts there and goes on through the bands that follow until the next such band, which has its own
__global__ __launch_bounds__(UNF_BLOCK) void png_unfilter_kernel(Unf u) {
  __shared__ unsigned ring_s[2][UNF_BLOCK];
  const unsigned f = blockIdx.y, tid = threadIdx.x;
  const int bands = (u.h + UNF_BLOCK - 1) / UNF_BLOCK, w = u.w, ch = u.ch;
  const long long rb = 1ll + (long long)w * ch;
  const unsigned char* __restrict__ in = u.filtered + (long long)f * u.stride;
  unsigned char* out = u.out + (long long)f * u.h * w * ch;
  const int b0 = (int)blockIdx.x;
  if (b0 > 0) {
    const unsigned t0 = in[(long long)b0 * UNF_BLOCK * rb];
    if (t0 >= 2u && t0 <= 4u) return;                                                     // the band before leads into this one
  }
  for (int band = b0; band < bands; ++band) {
    const int row0 = band * UNF_BLOCK, rows = u.h - row0 < UNF_BLOCK ? u.h - row0 : UNF_BLOCK;
    if (band > b0) {
      const unsigned t0 = in[(long long)row0 * rb];
      if (t0 < 2u || t0 > 4u) break;                                                      // another workgroup's
    }
    const int y = row0 + (int)tid;
    const bool active = (int)tid < rows;
    unsigned type = active ? in[(long long)y * rb] : 0u;
    if (type > 4u) { atomicOr(u.status + f, (unsigned)TT_PNG_UNFILTER_STATUS_TYPE); type = 0u; }
    const unsigned char* __restrict__ row = in + (long long)(active ? y : 0) * rb + 1;
    unsigned char* dst = out + (long long)(active ? y : 0) * w * ch;
    const unsigned char* above = out + (long long)(y > 0 && active ? y - 1 : 0) * w * ch;  // lane 0: the last row of the band before
    unsigned left = 0, prev_up = 0;
    const int steps = w + rows - 1;
    for (int t = 0; t < steps; ++t) {
      const int x = t - (int)tid;
      if (active && x >= 0 && x < w) {
        unsigned up = 0;
        if (tid > 0) up = ring_s[(t - 1) & 1][tid - 1];
        else if (y > 0 && type >= 2u)
          for (int c = 0; c < ch; ++c) up |= (unsigned)above[(long long)x * ch + c] << (8 * c);
        const unsigned ul = x == 0 ? 0u : prev_up, lf = x == 0 ? 0u : left;
        unsigned px = 0;
        for (int c = 0; c < ch; ++c) {
          const unsigned v = row[(long long)x * ch + c], a = (lf >> (8 * c)) & 255u, b = (up >> (8 * c)) & 255u, cc = (ul >> (8 * c)) & 255u;
          const unsigned pred = type == 0u ? 0u : (type == 1u ? a : (type == 2u ? b : (type == 3u ? (a + b) >> 1 : paeth(a, b, cc))));
          const unsigned r = (v + pred) & 255u;
          dst[(long long)x * ch + c] = (unsigned char)r;
          px |= r << (8 * c);
        }
        ring_s[t & 1][tid] = px;
        left = px;
        prev_up = up;
      }
      __syncthreads();
    }
    __syncthreads();                                                                      // the band's last row is in memory for the next band's lane 0
  }
}

struct Plan {                                      // the workspace, each part at a multiple of 16; ok = 0: refused arguments
  int ok;
  long long chunks_per, rec_at, src_at, pairs_at, total;
};

long long up16(long long v) { return (v + 15) / 16 * 16; }

Plan plan(long long n, long long out_bytes, long long max_out) {
  Plan pl = {};
  if (n <= 0 || n > TT_INFLATE_MAX_STREAMS || out_bytes <= 0 || out_bytes >= (1ll << 31) || max_out <= 0 || max_out > out_bytes) return pl;
  pl.chunks_per = (max_out + CHUNK - 1) / CHUNK;
  pl.rec_at = 0;
  pl.src_at = up16(n * (long long)sizeof(StreamRec));
  pl.pairs_at = pl.src_at + up16(out_bytes * 4);
  pl.total = pl.pairs_at + up16(n * pl.chunks_per * 8);
  pl.ok = 1;
  return pl;
}

}  // namespace

extern "C" int64_t tt_png_decode_ws_bytes(int32_t n, int64_t out_bytes, int64_t max_out) {
  const Plan pl = plan(n, out_bytes, max_out);
  return pl.ok ? pl.total : 0;
}

extern "C" int tt_png_inflate(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const uint32_t* lengths, const uint32_t* expected,
                              const int64_t* out_offsets, int32_t n, int64_t max_out, uint8_t* out, int64_t out_bytes, uint32_t* status, void* ws,
                              int64_t ws_bytes, tt_stream_t stream) {
  const char* who = "tt_png_inflate";
  const void* ptrs[] = {data, offsets, out_offsets, lengths, expected, out, status, ws};
  const char* names[] = {"data", "offsets", "out_offsets", "lengths", "expected", "out", "status", "ws"};
  for (int i = 0; i < 8; ++i)
    if (!ptrs[i]) TT_FAIL(TT_EINVAL, "%s: null %s", who, names[i]);
  if (n <= 0 || data_bytes <= 0 || out_bytes <= 0 || max_out <= 0)
    TT_FAIL(TT_EINVAL, "%s: empty problem (n = %d, data_bytes = %lld, out_bytes = %lld, max_out = %lld)", who, n, (long long)data_bytes, (long long)out_bytes,
            (long long)max_out);
  if (max_out > out_bytes) TT_FAIL(TT_EINVAL, "%s: max_out = %lld above out_bytes = %lld", who, (long long)max_out, (long long)out_bytes);
  for (int i = 1; i <= 2; ++i)
    if ((uintptr_t)ptrs[i] & 7) TT_FAIL(TT_EINVAL, "%s: %s is not 8-byte aligned", who, names[i]);
  for (int i = 3; i <= 4; ++i)
    if ((uintptr_t)ptrs[i] & 3) TT_FAIL(TT_EINVAL, "%s: %s is not 4-byte aligned", who, names[i]);
  if ((uintptr_t)status & 3) TT_FAIL(TT_EINVAL, "%s: status is not 4-byte aligned", who);
  if ((uintptr_t)ws & 15) TT_FAIL(TT_EINVAL, "%s: ws is not 16-byte aligned", who);
  if (n > TT_INFLATE_MAX_STREAMS) TT_FAIL(TT_EUNSUPPORTED, "%s: %d streams: more than one grid covers (%d)", who, n, TT_INFLATE_MAX_STREAMS);
  if (data_bytes >= (1ll << 29))
    TT_FAIL(TT_EUNSUPPORTED, "%s: data_bytes = %lld: the kernels' 32-bit bit offsets address fewer than 2^29 = 536870912", who, (long long)data_bytes);
  if (out_bytes >= (1ll << 31))
    TT_FAIL(TT_EUNSUPPORTED, "%s: out_bytes = %lld: a source word indexes fewer than 2^31 = 2147483648 bytes", who, (long long)out_bytes);
  const Plan pl = plan(n, out_bytes, max_out);
  if (!pl.ok || ws_bytes < pl.total)
    TT_FAIL(TT_EINVAL, "%s: ws too small: %lld bytes, tt_png_decode_ws_bytes = %lld", who, (long long)ws_bytes, pl.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  Inf d;
  d.data = data;
  d.data_bytes = data_bytes;
  d.offsets = (const long long*)offsets;
  d.lengths = lengths;
  d.expected = expected;
  d.out_offsets = (const long long*)out_offsets;
  d.n = n;
  d.out = out;
  d.out_bytes = out_bytes;
  d.max_out = (unsigned)max_out;
  d.chunks_per = (unsigned)pl.chunks_per;
  d.status = status;
  d.rec = (StreamRec*)(w + pl.rec_at);
  d.src = (unsigned*)(w + pl.src_at);
  d.pairs = (unsigned*)(w + pl.pairs_at);
  if (hipMemsetAsync(status, 0, (size_t)n * sizeof(uint32_t), st) != hipSuccess) TT_FAIL(TT_ELAUNCH, "%s: hipMemsetAsync failed", who);
  int rounds = 0;                                                                         // ceil(log2(max_out)): a byte's chain of copies is shorter than max_out
  while ((1ll << rounds) < max_out) ++rounds;
  hipLaunchKernelGGL(inflate_tokens_kernel, dim3((unsigned)n), dim3(INF_BLOCK), 0, st, d);
  const dim3 jump_grid((unsigned)((max_out + JMP_BLOCK - 1) / JMP_BLOCK), (unsigned)n);
  for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(inflate_jump_kernel, jump_grid, dim3(JMP_BLOCK), 0, st, d);
  hipLaunchKernelGGL(inflate_bytes_kernel, dim3((unsigned)pl.chunks_per, (unsigned)n), dim3(BYT_BLOCK), 0, st, d);
  hipLaunchKernelGGL(inflate_adler_kernel, dim3((unsigned)n), dim3(BYT_BLOCK), 0, st, d);
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}

extern "C" int tt_png_unfilter(const uint8_t* filtered, int32_t n, int32_t h, int32_t w, int32_t ch, uint8_t* out, uint32_t* status, tt_stream_t stream) {
  const char* who = "tt_png_unfilter";
  if (!filtered || !out || !status) TT_FAIL(TT_EINVAL, "%s: null %s", who, !filtered ? "filtered" : (!out ? "out" : "status"));
  if (!tt_png_shape_ok(n, h, w, ch)) TT_FAIL(TT_EINVAL, "%s: n = %d, h = %d, w = %d (positive) and ch = %d (1 .. 4)", who, n, h, w, ch);
  if ((uintptr_t)filtered & 15) TT_FAIL(TT_EINVAL, "%s: filtered is not 16-byte aligned", who);
  if ((uintptr_t)status & 3) TT_FAIL(TT_EINVAL, "%s: status is not 4-byte aligned", who);
  if (tt_png_stream_bytes(h, w, ch) >= (1ll << 31)) TT_FAIL(TT_EUNSUPPORTED, "%s: a stream of %lld bytes (fewer than 2^31)", who, (long long)tt_png_stream_bytes(h, w, ch));
  if (n > TT_INFLATE_MAX_STREAMS) TT_FAIL(TT_EUNSUPPORTED, "%s: %d frames: more than one grid covers (%d)", who, n, TT_INFLATE_MAX_STREAMS);
  Unf u;
  u.filtered = filtered;
  u.stride = tt_png_frame_stride(h, w, ch);
  u.n = n;
  u.h = h;
  u.w = w;
  u.ch = ch;
  u.out = out;
  u.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, (size_t)n * sizeof(uint32_t), st) != hipSuccess) TT_FAIL(TT_ELAUNCH, "%s: hipMemsetAsync failed", who);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)((h + UNF_BLOCK - 1) / UNF_BLOCK), (unsigned)n), dim3(UNF_BLOCK), 0, st, u);
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}
