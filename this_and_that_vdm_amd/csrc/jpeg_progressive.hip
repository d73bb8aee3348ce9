// libttvdm: progressive JPEG scans on the device (include/ttvdm.h, "JPEG import", rule 4b): tt_jpeg_entropy_progressive.  The items are
// (frame, scan) pairs: all are unstuffed at once by rule 3's kernels (jpeg_device.h), then one launch a ROUND applies scan s of every
// frame that has one into tt_jpeg_coeffs' layout -- DC first, DC refine, AC first, AC refine, the kind read from a device descriptor --,
// one workgroup a frame.  tt_jpeg_pixels (jpeg_decode.hip) finishes the job.  Integers only; the one atomic is an OR into a status word.
#include "jpeg_device.h"

namespace {

constexpr int MASK_STAGE = 1024;                     // masks of an AC-refine scan staged in LDS at a time
constexpr unsigned LANE_BLOCKS_MAX = 1u << 22;       // a lane's blocks completed saturate here: 256 lanes stay below 2^31
constexpr unsigned SCAN_BLOCKS_MAX = 0x7fffffffu;    // ... and a scan's here (EOB runs of a crafted stream)
constexpr unsigned IN_RUN = 0x80000000u;             // a recorded position's flag: the block lies inside an EOB run

// the scan's block order -> the layout's (rule 4b, "block map")
struct ScanGeo {
  unsigned nblocks;                                  // of the scan
  unsigned bw, mcus_x;                               // mode 2: the component's blocks per row; MCUs per row
  int mode;                                          // 0: block k; 1: block `off` of MCU k, bpm blocks each; 2: the 4:2:0 Y plane
  int bpm, off;
};
__device__ __forceinline__ unsigned layout_block(const ScanGeo& g, unsigned k) {
  if (g.mode == 0) return k;
  if (g.mode == 1) return k * (unsigned)g.bpm + (unsigned)g.off;
  const unsigned by = k / g.bw, bx = k - by * g.bw;
  return ((by >> 1) * g.mcus_x + (bx >> 1)) * 6u + (by & 1u) * 2u + (bx & 1u);
}

// a scan's constants, uniform over the workgroup
struct ProgScan {
  unsigned L;                                        // bits of the plain stream
  unsigned ss, se, al;
  bool dc, inter;                                    // a DC scan; an interleaved one (every component, MCU order)
  int bpm;
  unsigned comp;                                     // the component of a single-component scan
  unsigned blocks;                                   // tt_jpeg_blocks
  ScanGeo geo;
};

// the 32 bits at bit p of the plain stream in global memory (big-endian dwords; words behind the stride read as zero)
__device__ __forceinline__ unsigned stream_bits(const unsigned* __restrict__ words, long long stride_words, unsigned p) {
  const long long wi = p >> 5;
  const unsigned a = wi < stride_words ? __builtin_bswap32(words[wi]) : 0u, b = wi + 1 < stride_words ? __builtin_bswap32(words[wi + 1]) : 0u;
  return (unsigned)(((((unsigned long long)a << 32) | b) << (p & 31u)) >> 32);
}

// what is left of the stream behind bit p is not fewer than 8 one-bits
__device__ __forceinline__ bool tail_bad(const unsigned char* __restrict__ stream, unsigned nbytes, unsigned p) {
  const unsigned L = nbytes * 8u, left = L - min(p, L);
  const unsigned ones = left ? (1u << min(left, 8u)) - 1u : 0u;
  return left >= 8u || (left && ((unsigned)stream[nbytes - 1] & ones) != ones);
}

// f_i of a first scan (Ah = 0): the whole symbols that start in [max(st.p, start), end); st becomes the exit state -- DC: (p, block within
// the MCU), AC: (p, z) --; returns the blocks completed, EOB runs included.  WRITE: the values go to the frame's coefficients `fc` through
// the block map, the first block touched is `block`.  At most SUBSEQ iterations: every one takes a bit or more.
template <bool WRITE>
__device__ __forceinline__ unsigned first_span(const unsigned* win_s, unsigned win0, const unsigned* tab_s, const ProgScan& sc, unsigned start, unsigned end,
                                               DecState& st, short* __restrict__ fc, unsigned block, unsigned& err) {
  unsigned p = st.p, m = st.mz >> 6, z = st.mz & 63u, done = 0u;
  if (p < start) return 0u;                          // a lane before this one stopped at the end of the stream: pass the state on
  for (int it = 0; it < SUBSEQ && p < end; ++it) {
    const unsigned v = window_bits(win_s, win0, p);
    const unsigned avail = sc.L - p;
    const unsigned slot = sc.dc ? (sc.inter ? (sc.bpm == 6 ? (m < 4u ? 0u : m - 3u) : min(m, 2u)) : sc.comp) : 0u;
    unsigned len, sym;
    huff_lookup(tab_s + slot * TT_JPEG_DECODE_WORDS, v, len, sym);
    if (len == 0u) {
      if (avail < 16u) break;                        // no code within the bits left: the lane stops
      if (WRITE) err |= TT_JPEG_STATUS_CODE;
      p += 1u;                                       // no code at all: skip one bit
      continue;
    }
    const unsigned n = sym & 15u, r = sym >> 4;
    if (!sc.dc && n == 0u && r < 15u) {              // EOBn: a run of blocks that end here
      if (len + r > avail) break;
      const unsigned extra = r ? (v << len) >> (32u - r) : 0u;
      p += len + r;
      done = min(done + (1u << r) + extra, LANE_BLOCKS_MAX);
      z = sc.ss;
      continue;
    }
    if (len + n > avail) break;                      // the symbol would read beyond L: the lane stops
    const unsigned raw = n ? (v << len) >> (32u - n) : 0u;
    const int value = n ? huff_extend(raw, n) : 0;
    p += len + n;
    const unsigned at = block + done;
    bool ends = false;
    if (sc.dc) {
      if (WRITE) {
        if (sym > 11u) err |= TT_JPEG_STATUS_CODE;
        const unsigned lb = layout_block(sc.geo, at);
        if (at < sc.geo.nblocks && lb < sc.blocks) fc[(long long)lb * 64] = (short)value;
      }
      if (sc.inter) m = (int)m + 1 >= sc.bpm ? 0u : m + 1u;
      ends = true;
    } else if (n == 0u) {
      z += 16u;                                      // ZRL
      ends = z > sc.se;
    } else {
      z += r;
      if (z > sc.se) {
        ends = true;                                 // a run that passes Se: the block ends
        if (WRITE) err |= TT_JPEG_STATUS_CODE;
      } else {
        if (WRITE) {
          const unsigned lb = layout_block(sc.geo, at);
          if (at < sc.geo.nblocks && lb < sc.blocks) fc[(long long)lb * 64 + z] = (short)((unsigned)value << sc.al);
        }
        ++z;
        ends = z > sc.se;
      }
    }
    if (ends) {
      if (!sc.dc) z = sc.ss;
      done = min(done + 1u, LANE_BLOCKS_MAX);
    }
  }
  st.p = p;
  st.mz = m << 6 | z;
  return done;
}

// one correction bit for an already-nonzero coefficient (T.81 G.1.2.3)
__device__ __forceinline__ void refine_coef(short* __restrict__ at, unsigned bit, int p1) {
  const int c = *at;
  if (bit && (c & p1) == 0) *at = (short)(c >= 0 ? c + p1 : c - p1);
}

// grid (n), ELANES lanes: round `round` -- scan `round` of every frame that has one.  Nothing another workgroup writes in this launch is read.
__global__ __launch_bounds__(ELANES) void jpeg_progressive_round_kernel(const unsigned char* __restrict__ plain, long long plain_stride,
                                                                       const unsigned* __restrict__ plain_bytes, long long max_bytes,
                                                                       const unsigned* __restrict__ desc, const unsigned* __restrict__ tables, int nscans,
                                                                       int round, int h, int w, TtJpegGeometry geo, unsigned blocks, short* __restrict__ coeffs,
                                                                       unsigned* __restrict__ status, unsigned long long* __restrict__ masks,
                                                                       unsigned* __restrict__ starts) {
  __shared__ unsigned win_s[SEQ_WORDS + 2];
  __shared__ unsigned tab_s[3 * TT_JPEG_DECODE_WORDS];
  __shared__ unsigned ex_p[ELANES], ex_mz[ELANES];
  __shared__ unsigned long long mask_s[MASK_STAGE];
  __shared__ unsigned red_s[EWAVES];
  __shared__ unsigned walk_s[4];                     // the walk's bit position, block, "finished"
  const int tid = threadIdx.x;
  const int f = blockIdx.x;
  const long long item = (long long)f * nscans + round;
  const unsigned* __restrict__ d = desc + item * TT_JPEG_SCAN_WORDS;
  const unsigned comps = d[0];
  if (comps == 0u) return;                           // uniform: the frame has no such scan
  const unsigned every = (1u << geo.ncomp) - 1u;
  ProgScan sc;
  sc.ss = min(d[1], 63u);
  sc.se = min(d[2], 63u);
  sc.al = min(d[4], 13u);
  const bool refine = d[3] != 0u;
  sc.dc = sc.ss == 0u;
  const bool single = __popc(comps) == 1;
  if (comps > every || (sc.dc ? !(single || comps == every) : (!single || sc.se < sc.ss))) {       // uniform: numbers no scan has
    if (tid == 0) atomicOr(&status[f], TT_JPEG_STATUS_SPAN);
    return;
  }
  sc.inter = geo.ncomp > 1 && comps == every;
  sc.comp = (unsigned)(__ffs((int)comps) - 1);
  sc.bpm = geo.blocks_per_mcu;
  sc.blocks = blocks;
  const unsigned mcus = (unsigned)geo.mcus_x * (unsigned)geo.mcus_y;
  sc.geo.bw = 1u;
  sc.geo.mcus_x = (unsigned)geo.mcus_x;
  sc.geo.bpm = sc.bpm;
  if (sc.inter || geo.ncomp == 1) { sc.geo.mode = 0; sc.geo.off = 0; sc.geo.nblocks = blocks; }
  else if (sc.bpm == 6 && sc.comp == 0u) { sc.geo.mode = 2; sc.geo.off = 0; sc.geo.bw = (unsigned)(w + 7) / 8u; sc.geo.nblocks = sc.geo.bw * ((unsigned)(h + 7) / 8u); }
  else { sc.geo.mode = 1; sc.geo.off = sc.bpm == 6 ? 3 + (int)sc.comp : (int)sc.comp; sc.geo.nblocks = mcus; }
  const unsigned nblocks = sc.geo.nblocks;
  const unsigned* __restrict__ tset = tables + item * (3 * TT_JPEG_DECODE_WORDS);
  for (int i = tid; i < 3 * TT_JPEG_DECODE_WORDS; i += ELANES) tab_s[i] = tset[i];
  const unsigned nbytes = (unsigned)min((long long)plain_bytes[item], max_bytes);
  const unsigned char* __restrict__ stream = plain + item * plain_stride;
  const unsigned* __restrict__ words = (const unsigned*)stream;
  const long long stride_words = plain_stride / 4;
  short* __restrict__ fc = coeffs + (long long)f * blocks * 64;
  sc.L = nbytes * 8u;                                // max_bytes < 2^28: below 2^31
  unsigned err = 0u;
  __syncthreads();

  if (sc.dc && refine) {                             // ---- DC refine: bit k is block k's
    const short bit = (short)(1u << sc.al);
    for (unsigned k = tid; k < nblocks; k += ELANES) {
      const unsigned lb = layout_block(sc.geo, k);
      if (k < sc.L && lb < blocks && (((unsigned)stream[k >> 3] >> (7u - (k & 7u))) & 1u)) fc[(long long)lb * 64] |= bit;
    }
    if (tid == 0) {
      if (sc.L < nblocks) err |= TT_JPEG_STATUS_BLOCKS;
      if (tail_bad(stream, nbytes, min(nblocks, sc.L))) err |= TT_JPEG_STATUS_TAIL;
    }
  } else if (!refine) {                              // ---- DC first, AC first: rule 4's lanes and passes
    DecState carried = {0u, sc.dc ? 0u : sc.ss};     // the true state at the head of the sequence
    unsigned base = 0u;                              // blocks completed before the sequence
    const unsigned nseq = (sc.L + SEQ_BITS - 1u) / SEQ_BITS;
    for (unsigned q = 0; q < nseq; ++q) {
      const unsigned win0 = q * SEQ_BITS;
      __syncthreads();                               // the window and the states of the sequence before are done with
      for (unsigned i = tid; i < SEQ_WORDS + 2u; i += ELANES) {                 // words behind L: no result depends on them (rule 4)
        const long long gw = (long long)q * SEQ_WORDS + i;
        win_s[i] = gw < stride_words ? __builtin_bswap32(words[gw]) : 0u;
      }
      __syncthreads();
      const unsigned start = win0 + (unsigned)tid * SUBSEQ, end = min(start + (unsigned)SUBSEQ, sc.L);
      const bool active = start < sc.L;
      const int last = (int)min((unsigned)ELANES - 1u, (sc.L - win0 - 1u) / (unsigned)SUBSEQ);
      unsigned none = 0u;
      DecState used = carried, x;
      if (tid) { used.p = start; used.mz = sc.dc ? 0u : sc.ss; }
      x = used;
      unsigned done = first_span<false>(win_s, win0, tab_s, sc, start, end, x, fc, 0u, none);
      ex_p[tid] = x.p;
      ex_mz[tid] = x.mz;
      for (int pass = 1; pass < ELANES; ++pass) {     // after k passes the first k + 1 lanes are exact
        __syncthreads();
        DecState entry = carried;
        if (tid) { entry.p = ex_p[tid - 1]; entry.mz = ex_mz[tid - 1]; }
        const bool changed = active && !same(entry, used);
        if (!__syncthreads_or(changed)) break;       // uniform: nobody's entry moved, the states are final
        if (changed) {
          used = entry;
          x = used;
          done = first_span<false>(win_s, win0, tab_s, sc, start, end, x, fc, 0u, none);
          ex_p[tid] = x.p;
          ex_mz[tid] = x.mz;
        }
      }
      unsigned all;
      const unsigned first = base + block_scan_excl<EWAVES>(done, red_s, all);
      x = used;
      first_span<true>(win_s, win0, tab_s, sc, start, end, x, fc, first, err);
      carried.p = ex_p[last];
      carried.mz = ex_mz[last];
      base = min(base + all, SCAN_BLOCKS_MAX);
    }
    if (tid == 0) {
      if (base != nblocks) err |= TT_JPEG_STATUS_BLOCKS;
      if (tail_bad(stream, nbytes, carried.p)) err |= TT_JPEG_STATUS_TAIL;
    }
    if (sc.dc) {                                     // the differences -> pred << Al, per component over the scan's block order
      for (unsigned c = 0; c < 3u; ++c) {
        if (!((comps >> c) & 1u)) continue;          // uniform
        const unsigned nk = (sc.inter && sc.bpm == 6 && c == 0u) ? 4u : 1u, k0 = c == 0u ? 0u : (sc.bpm == 6 ? 3u + c : c);
        const unsigned count = sc.inter ? mcus * nk : nblocks;
        unsigned carry = 0u;
        for (unsigned at = 0; at < count; at += ELANES) {
          __syncthreads();                           // red_s is free; the differences of the last pass are stored
          const unsigned j = at + tid;
          const unsigned lb = sc.inter ? (j / nk) * (unsigned)sc.bpm + k0 + j % nk : layout_block(sc.geo, j);
          const bool ok = j < count && lb < blocks;
          const unsigned diff = ok ? (unsigned)(int)fc[(long long)lb * 64] : 0u;
          unsigned all;
          const unsigned before = carry + block_scan_excl<EWAVES>(diff, red_s, all);
          if (ok) fc[(long long)lb * 64] = (short)((before + diff) << sc.al);
          carry += all;
        }
      }
    }
  } else {                                           // ---- AC refine: masks, one lane's walk over bit positions, replay
    const unsigned long long band = (sc.se == 63u ? ~0ull : ((1ull << (sc.se + 1u)) - 1ull)) & ~((1ull << sc.ss) - 1ull);
    unsigned long long* __restrict__ mk = masks + (long long)f * blocks;
    unsigned* __restrict__ st = starts + (long long)f * blocks;
    const int p1 = 1 << sc.al;
    for (unsigned k = tid; k < nblocks; k += ELANES) {
      const unsigned lb = layout_block(sc.geo, k);
      unsigned long long m = 0ull;
      if (lb < blocks) {
        const uint4* __restrict__ q = (const uint4*)(fc + (long long)lb * 64);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const uint4 v = q[u];
          const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if ((wd[j >> 1] >> (16 * (j & 1))) & 0xffffu) m |= 1ull << (8 * u + j);
        }
      }
      mk[k] = m & band;
    }
    if (tid == 0) { walk_s[0] = 0u; walk_s[1] = 0u; walk_s[2] = 0u; }
    unsigned p = 0u, b = 0u, z = sc.ss, run = 0u;     // lane 0's true state
    bool fresh = true;                               // the block's position is not recorded yet
    const unsigned nstages = sc.L / (SEQ_BITS - 31u) + nblocks / MASK_STAGE + 2u;
    for (unsigned stage = 0; stage < nstages; ++stage) {
      __syncthreads();                               // the masks (first trip), lane 0's records and walk_s are stored
      const unsigned P = walk_s[0], B = walk_s[1];
      if (walk_s[2]) break;                          // uniform
      const unsigned w0 = P >> 5;
      for (unsigned i = tid; i < SEQ_WORDS + 2u; i += ELANES) {
        const long long gw = (long long)w0 + i;
        win_s[i] = gw < stride_words ? __builtin_bswap32(words[gw]) : 0u;
      }
      for (unsigned i = tid; i < (unsigned)MASK_STAGE; i += ELANES) mask_s[i] = B + i < nblocks ? mk[B + i] : 0ull;
      __syncthreads();
      if (tid == 0) {
        const unsigned win0 = w0 * 32u, wend = win0 + SEQ_BITS, bend = min(B + (unsigned)MASK_STAGE, nblocks);
        bool finished = false;
        for (unsigned it = 0; it < SEQ_BITS + (unsigned)MASK_STAGE; ++it) {      // every trip takes a bit or a block
          if (b >= nblocks || p > sc.L) { finished = true; break; }
          if (b >= bend || p >= wend) break;
          const unsigned long long M = mask_s[b - B];
          if (run) {                                 // inside an EOB run: the block's correction bits
            st[b] = p | IN_RUN;
            p += (unsigned)__popcll(M);
            --run; ++b;
            continue;
          }
          if (fresh) { st[b] = p; fresh = false; }
          const unsigned avail = sc.L - p;
          const unsigned v = window_bits(win_s, win0, p);
          unsigned len, sym;
          huff_lookup(tab_s, v, len, sym);
          if (len == 0u || len > avail) {            // no code, or none within the bits left: the walk stops
            if (len == 0u && avail >= 16u) err |= TT_JPEG_STATUS_CODE;
            finished = true;
            break;
          }
          const unsigned r = sym >> 4, s = sym & 15u;
          const unsigned long long ahead = ~0ull << z;                         // the band's positions z .. Se (M and band end at Se)
          if (s == 0u && r < 15u) {                  // EOBn: this block's rest, then run - 1 more
            if (len + r > avail) { finished = true; break; }
            run = (1u << r) + (r ? (v << len) >> (32u - r) : 0u) - 1u;
            p += len + r + (unsigned)__popcll(M & ahead);
            ++b; z = sc.ss; fresh = true;
            continue;
          }
          if (s > 1u) err |= TT_JPEG_STATUS_CODE;
          const unsigned sign = s ? 1u : 0u;
          if (len + sign > avail) { finished = true; break; }
          unsigned long long zeros = ~M & band & ahead;
#pragma unroll
          for (unsigned i = 0; i < 15u; ++i)
            if (i < r) zeros &= zeros - 1ull;        // drop the R zero-history positions skipped
          const unsigned k = zeros ? (unsigned)__ffsll((long long)zeros) - 1u : sc.se + 1u;
          const unsigned long long below = k >= 64u ? ~0ull : ((1ull << k) - 1ull);
          p += len + sign + (unsigned)__popcll(M & ahead & below);
          if (k > sc.se && s) err |= TT_JPEG_STATUS_CODE;                      // a new coefficient behind the band
          z = k + 1u;
          if (z > sc.se) { ++b; z = sc.ss; fresh = true; }
        }
        walk_s[0] = min(p, sc.L);
        walk_s[1] = b;
        walk_s[2] = (finished || b >= nblocks) ? 1u : 0u;
      }
    }
    __syncthreads();
    const unsigned reached = min(walk_s[1], nblocks);
    if (tid == 0) {
      if (b != nblocks || p > sc.L) err |= TT_JPEG_STATUS_BLOCKS;
      if (tail_bad(stream, nbytes, p)) err |= TT_JPEG_STATUS_TAIL;
    }
    for (unsigned k = tid; k < reached; k += ELANES) {                           // replay: a lane, a block
      const unsigned lb = layout_block(sc.geo, k);
      if (lb >= blocks) continue;
      short* __restrict__ blk = fc + (long long)lb * 64;
      const unsigned s0 = st[k];
      unsigned q = s0 & ~IN_RUN, zz = sc.ss;
      bool in_run = (s0 & IN_RUN) != 0u;
      for (int code = 0; code < 64 && !in_run && zz <= sc.se; ++code) {
        if (q >= sc.L) break;
        const unsigned v = stream_bits(words, stride_words, q);
        unsigned len, sym;
        huff_lookup(tab_s, v, len, sym);
        if (len == 0u || len > sc.L - q) break;
        const unsigned r = sym >> 4, s = sym & 15u;
        if (s == 0u && r < 15u) { q += len + r; in_run = true; break; }
        const int value = ((v << len) >> 31) ? p1 : -p1;
        q += len + (s ? 1u : 0u);
        int rr = (int)r;
        for (; zz <= sc.se; ++zz) {
          if (blk[zz]) {
            refine_coef(blk + zz, q < sc.L ? (stream_bits(words, stride_words, q) >> 31) : 0u, p1);
            ++q;
          } else if (--rr < 0) break;
        }
        if (s && zz <= sc.se) blk[zz] = (short)value;
        ++zz;
      }
      if (in_run)
        for (; zz <= sc.se; ++zz)
          if (blk[zz]) {
            refine_coef(blk + zz, q < sc.L ? (stream_bits(words, stride_words, q) >> 31) : 0u, p1);
            ++q;
          }
    }
  }
  if (err) atomicOr(&status[f], err);
}

// item i belongs to frame i / nscans
__global__ void jpeg_progressive_items_kernel(int* __restrict__ item_frame, int items, int nscans) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < items) item_frame[i] = i / nscans;
}

}  // namespace

extern "C" int tt_jpeg_entropy_progressive(const uint8_t* scans, int64_t scans_bytes, const int64_t* offsets, const uint32_t* lengths, const uint32_t* desc,
                                           const uint32_t* tables, int64_t max_bytes, int32_t n, int32_t nscans, int32_t h, int32_t w, int32_t ch,
                                           int32_t subsampling, int16_t* coeffs, uint32_t* status, void* ws, int64_t ws_bytes, tt_stream_t stream) {
  const char* who = "tt_jpeg_entropy_progressive";
  if (!scans || !offsets || !lengths || !desc || !tables || !coeffs || !status || !ws)
    TT_FAIL(TT_EINVAL, "%s: null %s", who,
            !scans ? "scans" : (!offsets ? "offsets" : (!lengths ? "lengths" : (!desc ? "desc" : (!tables ? "tables" : (!coeffs ? "coeffs" : (!status ? "status" : "ws")))))));
  const int rc = tt_jpeg_refuse_shape(who, n, h, w, ch, subsampling, "");
  if (rc != TT_OK) return rc;
  if (nscans <= 0) TT_FAIL(TT_EINVAL, "%s: nscans = %d", who, nscans);
  if (nscans > TT_JPEG_MAX_SCANS) TT_FAIL(TT_EUNSUPPORTED, "%s: %d scans a frame (at most %d)", who, nscans, TT_JPEG_MAX_SCANS);
  if ((int64_t)n * nscans > TT_JPEG_MAX_ITEMS)
    TT_FAIL(TT_EUNSUPPORTED, "%s: %d frames of %d scans: more items than one grid covers (%d)", who, n, nscans, TT_JPEG_MAX_ITEMS);
  if (scans_bytes <= 0 || max_bytes <= 0) TT_FAIL(TT_EINVAL, "%s: empty scans (scans_bytes = %lld, max_bytes = %lld)", who, (long long)scans_bytes, (long long)max_bytes);
  if (max_bytes >= (1ll << 28)) TT_FAIL(TT_EUNSUPPORTED, "%s: max_bytes = %lld (a scan below 2^28 bytes)", who, (long long)max_bytes);
  if ((uintptr_t)offsets & 7) TT_FAIL(TT_EINVAL, "%s: offsets is not 8-byte aligned", who);
  if ((uintptr_t)lengths & 3) TT_FAIL(TT_EINVAL, "%s: lengths is not 4-byte aligned", who);
  if ((uintptr_t)desc & 15) TT_FAIL(TT_EINVAL, "%s: desc is not 16-byte aligned", who);
  if ((uintptr_t)tables & 15) TT_FAIL(TT_EINVAL, "%s: tables is not 16-byte aligned", who);
  if ((uintptr_t)coeffs & 15) TT_FAIL(TT_EINVAL, "%s: coeffs is not 16-byte aligned", who);
  if ((uintptr_t)status & 3) TT_FAIL(TT_EINVAL, "%s: status is not 4-byte aligned", who);
  if ((uintptr_t)ws & 15) TT_FAIL(TT_EINVAL, "%s: ws is not 16-byte aligned", who);
  const TtJpegProgressiveWs lay(n, nscans, max_bytes, h, w, ch, subsampling);
  if (!lay.total || ws_bytes < lay.total)
    TT_FAIL(TT_EINVAL, "%s: ws too small: %lld bytes, tt_jpeg_entropy_progressive_ws_bytes = %lld", who, (long long)ws_bytes, (long long)lay.total);
  const TtJpegGeometry geo = tt_jpeg_geometry(h, w, ch, subsampling);
  const long long blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  const int items = n * nscans, chunks = (int)lay.items.chunks;
  const long long plain_stride = lay.items.plain_stride;
  unsigned* plain_bytes = (unsigned*)((char*)ws + lay.items.plain_bytes);
  unsigned* chunk_drop = (unsigned*)((char*)ws + lay.items.chunk_drop);
  unsigned char* plain = (unsigned char*)ws + lay.items.plain;
  int* item_frame = (int*)((char*)ws + lay.item_frame);
  unsigned long long* masks = (unsigned long long*)((char*)ws + lay.masks);
  unsigned* starts = (unsigned*)((char*)ws + lay.starts);
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t) * (size_t)n, s);
  if (e == hipSuccess) e = hipMemsetAsync(coeffs, 0, (size_t)n * (size_t)blocks * 128, s);
  if (e != hipSuccess) TT_FAIL(TT_ELAUNCH, "%s: zeroing coeffs and status: %s", who, hipGetErrorString(e));
  hipLaunchKernelGGL(jpeg_progressive_items_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, item_frame, items, (int)nscans);
  const dim3 per_chunk((unsigned)chunks, (unsigned)items);
  hipLaunchKernelGGL(jpeg_unstuff_count_kernel, per_chunk, dim3(UBLOCK), 0, s, (const unsigned char*)scans, (long long)scans_bytes, (const long long*)offsets,
                     (const unsigned*)lengths, (long long)max_bytes, chunk_drop, chunks, (unsigned*)status, (const int*)item_frame, (int)n);
  hipLaunchKernelGGL(jpeg_unstuff_scan_kernel, dim3((unsigned)items), dim3(SCAN_BLOCK), 0, s, chunk_drop, chunks, (const long long*)offsets, (const unsigned*)lengths,
                     (long long)scans_bytes, (long long)max_bytes, plain_bytes);
  hipLaunchKernelGGL(jpeg_unstuff_gather_kernel, per_chunk, dim3(UBLOCK), 0, s, (const unsigned char*)scans, (long long)scans_bytes, (const long long*)offsets,
                     (const unsigned*)lengths, (long long)max_bytes, (const unsigned*)chunk_drop, chunks, plain, plain_stride);
  for (int round = 0; round < nscans; ++round)
    hipLaunchKernelGGL(jpeg_progressive_round_kernel, dim3((unsigned)n), dim3(ELANES), 0, s, (const unsigned char*)plain, plain_stride, (const unsigned*)plain_bytes,
                       (long long)max_bytes, (const unsigned*)desc, (const unsigned*)tables, (int)nscans, round, (int)h, (int)w, geo, (unsigned)blocks, (short*)coeffs,
                       (unsigned*)status, masks, starts);
  TT_CHECK_LAUNCH(who);
  return TT_OK;
}
