// The host half of the JPEG export and import (jpeg_host.cpp) and the one statement of the JPEG problem its device halves (jpeg.hip,
// jpeg_decode.hip) share with it: plain C++17, no HIP include -- it also compiles on its own with any host compiler (together with
// lib.cpp, which holds tt_set_error), which is how tests/test_jpeg_export_cpu.py builds it under the sanitizers.
#pragma once
#include "ttvdm.h"
#include "host_common.h"

constexpr int TT_JPEG_CODE_LIMIT = 15;             // the optimized tables' longest code (T.81 allows 16; the package-merge is limited to 15)
constexpr int TT_JPEG_BLOCK_BYTES = TT_JPEG_BLOCK_BITS / 8;
// the natural (row-major) index of the k-th coefficient of the zig-zag scan: the initialiser of every unit's table
#define TT_JPEG_ZIGZAG {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
// what tt_jpeg_coeffs accepts as a problem: the one statement of it, shared by the entry points (jpeg.hip) and the size queries
inline bool tt_jpeg_shape_ok(int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  return h > 0 && w > 0 && (ch == 1 || ch == 3) && (subsampling == TT_JPEG_444 || subsampling == TT_JPEG_420);
}
// ... and why a device entry point `who` refuses one; `channel_note` ends the sentence about the channels
inline int tt_jpeg_refuse_shape(const char* who, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, const char* channel_note) {
  if (n <= 0 || h <= 0 || w <= 0) TT_FAIL(TT_EINVAL, "%s: empty problem (n = %d, h = %d, w = %d)", who, n, h, w);
  if (ch != 1 && ch != 3) TT_FAIL(TT_EINVAL, "%s: %d channels (1: grey, or 3: RGB%s)", who, ch, channel_note);
  if (subsampling != TT_JPEG_444 && subsampling != TT_JPEG_420)
    TT_FAIL(TT_EINVAL, "%s: subsampling = %d (0: 4:4:4, or 2: 4:2:0)", who, subsampling);
  if ((long long)h * w * ch >= (1ll << 31)) TT_FAIL(TT_EUNSUPPORTED, "%s: a frame of %lld bytes (below 2^31)", who, (long long)h * w * ch);
  if (tt_jpeg_scan_bound(h, w, ch, subsampling) >= (1ll << 31))
    TT_FAIL(TT_EUNSUPPORTED, "%s: a scan bound of %lld bytes per frame (below 2^31)", who, (long long)tt_jpeg_scan_bound(h, w, ch, subsampling));
  if (n > 65535) TT_FAIL(TT_EUNSUPPORTED, "%s: %d frames: more than one grid covers (65535)", who, n);
  return TT_OK;
}
// the scan's geometry: MCUs per row and per column, blocks per MCU (grey is one block an MCU whatever the subsampling)
struct TtJpegGeometry { int32_t mcus_x, mcus_y, blocks_per_mcu, ncomp; };
inline TtJpegGeometry tt_jpeg_geometry(int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  const bool sub = ch == 3 && subsampling == TT_JPEG_420;
  const int32_t side = sub ? 16 : 8;
  return {(w + side - 1) / side, (h + side - 1) / side, ch == 1 ? 1 : (sub ? 6 : 3), ch == 1 ? 1 : 3};
}
// restart intervals (export rule 6a): how many a frame's scan has with an interval of `ri` MCUs -- 1 without (ri = 0) --, one marker fewer
inline int64_t tt_jpeg_intervals(int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t ri) {
  const TtJpegGeometry g = tt_jpeg_geometry(h, w, ch, subsampling);
  const int64_t mcus = (int64_t)g.mcus_x * g.mcus_y;
  return ri > 0 ? (mcus + ri - 1) / ri : 1;
}
// the quantiser tables as the kernels take them: a kernel argument, read through scalar loads
struct TtJpegQuant { uint8_t q[2][64]; };
void tt_jpeg_fill_quant(int32_t quality, TtJpegQuant* out);
// JPEG import: the lanes of the entropy decoder's one workgroup per frame, and a frame's stride in the workspace's plain (unstuffed)
// streams: the stream, then 16 bytes the decoder's whole-dword window may read past its end
constexpr int TT_JPEG_DECODE_LANES = 256;
inline int64_t tt_jpeg_plain_stride(int64_t max_bytes) { return (max_bytes + 15) / 16 * 16 + 16; }

// The workspaces' layouts: byte offsets of the sub-buffers, each a multiple of 16, and the total the size query returns (0: a problem
// the entry point refuses).  The size queries and the entry points both read these, and nothing else carves a workspace.
inline int64_t tt_jpeg_up16(int64_t v) { return (v + 15) / 16 * 16; }
// tt_jpeg_scan: a frame's unstuffed scan is at most half its tt_jpeg_scan_bound (a multiple of 8 bytes), stuffed in chunks of TT_JPEG_CHUNK.
// With a restart interval (ri > 0; tt_jpeg_scan_restart) the bound is tt_jpeg_scan_bound_restart, and two sub-buffers follow the streams:
// per interval the bits its pad and marker and those of the intervals before it add, and per frame a bitmap of its unstuffed bytes whose
// set bits are the markers' 0xFF bytes.  ri = 0 is tt_jpeg_scan's layout, byte for byte.
struct TtJpegScanWs {
  int64_t plain_stride, chunks;                    // per frame: bytes of its region of `plain`, stuffing chunks
  int64_t bits, plain_bytes, chunk_ff, plain;      // uint32 per block; uint32 per frame; uint32 per chunk; the unstuffed streams
  int64_t intervals, mark_words, extra, marks;     // ri > 0: per frame its intervals and bitmap words; uint32 per interval; the bitmaps
  int64_t total;
  TtJpegScanWs(int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t ri = 0)
      : plain_stride(0), chunks(0), bits(0), plain_bytes(0), chunk_ff(0), plain(0), intervals(0), mark_words(0), extra(0), marks(0), total(0) {
    const int64_t blocks = tt_jpeg_blocks(h, w, ch, subsampling);
    if (!blocks || n <= 0) return;
    const int64_t bytes = (ri > 0 ? tt_jpeg_scan_bound_restart(h, w, ch, subsampling, ri) : tt_jpeg_scan_bound(h, w, ch, subsampling)) / 2;
    plain_stride = tt_jpeg_up16(bytes);
    chunks = (bytes + TT_JPEG_CHUNK - 1) / TT_JPEG_CHUNK;
    plain_bytes = bits + tt_jpeg_up16(4 * n * blocks);
    chunk_ff = plain_bytes + tt_jpeg_up16(4 * (int64_t)n);
    plain = chunk_ff + tt_jpeg_up16(4 * n * chunks);
    total = plain + n * plain_stride;
    if (ri > 0) {
      intervals = tt_jpeg_intervals(h, w, ch, subsampling, ri);
      mark_words = (plain_stride + 31) / 32;
      extra = total;
      marks = extra + tt_jpeg_up16(4 * n * intervals);
      total = marks + tt_jpeg_up16(4 * n * mark_words);
    }
  }
};
// tt_jpeg_entropy: scans of at most max_bytes each, unstuffed in chunks of TT_JPEG_CHUNK
struct TtJpegEntropyWs {
  int64_t plain_stride, chunks;                    // per frame: tt_jpeg_plain_stride, unstuffing chunks
  int64_t plain_bytes, chunk_drop, plain;          // uint32 per frame; uint32 per chunk; the unstuffed streams
  int64_t total;
  TtJpegEntropyWs(int32_t n, int64_t max_bytes) : plain_stride(0), chunks(0), plain_bytes(0), chunk_drop(0), plain(0), total(0) {
    if (n <= 0 || max_bytes <= 0 || max_bytes >= (1ll << 28)) return;
    plain_stride = tt_jpeg_plain_stride(max_bytes);
    chunks = (max_bytes + TT_JPEG_CHUNK - 1) / TT_JPEG_CHUNK;
    chunk_drop = plain_bytes + tt_jpeg_up16(4 * (int64_t)n);
    plain = chunk_drop + tt_jpeg_up16(4 * n * chunks);
    total = plain + n * plain_stride;
  }
};
// tt_jpeg_entropy_progressive: tt_jpeg_entropy's layout over the n x nscans items, then per item its frame, then the AC-refine scans'
// per-block masks and positions, one set a frame (a frame runs one scan at a time)
constexpr int TT_JPEG_MAX_ITEMS = 65535;           // (frame, scan) pairs of a call: a grid dimension
struct TtJpegProgressiveWs {
  TtJpegEntropyWs items;
  int64_t item_frame, masks, starts;               // int32 per item; uint64 per frame and block; uint32 per frame and block
  int64_t total;
  TtJpegProgressiveWs(int32_t n, int32_t nscans, int64_t max_bytes, int32_t h, int32_t w, int32_t ch, int32_t subsampling)
      : items(n > 0 && nscans > 0 && nscans <= TT_JPEG_MAX_SCANS && (int64_t)n * nscans <= TT_JPEG_MAX_ITEMS ? n * nscans : 0, max_bytes), item_frame(0), masks(0),
        starts(0), total(0) {
    const int64_t blocks = tt_jpeg_blocks(h, w, ch, subsampling);
    if (!items.total || !blocks) return;
    item_frame = items.total;
    masks = item_frame + tt_jpeg_up16(4 * (int64_t)n * nscans);
    starts = masks + tt_jpeg_up16(8 * n * blocks);
    total = starts + tt_jpeg_up16(4 * n * blocks);
  }
};
