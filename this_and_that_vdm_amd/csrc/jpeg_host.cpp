// libttvdm: the host half of the JPEG export -- tt_jpeg_quant_tables (the Annex K tables scaled by a quality), tt_jpeg_standard_table
// (the four Annex K.3 Huffman tables), tt_jpeg_optimized_table (a table from symbol counts: the library's length-limited package-merge,
// a reserved symbol keeping the all-ones code free) and the sizes tt_jpeg_coeffs / tt_jpeg_scan work with.  include/ttvdm.h states them
// rule by rule; integers only, no device.
#include "jpeg_host.h"
#include "huffman_host.h"

#include <string.h>

namespace {

const uint8_t LUM_Q[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                           14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t CHR_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// T.81 Annex K.3: BITS and HUFFVAL.  The AC tables' tails are runs of (run, size) with size 1 .. 10 that the loops below write out.
const uint8_t DC_LUM_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t DC_CHR_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t AC_LUM_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t AC_CHR_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t AC_LUM_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const uint8_t AC_CHR_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// T.81 Annex C: BITS and HUFFVAL -> per symbol its code (from the most significant bit) | length << 16; 0 for a symbol without a code
void code_table(const uint8_t* bits, const uint8_t* huffval, uint32_t* codes) {
  memset(codes, 0, sizeof(uint32_t) * TT_JPEG_TABLE_WORDS);
  uint32_t code = 0;
  int k = 0;
  for (int length = 1; length <= 16; ++length) {
    for (int i = 0; i < bits[length - 1]; ++i) codes[huffval[k++]] = code++ | (uint32_t)length << 16;
    code <<= 1;
  }
}

}  // namespace

void tt_jpeg_fill_quant(int32_t quality, TtJpegQuant* out) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = ((t ? CHR_Q[i] : LUM_Q[i]) * s + 50) / 100;
      out->q[t][i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

extern "C" int64_t tt_jpeg_blocks(int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  if (!tt_jpeg_shape_ok(h, w, ch, subsampling)) return 0;
  const TtJpegGeometry g = tt_jpeg_geometry(h, w, ch, subsampling);
  return (int64_t)g.mcus_x * g.mcus_y * g.blocks_per_mcu;
}

extern "C" int64_t tt_jpeg_scan_bound(int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  const int64_t blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  return blocks ? (2 * blocks * TT_JPEG_BLOCK_BYTES + 2 + 15) / 16 * 16 : 0;       // every byte stuffed, the padded last byte too
}

extern "C" int64_t tt_jpeg_scan_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  return TtJpegScanWs(n, h, w, ch, subsampling).total;
}

extern "C" int64_t tt_jpeg_scan_bound_restart(int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval) {
  const int64_t plain = tt_jpeg_scan_bound(h, w, ch, subsampling);
  if (!plain || restart_interval < 0 || restart_interval > 65535) return 0;
  if (!restart_interval) return plain;
  // per marker: the pad byte, which may be 0xFF and then doubles, and the marker's two bytes, never stuffed -- 4 bytes.  6 are taken, so
  // that HALF the bound still holds the unstuffed stream (pad 1 + marker 2), which is what the workspace is cut by
  return tt_jpeg_up16(plain + 6 * (tt_jpeg_intervals(h, w, ch, subsampling, restart_interval) - 1));
}

extern "C" int64_t tt_jpeg_scan_restart_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval) {
  if (restart_interval < 0 || restart_interval > 65535) return 0;
  return TtJpegScanWs(n, h, w, ch, subsampling, restart_interval).total;
}

extern "C" int tt_jpeg_quant_tables(int32_t quality, uint8_t* tables) {
  if (!tables) TT_FAIL(TT_EINVAL, "tt_jpeg_quant_tables: null tables");
  if (quality < 1 || quality > 100) TT_FAIL(TT_EINVAL, "tt_jpeg_quant_tables: quality = %d (1 to 100)", quality);
  TtJpegQuant q;
  tt_jpeg_fill_quant(quality, &q);
  memcpy(tables, q.q, sizeof(q.q));
  return TT_OK;
}

extern "C" int tt_jpeg_standard_table(int32_t which, uint8_t* bits, uint8_t* huffval, int32_t* nvals, uint32_t* codes) {
  if (!bits || !huffval || !nvals || !codes)
    TT_FAIL(TT_EINVAL, "tt_jpeg_standard_table: null %s", !bits ? "bits" : (!huffval ? "huffval" : (!nvals ? "nvals" : "codes")));
  if (which < 0 || which > 3) TT_FAIL(TT_EINVAL, "tt_jpeg_standard_table: which = %d (0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance)", which);
  memset(huffval, 0, 256);
  if (which == 0 || which == 2) {
    memcpy(bits, which ? DC_CHR_BITS : DC_LUM_BITS, 16);
    for (int i = 0; i < 12; ++i) huffval[i] = (uint8_t)i;
    *nvals = 12;
  } else {
    memcpy(bits, which == 3 ? AC_CHR_BITS : AC_LUM_BITS, 16);
    memcpy(huffval, which == 3 ? AC_CHR_VALS : AC_LUM_VALS, 162);
    *nvals = 162;
  }
  code_table(bits, huffval, codes);
  return TT_OK;
}

extern "C" int tt_jpeg_optimized_table(const uint32_t* counts, uint8_t* bits, uint8_t* huffval, int32_t* nvals, uint32_t* codes) {
  if (!counts || !bits || !huffval || !nvals || !codes)
    TT_FAIL(TT_EINVAL, "tt_jpeg_optimized_table: null %s", !counts ? "counts" : (!bits ? "bits" : (!huffval ? "huffval" : (!nvals ? "nvals" : "codes"))));
  // entry 0 is the reserved symbol with the least count there is: first in the package-merge's leaf order, it gets a longest code, and
  // as the LAST code of that length in canonical order the code of one-bits only.  It is then dropped, as libjpeg drops its symbol 256.
  uint32_t shifted[257];
  uint8_t lengths[257];
  shifted[0] = 1;
  memcpy(shifted + 1, counts, 256 * sizeof(uint32_t));
  const int rc = tt_code_lengths("tt_jpeg_optimized_table", shifted, 257, TT_JPEG_CODE_LIMIT, lengths);
  if (rc != TT_OK) return rc;
  memset(bits, 0, 16);
  memset(huffval, 0, 256);
  int k = 0;
  for (int length = 1; length <= TT_JPEG_CODE_LIMIT; ++length)
    for (int s = 0; s < 256; ++s)
      if (lengths[s + 1] == length) { ++bits[length - 1]; huffval[k++] = (uint8_t)s; }
  *nvals = k;
  code_table(bits, huffval, codes);
  return TT_OK;
}

// ---------------------------------------------------------------- JPEG import, rules 1 and 2 (include/ttvdm.h)
namespace {

const uint8_t ZIGZAG[64] = TT_JPEG_ZIGZAG;

const char* frame_kind(int marker) {
  switch (marker) {
    case 0xc1: return "SOF1: extended sequential";
    case 0xc2: return "SOF2: progressive";
    case 0xc3: return "SOF3: lossless";
    case 0xc9: case 0xca: case 0xcb: case 0xcd: case 0xce: case 0xcf: return "arithmetic coding";
    default: return "a differential (hierarchical) frame";
  }
}

}  // namespace

// One parser behind both entry points.  ri == NULL: tt_jpeg_parse, which refuses restart intervals by name.  Else tt_jpeg_parse_spans:
// *ri gets the interval of the last DRI segment, and the scan is walked marker by marker into spans (rule 1a of the import).
static int parse_file(const uint8_t* data, int64_t size, TtJpegHeader* header, int32_t* ri, int64_t* span_offsets, int64_t* span_lengths,
                      int64_t span_cap, int64_t* nspans) {
  // rule 1's refusals carry tt_jpeg_parse's name from either entry point (callers match on them); rule 1a's carry tt_jpeg_parse_spans'
  const char* who = "tt_jpeg_parse";
  const char* who_spans = "tt_jpeg_parse_spans";
  if (!data || !header) TT_FAIL(TT_EINVAL, "%s: null %s", who, !data ? "data" : "header");
  if (size <= 0) TT_FAIL(TT_EINVAL, "%s: size = %lld", who, (long long)size);
  if (size < 2 || data[0] != 0xff || data[1] != 0xd8) TT_FAIL(TT_EINVAL, "%s: no SOI marker: not a JPEG file", who);
  TtJpegHeader hd;
  memset(&hd, 0, sizeof(hd));
  uint8_t quant[4][64];
  bool have_quant[4] = {false, false, false, false}, have_huff[4] = {false, false, false, false}, have_frame = false, have_dri = false;
  int interval = 0;
  int comp_id[3] = {0, 0, 0}, comp_quant[3] = {0, 0, 0};
  int64_t at = 2;
  for (;;) {
    if (at + 4 > size) TT_FAIL(TT_EINVAL, "%s: the file ends before its scan (a marker segment at byte %lld)", who, (long long)at);
    if (data[at] != 0xff) TT_FAIL(TT_EINVAL, "%s: byte %lld is 0x%02x where a marker begins", who, (long long)at, data[at]);
    const int marker = data[at + 1];
    if (marker == 0xff) { ++at; continue; }                          // fill bytes before a marker
    if (marker == 0xd9) TT_FAIL(TT_EINVAL, "%s: the file ends before its scan (EOI at byte %lld)", who, (long long)at);
    if (marker == 0x01 || (marker >= 0xd0 && marker <= 0xd8)) TT_FAIL(TT_EINVAL, "%s: marker 0x%02x at byte %lld, before the scan", who, marker, (long long)at);
    const int64_t len = ((int64_t)data[at + 2] << 8) | data[at + 3];
    if (len < 2 || at + 2 + len > size) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of segment 0x%02x at byte %lld", who, marker, (long long)at);
    const uint8_t* p = data + at + 4;
    const int64_t n = len - 2;
    if (marker == 0xc0) {
      if (have_frame) TT_FAIL(TT_EUNSUPPORTED, "%s: a second frame header", who);
      if (n < 6) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of its SOF0 segment", who);
      if (p[0] != 8) TT_FAIL(TT_EUNSUPPORTED, "%s: %d-bit samples (8-bit only; 12-bit files are not decoded)", who, p[0]);
      hd.h = (p[1] << 8) | p[2];
      hd.w = (p[3] << 8) | p[4];
      const int nc = p[5];
      if (nc == 4) TT_FAIL(TT_EUNSUPPORTED, "%s: four components (CMYK / YCCK files are not decoded)", who);
      if (nc != 1 && nc != 3) TT_FAIL(TT_EUNSUPPORTED, "%s: %d components (1: grey, or 3: YCbCr)", who, nc);
      if (n < 6 + 3 * nc) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of its SOF0 segment", who);
      if (hd.h <= 0 || hd.w <= 0) TT_FAIL(TT_EUNSUPPORTED, "%s: a frame of %d x %d (a height of 0 waits for a DNL marker)", who, hd.h, hd.w);
      hd.ch = nc;
      int samp[3] = {0x11, 0x11, 0x11};
      for (int c = 0; c < nc; ++c) {
        comp_id[c] = p[6 + 3 * c];
        samp[c] = p[7 + 3 * c];
        comp_quant[c] = p[8 + 3 * c];
        if (comp_quant[c] > 3) TT_FAIL(TT_EINVAL, "%s: component %d names quantiser table %d (0 to 3)", who, c, comp_quant[c]);
      }
      if (nc == 1) hd.subsampling = TT_JPEG_444;                     // one component: whatever its sampling factors say, 1 x 1
      else if (samp[0] == 0x11 && samp[1] == 0x11 && samp[2] == 0x11) hd.subsampling = TT_JPEG_444;
      else if (samp[0] == 0x22 && samp[1] == 0x11 && samp[2] == 0x11) hd.subsampling = TT_JPEG_420;
      else TT_FAIL(TT_EUNSUPPORTED, "%s: sampling %dx%d / %dx%d / %dx%d (4:4:4 or 4:2:0; 4:2:2 and others are not decoded)", who, samp[0] >> 4,
                   samp[0] & 15, samp[1] >> 4, samp[1] & 15, samp[2] >> 4, samp[2] & 15);
      have_frame = true;
    } else if ((marker >= 0xc1 && marker <= 0xcf) && marker != 0xc4 && marker != 0xc8 && marker != 0xcc) {
      TT_FAIL(TT_EUNSUPPORTED, "%s: %s (baseline SOF0 only)", who, frame_kind(marker));
    } else if (marker == 0xcc) {
      TT_FAIL(TT_EUNSUPPORTED, "%s: arithmetic coding (a DAC segment)", who);
    } else if (marker == 0xdb) {
      int64_t k = 0;
      while (k < n) {
        const int pq = p[k] >> 4, tq = p[k] & 15;
        if (pq != 0) TT_FAIL(TT_EUNSUPPORTED, "%s: a 16-bit DQT (8-bit quantiser tables only)", who);
        if (tq > 3) TT_FAIL(TT_EINVAL, "%s: DQT defines table %d (0 to 3)", who, tq);
        if (k + 65 > n) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of a DQT table", who);
        for (int z = 0; z < 64; ++z) quant[tq][ZIGZAG[z]] = p[k + 1 + z];
        have_quant[tq] = true;
        k += 65;
      }
    } else if (marker == 0xc4) {
      int64_t k = 0;
      while (k < n) {
        const int tc = p[k] >> 4, th = p[k] & 15;
        if (tc > 1) TT_FAIL(TT_EINVAL, "%s: DHT table class %d (0: DC, or 1: AC)", who, tc);
        if (th > 1) TT_FAIL(TT_EUNSUPPORTED, "%s: Huffman table index %d (baseline: 0 or 1)", who, th);
        if (k + 17 > n) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of a DHT table", who);
        int total = 0;
        for (int l = 0; l < 16; ++l) total += p[k + 1 + l];
        if (total > 256) TT_FAIL(TT_EINVAL, "%s: a DHT table of %d codes (256 at most)", who, total);
        if (k + 17 + total > n) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of a DHT table", who);
        const int slot = th * 2 + tc;                                // DC 0, AC 0, DC 1, AC 1
        memcpy(hd.bits[slot], p + k + 1, 16);
        memset(hd.huffval[slot], 0, 256);
        memcpy(hd.huffval[slot], p + k + 17, (size_t)total);
        have_huff[slot] = true;
        k += 17 + total;
      }
    } else if (marker == 0xdd) {
      if (n < 2) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of its DRI segment", who);
      const int v = (p[0] << 8) | p[1];
      if (!ri && v) TT_FAIL(TT_EUNSUPPORTED, "%s: a restart interval of %d MCUs (files with restart markers are not decoded)", who, v);
      if (have_dri && v != interval) TT_FAIL(TT_EINVAL, "%s: two DRI segments that disagree (restart intervals of %d and %d MCUs)", who_spans, interval, v);
      have_dri = true;
      interval = v;
    } else if (marker == 0xee) {
      if (n >= 5 && memcmp(p, "Adobe", 5) == 0) TT_FAIL(TT_EUNSUPPORTED, "%s: an Adobe APP14 segment (Adobe colour transforms are not decoded)", who);
    } else if (marker == 0xda) {
      if (!have_frame) TT_FAIL(TT_EINVAL, "%s: SOS before SOF0", who);
      if (n < 1 || n != 4 + 2 * p[0]) TT_FAIL(TT_EINVAL, "%s: an SOS segment of %lld bytes for %d components", who, (long long)n, n < 1 ? 0 : p[0]);
      if (p[0] != hd.ch) TT_FAIL(TT_EUNSUPPORTED, "%s: several scans: the first holds %d of %d components (one interleaved scan only)", who, p[0], hd.ch);
      for (int c = 0; c < hd.ch; ++c) {
        if (p[1 + 2 * c] != comp_id[c]) TT_FAIL(TT_EUNSUPPORTED, "%s: the scan's component %d is not the frame's (components in frame order only)", who, c);
        const int td = p[2 + 2 * c] >> 4, ta = p[2 + 2 * c] & 15;
        if (td > 1 || ta > 1) TT_FAIL(TT_EUNSUPPORTED, "%s: Huffman table index %d (baseline: 0 or 1)", who, td > 1 ? td : ta);
        if (!have_huff[td * 2]) TT_FAIL(TT_EUNSUPPORTED, "%s: missing DC Huffman table %d (component %d)", who, td, c);
        if (!have_huff[ta * 2 + 1]) TT_FAIL(TT_EUNSUPPORTED, "%s: missing AC Huffman table %d (component %d)", who, ta, c);
        if (!have_quant[comp_quant[c]]) TT_FAIL(TT_EUNSUPPORTED, "%s: missing quantiser table %d (component %d)", who, comp_quant[c], c);
        hd.dc_table[c] = td;
        hd.ac_table[c] = ta;
        memcpy(hd.quant[c], quant[comp_quant[c]], 64);
      }
      const uint8_t* t = p + 1 + 2 * hd.ch;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0)
        TT_FAIL(TT_EUNSUPPORTED, "%s: a scan of coefficients %d to %d, approximation 0x%02x (progressive; sequential 0 to 63 only)", who, t[0], t[1], t[2]);
      hd.scan_offset = at + 2 + len;
      break;
    }                                                               // APPn, COM and anything else with a length: skipped
    at += 2 + len;
  }
  // the entropy-coded segment ends at the first marker that is neither a stuffed FF 00 nor fill
  // ... and, for tt_jpeg_parse_spans, is cut into spans at the RSTn markers, which must come in the order 0 .. 7, 0 ..
  int64_t i = hd.scan_offset, first = hd.scan_offset, markers = 0;
  for (;; ++i) {
    if (i + 1 >= size) TT_FAIL(TT_EINVAL, "%s: the file ends before EOI (%lld bytes)", who, (long long)size);
    if (data[i] != 0xff || data[i + 1] == 0x00) continue;
    const int m = data[i + 1];
    if (m == 0xd9) break;
    if (m >= 0xd0 && m <= 0xd7 && ri) {
      if (interval == 0)
        TT_FAIL(TT_EINVAL, "%s: a restart marker (RST%d at byte %lld) in a file %s", who_spans, m - 0xd0, (long long)i, have_dri ? "whose DRI segment says 0" : "with no DRI segment");
      if (m - 0xd0 != (int)(markers & 7))
        TT_FAIL(TT_EINVAL, "%s: restart marker %lld at byte %lld is RST%d where RST%d is due", who_spans, (long long)markers, (long long)i, m - 0xd0, (int)(markers & 7));
      if (span_offsets && span_lengths && markers < span_cap) { span_offsets[markers] = first; span_lengths[markers] = i - first; }
      ++markers;
      first = i + 2;
      ++i;
      continue;
    }
    if (m >= 0xd0 && m <= 0xd7) TT_FAIL(TT_EUNSUPPORTED, "%s: a restart marker in the scan (files with restart markers are not decoded)", who);
    if (m == 0xda || m == 0xc4 || m == 0xdb) TT_FAIL(TT_EUNSUPPORTED, "%s: several scans (marker 0x%02x behind the first; one interleaved scan only)", who, m);
    TT_FAIL(TT_EINVAL, "%s: marker 0x%02x inside the scan at byte %lld", who, m, (long long)i);
  }
  hd.scan_bytes = i - hd.scan_offset;
  if (ri) {
    const TtJpegGeometry geo = tt_jpeg_geometry(hd.h, hd.w, hd.ch, hd.subsampling);
    const int64_t mcus = (int64_t)geo.mcus_x * geo.mcus_y, due = interval ? (mcus + interval - 1) / interval - 1 : 0;
    if (markers != due)
      TT_FAIL(TT_EINVAL, "%s: %lld restart markers where a restart interval of %d over %lld MCUs has %lld", who_spans, (long long)markers, interval, (long long)mcus,
              (long long)due);
    if (span_offsets && span_lengths) {
      if (span_cap < markers + 1) TT_FAIL(TT_EINVAL, "%s: span_cap too small: %lld for %lld spans", who_spans, (long long)span_cap, (long long)(markers + 1));
      span_offsets[markers] = first;
      span_lengths[markers] = i - first;
    }
    *ri = interval;
    *nspans = markers + 1;
  }
  *header = hd;
  return TT_OK;
}

extern "C" int tt_jpeg_parse(const uint8_t* data, int64_t size, TtJpegHeader* header) {
  return parse_file(data, size, header, nullptr, nullptr, nullptr, 0, nullptr);
}

extern "C" int tt_jpeg_parse_spans(const uint8_t* data, int64_t size, TtJpegHeader* header, int32_t* restart_interval, int64_t* span_offsets,
                                   int64_t* span_lengths, int64_t span_cap, int64_t* nspans) {
  if (!restart_interval || !nspans) TT_FAIL(TT_EINVAL, "tt_jpeg_parse_spans: null %s", !restart_interval ? "restart_interval" : "nspans");
  if ((span_offsets == nullptr) != (span_lengths == nullptr)) TT_FAIL(TT_EINVAL, "tt_jpeg_parse_spans: span_offsets and span_lengths go together (both, or neither to count)");
  if (span_offsets && span_cap < 1) TT_FAIL(TT_EINVAL, "tt_jpeg_parse_spans: span_cap = %lld (1 or more)", (long long)span_cap);
  return parse_file(data, size, header, restart_interval, span_offsets, span_lengths, span_cap, nspans);
}

// ---------------------------------------------------------------- JPEG import, rule 1b: progressive files
// One walk over the file's markers: the tables in force are snapshotted at every SOS, the progression is checked scan by scan as libjpeg
// does (coef_al: per component and coefficient the Al it has reached, -1 before its first visit).  Every trip of both loops advances `at`.
extern "C" int tt_jpeg_parse_progressive(const uint8_t* data, int64_t size, TtJpegProgressiveHeader* header, TtJpegScan* scans, int64_t scan_cap,
                                         int64_t* nscans) {
  const char* who = "tt_jpeg_parse_progressive";
  if (!data || !header || !nscans) TT_FAIL(TT_EINVAL, "%s: null %s", who, !data ? "data" : (!header ? "header" : "nscans"));
  if (size <= 0) TT_FAIL(TT_EINVAL, "%s: size = %lld", who, (long long)size);
  if (scans && scan_cap < 1) TT_FAIL(TT_EINVAL, "%s: scan_cap = %lld (1 or more)", who, (long long)scan_cap);
  if (size < 2 || data[0] != 0xff || data[1] != 0xd8) TT_FAIL(TT_EINVAL, "%s: no SOI marker: not a JPEG file", who);
  TtJpegProgressiveHeader hd;
  memset(&hd, 0, sizeof(hd));
  uint8_t quant[4][64], bits[2][4][16], huffval[2][4][256];
  bool have_quant[4] = {false, false, false, false}, have_huff[2][4] = {{false, false, false, false}, {false, false, false, false}}, have_frame = false;
  int comp_id[3] = {0, 0, 0}, comp_quant[3] = {0, 0, 0};
  int8_t coef_al[3][64];
  memset(coef_al, -1, sizeof(coef_al));
  int64_t count = 0, at = 2;
  for (;;) {
    if (at + 2 > size) TT_FAIL(TT_EINVAL, "%s: the file ends before EOI (%lld bytes)", who, (long long)size);
    if (data[at] != 0xff) TT_FAIL(TT_EINVAL, "%s: byte %lld is 0x%02x where a marker begins", who, (long long)at, data[at]);
    const int marker = data[at + 1];
    if (marker == 0xff) { ++at; continue; }                          // fill bytes before a marker
    if (marker == 0xd9) break;
    if (marker == 0x01 || (marker >= 0xd0 && marker <= 0xd8)) TT_FAIL(TT_EINVAL, "%s: marker 0x%02x at byte %lld, outside a scan", who, marker, (long long)at);
    if (at + 4 > size) TT_FAIL(TT_EINVAL, "%s: the file ends before EOI (a marker segment at byte %lld)", who, (long long)at);
    const int64_t len = ((int64_t)data[at + 2] << 8) | data[at + 3];
    if (len < 2 || at + 2 + len > size) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of segment 0x%02x at byte %lld", who, marker, (long long)at);
    const uint8_t* p = data + at + 4;
    const int64_t n = len - 2;
    if (marker == 0xc0) {
      TT_FAIL(TT_EUNSUPPORTED, "%s: a baseline (SOF0) file: tt_jpeg_parse_spans and tt_jpeg_entropy_spans decode it", who);
    } else if (marker == 0xc2) {
      if (have_frame) TT_FAIL(TT_EUNSUPPORTED, "%s: a second frame header", who);
      if (n < 6) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of its SOF2 segment", who);
      if (p[0] != 8) TT_FAIL(TT_EUNSUPPORTED, "%s: %d-bit samples (8-bit only; 12-bit files are not decoded)", who, p[0]);
      hd.h = (p[1] << 8) | p[2];
      hd.w = (p[3] << 8) | p[4];
      const int nc = p[5];
      if (nc == 4) TT_FAIL(TT_EUNSUPPORTED, "%s: four components (CMYK / YCCK files are not decoded)", who);
      if (nc != 1 && nc != 3) TT_FAIL(TT_EUNSUPPORTED, "%s: %d components (1: grey, or 3: YCbCr)", who, nc);
      if (n < 6 + 3 * nc) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of its SOF2 segment", who);
      if (hd.h <= 0 || hd.w <= 0) TT_FAIL(TT_EUNSUPPORTED, "%s: a frame of %d x %d (a height of 0 waits for a DNL marker)", who, hd.h, hd.w);
      hd.ch = nc;
      int samp[3] = {0x11, 0x11, 0x11};
      for (int c = 0; c < nc; ++c) {
        comp_id[c] = p[6 + 3 * c];
        samp[c] = p[7 + 3 * c];
        comp_quant[c] = p[8 + 3 * c];
        if (comp_quant[c] > 3) TT_FAIL(TT_EINVAL, "%s: component %d names quantiser table %d (0 to 3)", who, c, comp_quant[c]);
      }
      if (nc == 3 && (comp_id[0] == comp_id[1] || comp_id[0] == comp_id[2] || comp_id[1] == comp_id[2]))
        TT_FAIL(TT_EINVAL, "%s: two components with the identifier %d", who, comp_id[comp_id[0] == comp_id[2] ? 0 : 1]);
      if (nc == 1) hd.subsampling = TT_JPEG_444;                     // one component: whatever its sampling factors say, 1 x 1
      else if (samp[0] == 0x11 && samp[1] == 0x11 && samp[2] == 0x11) hd.subsampling = TT_JPEG_444;
      else if (samp[0] == 0x22 && samp[1] == 0x11 && samp[2] == 0x11) hd.subsampling = TT_JPEG_420;
      else TT_FAIL(TT_EUNSUPPORTED, "%s: sampling %dx%d / %dx%d / %dx%d (4:4:4 or 4:2:0; 4:2:2 and others are not decoded)", who, samp[0] >> 4,
                   samp[0] & 15, samp[1] >> 4, samp[1] & 15, samp[2] >> 4, samp[2] & 15);
      have_frame = true;
    } else if ((marker >= 0xc1 && marker <= 0xcf) && marker != 0xc4 && marker != 0xc8 && marker != 0xcc) {
      TT_FAIL(TT_EUNSUPPORTED, "%s: %s (Huffman-coded progressive SOF2 only)", who, frame_kind(marker));
    } else if (marker == 0xcc) {
      TT_FAIL(TT_EUNSUPPORTED, "%s: arithmetic coding (a DAC segment)", who);
    } else if (marker == 0xdb) {
      if (count) TT_FAIL(TT_EUNSUPPORTED, "%s: a DQT behind the first SOS (byte %lld): quantiser tables that change between scans are not decoded", who, (long long)at);
      int64_t k = 0;
      while (k < n) {
        const int pq = p[k] >> 4, tq = p[k] & 15;
        if (pq != 0) TT_FAIL(TT_EUNSUPPORTED, "%s: a 16-bit DQT (8-bit quantiser tables only)", who);
        if (tq > 3) TT_FAIL(TT_EINVAL, "%s: DQT defines table %d (0 to 3)", who, tq);
        if (k + 65 > n) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of a DQT table", who);
        for (int z = 0; z < 64; ++z) quant[tq][ZIGZAG[z]] = p[k + 1 + z];
        have_quant[tq] = true;
        k += 65;
      }
    } else if (marker == 0xc4) {
      int64_t k = 0;
      while (k < n) {
        const int tc = p[k] >> 4, th = p[k] & 15;
        if (tc > 1) TT_FAIL(TT_EINVAL, "%s: DHT table class %d (0: DC, or 1: AC)", who, tc);
        if (th > 3) TT_FAIL(TT_EINVAL, "%s: Huffman table index %d (0 to 3)", who, th);
        if (k + 17 > n) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of a DHT table", who);
        int total = 0;
        for (int l = 0; l < 16; ++l) total += p[k + 1 + l];
        if (total > 256) TT_FAIL(TT_EINVAL, "%s: a DHT table of %d codes (256 at most)", who, total);
        if (k + 17 + total > n) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of a DHT table", who);
        memcpy(bits[tc][th], p + k + 1, 16);
        memset(huffval[tc][th], 0, 256);
        memcpy(huffval[tc][th], p + k + 17, (size_t)total);
        have_huff[tc][th] = true;
        k += 17 + total;
      }
    } else if (marker == 0xdd) {
      if (n < 2) TT_FAIL(TT_EINVAL, "%s: the file ends before the end of its DRI segment", who);
      const int v = (p[0] << 8) | p[1];
      if (v) TT_FAIL(TT_EUNSUPPORTED, "%s: restart intervals in a progressive file (DRI of %d MCUs) are not decoded", who, v);
    } else if (marker == 0xee) {
      if (n >= 5 && memcmp(p, "Adobe", 5) == 0) TT_FAIL(TT_EUNSUPPORTED, "%s: an Adobe APP14 segment (Adobe colour transforms are not decoded)", who);
    } else if (marker == 0xda) {
      if (!have_frame) TT_FAIL(TT_EINVAL, "%s: SOS before SOF2", who);
      if (n < 1 || p[0] < 1 || p[0] > 4 || n != 4 + 2 * p[0]) TT_FAIL(TT_EINVAL, "%s: an SOS segment of %lld bytes for %d components", who, (long long)n, n < 1 ? 0 : p[0]);
      if (count >= TT_JPEG_MAX_SCANS) TT_FAIL(TT_EUNSUPPORTED, "%s: more than %d scans", who, TT_JPEG_MAX_SCANS);
      const int ns = p[0];
      const uint8_t* t = p + 1 + 2 * ns;
      const int ss = t[0], se = t[1], ah = t[2] >> 4, al = t[2] & 15;
      TtJpegScan sc;
      memset(&sc, 0, sizeof(sc));
      int which[4] = {0, 0, 0, 0};
      for (int i = 0; i < ns; ++i) {
        int c = 0;
        while (c < hd.ch && comp_id[c] != p[1 + 2 * i]) ++c;
        if (c == hd.ch) TT_FAIL(TT_EINVAL, "%s: scan %lld names component %d, which the frame does not have", who, (long long)count, p[1 + 2 * i]);
        if (sc.comps & (1 << c)) TT_FAIL(TT_EINVAL, "%s: scan %lld names component %d twice", who, (long long)count, p[1 + 2 * i]);
        sc.comps |= 1 << c;
        which[i] = c;
      }
      if (al > 13) TT_FAIL(TT_EINVAL, "%s: scan %lld: Al = %d (13 at most)", who, (long long)count, al);
      if (ss == 0) {
        if (se != 0) TT_FAIL(TT_EINVAL, "%s: scan %lld: a DC scan with Se = %d (Ss = 0 goes with Se = 0)", who, (long long)count, se);
        bool ordered = ns == 1 || ns == hd.ch;
        for (int i = 0; i < ns && ns > 1; ++i) ordered = ordered && which[i] == i;
        if (!ordered) TT_FAIL(TT_EINVAL, "%s: scan %lld: a component subset (a DC scan holds every component in frame order, or one)", who, (long long)count);
      } else {
        if (ns != 1) TT_FAIL(TT_EINVAL, "%s: scan %lld: an AC scan of %d components (one only)", who, (long long)count, ns);
        if (se < ss || se > 63) TT_FAIL(TT_EINVAL, "%s: scan %lld: band %d to %d (Ss <= Se <= 63)", who, (long long)count, ss, se);
        if (coef_al[which[0]][0] < 0) TT_FAIL(TT_EINVAL, "%s: scan %lld: an AC scan of component %d before its DC scan", who, (long long)count, which[0]);
      }
      for (int i = 0; i < ns; ++i) {
        const int c = which[i];
        for (int k = ss; k <= se; ++k) {
          const int before = coef_al[c][k];
          if (before < 0 ? ah != 0 : (ah != before || al != ah - 1))
            TT_FAIL(TT_EINVAL, "%s: scan %lld: successive approximation Ah = %d, Al = %d where coefficient %d of component %d %s %d", who, (long long)count, ah,
                    al, k, c, before < 0 ? "is new: Ah" : "stands at Al", before < 0 ? 0 : before);
          coef_al[c][k] = (int8_t)al;
        }
        const int td = p[2 + 2 * i] >> 4, ta = p[2 + 2 * i] & 15;
        if (ss == 0 && ah == 0) {
          if (td > 3) TT_FAIL(TT_EINVAL, "%s: Huffman table index %d (0 to 3)", who, td);
          if (!have_huff[0][td]) TT_FAIL(TT_EUNSUPPORTED, "%s: missing DC Huffman table %d (scan %lld, component %d)", who, td, (long long)count, c);
          memcpy(sc.bits[c], bits[0][td], 16);
          memcpy(sc.huffval[c], huffval[0][td], 256);
        } else if (ss > 0) {
          if (ta > 3) TT_FAIL(TT_EINVAL, "%s: Huffman table index %d (0 to 3)", who, ta);
          if (!have_huff[1][ta]) TT_FAIL(TT_EUNSUPPORTED, "%s: missing AC Huffman table %d (scan %lld, component %d)", who, ta, (long long)count, c);
          memcpy(sc.bits[0], bits[1][ta], 16);
          memcpy(sc.huffval[0], huffval[1][ta], 256);
        }
      }
      if (count == 0)
        for (int c = 0; c < hd.ch; ++c) {
          if (!have_quant[comp_quant[c]]) TT_FAIL(TT_EUNSUPPORTED, "%s: missing quantiser table %d (component %d)", who, comp_quant[c], c);
          memcpy(hd.quant[c], quant[comp_quant[c]], 64);
        }
      sc.ss = ss; sc.se = se; sc.ah = ah; sc.al = al;
      sc.offset = at + 2 + len;
      // the entropy-coded segment ends at the first marker that is neither a stuffed FF 00 nor fill
      int64_t i = sc.offset;
      for (;; ++i) {
        if (i + 1 >= size) TT_FAIL(TT_EINVAL, "%s: the file ends before EOI (inside scan %lld, %lld bytes)", who, (long long)count, (long long)size);
        if (data[i] == 0xff && data[i + 1] != 0x00) break;           // fill bytes (FF FF) are the next marker's
      }
      if (data[i + 1] >= 0xd0 && data[i + 1] <= 0xd7)
        TT_FAIL(TT_EINVAL, "%s: a restart marker (RST%d at byte %lld) in a file with no restart interval", who, data[i + 1] - 0xd0, (long long)i);
      sc.bytes = i - sc.offset;
      if (scans && count < scan_cap) scans[count] = sc;
      ++count;
      at = i;
      continue;
    }                                                               // APPn, COM and anything else with a length: skipped
    at += 2 + len;
  }
  if (!have_frame) TT_FAIL(TT_EINVAL, "%s: EOI before SOF2", who);
  if (!count) TT_FAIL(TT_EINVAL, "%s: the file ends before its first scan (EOI at byte %lld)", who, (long long)at);
  for (int c = 0; c < hd.ch; ++c)
    for (int k = 0; k < 64; ++k)
      if (coef_al[c][k] != 0)
        TT_FAIL(TT_EUNSUPPORTED, "%s: incomplete progression: coefficient %d of component %d %s at EOI (libjpeg smooths such files; they are not decoded)", who, k, c,
                coef_al[c][k] < 0 ? "was never sent" : "has not reached Al = 0");
  if (scans && scan_cap < count) TT_FAIL(TT_EINVAL, "%s: scan_cap too small: %lld for %lld scans", who, (long long)scan_cap, (long long)count);
  hd.nscans = (int32_t)count;
  *header = hd;
  *nscans = count;
  return TT_OK;
}

extern "C" int64_t tt_jpeg_entropy_progressive_ws_bytes(int32_t n, int32_t nscans, int64_t max_bytes, int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  return TtJpegProgressiveWs(n, nscans, max_bytes, h, w, ch, subsampling).total;
}

extern "C" int tt_jpeg_decode_table(const uint8_t* bits, const uint8_t* huffval, uint32_t* table) {
  if (!bits || !huffval || !table) TT_FAIL(TT_EINVAL, "tt_jpeg_decode_table: null %s", !bits ? "bits" : (!huffval ? "huffval" : "table"));
  int total = 0;
  uint32_t space = 0;                                                // of 65536: the code space the lengths take
  for (int l = 1; l <= 16; ++l) {
    total += bits[l - 1];
    space += (uint32_t)bits[l - 1] << (16 - l);
  }
  if (total > 256) TT_FAIL(TT_EINVAL, "tt_jpeg_decode_table: BITS counts %d codes (256 at most)", total);
  if (space > 65536u) TT_FAIL(TT_EINVAL, "tt_jpeg_decode_table: BITS oversubscribes the code space (%u / 65536)", space);
  memset(table, 0, sizeof(uint32_t) * TT_JPEG_DECODE_WORDS);
  uint16_t look[256];
  memset(look, 0, sizeof(look));
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    table[145 + l] = (uint32_t)(k - (int32_t)code);
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code)
      if (l <= 8)
        for (uint32_t fill = 0; fill < (1u << (8 - l)); ++fill) look[((code << (8 - l)) | fill) & 255u] = (uint16_t)(l << 8 | huffval[k]);
    table[128 + l] = bits[l - 1] ? code - 1 : 0xffffffffu;
    code <<= 1;
  }
  for (int i = 0; i < 128; ++i) table[i] = look[2 * i] | (uint32_t)look[2 * i + 1] << 16;
  for (int i = 0; i < 64; ++i)
    table[192 + i] = huffval[4 * i] | (uint32_t)huffval[4 * i + 1] << 8 | (uint32_t)huffval[4 * i + 2] << 16 | (uint32_t)huffval[4 * i + 3] << 24;
  return TT_OK;
}

extern "C" int64_t tt_jpeg_sequence_bits(void) { return (int64_t)TT_JPEG_SUBSEQ_BITS * TT_JPEG_DECODE_LANES; }

extern "C" int64_t tt_jpeg_entropy_ws_bytes(int32_t n, int64_t max_bytes) {
  return TtJpegEntropyWs(n, max_bytes).total;
}
