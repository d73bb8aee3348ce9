// libttvdm: the host half of the JPEG export -- tt_jpeg_quant_tables (the Annex K tables scaled by a quality), tt_jpeg_standard_table
// (the four Annex K.3 Huffman tables), tt_jpeg_optimized_table (a table from symbol counts: the library's length-limited package-merge,
// a reserved symbol keeping the all-ones code free) and the sizes tt_jpeg_coeffs / tt_jpeg_scan work with.  include/ttvdm.h states them
// rule by rule; integers only, no device.
#include "jpeg_host.h"

#include <string.h>

#define TT_FAIL(code, ...) do { tt_set_error(__VA_ARGS__); return (code); } while (0)

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
  const int64_t blocks = tt_jpeg_blocks(h, w, ch, subsampling);
  if (!blocks || n <= 0) return 0;
  const int64_t plain = tt_jpeg_scan_bound(h, w, ch, subsampling) / 2;              // the unstuffed bits of a frame, a multiple of 8 bytes
  const int64_t chunks = (plain + TT_JPEG_CHUNK - 1) / TT_JPEG_CHUNK;
  const auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
  return up(4 * n * blocks) + up(4 * (int64_t)n) + up(4 * n * chunks) + n * up(plain);
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
  const int rc = tt_png_code_lengths(shifted, 257, TT_JPEG_CODE_LIMIT, lengths);
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
