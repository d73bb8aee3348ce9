// The host half of the JPEG export (jpeg_host.cpp): plain C++17, no HIP include -- it also compiles on its own with any host compiler
// (together with png_host.cpp, whose package-merge it calls, and lib.cpp, which holds tt_set_error), which is how
// tests/test_jpeg_export_cpu.py builds it under the sanitizers.
#pragma once
#include "ttvdm.h"

void tt_set_error(const char* fmt, ...);           // lib.cpp

constexpr int TT_JPEG_CODE_LIMIT = 15;             // the optimized tables' longest code (T.81 allows 16; the package-merge is limited to 15)
constexpr int TT_JPEG_BLOCK_BYTES = TT_JPEG_BLOCK_BITS / 8;
// what tt_jpeg_coeffs accepts as a problem: the one statement of it, shared by the entry points (jpeg.hip) and the size queries
inline bool tt_jpeg_shape_ok(int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  return h > 0 && w > 0 && (ch == 1 || ch == 3) && (subsampling == TT_JPEG_444 || subsampling == TT_JPEG_420);
}
// the scan's geometry: MCUs per row and per column, blocks per MCU (grey is one block an MCU whatever the subsampling)
struct TtJpegGeometry { int32_t mcus_x, mcus_y, blocks_per_mcu, ncomp; };
inline TtJpegGeometry tt_jpeg_geometry(int32_t h, int32_t w, int32_t ch, int32_t subsampling) {
  const bool sub = ch == 3 && subsampling == TT_JPEG_420;
  const int32_t side = sub ? 16 : 8;
  return {(w + side - 1) / side, (h + side - 1) / side, ch == 1 ? 1 : (sub ? 6 : 3), ch == 1 ? 1 : 3};
}
// the quantiser tables as the kernels take them: a kernel argument, read through scalar loads
struct TtJpegQuant { uint8_t q[2][64]; };
void tt_jpeg_fill_quant(int32_t quality, TtJpegQuant* out);
// JPEG import: the lanes of the entropy decoder's one workgroup per frame, and a frame's stride in the workspace's plain (unstuffed)
// streams: the stream, then 16 bytes the decoder's whole-dword window may read past its end
constexpr int TT_JPEG_DECODE_LANES = 256;
inline int64_t tt_jpeg_plain_stride(int64_t max_bytes) { return (max_bytes + 15) / 16 * 16 + 16; }
