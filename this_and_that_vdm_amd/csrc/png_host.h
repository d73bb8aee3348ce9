// The host half of the PNG export (png_host.cpp): plain C++17, no HIP include -- it also compiles on its own with any host compiler
// (together with lib.cpp, which holds tt_set_error), which is how tests/test_png_export_cpu.py builds it under the sanitizers.
#pragma once
#include "ttvdm.h"
#include "host_common.h"

constexpr int TT_PNG_LIT_LIMIT = 15;               // DEFLATE's longest literal/length code ...
constexpr int TT_PNG_CL_LIMIT = 7;                 // ... and its longest code-length code
constexpr int TT_PNG_CL_SYMS = 19;
// what tt_png_filter accepts as a problem: the one statement of it, shared by the three kernels' entry points (png.hip)
inline bool tt_png_shape_ok(int32_t n, int32_t h, int32_t w, int32_t ch) { return n > 0 && h > 0 && w > 0 && ch >= 1 && ch <= 4; }
// extra bits of length symbol s (257 .. 285)
inline int tt_png_length_extra(int s) { return s < 265 || s == 285 ? 0 : (s - 261) / 4; }
