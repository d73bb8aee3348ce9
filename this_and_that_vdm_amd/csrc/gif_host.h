// The host half of the GIF export and import (gif_host.cpp): plain C++17, no HIP include -- it also compiles on its own with any host
// compiler (together with lib.cpp, which holds tt_set_error), which is how tests/test_gif_export_cpu.py and tests/test_gif_decode_cpu.py
// build it under the sanitizers.
#pragma once
#include "ttvdm.h"
#include "host_common.h"

// GIF's LZW: codes are at most 12 bits wide, so the table ends at entry 4095
constexpr int TT_LZW_MAX_BITS = 12;
constexpr int TT_LZW_MAX_CODES = 1 << TT_LZW_MAX_BITS;
