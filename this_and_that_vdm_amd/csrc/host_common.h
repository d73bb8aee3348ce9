// What every unit of libttvdm shares on the host side, device halves and plain C++ host halves alike: the last error's text and the
// "say why, return the code" macro.  No HIP include.
#pragma once

void tt_set_error(const char* fmt, ...);           // lib.cpp
#define TT_FAIL(code, ...) do { tt_set_error(__VA_ARGS__); return (code); } while (0)
