// instantiation unit: the wide (windowed) variants of tt_gemm's tiled template, TT_F32 (TT_GEMM_WIDE_TILES_F32 in gemm_tiles.h)
#include "gemm_launch.h"
namespace ttg {
void launch_wide_f32(GemmP& p, int cfg, hipStream_t st) {
  using Tag = f32_tag;
  switch (cfg) { TT_GEMM_WIDE_TILES_F32(TT_WIDE_CASE) }
}
}
