// instantiation unit: the wide (windowed) variants of tt_gemm's tiled template for one storage type (TT_GEMM_WIDE_TILES in gemm_tiles.h)
#include "gemm_launch.h"
namespace ttg {
void launch_wide_bf16(GemmP& p, int cfg, hipStream_t st) {
  using Tag = bf16_tag;
  switch (cfg) { TT_GEMM_WIDE_TILES(TT_WIDE_CASE) }
}
}
