// instantiation unit: the TT_F32 tile configurations (TT_GEMM_TILES_F32 in gemm_tiles.h)
#include "gemm_launch.h"
namespace ttg {
template <>
void launch<f32_tag>(GemmP& p, int cfg, hipStream_t st) {
  using Tag = f32_tag;
  switch (cfg) { TT_GEMM_TILES_F32(TT_TILE_CASE) }
}

void launch_f32(GemmP& p, int cfg, hipStream_t st) { launch<f32_tag>(p, cfg, st); }
}
