// instantiation unit: every tt_gemm tile configuration for one storage type (see gemm_launch.h)
#include "gemm_launch.h"
#include "gemm_sq320.h"
namespace ttg {
void launch_f16(GemmP& p, int cfg, hipStream_t st) { launch<f16_tag>(p, cfg, st); }
void launch_sq320_f16(const GemmP& p, hipStream_t st) { launch_sq320_tag<f16_tag>(p, st); }
}
