#!/bin/bash
# Resource usage of every gemm_kernel / sq320_kernel instance of tt_gemm's instantiation units, from hipcc's own report
# (-Rpass-analysis=kernel-resource-usage): VGPRs, SGPRs, scratch bytes per lane, waves per SIMD, spills.
#   tools/gemm_regs.sh [regex on the demangled instance name] [unit ...]
# units: bf16 f16 f32 wide_bf16 wide_f16 wide_f32 (default: all six; each is a full compile of gemm_inst_<unit>.hip, device side only)
cd "$(dirname "$0")/../this_and_that_vdm_amd/csrc" || exit 1
filter="${1:-.}"
shift
units="${*:-bf16 f16 f32 wide_bf16 wide_f16 wide_f32}"
for u in $units; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 --cuda-device-only -O3 -std=c++17 -fPIC -I../../include -I. -Wno-unused-result \
    -c "gemm_inst_$u.hip" -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 |
    sed -E 's/ *\[-Rpass-analysis=kernel-resource-usage\]$//' |
    awk -v unit="$u" '
      / error: / { print; next }
      /remark: Function Name:/ { name = $NF }
      /remark: +VGPRs:/ { vgpr = $NF }
      /remark: +TotalSGPRs:/ { sgpr = $NF }
      /remark: +ScratchSize/ { scratch = $NF }
      /remark: +Occupancy/ { occ = $NF }
      /remark: +SGPRs Spill:/ { sspill = $NF }
      /remark: +VGPRs Spill:/ { vspill = $NF }
      /remark: +LDS Size/ { print unit, name, "vgpr", vgpr, "sgpr", sgpr, "scratch", scratch, "waves", occ, "sgpr_spill", sspill, "vgpr_spill", vspill }' |
    c++filt | sed -E 's/void ttg:://; s/\(ttg::GemmP\)//' | grep -E "_kernel<" | grep -E "$filter" | sort -u
done
