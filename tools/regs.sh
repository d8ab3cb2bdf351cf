#!/bin/bash
# tools/regs.sh [extra -D flags]: register use of the kernels that trace rays (hipcc -Rpass-analysis=kernel-resource-usage on csrc/rt_kernels.hip and rt_kernels_fp16.hip),
# then of the kernels that share csrc/rt_temporal.h and csrc/rt_filter.h (k_temporal_accumulate, its moving twin and the rectified kernels, the budget key kernels, the denoisers' kernels) and k_world_set_geometry with the Makefile's flags for their files
cd "$(dirname "$0")/../dd2360-raytracing_amd"
F="--offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero -fPIC -Wno-unused-function $*"
for f in rt_kernels rt_kernels_fp16; do
  /opt/rocm/bin/hipcc $F -fno-slp-vectorize -DRT_SPLIT_LIST -c --cuda-device-only -o /dev/null csrc/$f.hip -Rpass-analysis=kernel-resource-usage 2>&1 | grep "remark:" |
  awk '/Function Name:/{n=$5} / VGPRs:/{v=$4} /TotalSGPRs:/{s=$4} /ScratchSize/{sc=$5} /VGPRs Spill/{vs=$5} /SGPRs Spill/{ss=$5} /Occupancy/{o=$5} /LDS Size/{print n, "VGPR", v, "SGPR", s, "scratch", sc, "vspill", vs, "sspill", ss, "occ", o}' | c++filt | grep -E "k_render<|k_render_h<|k_tile_cost" | sed 's/(rt::RenderArgs.*)//'
done
for f in rt_temporal rt_budget rt_animate rt_rectify rt_denoise; do
  /opt/rocm/bin/hipcc $F -c --cuda-device-only -o /dev/null csrc/$f.hip -Rpass-analysis=kernel-resource-usage 2>&1 | grep "remark:" |
  awk '/Function Name:/{n=$5} / VGPRs:/{v=$4} /TotalSGPRs:/{s=$4} /ScratchSize/{sc=$5} /VGPRs Spill/{vs=$5} /SGPRs Spill/{ss=$5} /Occupancy/{o=$5} /LDS Size/{print n, "VGPR", v, "SGPR", s, "scratch", sc, "vspill", vs, "sspill", ss, "occ", o, "LDS", $6}' | c++filt | grep -E "k_temporal_accumulate|k_budget_keys|k_world_set_geometry|k_denoise" | sed 's/(.*)//'
done
