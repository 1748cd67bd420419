#!/bin/bash
# tools/resources.sh — per-kernel VGPR / SGPR / scratch / occupancy of rtg_kernels.hip (gfx950)
# RES_REFIT=1: the scene-update kernels (rtg_refit.hip) with the Makefile's flags for them instead
cd "$(dirname "$0")/.."
# RES_QUERY=1: the ray-query kernels (rtg_query.hip) with the Makefile's flags for them instead
src=rtg_kernels.hip
extra=
if [ -n "${RES_QUERY:-}" ]; then
  src=rtg_query.hip
  extra="-fPIC -Xclang -target-feature -Xclang -packed-fp32-ops"
fi
if [ -n "${RES_REFIT:-}" ]; then
  src=rtg_refit.hip
  extra="-fPIC -fslp-vectorize -Xclang -target-feature -Xclang -packed-fp32-ops"
fi
# RES_SORT=1: the ray-sort kernels (rtg_raysort.hip)
if [ -n "${RES_SORT:-}" ]; then
  src=rtg_raysort.hip
  extra="-fPIC -fslp-vectorize"
fi
# RES_NEAREST=1: the proximity-query kernels (rtg_nearest.hip), the ray-query kernels' flags
if [ -n "${RES_NEAREST:-}" ]; then
  src=rtg_nearest.hip
  extra="-fPIC -Xclang -target-feature -Xclang -packed-fp32-ops"
fi
# RES_NEAREST_K=1: the k-nearest kernels (rtg_nearest_k.hip), the same flags
if [ -n "${RES_NEAREST_K:-}" ]; then
  src=rtg_nearest_k.hip
  extra="-fPIC -Xclang -target-feature -Xclang -packed-fp32-ops"
fi
/opt/rocm/bin/hipcc -std=c++17 -O3 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -Iinclude \
  -Iraytracing-practice_amd/csrc ${RES_DEFS:-} $extra -c raytracing-practice_amd/csrc/$src -o /tmp/rtg_res.o \
  -Rpass-analysis=kernel-resource-usage 2>&1 |
  python3 -c '
import re, sys
cur = None
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1); print(cur[:90], end=""); continue
    for key in ("VGPRs:", "SGPRs Spill:", "ScratchSize [bytes/lane]:", "Occupancy [waves/SIMD]:", "LDS Size [bytes/block]:"):
        if key in line:
            print("  %s %s" % (key.split()[0], line.split(key)[1].split()[0]), end="")
            if key.startswith("LDS"): print()
'
