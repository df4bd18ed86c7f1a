#!/bin/bash
# usage: scripts/build_variant.sh <name> [extra hipcc flags...] -> raytracing_weekend_amd/csrc/variants/librtw_<name>.so: the product's
# build (__graft_entry__.build_hip: the same units, the same unit flags) with the extra flags on every unit
# (experiment binaries: git-ignored, they travel to the GPU box; select one with RTW_HIP_LIB=<path>)
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
N=$1; shift
mkdir -p $R/raytracing_weekend_amd/csrc/variants
cd $R && python3 -c 'import sys, __graft_entry__ as g; g.build_hip(sys.argv[1], ["-Rpass-analysis=kernel-resource-usage"] + sys.argv[2:])' \
  raytracing_weekend_amd/csrc/variants/librtw_$N.so "$@" 2>&1 \
  | { grep -E "error|k_pathILi0ELi0" -A8 || true; } | { grep -E "error|VGPRs:|SGPRs:|Scratch|Occupancy" || true; } | sed 's/.*remark: *//; s/ \[-Rpass.*//' | tr '\n' ' '
echo " <- $N"
