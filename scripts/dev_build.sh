#!/bin/bash
# development aid: quick build of a subset of the kernel variants into csrc/librmpc_hip_dev.so -- the host unit, the world unit and
# ONE variant unit holding the variants of the mask (__graft_entry__.compile_library)
#   scripts/dev_build.sh 0x4 [-DRMPC_STAMPS ...]     (bit i = variant i of RMPC_VARIANTS in rmpc_variants.hip: 0 point robot,
#                                                      2 panda, 5 boxer + slack, 6 .. 10 chains n = 2, 4, 5, 6, 8)
# use with RMPC_ALLOW_STALE=1 RMPC_LIB_PATH=$PWD/robot_mpcs_amd/csrc/librmpc_hip_dev.so
set -e
cd "$(dirname "$0")/.."
mask=${1:-0x3f}; shift || true
python -c 'import sys, __graft_entry__ as g; g.compile_library(g.CSRC + "/librmpc_hip_dev.so", "dev", [int(sys.argv[1], 0)], sys.argv[2:])' \
  "$mask" "$@"
ls -la robot_mpcs_amd/csrc/librmpc_hip_dev.so
