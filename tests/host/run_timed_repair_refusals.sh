#!/bin/bash
# Builds tests/host/timed_repair_refusals.cpp (rmpc_world.hip and a main of its own) with AddressSanitizer + UBSan on the
# host side and runs it: the argument checks of the repaired timed routes' entries (include/rmpc_timed_repair.h).  Needs
# no GPU: every call is refused before the first HIP call.
#   bash tests/host/run_timed_repair_refusals.sh
set -e
cd "$(dirname "$0")/../.."
OUT=tests/host/timed_repair_refusals_asan
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  tests/host/timed_repair_refusals.cpp -o $OUT
ASAN_OPTIONS=detect_leaks=0 $OUT
