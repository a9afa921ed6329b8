#!/bin/bash
# Builds tests/host/NAME_refusals.cpp (rmpc_world.hip and a main of its own) with AddressSanitizer + UBSan on the host side
# and runs it: the argument checks of one family of entries.  Needs no GPU: every call is refused before the first HIP
# call.  NAME is one of grid_large, search, tours, timed_tours, timed_replan, timed_repair.
#   bash tests/host/run_refusals.sh NAME
set -e
cd "$(dirname "$0")/../.."
[ -f "tests/host/${1}_refusals.cpp" ] || { echo "usage: $0 NAME (tests/host/NAME_refusals.cpp)" >&2; exit 2; }
OUT=tests/host/${1}_refusals_asan
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  tests/host/${1}_refusals.cpp -o $OUT
ASAN_OPTIONS=detect_leaks=0 $OUT
