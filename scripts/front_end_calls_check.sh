#!/bin/bash
# builds scripts/front_end_calls_check.cpp with the scene-file front end (HOST, default pbrt-v3-rs_amd/host) and the library's host-side math under the address and
# undefined-behaviour sanitizers and runs it from the repository's root (CPU only); CXX names the compiler.
# The program's output (stdout) is what tests/golden/front_end_calls.txt holds.  HOST=<a copy of another commit's host directory> records that commit's front end.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
HOST=${HOST:-$R/pbrt-v3-rs_amd/host}
OUT=${OUT:-$R/build/front_end_calls_check}
mkdir -p "$(dirname "$OUT")"
SRCS=$(ls "$HOST"/*.cpp | grep -v '/main\.cpp$')
${CXX:-g++} -std=c++17 -O2 -g -ffp-contract=off -fno-fast-math -fsanitize=address,undefined -fno-sanitize-recover=all -DFRONT_END_HOST_HEADER="\"$HOST/pbrt_host.hpp\"" \
    $R/scripts/front_end_calls_check.cpp $SRCS $R/pbrt-v3-rs_amd/csrc/host_setup.cpp $R/pbrt-v3-rs_amd/csrc/bvh_build.cpp -lz -o "$OUT"
cd $R
"$OUT" "$@"
