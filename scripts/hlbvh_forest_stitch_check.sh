#!/bin/bash
# builds scripts/hlbvh_forest_stitch_check.cpp (with the host BVH builder it compares against) for the host under the address and undefined-behaviour sanitizers and runs it
# (CPU only); CXX names the compiler
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -pthread -fsanitize=address,undefined -fno-sanitize-recover=all $R/scripts/hlbvh_forest_stitch_check.cpp $R/pbrt-v3-rs_amd/csrc/bvh_build.cpp \
    -o $R/build/hlbvh_forest_stitch_check
$R/build/hlbvh_forest_stitch_check
