#!/bin/bash
# builds scripts/sah_quadric_steps_check.cpp and the host builder for the host under the address and undefined-behaviour sanitizers and runs it (CPU only); CXX names the compiler
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -pthread -fsanitize=address,undefined -fno-sanitize-recover=all $R/scripts/sah_quadric_steps_check.cpp $R/pbrt-v3-rs_amd/csrc/bvh_build.cpp -o $R/build/sah_quadric_steps_check
$R/build/sah_quadric_steps_check
