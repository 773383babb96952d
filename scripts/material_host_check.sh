#!/bin/bash
# builds scripts/material_host_check.cpp and the material unit for the host under the address and undefined-behaviour sanitizers and runs it (CPU only); CXX names the compiler.
# The program's output (stdout) is what tests/golden/material_host_sequences.txt holds; arguments are passed on to it.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fsanitize=address,undefined -fno-sanitize-recover=all -I$R/pbrt-v3-rs_amd/csrc $R/scripts/material_host_check.cpp $R/pbrt-v3-rs_amd/csrc/material_host.cpp -o $R/build/material_host_check
$R/build/material_host_check "$@"
