#!/bin/bash
# builds scripts/ewa_loop_check.cpp for the host at the optimisation level given (-O0, -O2, ...) under the address and undefined-behaviour sanitizers and runs it (CPU only); CXX names the compiler
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=${1:--O2}
mkdir -p "$R/build"
"${CXX:-g++}" -std=c++17 "$O" -g -ffp-contract=off -fno-fast-math -fsanitize=undefined,address -fno-sanitize-recover "$R/scripts/ewa_loop_check.cpp" -o "$R/build/ewa_loop_check_${O#-}"
"$R/build/ewa_loop_check_${O#-}"
