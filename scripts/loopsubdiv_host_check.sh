#!/bin/bash
# builds scripts/loopsubdiv_host_check.cpp (over pbrt-v3-rs_amd/csrc/loopsubdiv_host.h) for the host under the address and undefined-behaviour sanitizers and runs it with the
# arguments given (CPU only); CXX names the compiler
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all $R/scripts/loopsubdiv_host_check.cpp -o $R/build/loopsubdiv_host_check
$R/build/loopsubdiv_host_check "$@"
