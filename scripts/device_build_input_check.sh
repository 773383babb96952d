#!/bin/bash
# builds scripts/device_build_input_check.cpp (header only: csrc/device_build_input.h) for the host under the address and undefined-behaviour sanitizers and runs it
# (CPU only); CXX names the compiler
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all $R/scripts/device_build_input_check.cpp -o $R/build/device_build_input_check
$R/build/device_build_input_check
