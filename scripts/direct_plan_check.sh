#!/bin/bash
# builds scripts/direct_plan_check.cpp for the host under the address and undefined-behaviour sanitizers and runs it (CPU only); CXX names the compiler
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all $R/scripts/direct_plan_check.cpp -o $R/build/direct_plan_check
$R/build/direct_plan_check
