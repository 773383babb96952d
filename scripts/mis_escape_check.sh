#!/bin/bash
# builds and runs scripts/mis_escape_check.cpp (CPU only: the header is plain C++17); EXTRA adds compiler flags (a sanitizer build: EXTRA="-fsanitize=undefined,address")
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
CXX=${CXX:-$(command -v g++ || command -v c++ || echo /opt/rocm/bin/hipcc)}
$CXX -std=c++17 -O1 -Wall $EXTRA $R/scripts/mis_escape_check.cpp -o $R/build/mis_escape_check
$R/build/mis_escape_check
