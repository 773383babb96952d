#!/bin/bash
# builds and runs scripts/shade_rows_check.cpp (CPU only: the header is plain C++17); EXTRA adds compiler flags (a sanitizer build: EXTRA="-fsanitize=undefined,address")
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
CXX=${CXX:-$(command -v g++ || command -v c++ || echo /opt/rocm/bin/hipcc)}
$CXX -std=c++17 -O1 -Wall $EXTRA $R/scripts/shade_rows_check.cpp -o $R/build/shade_rows_check
$R/build/shade_rows_check
