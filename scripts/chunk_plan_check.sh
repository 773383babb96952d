#!/bin/bash
# builds and runs scripts/chunk_plan_check.cpp (CPU only) against the built libpbrt_hip.so; EXTRA adds compiler flags (a sanitizer build: EXTRA="-Xarch_host -fsanitize=undefined")
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/build
/opt/rocm/bin/hipcc -std=c++17 -O2 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -x hip $EXTRA $R/scripts/chunk_plan_check.cpp -L$R/pbrt-v3-rs_amd -lpbrt_hip -Wl,-rpath,$R/pbrt-v3-rs_amd -o $R/build/chunk_plan_check
$R/build/chunk_plan_check
