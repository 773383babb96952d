// loopsubdiv.hip's one entry: LoopSubDiv::subdivide's levels, limit positions, normals and world pass on the current device, from the control mesh of loopsubdiv_host.h
#pragma once
#include "loopsubdiv_host.h"
#include <hip/hip_runtime.h>
#include <string>

namespace phost {
// Refines the control mesh `c` (positions P) n_levels times and copies the limit mesh out: out_P / out_N 3 * c.out_verts floats, out_idx 3 * c.out_faces.  o2w_m null: object space.
// Returns 0, or -1 with `err` set.  With PBRT_HIP_BUILD_PROFILE in the environment (as for the device tree builders) the kernels' time by HIP events goes to stderr.
int loopsubdiv_device(const ploop::Control& c, const float* P, int n_levels, const float* o2w_m, const float* o2w_minv, hipStream_t stream, float* out_P, float* out_N,
                      uint32_t* out_idx, std::string& err);
}  // namespace phost
