// What the device-side builders (bvh_device.hip, bvh_sah_device.hip, loopsubdiv.hip) share on the HIP side: the scratch arena (device_arena.h), the upload of a checked BuildInput
// (device_build_input.h), the PBRT_HIP_BUILD_PROFILE lap printer and the one-block exclusive scan.
#pragma once
#include "device_arena.h"
#include "device_build_input.h"
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace phost {

// a failed HIP call inside a builder: `err` says which, the builder answers -1 (the arena frees what was allocated)
#define PH_BUILD_CHECK(call) \
    do { hipError_t e__ = (call); if (e__ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e__); (void)hipGetLastError(); return -1; } } while (0)

struct DeviceEvent { hipEvent_t e = nullptr; ~DeviceEvent() { if (e) (void)hipEventDestroy(e); } };

inline bool build_profile_on() { return std::getenv("PBRT_HIP_BUILD_PROFILE") != nullptr; }
// With PBRT_HIP_BUILD_PROFILE set: lap(what) waits for the stream and prints "<label>: <what> at <seconds since construction> s" to stderr.  seconds() is a build's build_seconds.
struct BuildLaps {
    std::string label; hipStream_t stream; bool on = build_profile_on(); std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    void operator()(const char* what) const { if (on) { (void)hipStreamSynchronize(stream); std::fprintf(stderr, "%s: %-28s at %.3f s\n", label.c_str(), what, seconds()); } }
};

// The device copies of a BuildInput's arrays; null where the input has none (items without a forest, flags, mesh ids, quadric slots).
struct DeviceBuildInput { float* P = nullptr; uint32_t* idx = nullptr, *tri_flags = nullptr, *tri_mesh = nullptr, *items = nullptr, *tree_start = nullptr, *prim_quadric = nullptr; float* quad_bounds = nullptr; };
// Allocates them in `arena` and queues the copies on its stream; arena.ok() says whether all of it worked.  `in` has passed check_device_build_input.
inline DeviceBuildInput upload_build_input(DeviceArena& arena, const BuildInput& in, const DeviceBuildItems& b) {
    DeviceBuildInput d;
    d.P = arena.upload(in.P, count_build_verts(in) * 3); d.idx = arena.upload(in.idx, in.n_tris * 3);
    if (in.tri_flags) d.tri_flags = arena.upload(in.tri_flags, in.n_tris);
    if (in.tri_mesh) d.tri_mesh = arena.upload(in.tri_mesh, in.n_tris);
    if (b.items()) d.items = arena.upload(b.items(), b.n);
    d.tree_start = arena.upload(b.tree_start(), (size_t)b.n_trees + 1);
    if (in.prim_quadric) { d.prim_quadric = arena.upload(in.prim_quadric, in.n_tris); d.quad_bounds = arena.upload(in.quad_bounds, in.n_quadrics * 6); }
    return d;
}

// exclusive scan of `m` counters in place, one block of 1024 threads (a thread past the end of the array takes the empty range [m, m))
static __global__ __launch_bounds__(1024) void exclusive_scan_kernel(uint32_t* a, uint32_t m) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (m + 1023u) / 1024u, lo = threadIdx.x * per < m ? threadIdx.x * per : m, hi = lo + per < m ? lo + per : m;
    uint32_t sum = 0u;
    for (uint32_t i = lo; i < hi; i++) sum += a[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024u; o <<= 1) {
        const uint32_t add = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t i = lo; i < hi; i++) { const uint32_t v = a[i]; a[i] = run; run += v; }
}

}  // namespace phost
