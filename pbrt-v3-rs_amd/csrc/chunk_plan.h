// How many samples per pixel a wavefront driver keeps in flight at once, and the device buffers that grow with that number.  Shared by the path driver (wavefront.hip) and the
// Whitted driver (whitted.hip); host only.  A driver lists its chunk-scaled buffers once, as a ChunkTable: the memory estimate, the allocation for a chunk of B paths and the
// release before a smaller retry are all read off that list, so they cannot disagree.  plan_chunk_spp is plain arithmetic (scripts/chunk_plan_check.cpp runs it on the CPU).
#pragma once
#include "scene_host.h"
#include <algorithm>
#include <cstdlib>

namespace phost {
// One buffer of per_path * B bytes.  `allocated` false: the scene does not use the buffer, so it is not allocated now; its per_path still counts in the estimate, and what an
// earlier render left in it counts as held and is released on a retry.
struct ChunkBuf { DevBuf* buf; size_t per_path; bool allocated = true; };
using ChunkTable = std::vector<ChunkBuf>;
// What differs between the drivers: most and fewest paths per chunk where memory decides, the bound on n_px * chunk_spp its 32-bit queue positions allow, the prefix of its error texts.
struct ChunkPolicy { size_t ceiling, floor, limit; const char* prefix; };

inline size_t chunk_bytes_per_path(const ChunkTable& t) { size_t n = 0; for (const ChunkBuf& c : t) n += c.per_path; return n; }
inline size_t chunk_bytes_held(const ChunkTable& t) { size_t n = 0; for (const ChunkBuf& c : t) n += c.buf->bytes; return n; }
inline void release_buf(DevBuf& b) { if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; } }
inline void chunk_release(const ChunkTable& t) { for (const ChunkBuf& c : t) release_buf(*c.buf); }
inline int chunk_alloc(PbrtHipScene* s, const ChunkTable& t, size_t B) {
    for (const ChunkBuf& c : t) if (c.allocated) { if (int rc = ensure_buf(s, *c.buf, B * c.per_path)) return rc; }
    return PBRT_HIP_OK;
}

// Samples per pixel of one chunk.  free_b / total_b: hipMemGetInfo's answer, total_b = 0 where it gave none (the ceiling applies then).  Of the free memory 80 % count as
// available, plus what the table's buffers hold already (a chunk may reuse it; other contexts on the card keep theirs), less `reserve`, what the caller has yet to allocate
// besides the chunk; at most 30 % of the device's memory goes to one chunk.  max_paths_env: the text of PBRT_HIP_MAX_PATHS or null; a positive value replaces the estimate.
inline uint32_t plan_chunk_spp(const ChunkPolicy& pol, size_t free_b, size_t total_b, size_t held, size_t reserve, size_t per_path, const char* max_paths_env, uint32_t n_px, uint32_t spp) {
    size_t max_paths = pol.ceiling;
    if (total_b) {
        size_t avail = free_b / 10 * 8 + held;
        avail = avail > reserve ? avail - reserve : 0;
        max_paths = std::max(pol.floor, std::min(pol.ceiling, std::min(total_b / 10 * 3, avail) / per_path));
    }
    if (max_paths_env) { long long v = std::atoll(max_paths_env); if (v > 0) max_paths = (size_t)v; }
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(spp, max_paths / std::max<uint32_t>(n_px, 1)));
}
// ... for the current device, as it is now
inline uint32_t plan_chunk_spp_now(const ChunkPolicy& pol, const ChunkTable& t, size_t reserve, uint32_t n_px, uint32_t spp) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;
    return plan_chunk_spp(pol, free_b, total_b, chunk_bytes_held(t), reserve, chunk_bytes_per_path(t), std::getenv("PBRT_HIP_MAX_PATHS"), n_px, spp);
}

// Allocates the table for n_px * chunk_spp paths.  The estimate can be wrong (fragmentation, another context allocating meanwhile): on hipErrorOutOfMemory the table is released,
// chunk_spp halved and the allocation tried again, until one sample per pixel does not fit either.  A retry that succeeded leaves no error text behind.
// (test hook: PBRT_HIP_TEST_CHUNK_OOM=k makes the first k attempts of every render call fail as an out-of-memory allocation would)
inline int chunk_alloc_or_halve(PbrtHipScene* s, const ChunkPolicy& pol, const ChunkTable& t, uint32_t n_px, uint32_t& chunk_spp) {
    const std::string prefix = pol.prefix;
    const char* e = std::getenv("PBRT_HIP_TEST_CHUNK_OOM");
    int forced_oom = e ? std::max(0, std::atoi(e)) : 0;
    for (bool retried = false;; retried = true) {
        if ((size_t)n_px * chunk_spp >= pol.limit) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, prefix + ": tile range too large for one rank; use more tile_parts");
        int rc;
        if (forced_oom > 0) { forced_oom--; rc = set_err(s, PBRT_HIP_ERR_OOM, prefix + ": out of device memory (forced by PBRT_HIP_TEST_CHUNK_OOM)"); }
        else rc = chunk_alloc(s, t, (size_t)n_px * chunk_spp);
        if (rc == PBRT_HIP_OK) { if (retried) s->err.clear(); return rc; }
        if (rc != PBRT_HIP_ERR_OOM || chunk_spp == 1) return rc;
        chunk_release(t);
        chunk_spp = (chunk_spp + 1) / 2;
    }
}
// What the render's chunk came to, for pbrt_hip_get_render_footprint: paths per chunk and the bytes of the table's buffers for them
inline void chunk_note_footprint(PbrtHipScene* s, size_t paths, const ChunkTable& t) {
    size_t per_path = 0;
    for (const ChunkBuf& c : t) if (c.allocated) per_path += c.per_path;
    s->footprint[4] = paths; s->footprint[5] = paths * per_path;
}
}  // namespace phost
