// Which of a rank's tiles have their sample records resident at once.  A FilmTile takes samples from its own tile only (film_tile.rs:62-108) and the rank's pixel list is
// tile-major, so a run of whole tiles with all of their samples is self-contained: the drivers (wavefront.hip, whitted.hip) render a frame band by band, each band's records in
// the same buffers, and the film pass of a band fills exactly that band's slots of the tile buffer.  Plain arithmetic, no device code: scripts/band_plan_check.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace phost {
constexpr uint64_t kSampleRecordBytes = 20;   // {L.rgb, p_film.x} + p_film.y per camera sample
// tiles [tile0, tile0 + n_tiles) of the rank's tile list = pixels [px0, px0 + n_px) of its pixel list
struct SampleBand { uint32_t tile0, n_tiles, px0, n_px; };

inline uint64_t band_record_bytes(uint64_t n_px, uint32_t spp) { return n_px * spp * kSampleRecordBytes; }

// Consecutive runs of tiles in increasing index, each as long as its records (pixels * spp * 20 B) stay within `budget`.  A run is never less than one tile: a budget below one
// tile's records gives one tile per band, and the caller reports the overshoot.  tile_px[i] = pixels of the rank's i-th tile.
inline std::vector<SampleBand> plan_bands(const uint32_t* tile_px, size_t n_tiles, uint32_t spp, uint64_t budget) {
    std::vector<SampleBand> bands;
    const uint64_t max_px = budget / (std::max<uint64_t>(spp, 1) * kSampleRecordBytes);   // (no product of pixels and spp: it cannot overflow)
    uint64_t px_seen = 0;
    for (size_t t = 0; t < n_tiles; t++) {
        if (bands.empty() || (uint64_t)bands.back().n_px + tile_px[t] > max_px) bands.push_back({(uint32_t)t, 0u, (uint32_t)px_seen, 0u});
        bands.back().n_tiles++; bands.back().n_px += tile_px[t];
        px_seen += tile_px[t];
    }
    return bands;
}

// The budget where the caller set none.  A frame whose records fit keeps them all: one band, as before there were bands.  "Fit" is what the drivers could fall back to before:
// all records next to the smallest chunk (one sample per pixel, `min_chunk`) within the free memory plus what the workspace holds already (`held`: records and chunk buffers
// of an earlier render, which are reused).  free_b / total_b: hipMemGetInfo's answer, total_b = 0 where it gave none (one band then).
// A frame that does not fit gets half of the memory the chunk planner counts as available (80 % of the free memory plus what is held); the other half is the chunk's.
inline uint64_t auto_record_budget(uint64_t rec_need, uint64_t free_b, uint64_t total_b, uint64_t held, uint64_t min_chunk) {
    if (!total_b || rec_need + min_chunk <= free_b + held) return rec_need;
    return std::max<uint64_t>((free_b / 10 * 8 + held) / 2, 1);
}
}  // namespace phost
