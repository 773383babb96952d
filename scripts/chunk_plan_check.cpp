// The chunk planner of the wavefront drivers (pbrt-v3-rs_amd/csrc/chunk_plan.h) on the CPU.  Prints, from the built library, what each driver's chunk
// table sums to per scene class; then answers every line of standard input
//     <ceiling> <floor> <free> <total> <held> <reserve> <per_path> <PBRT_HIP_MAX_PATHS or -> <n_px> <spp>
// with plan_chunk_spp's chunk_spp.  tests/test_chunk_plan_cpu.py holds the cases and what the drivers computed for them before they shared this code.
// Build and run:  bash scripts/chunk_plan_check.sh < cases
#include "../pbrt-v3-rs_amd/csrc/chunk_plan.h"
#include <cstdio>
#include <cstring>

int main() {
    for (int general = 0; general < 2; general++)
        for (int textured = 0; textured < 2; textured++) std::printf("table path general %d textured %d = %zu\n", general, textured, phost::path_chunk_bytes_per_path(general, textured));
    for (unsigned n_frames : {1u, 5u, 16u}) std::printf("table whitted n_frames %u = %zu\n", n_frames, phost::whitted_chunk_bytes_per_sample(n_frames));
    unsigned long long ceiling, floor, free_b, total_b, held, reserve, per_path, n_px, spp;
    char env[64];
    while (std::scanf("%llu %llu %llu %llu %llu %llu %llu %63s %llu %llu", &ceiling, &floor, &free_b, &total_b, &held, &reserve, &per_path, env, &n_px, &spp) == 10) {
        const phost::ChunkPolicy pol{(size_t)ceiling, (size_t)floor, 0, ""};
        std::printf("plan = %u\n", phost::plan_chunk_spp(pol, free_b, total_b, held, reserve, per_path, std::strcmp(env, "-") ? env : nullptr, (uint32_t)n_px, (uint32_t)spp));
    }
    return 0;
}
