// The band planner of the wavefront drivers (pbrt-v3-rs_amd/csrc/band_plan.h) on the CPU; needs neither the built library nor a device.  Answers every line of standard input:
//     plan <spp> <budget> <n_tiles> <pixels of tile 0> <pixels of tile 1> ...     ->   bands = <tile0>:<n_tiles>:<px0>:<n_px> ...
//     auto <rec_need> <free> <total> <held> <min_chunk>                           ->   auto = <budget>
// tests/test_band_plan_cpu.py holds the cases and checks the answers.  Build and run under the address and undefined-behaviour sanitizers:  bash scripts/band_plan_check.sh < cases
#include "../pbrt-v3-rs_amd/csrc/band_plan.h"
#include <cstdio>
#include <cstring>

int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            unsigned long long spp, budget, n_tiles;
            if (std::scanf("%llu %llu %llu", &spp, &budget, &n_tiles) != 3) return 2;
            std::vector<uint32_t> px(n_tiles);
            for (uint32_t& v : px) { unsigned long long t; if (std::scanf("%llu", &t) != 1) return 2; v = (uint32_t)t; }
            std::printf("bands =");
            for (const phost::SampleBand& b : phost::plan_bands(px.data(), px.size(), (uint32_t)spp, budget)) std::printf(" %u:%u:%u:%u", b.tile0, b.n_tiles, b.px0, b.n_px);
            std::printf("\n");
        } else if (!std::strcmp(what, "auto")) {
            unsigned long long need, free_b, total_b, held, min_chunk;
            if (std::scanf("%llu %llu %llu %llu %llu", &need, &free_b, &total_b, &held, &min_chunk) != 5) return 2;
            std::printf("auto = %llu\n", (unsigned long long)phost::auto_record_budget(need, free_b, total_b, held, min_chunk));
        } else return 2;
    }
    return 0;
}
