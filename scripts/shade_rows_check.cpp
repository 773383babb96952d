// The shade pass's row table (pbrt-v3-rs_amd/csrc/shade_shapes.h) on the CPU: prints, for each of the 32 combinations of scene features and with / without PBRT_HIP_SHADE_ROW=full,
//     pick infinite=<0|1> area=<0|1> delta=<0|1> sobol=<0|1> spatial=<0|1> full=<0|1> row=<index> covers=<0|1>
// then one line per row with what it compiles.  tests/test_shade_rows_cpu.py holds what the lines must say.
// Build and run:  bash scripts/shade_rows_check.sh
#include "../pbrt-v3-rs_amd/csrc/shade_shapes.h"
#include <cstdio>

template <class R> static void print_row(int i, const char* name) {
    std::printf("row %d %s infinite=%d area=%d delta=%d halton=%d sobol=%d spatial=%d phi_skip=%d lean_lds=%d\n", i, name, (int)R::infinite, (int)R::area, (int)R::delta, (int)R::halton,
                (int)R::sobol, (int)R::spatial, (int)R::phi_skip, (int)R::lean_lds);
}

int main() {
    for (int full = 0; full < 2; full++)
        for (int k = 0; k < 32; k++) {
            const ph::ShadeFeatures f = ph::shade_features_of_bits(k);
            const int row = ph::pick_shade_row(f, full != 0);
            std::printf("pick infinite=%d area=%d delta=%d sobol=%d spatial=%d full=%d row=%d covers=%d\n", (int)f.infinite, (int)f.area, (int)f.delta, (int)f.sobol, (int)f.spatial, full, row,
                        (int)(row >= 0 && ph::ShadeRows::covers(row, f)));
        }
    std::printf("rows %d sky %d full %d\n", ph::ShadeRows::n, ph::kShadeRowSky, ph::kShadeRowFull);
    print_row<ph::ShadeRowSky>(ph::kShadeRowSky, "sky");
    print_row<ph::ShadeRowFull>(ph::kShadeRowFull, "full");
    return 0;
}
