// The shade pass's row table (pbrt-v3-rs_amd/csrc/shade_shapes.h) on the CPU: prints, for each of the 32 combinations of scene features and with / without PBRT_HIP_SHADE_ROW=full,
//     pick infinite=<0|1> area=<0|1> delta=<0|1> sobol=<0|1> spatial=<0|1> full=<0|1> row=<index> covers=<0|1>
// then one line per row with what it compiles.  After the rows, the two tables of what the shade side launches and their pickers: for each of the 8 trait sets x 32 feature
// sets x with / without full,
//     shade_pick general=<0|1> textured=<0|1> quadric=<0|1> infinite=.. area=.. delta=.. sobol=.. spatial=.. full=<0|1> variant=<index> gen=<0|1> tex=<0|1> quad=<0|1> row=<index>
// for each of the 8 rounds a textured scene can have,
//     tex_pick camera=<0|1> simple_textures=<0|1> quadrics=<0|1> variant=<index> simple=<0|1> cam=<0|1> waves=<n> quad=<0|1> launched=<0|1>
// (the members are the picked variant's), and one shade_variant / tex_variant line per entry of each table, the two anchors included.
// tests/test_shade_rows_cpu.py holds what the lines must say.
// Build and run:  bash scripts/shade_rows_check.sh
#include "../pbrt-v3-rs_amd/csrc/shade_shapes.h"
#include <cstdio>
#include <vector>

template <class R> static void print_row(int i, const char* name) {
    std::printf("row %d %s infinite=%d area=%d delta=%d halton=%d sobol=%d spatial=%d phi_skip=%d lean_lds=%d\n", i, name, (int)R::infinite, (int)R::area, (int)R::delta, (int)R::halton,
                (int)R::sobol, (int)R::spatial, (int)R::phi_skip, (int)R::lean_lds);
}

struct ShadeMembers { int gen, tex, quad, row; };
struct TexMembers { int simple, cam, waves, quad, launched; };
template <class... V> static std::vector<ShadeMembers> members_of(ph::ShadeVariantTable<V...>) {
    return {ShadeMembers{(int)V::gen, (int)V::tex, (int)V::quadric, ph::ShadeRows::index_of<typename V::Row>()}...};
}
template <class... V> static std::vector<TexMembers> members_of(ph::TexVariantTable<V...>) {
    return {TexMembers{(int)V::simple, (int)V::camera, V::waves, (int)V::quadric, (int)V::launched}...};
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

    const std::vector<ShadeMembers> sv = members_of(ph::ShadeVariants{});
    const std::vector<TexMembers> tv = members_of(ph::TexVariants{});
    for (int k = 0; k < 512; k++) {
        const ph::ShadeTraits t{(k & 32) != 0, (k & 64) != 0, (k & 128) != 0};
        const ph::ShadeFeatures f = ph::shade_features_of_bits(k & 31);
        const int full = k >> 8, v = ph::pick_shade_variant(t, f, full != 0);
        if (v < 0 || v >= (int)sv.size()) { std::printf("shade_pick %d: no variant\n", k); return 1; }
        std::printf("shade_pick general=%d textured=%d quadric=%d infinite=%d area=%d delta=%d sobol=%d spatial=%d full=%d variant=%d gen=%d tex=%d quad=%d row=%d\n", (int)t.general,
                    (int)t.textured, (int)t.quadric, (int)f.infinite, (int)f.area, (int)f.delta, (int)f.sobol, (int)f.spatial, full, v, sv[v].gen, sv[v].tex, sv[v].quad, sv[v].row);
    }
    for (int k = 0; k < 8; k++) {
        const int v = ph::pick_tex_variant((k & 1) != 0, (k & 2) != 0, (k & 4) != 0);
        if (v < 0 || v >= (int)tv.size()) { std::printf("tex_pick %d: no variant\n", k); return 1; }
        std::printf("tex_pick camera=%d simple_textures=%d quadrics=%d variant=%d simple=%d cam=%d waves=%d quad=%d launched=%d\n", k & 1, (k >> 1) & 1, (k >> 2) & 1, v, tv[v].simple, tv[v].cam,
                    tv[v].waves, tv[v].quad, tv[v].launched);
    }
    for (size_t i = 0; i < sv.size(); i++) std::printf("shade_variant %d gen=%d tex=%d quad=%d row=%d\n", (int)i, sv[i].gen, sv[i].tex, sv[i].quad, sv[i].row);
    for (size_t i = 0; i < tv.size(); i++)
        std::printf("tex_variant %d simple=%d cam=%d waves=%d quad=%d launched=%d\n", (int)i, tv[i].simple, tv[i].cam, tv[i].waves, tv[i].quad, tv[i].launched);
    return 0;
}
