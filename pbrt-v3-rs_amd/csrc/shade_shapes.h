// The shade pass's rows (wavefront.hip, shade_kernel): what a scene's lights, sampler and light-sampling strategy can make a path vertex do, in the manner of traverse.h's TravShapes.
// A row names the branches that are COMPILED: the kinds of light light_sample_li / light_pdf_li / the MIS resolve handle, the samplers sampler_dim / cursor_for evaluate, the spatial
// light distribution's look-up.  A branch a row leaves out has a condition that is false at every vertex of every scene the row is picked for, so what remains executes the same
// operations in the same order and the film does not depend on the row.  Plain C++ (no device code): the host's picker and scripts/shade_rows_check.cpp read the same table.
#pragma once

namespace ph {

// What a scene can ask of the shade pass.  `area` covers every emissive primitive (area lights of the light list AND the emission-only ones of instanced objects: MeshRec::first_light >= 0),
// `delta` the five kinds without extent (distant, point, spot, projection, goniometric); `sobol`: the sampler is SobolSampler, else HaltonSampler; `spatial`: the render call uses the
// spatial light distribution (light strategy 2 with more than one light).
struct ShadeFeatures { bool infinite, area, delta, sobol, spatial; };

// Every kind, both samplers, the spatial distribution: the kernel as it was before the table existed.  PBRT_HIP_SHADE_ROW=full picks it for every scene.
struct ShadeRowFull {
    static constexpr bool infinite = true, area = true, delta = true, halton = true, sobol = true, spatial = true;
    static constexpr bool phi_skip = false;   // light_pdf_li of a constant infinite light computes phi although both entries of its cond_func row are equal
    static constexpr bool lean_lds = false;   // the staged rays carry t_max and time; the drawn sampler dimensions have rows of their own
};
// Infinite lights only (any number, none included), Halton, no spatial distribution: the headline workload.
struct ShadeRowSky {
    static constexpr bool infinite = true, area = false, delta = false, halton = true, sobol = false, spatial = false;
    static constexpr bool phi_skip = true, lean_lds = true;
};

template <class R> constexpr bool shade_row_covers(ShadeFeatures f) {
    return (!f.infinite || R::infinite) && (!f.area || R::area) && (!f.delta || R::delta) && (f.sobol ? R::sobol : R::halton) && (!f.spatial || R::spatial);
}
// Every row that is compiled, leanest first: a scene takes the first row that covers it.
template <class... R> struct ShadeRowTable {
    static constexpr int n = (int)sizeof...(R);
    static constexpr int find(ShadeFeatures f) { int i = 0, at = -1; ((at = (at < 0 && shade_row_covers<R>(f)) ? i : at, i++), ...); return at; }
    static constexpr bool covers(int row, ShadeFeatures f) { int i = 0; bool c = false; ((c = (i == row) ? shade_row_covers<R>(f) : c, i++), ...); return c; }
};
using ShadeRows = ShadeRowTable<ShadeRowSky, ShadeRowFull>;
constexpr int kShadeRowSky = 0, kShadeRowFull = ShadeRows::n - 1;

// The scene's row.  force_full: PBRT_HIP_SHADE_ROW=full (a same-library A/B against the kernel that compiles everything).
constexpr int pick_shade_row(ShadeFeatures f, bool force_full = false) { return force_full ? kShadeRowFull : ShadeRows::find(f); }
constexpr ShadeFeatures shade_features_of_bits(int k) { return ShadeFeatures{(k & 1) != 0, (k & 2) != 0, (k & 4) != 0, (k & 8) != 0, (k & 16) != 0}; }
constexpr bool every_scene_has_a_shade_row() {
    for (int k = 0; k < 32; k++) {
        const int row = pick_shade_row(shade_features_of_bits(k));
        if (row < 0 || !ShadeRows::covers(row, shade_features_of_bits(k))) return false;
    }
    return true;
}
static_assert(every_scene_has_a_shade_row(), "a combination of scene features has no row in ShadeRows");
static_assert(shade_row_covers<ShadeRowFull>(ShadeFeatures{true, true, true, false, true}) && shade_row_covers<ShadeRowFull>(ShadeFeatures{true, true, true, true, true}), "the last row compiles everything");
static_assert(pick_shade_row(ShadeFeatures{true, false, false, false, false}) == kShadeRowSky, "infinite lights + Halton + no spatial distribution is the headline row");

}  // namespace ph
