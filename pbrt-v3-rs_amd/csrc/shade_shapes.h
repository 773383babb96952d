// The shade pass's rows (wavefront.hip, shade_kernel): what a scene's lights, sampler and light-sampling strategy can make a path vertex do, in the manner of traverse.h's TravShapes.
// A row names the branches that are COMPILED: the kinds of light light_sample_li / light_pdf_li / the MIS resolve handle, the samplers sampler_dim / cursor_for evaluate, the spatial
// light distribution's look-up.  A branch a row leaves out has a condition that is false at every vertex of every scene the row is picked for, so what remains executes the same
// operations in the same order and the film does not depend on the row.
// Below the rows, the two tables of what the shade side launches: ShadeVariants, shade_kernel's <GEN, TEX, QUADRIC, Row> with pick_shade_variant, and TexVariants, texture_kernel's
// <SIMPLE, CAMERA, WAVES, QUADRIC> with pick_tex_variant.  wavefront.hip expands each table into its launchers (dispatch_shade_variant, dispatch_tex_variant) and launches the
// index the picker gives, so a kernel is named in one place.  Plain C++ (no device code): the host's pickers and scripts/shade_rows_check.cpp read the same tables.
#pragma once
#include <type_traits>

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
    static constexpr bool sphere_lights = false;   // an area light's shape is a triangle
};
// Infinite lights only (any number, none included), Halton, no spatial distribution: the headline workload.
struct ShadeRowSky {
    static constexpr bool infinite = true, area = false, delta = false, halton = true, sobol = false, spatial = false;
    static constexpr bool phi_skip = true, lean_lds = true;
    static constexpr bool sphere_lights = false;
};
// The full row where an area light's shape may be a sphere (pbrt_hip_add_sphere_light with pbrt_hip_set_path_sphere_lights on), a disk or a cylinder (pbrt_hip_add_quadric_light): sample_li, pdf_li and the MIS resolve ask the light's
// primitive whether it is a quadric (sphere_light.h).  NOT a row of ShadeRows and in no variant of ShadeVariants: wavefront.hip names the one kernel compiled on it next to its
// launchers and the driver picks it before the table's picker, for such a scene alone, so every other scene launches what pick_shade_variant gives it.
struct ShadeRowSphereLights : ShadeRowFull {
    static constexpr bool sphere_lights = true;
};

template <class R> constexpr bool shade_row_covers(ShadeFeatures f) {
    return (!f.infinite || R::infinite) && (!f.area || R::area) && (!f.delta || R::delta) && (f.sobol ? R::sobol : R::halton) && (!f.spatial || R::spatial);
}
// Every row that is compiled, leanest first: a scene takes the first row that covers it.
template <class... R> struct ShadeRowTable {
    static constexpr int n = (int)sizeof...(R);
    static constexpr int find(ShadeFeatures f) { int i = 0, at = -1; ((at = (at < 0 && shade_row_covers<R>(f)) ? i : at, i++), ...); return at; }
    static constexpr bool covers(int row, ShadeFeatures f) { int i = 0; bool c = false; ((c = (i == row) ? shade_row_covers<R>(f) : c, i++), ...); return c; }
    template <class Q> static constexpr int index_of() { int i = 0, at = -1; ((at = std::is_same_v<Q, R> ? i : at, i++), ...); return at; }
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

// ---- shade_kernel's variants ------------------------------------------------------------------------------------------------------------------------------------------------
// What a scene's materials and shapes ask of the shade pass: `general` some material is not matte (the general-BSDF code), `textured` some material evaluates a texture per hit
// (the shade pass reads the texture pass's records), `quadric` the scene holds a quadric shape (surface data from the parametric form, quadric.h).
struct ShadeTraits { bool general, textured, quadric; };
template <bool GEN, bool TEX, bool QUADRIC, class R> struct ShadeVariant { static constexpr bool gen = GEN, tex = TEX, quadric = QUADRIC; using Row = R; };
template <class... V> struct ShadeVariantTable {
    static constexpr int n = (int)sizeof...(V);
    // the variant with these template arguments, -1 if it is not compiled
    static constexpr int find(bool gen, bool tex, bool quadric, int row) {
        int i = 0, at = -1; ((at = (V::gen == gen && V::tex == tex && V::quadric == quadric && ShadeRows::index_of<typename V::Row>() == row) ? i : at, i++), ...); return at;
    }
    static constexpr int row_of(int v) { int i = 0, r = -1; ((r = (i == v) ? ShadeRows::index_of<typename V::Row>() : r, i++), ...); return r; }
};
// Every shade_kernel that is compiled.  The rows leaner than the full one exist for the texture-free matte kernel only; a quadric scene takes <true, true, true> whatever its materials are.
using ShadeVariants = ShadeVariantTable<ShadeVariant<false, false, false, ShadeRowSky>, ShadeVariant<true, true, true, ShadeRowFull>, ShadeVariant<true, true, false, ShadeRowFull>,
                                        ShadeVariant<false, true, false, ShadeRowFull>, ShadeVariant<true, false, false, ShadeRowFull>, ShadeVariant<false, false, false, ShadeRowFull>>;
// The scene's variant: the full row whenever a trait is set, else the row of its features; then the kernel of its traits on that row.
constexpr int pick_shade_variant(ShadeTraits t, ShadeFeatures f, bool force_full = false) {
    const int row = (t.general || t.textured || t.quadric) ? kShadeRowFull : pick_shade_row(f, force_full);
    return ShadeVariants::find(t.general || t.quadric, t.textured || t.quadric, t.quadric, row);
}
constexpr bool every_scene_has_a_shade_variant() {
    for (int k = 0; k < 512; k++) {
        const ShadeFeatures f = shade_features_of_bits(k & 31);
        const int v = pick_shade_variant(ShadeTraits{(k & 32) != 0, (k & 64) != 0, (k & 128) != 0}, f, (k & 256) != 0);
        if (v < 0 || !ShadeRows::covers(ShadeVariants::row_of(v), f)) return false;
    }
    return true;
}
static_assert(every_scene_has_a_shade_variant(), "a combination of scene traits and features has no variant in ShadeVariants whose row covers it");

// ---- texture_kernel's variants ----------------------------------------------------------------------------------------------------------------------------------------------
// <SIMPLE, CAMERA, WAVES, QUADRIC> as wavefront.hip's texture_kernel spells them.  LAUNCHED = false: compiled, never launched — an anchor that fixes the register budget of the
// out-of-line evaluator the launched forms call (TexEval::run, texture.h).  The backend compiles a device function for the largest waves per SIMD among its callers, so the two
// anchors keep it at 4 waves without differentials and 3 with them — the budget the texture pass was tuned with.  Without them the later-round general pass spills 356 VGPRs
// instead of 48 and configs[4] loses 1.2 % (texture pass + 3.4 %).
template <bool SIMPLE, bool CAMERA, int WAVES, bool QUADRIC = false, bool LAUNCHED = true> struct TexVariant {
    static constexpr bool simple = SIMPLE, camera = CAMERA, quadric = QUADRIC, launched = LAUNCHED; static constexpr int waves = WAVES;
};
template <class... V> struct TexVariantTable {
    static constexpr int n = (int)sizeof...(V);
    // the launched variant with these features, -1 if there is none
    static constexpr int find(bool simple, bool camera, bool quadric) { int i = 0, at = -1; ((at = (V::launched && V::simple == simple && V::camera == camera && V::quadric == quadric) ? i : at, i++), ...); return at; }
};
using TexVariants = TexVariantTable<TexVariant<false, true, 2, true>, TexVariant<true, true, 3>, TexVariant<false, true, 2>,      // camera rays (round 0): differentials, filtered look-ups
                                    TexVariant<false, false, 3, true>, TexVariant<true, false, 4>, TexVariant<false, false, 3>,   // later rounds
                                    TexVariant<false, false, 4, false, false>, TexVariant<false, true, 3, false, false>>;         // the two anchors
// The round's variant.  A quadric scene runs the general evaluator whatever its textures are.
constexpr int pick_tex_variant(bool camera_round, bool simple_textures, bool has_quadrics) { return TexVariants::find(simple_textures && !has_quadrics, camera_round, has_quadrics); }
static_assert(pick_tex_variant(false, false, false) >= 0 && pick_tex_variant(false, false, true) >= 0 && pick_tex_variant(false, true, false) >= 0 && pick_tex_variant(false, true, true) >= 0 &&
              pick_tex_variant(true, false, false) >= 0 && pick_tex_variant(true, false, true) >= 0 && pick_tex_variant(true, true, false) >= 0 && pick_tex_variant(true, true, true) >= 0,
              "a round of some textured scene has no launched variant in TexVariants");

}  // namespace ph
