// How many sampler dimensions one camera sample may draw under the recursive integrators (whitted.hip), and whether the sampler's tables hold that many.  Host only, plain
// arithmetic with no device or scene types: scripts/direct_plan_check.cpp runs it on the CPU.
//
// li draws 5 dimensions for the camera sample, then at every vertex of its recursion tree the light loop's, and at every vertex above the last level 2 for specular_reflect
// and 2 for specular_transmit (core/src/integrator/sampler_integrator.rs:79-238).  The light loop draws
//   Whitted                 one get_2d per light                                           (integrators/src/whitted.rs:88-104)
//   direct lighting, all    get_2d + get_2d per light: uniform_sample_all_lights AS IT RUNS (core/src/integrator/common.rs:42-57) — the tile samplers hold no sample arrays
//                           (samplers/src/halton.rs:177-183, sobol.rs:110-112), so the single-sample branch is the only one taken and n_light_samples never matters
//   direct lighting, one    get_1d + get_2d + get_2d where the scene has a light           (common.rs:111-119)
// The tree is binary where the scene has specular reflection AND transmission lobes, a chain with one kind, a single vertex with neither.
#pragma once

namespace phost {

inline long long whitted_light_dims(long long n_lights) { return 2 * n_lights; }
// strategy: 0 all, 1 one
inline long long direct_light_dims(int strategy, long long n_lights) { return strategy == 1 ? (n_lights > 0 ? 5 : 0) : 4 * n_lights; }

// refl / trans: some material of the scene has a specular reflection / transmission lobe.  max_depth in 0 .. 16 (a depth of 0 still shades the camera ray's vertex).
inline long long dimension_bound(bool refl, bool trans, int max_depth, long long light_dims) {
    const int d = max_depth > 1 ? max_depth : 1;
    long long vertices = 1, inner = d > 1 ? 1 : 0;
    if (refl && trans) { vertices = (1ll << d) - 1; inner = (1ll << (d - 1)) - 1; }
    else if (refl || trans) { vertices = d; inner = d - 1; }
    return 5 + vertices * light_dims + inner * 4;
}

// A render is refused (PBRT_HIP_ERR_UNSUPPORTED) where the bound reaches the sampler's dimension table — 1000 primes for Halton (sampler_kind 0), 1024 Sobol' dimensions — or,
// under Sobol', exceeds the dimensions of the tables the caller gave (pbrt_hip_set_sobol_tables; sobol_dims_given is not read for Halton).
enum DimensionRefusal { DIMS_OK = 0, DIMS_OVER_TABLE = 1, DIMS_OVER_SOBOL_GIVEN = 2 };
inline DimensionRefusal dimension_refusal(long long dims, int sampler_kind, long long sobol_dims_given) {
    if (dims >= (sampler_kind == 0 ? 1000 : 1024)) return DIMS_OVER_TABLE;
    if (sampler_kind == 1 && dims > sobol_dims_given) return DIMS_OVER_SOBOL_GIVEN;
    return DIMS_OK;
}

}  // namespace phost
