// The escape query: estimate_direct's BSDF-sampled ray (integrator/common.rs:262-283) in a scene without area lights.  The shade pass reads one thing from that ray's hit record —
// did it hit anything (hprim != 0xFFFFFFFF, wavefront.hip, K6) —, so the traversal kernel may stop it at the first primitive it accepts.  Until then its walk IS the closest-hit
// walk (same visiting order, same t_max, same test, same acceptance rule: BVHAccel::intersect, not intersect_p), so "found anything" is the same bit; after it the closest-hit walk
// only refines a value nobody reads.  The ray stays a closest-hit ray in every count and every buffer: its slot in rays_cl, keys_cl and the hit records, its place in n_cl.
//
// How the mark travels: the shade pass ORs PH_SORT_BINS into the ray's bin key; the binning (raysort.h) turns that into bit 31 of the ray's entry of `order`; the mixed
// traversal kernels of the eligible rows (traverse.h, ESCAPE) read it at the refill.  Nothing else ever sets either bit, and a frame for which mis_escape_eligible() is false
// sets neither: its keys, its `order` and its kernels are what they were.
// Plain C++17, no device code: scripts/mis_escape_check.cpp enumerates it on the CPU (tests/test_mis_escape_plan_cpu.py holds the table).
#pragma once
#include <cstdint>
#include "raysort_plan.h"

namespace ph {

#define PH_ORDER_ESCAPE 0x80000000u   // bit 31 of an entry of `order`: the closest-hit ray at that queue position is an escape query (positions stay below ChunkPolicy::limit = 0x7FFF0000)

// Is the frame's BSDF-sampled MIS ray an escape query?
//   area_lights: the scene holds an area light of any shape (triangle, sphere, disk, cylinder or quadric emitters: PbrtHipScene::lights_area) — the resolve then compares the hit
//                primitive with the sampled light and needs the closest hit;
//   alpha:       the traversal row's alpha class (0 none, 1 image-map masks, 2 any texture) — a masked row's acceptance waits for a texture verdict, left as it is;
//   quadric:     the traversal row tests quadric shapes;
//   counting:    traversal counting is on (pbrt_hip_set_traversal_counting): the frame is traced as the reference traces it, so the counts stay the oracle's.
// Flat and instanced rows both qualify.
constexpr bool mis_escape_eligible(bool area_lights, int alpha, bool quadric, bool counting) { return !area_lights && alpha == 0 && !quadric && !counting; }
// The same for a row of the traversal table: which mixed kernels are compiled with the query (every other instantiation keeps its instructions).
constexpr bool mis_escape_row(int alpha, bool quadric, bool counting) { return mis_escape_eligible(false, alpha, quadric, counting); }

// A closest-hit key as the binning sees it: bits 0 .. 11 the bin, bit 31 the mark.  A key below PH_SORT_BINS is itself.  A marked ray is binned where the extension ray of its
// cell is — the two leave the same hit point and walk the same part of the tree — and only its entry of `order` tells them apart.  (Left in the any-hit half of the joint key
// space, beside the shadow rays of its cell, where the bare PH_SORT_BINS bit would send it, the query gains nothing: configs[2] traversal 654.0 ms per frame against the parent's
// 654.1, and 631.1 binned here — the early stop is paid for by the lost neighbourhood.  DESIGN §4.3.)
constexpr uint32_t mis_escape_joint_key(uint32_t key) {
    const uint32_t mark = (key & PH_SORT_BINS) << 19;   // 4096 << 19 = bit 31
    return (key & (PH_SORT_BINS - 1u)) | mark;
}
static_assert((PH_SORT_BINS << 19) == PH_ORDER_ESCAPE, "the mark of a key moves to bit 31 by one shift");
static_assert(mis_escape_joint_key(PH_SORT_BINS - 1u) == PH_SORT_BINS - 1u && mis_escape_joint_key(0u) == 0u, "an unmarked key is binned as it was");

}  // namespace ph
