// The input stage of the device builders (bvh_device.hip, bvh_sah_device.hip), host only and without HIP so that it is testable on its own (scripts/device_build_input_check.cpp):
// what a BuildInput and its ForestSpec must satisfy before a kernel follows one of their indices, and the sizes both builders derive from them.
#pragma once
#include "bvh_build.h"
#include <algorithm>
#include <string>

namespace phost {

// What a device build runs over: the forest's item list, or (no forest) one tree whose item i is primitive slot i.  Valid after check_device_build_input.
struct DeviceBuildItems {
    const ForestSpec* forest;
    uint32_t n, n_trees, one_tree[2];
    DeviceBuildItems(const BuildInput& in, const ForestSpec* f) : forest(f), n((uint32_t)(f ? f->n_items : in.n_tris)), n_trees(f ? f->n_trees : 1u), one_tree{0u, n} {}
    const uint32_t* tree_start() const { return forest ? forest->tree_start : one_tree; }
    const uint32_t* items() const { return forest ? forest->items : nullptr; }   // null: item i is slot i
    size_t n_inst() const { return forest ? forest->n_inst : 0; }
    uint32_t top_end() const { return tree_start()[1]; }   // the scene's own tree is [0, top_end): instances and quadric slots stand there only
};

// 0, or -1 with `err` saying what is wrong.  Every index a kernel follows is checked here: tree ranges, items, instances' trees, quadric slots.
inline int check_device_build_input(const BuildInput& in, const ForestSpec* forest, std::string& err) {
    auto refuse = [&](const char* what) { err = what; return -1; };
    if (!forest && in.items) return refuse("device build: an item list without its forest (instanced scenes come as a forest, or take the host builder)");
    if (in.n_tris >= 0x3FFFFFFFu || (forest && (forest->n_items >= 0x3FFFFFFFu || forest->n_trees == 0 || !forest->tree_start || !forest->items)))
        return refuse("device build: bad arguments (a forest needs its items and tree ranges; at most 2^30 primitives)");
    const DeviceBuildItems b(in, forest);
    if (b.n == 0) return 0;
    const uint32_t* tree_start = b.tree_start(); const uint32_t* items = b.items();
    for (uint32_t t = 0; t < b.n_trees; t++) if (tree_start[t] >= tree_start[t + 1] || tree_start[t + 1] > b.n) return refuse("device build: empty or unordered tree range");
    if (tree_start[0] != 0 || tree_start[b.n_trees] != b.n) return refuse("device build: tree ranges do not cover the items");
    const size_t n_inst = b.n_inst();
    if (n_inst && (b.n_trees < 2 || !forest->inst_tree || !forest->inst_i2w)) return refuse("device build: instances without object trees");
    for (size_t k = 0; k < n_inst; k++) if (forest->inst_tree[k] == 0 || forest->inst_tree[k] >= b.n_trees) return refuse("device build: an instance names no object tree");
    if (items) for (uint32_t i = 0; i < b.n; i++) {
        const uint32_t it = items[i];
        if ((it & PH_ITEM_INST) ? (i >= b.top_end() || (size_t)(it & ~PH_ITEM_INST) >= n_inst) : (size_t)it >= in.n_tris) return refuse("device build: an item names no triangle or instance");
    }
    const uint32_t* pq = in.prim_quadric;   // null: every slot holds a triangle
    if (pq && !in.quad_bounds) return refuse("device build: quadric slots without their bounds");
    if (pq) for (uint32_t i = 0; i < b.n; i++) {   // a quadric stands in the scene's own tree only (object definitions hold none), and names one of the n_quadrics bounds
        const uint32_t it = items ? items[i] : i;
        if ((it & PH_ITEM_INST) || !pq[it]) continue;
        if ((forest && i >= b.top_end()) || (size_t)(pq[it] - 1u) >= in.n_quadrics) return refuse("device build: a quadric slot inside an object's tree, or one that names no quadric");
    }
    return 0;
}

// The vertices the triangle slots name: a quadric slot's index triple is {0, 0, 0} and stands for no vertex (a scene of quadrics only has none: nothing of P is read)
inline size_t count_build_verts(const BuildInput& in) {
    size_t n_verts = 0;
    const uint32_t* pq = in.prim_quadric;
    if (!pq) for (size_t i = 0; i < 3 * in.n_tris; i++) n_verts = std::max<size_t>(n_verts, (size_t)in.idx[i] + 1);
    else for (size_t t = 0; t < in.n_tris; t++) if (!pq[t]) for (int k = 0; k < 3; k++) n_verts = std::max<size_t>(n_verts, (size_t)in.idx[3 * t + k] + 1);
    return n_verts;
}

}  // namespace phost
