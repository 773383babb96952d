// The host's share of the HLBVH build on the device (bvh_device.hip): the kernels make every treelet of every tree of a forest [scene | object | object ..] — a scene without
// object instances is a forest of one tree; what is left is per TREE — the SAH over that tree's treelet roots (hlbvh.rs:296-432, build_upper_sah), where each treelet's
// interior nodes and leaf records go in the forest's arrays, the SAH nodes themselves, and, for a forest with objects, the host builder's node numbering.  Plain C++, no device
// code: scripts/hlbvh_forest_stitch_check.cpp runs it on the CPU against build_forest_host.
//
// Numbering.  The kernels number a treelet's interior nodes in the recursion's creation order (a node, its whole first subtree, the second), a tree's nodes as
// [SAH nodes | treelet 0's | treelet 1's ..].  A scene of one tree ships in that numbering.  build_bvh numbers a tree as it walks it depth first and gives BOTH interior children
// of a node their numbers when it visits the node (bvh_build.cpp), so for a forest renumber_like_host walks every tree once more and permutes it: afterwards the arrays are
// build_forest_host's entry by entry.
#pragma once
#include "bvh_build.h"
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace phost {

// one treelet as the kernels leave it: `first`, `n` = its range of the sorted item list (treelets in increasing `first`, so grouped by tree); interior / leaves / max_leaf =
// tallies of its nodes; depth = 1 + the deepest level (root = 0) at which it has a leaf; lo / hi = its root's box
struct StitchTreelet { uint32_t first, n, interior, leaves, max_leaf, depth; float lo[3], hi[3]; };

struct StitchPlan {
    std::vector<uint32_t> tl0;          // per tree (n_trees + 1): its first treelet
    std::vector<uint32_t> node_base;    // per tree (n_trees + 1): where its nodes start in the forest's node array
    std::vector<uint32_t> dense_base;   // per treelet: the forest index of its first interior node (kernel numbering)
    std::vector<uint32_t> out_base;     // per treelet: the forest position of its first leaf record
    std::vector<Node64> upper;          // every tree's SAH nodes in kernel numbering; tree t's are upper[upper0[t] .. upper0[t + 1]) and go to node_base[t] ..
    std::vector<uint32_t> upper0;
    std::vector<ForestTreeOut> trees;
    size_t interior_nodes = 0, leaf_nodes = 0, max_leaf_prims = 0;
    int max_depth = 0;
};

// Returns 0, -1 (the treelets do not tile the trees), -2 (the reference's assertions fire in some tree's SAH over the treelet roots, hlbvh.rs:338 / 356 / 418).
inline int plan_hlbvh_forest(const StitchTreelet* tl, size_t n_tl, const uint32_t* tree_start, uint32_t n_trees, StitchPlan& P) {
    P = StitchPlan();
    P.tl0.assign((size_t)n_trees + 1, 0u); P.node_base.assign((size_t)n_trees + 1, 0u); P.upper0.assign((size_t)n_trees + 1, 0u);
    P.dense_base.assign(n_tl, 0u); P.out_base.assign(n_tl, 0u); P.trees.assign(n_trees, ForestTreeOut{});
    size_t at = 0;
    for (uint32_t t = 0; t < n_trees; t++) {   // per-tree slices of the treelet list
        P.tl0[t] = (uint32_t)at;
        uint32_t pos = tree_start[t];
        while (at < n_tl && tl[at].first < tree_start[t + 1]) {
            if (tl[at].first != pos || tl[at].n == 0 || tl[at].n > tree_start[t + 1] - pos) return -1;
            pos += tl[at].n; at++;
        }
        if (pos != tree_start[t + 1] || at == P.tl0[t]) return -1;
    }
    P.tl0[n_trees] = (uint32_t)at;
    if (at != n_tl) return -1;
    std::vector<float> rb;
    std::vector<UpperNode> up;
    std::vector<int> stack;
    std::vector<std::pair<int, int>> dstack;
    uint32_t node_at = 0;
    for (uint32_t t = 0; t < n_trees; t++) {
        const uint32_t a = P.tl0[t], m = P.tl0[t + 1] - a;
        rb.resize(6 * (size_t)m);
        for (uint32_t k = 0; k < m; k++) for (int q = 0; q < 3; q++) { rb[6 * (size_t)k + q] = tl[a + k].lo[q]; rb[6 * (size_t)k + 3 + q] = tl[a + k].hi[q]; }
        int root = -1;
        if (build_upper_sah(rb.data(), m, up, root) != 0) return -2;
        const uint32_t n_upper = (uint32_t)up.size();
        P.node_base[t] = node_at; P.upper0[t] = (uint32_t)P.upper.size();
        { uint32_t acc = node_at + n_upper; for (uint32_t k = 0; k < m; k++) { P.dense_base[a + k] = acc; acc += tl[a + k].interior; } node_at = acc; }
        {   // depth-first walk of the SAH tree: the order in which the treelets' leaf ranges follow each other
            uint32_t acc = tree_start[t];
            stack.assign(1, root);
            while (!stack.empty()) {
                const int v = stack.back(); stack.pop_back();
                if (v < 0) { const uint32_t k = (uint32_t)(-1 - v); P.out_base[a + k] = acc; acc += tl[a + k].n; }
                else { stack.push_back(up[(size_t)v].kid[1]); stack.push_back(up[(size_t)v].kid[0]); }
            }
        }
        // a child of a SAH node is another SAH node or a treelet's root: that treelet's first interior node, or its single leaf
        auto ref_of = [&](int v) -> uint32_t {
            if (v >= 0) return P.node_base[t] + (uint32_t)v;
            const uint32_t k = a + (uint32_t)(-1 - v);
            return tl[k].interior ? P.dense_base[k] : (PH_LEAF_BIT | P.out_base[k]);
        };
        auto box_of = [&](int v, float lo[3], float hi[3]) {
            if (v >= 0) { for (int q = 0; q < 3; q++) { lo[q] = up[(size_t)v].lo[q]; hi[q] = up[(size_t)v].hi[q]; } }
            else { const uint32_t k = (uint32_t)(-1 - v); for (int q = 0; q < 3; q++) { lo[q] = rb[6 * (size_t)k + q]; hi[q] = rb[6 * (size_t)k + 3 + q]; } }
        };
        for (uint32_t v = 0; v < n_upper; v++) {
            const UpperNode& u = up[v];
            Node64 d;
            float l0[3], h0[3], l1[3], h1[3];
            box_of(u.kid[0], l0, h0); box_of(u.kid[1], l1, h1);
            d.x0[0] = l0[0]; d.x0[1] = h0[0]; d.y0[0] = l0[1]; d.y0[1] = h0[1]; d.z0[0] = l0[2]; d.z0[1] = h0[2];
            d.x1[0] = l1[0]; d.x1[1] = h1[0]; d.y1[0] = l1[1]; d.y1[1] = h1[1]; d.z1[0] = l1[2]; d.z1[1] = h1[2];
            d.c0 = ref_of(u.kid[0]); d.c1 = ref_of(u.kid[1]); d.axis = (uint32_t)u.axis; d.pad = 0;
            P.upper.push_back(d);
        }
        ForestTreeOut& fo = P.trees[t];
        fo.root_ref = ref_of(root); fo.n_items = tree_start[t + 1] - tree_start[t];
        box_of(root, fo.lo, fo.hi);
        // statistics as build_bvh tallies them: depth = the deepest INTERIOR node, the root at 1
        int depth = 0;
        dstack.assign(1, std::make_pair(root, 1));
        while (!dstack.empty()) {
            const std::pair<int, int> it = dstack.back(); dstack.pop_back();
            if (it.first >= 0) { depth = std::max(depth, it.second); dstack.push_back({up[(size_t)it.first].kid[0], it.second + 1}); dstack.push_back({up[(size_t)it.first].kid[1], it.second + 1}); }
            else { const StitchTreelet& q = tl[a + (uint32_t)(-1 - it.first)]; if (q.interior) depth = std::max(depth, it.second + (int)q.depth - 2); }
        }
        P.max_depth = std::max(P.max_depth, depth);
        for (uint32_t k = 0; k < m; k++) { P.leaf_nodes += tl[a + k].leaves; P.max_leaf_prims = std::max<size_t>(P.max_leaf_prims, tl[a + k].max_leaf); }
    }
    P.node_base[n_trees] = node_at; P.upper0[n_trees] = (uint32_t)P.upper.size();
    P.interior_nodes = node_at;
    return 0;
}

// nodes: the forest's node array in kernel numbering, with the treelets' nodes in place.  Puts the SAH nodes where they belong.
inline void place_upper_nodes(const StitchPlan& P, Node64* nodes) {
    for (size_t t = 0; t + 1 < P.node_base.size(); t++) std::copy(P.upper.begin() + P.upper0[t], P.upper.begin() + P.upper0[t + 1], nodes + P.node_base[t]);
}

// One tree, nodes [base, base + count), from kernel numbering to build_bvh's; the root keeps index `base`.  tmp: scratch of the caller.
inline void renumber_tree_like_host(Node64* nodes, uint32_t base, uint32_t count, std::vector<Node64>& tmp, std::vector<std::pair<uint32_t, uint32_t>>& stack) {
    if (count < 2) return;
    tmp.assign(nodes + base, nodes + base + count);
    uint32_t next = 1;
    stack.assign(1, std::make_pair(0u, 0u));   // (old, new), relative to base
    while (!stack.empty()) {
        const std::pair<uint32_t, uint32_t> it = stack.back(); stack.pop_back();
        Node64 nd = tmp[it.first];
        const uint32_t old0 = nd.c0, old1 = nd.c1;
        if (!(old0 & PH_LEAF_BIT)) nd.c0 = base + next++;
        if (!(old1 & PH_LEAF_BIT)) nd.c1 = base + next++;
        nodes[base + it.second] = nd;
        if (!(old1 & PH_LEAF_BIT)) stack.push_back({old1 - base, nd.c1 - base});
        if (!(old0 & PH_LEAF_BIT)) stack.push_back({old0 - base, nd.c0 - base});
    }
}
inline void renumber_like_host(const StitchPlan& P, Node64* nodes, uint32_t tree0, uint32_t tree1) {
    std::vector<Node64> tmp; std::vector<std::pair<uint32_t, uint32_t>> stack;
    for (uint32_t t = tree0; t < tree1; t++) renumber_tree_like_host(nodes, P.node_base[t], P.node_base[t + 1] - P.node_base[t], tmp, stack);
}

}  // namespace phost
