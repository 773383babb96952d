// CPU check of the host's share of the HLBVH forest build on the device (pbrt-v3-rs_amd/csrc/hlbvh_forest_stitch.h): per-tree slices of the treelet list, the SAH over each
// tree's treelet roots, the offsets that make per-tree numbers forest-wide references, and the host builder's node numbering.  The kernels' share — bounds, Morton codes, the
// stable sort by (tree, code), the treelets with their nodes in the recursion's creation order — is restated here in plain C++ (as bvh_device.hip does it, hlbvh.rs:62-294), so the
// whole build runs without a GPU and is compared with build_forest_host(.., split_method = 1, ..) on the same input: roots, bounds, n_items, every node and every leaf record.
// A scene without objects is a forest of one tree, which the device build ships in the kernels' numbering: for those the array BEFORE renumber_like_host is compared too.
// Built with the address and undefined-behaviour sanitizers by hlbvh_forest_stitch_check.sh; prints one line per case, exit status 1 on any difference.
#include "../pbrt-v3-rs_amd/csrc/hlbvh_forest_stitch.h"
#include <cstdio>
#include <cstring>
#include <string>

struct PbrtHipScene;
namespace phost { int set_err(PbrtHipScene*, int code, const std::string&) { return code; } }   // (guard.h's hook; nothing here reports through a scene handle)

using namespace phost;

static uint32_t g_rng = 12345u;
static float frand() { g_rng = g_rng * 1664525u + 1013904223u; return (float)(g_rng >> 8) * (1.0f / 16777216.0f); }

struct Scene {
    std::vector<float> P; std::vector<uint32_t> idx;
    std::vector<uint32_t> obj_tri0, obj_tri1, inst_object, top_items; std::vector<float> inst_i2w;
    uint32_t tri(float cx, float cy, float cz, float s) {
        const uint32_t v = (uint32_t)(P.size() / 3);
        for (int k = 0; k < 3; k++) { P.push_back(cx + s * (frand() - 0.5f)); P.push_back(cy + s * (frand() - 0.5f)); P.push_back(cz + s * (frand() - 0.5f)); }
        idx.push_back(v); idx.push_back(v + 1); idx.push_back(v + 2);
        return (uint32_t)(idx.size() / 3 - 1);
    }
    uint32_t object(uint32_t n_tris, float spread, float size) {
        obj_tri0.push_back((uint32_t)(idx.size() / 3));
        for (uint32_t i = 0; i < n_tris; i++) tri(spread * (frand() - 0.5f), spread * (frand() - 0.5f), spread * (frand() - 0.5f), size);
        obj_tri1.push_back((uint32_t)(idx.size() / 3));
        return (uint32_t)obj_tri0.size() - 1;
    }
    void top_tri(float spread) { top_items.push_back(tri(spread * (frand() - 0.5f), spread * (frand() - 0.5f), spread * (frand() - 0.5f), 0.3f)); }
    void instance(uint32_t ob, bool projective = false) {
        float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        m[0] = 0.5f + frand(); m[1] = 0.3f * (frand() - 0.5f); m[5] = 0.5f + frand(); m[6] = 0.2f * (frand() - 0.5f); m[10] = 0.5f + frand();
        m[3] = 8.0f * (frand() - 0.5f); m[7] = 8.0f * (frand() - 0.5f); m[11] = 8.0f * (frand() - 0.5f);
        if (projective) { m[12] = 0.01f; m[13] = -0.02f; m[15] = 1.25f; }
        top_items.push_back(PH_ITEM_INST | (uint32_t)inst_object.size());
        inst_object.push_back(ob); inst_i2w.insert(inst_i2w.end(), m, m + 16);
    }
};

static uint32_t left_shift_3(uint32_t x) {   // morton.rs:101-118
    uint32_t v = (x == (1u << 10)) ? x - 1 : x;
    v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}
static float fmn(float a, float b) { return a < b ? a : b; }
static float fmx(float a, float b) { return a > b ? a : b; }

// a treelet's nodes as emit_lbvh makes them (hlbvh.rs:199-294), interior nodes numbered in creation order
struct TNode { float lo[3], hi[3]; int kid[2]; uint32_t first, count, axis, dense; };
struct Emit {
    const std::vector<uint32_t>& codes; const std::vector<uint32_t>& ids; const std::vector<float>& blo; const std::vector<float>& bhi; uint32_t max_prims;
    std::vector<TNode> nodes; uint32_t interior = 0, leaves = 0, max_leaf = 0, depth = 0;
    int emit(uint32_t first, uint32_t n, int bit, uint32_t level) {
        for (;;) {
            if (bit == -1 || n < max_prims) {
                TNode l{}; l.kid[0] = l.kid[1] = -1; l.first = first; l.count = n;
                for (uint32_t k = 0; k < n; k++) for (int q = 0; q < 3; q++) {
                    const float a = blo[3 * (size_t)ids[first + k] + q], b = bhi[3 * (size_t)ids[first + k] + q];
                    l.lo[q] = k == 0 ? a : fmn(l.lo[q], a); l.hi[q] = k == 0 ? b : fmx(l.hi[q], b);
                }
                leaves++; max_leaf = std::max(max_leaf, n); depth = std::max(depth, level + 1);
                nodes.push_back(l); return (int)nodes.size() - 1;
            }
            const uint32_t mask = 1u << bit;
            if ((codes[first] & mask) != (codes[first + n - 1] & mask)) break;
            bit--;
        }
        const uint32_t mask = 1u << bit;
        uint32_t lo = 0, hi = n - 1;
        while (lo + 1 != hi) { const uint32_t mid = (lo + hi) / 2; if ((codes[first + lo] & mask) == (codes[first + mid] & mask)) lo = mid; else hi = mid; }
        const int self = (int)nodes.size();
        nodes.emplace_back();
        const uint32_t dense = interior++;
        const int k0 = emit(first, hi, bit - 1, level + 1), k1 = emit(first + hi, n - hi, bit - 1, level + 1);
        TNode& nd = nodes[(size_t)self];
        nd.kid[0] = k0; nd.kid[1] = k1; nd.axis = (uint32_t)(bit % 3); nd.dense = dense; nd.first = nd.count = 0;
        for (int q = 0; q < 3; q++) { nd.lo[q] = fmn(nodes[(size_t)k0].lo[q], nodes[(size_t)k1].lo[q]); nd.hi[q] = fmx(nodes[(size_t)k0].hi[q], nodes[(size_t)k1].hi[q]); }
        return self;
    }
};

static int g_bad = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (g_bad++ < 20) { std::printf("MISMATCH %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static bool same_boxes(const Node64& a, const Node64& b) {
    bool same = true;
    for (int q = 0; q < 2; q++) same = same && a.x0[q] == b.x0[q] && a.y0[q] == b.y0[q] && a.z0[q] == b.z0[q] && a.x1[q] == b.x1[q] && a.y1[q] == b.y1[q] && a.z1[q] == b.z1[q];
    return same;
}
// two trees in different numberings, walked from their roots in step: boxes, axes and leaf references node for node (interior references are followed, not compared)
static void walk_in_step(const char* name, const std::vector<Node64>& a, uint32_t root_a, const std::vector<Node64>& b, uint32_t root_b) {
    std::vector<std::pair<uint32_t, uint32_t>> stack(1, std::make_pair(root_a, root_b));
    size_t seen = 0;
    while (!stack.empty() && seen <= a.size()) {
        const std::pair<uint32_t, uint32_t> it = stack.back(); stack.pop_back();
        if ((it.first | it.second) & PH_LEAF_BIT) { EXPECT(it.first == it.second, "in step: leaf reference %08x, host %08x", it.first, it.second); continue; }
        EXPECT(it.first < a.size() && it.second < b.size(), "in step: reference %u / %u past the arrays", it.first, it.second);
        if (it.first >= a.size() || it.second >= b.size()) continue;
        seen++;
        const Node64& p = a[it.first]; const Node64& q = b[it.second];
        EXPECT(p.axis == q.axis, "in step: node %u axis %u, host node %u axis %u", it.first, p.axis, it.second, q.axis);
        EXPECT(same_boxes(p, q), "in step: node %u and host node %u: child boxes differ", it.first, it.second);
        stack.push_back({p.c1, q.c1}); stack.push_back({p.c0, q.c0});
    }
    EXPECT(seen == a.size() && seen == b.size(), "in step: %zu nodes reached of %zu, host %zu", seen, a.size(), b.size());
}

static void check(const char* name, Scene& sc, int max_prims, bool want_single_treelets, bool want_lone_object) {
    InstancedScene isc{sc.obj_tri0.data(), sc.obj_tri1.data(), sc.obj_tri0.size(), sc.inst_object.data(), sc.inst_i2w.data(), sc.inst_object.size(), sc.top_items.data(), sc.top_items.size()};
    ForestLayout L; forest_layout(isc, L);
    BuildInput in{}; in.P = sc.P.data(); in.idx = sc.idx.data(); in.n_tris = sc.idx.size() / 3; in.tri_flags = nullptr;
    BuildOutput want; std::vector<ForestTreeOut> want_trees;
    const int hrc = build_forest_host(in, isc, L, 1, max_prims, want, want_trees);
    EXPECT(hrc == 0, "host build returns %d", hrc);
    if (hrc != 0) return;
    const uint32_t n = (uint32_t)L.items.size(), n_trees = (uint32_t)L.tree_start.size() - 1;
    // ---- what the kernels do ----
    std::vector<float> blo(3 * (size_t)n), bhi(3 * (size_t)n), tb(6 * (size_t)n_trees), ib(6 * sc.inst_object.size());
    auto bounds_of = [&](uint32_t i0, uint32_t i1) {
        for (uint32_t i = i0; i < i1; i++) {
            const uint32_t it = L.items[i];
            for (int q = 0; q < 3; q++) {
                if (it & PH_ITEM_INST) { blo[3 * (size_t)i + q] = ib[6 * (size_t)(it & ~PH_ITEM_INST) + q]; bhi[3 * (size_t)i + q] = ib[6 * (size_t)(it & ~PH_ITEM_INST) + 3 + q]; }
                else {
                    const float a = sc.P[3 * (size_t)sc.idx[3 * (size_t)it] + q], b = sc.P[3 * (size_t)sc.idx[3 * (size_t)it + 1] + q], c = sc.P[3 * (size_t)sc.idx[3 * (size_t)it + 2] + q];
                    blo[3 * (size_t)i + q] = fmn(fmn(a, b), c); bhi[3 * (size_t)i + q] = fmx(fmx(a, b), c);
                }
            }
        }
    };
    auto tree_bounds = [&](uint32_t t) {
        for (uint32_t i = L.tree_start[t]; i < L.tree_start[t + 1]; i++) for (int q = 0; q < 3; q++) {
            const bool f = i == L.tree_start[t];
            tb[6 * (size_t)t + q] = f ? blo[3 * (size_t)i + q] : fmn(tb[6 * (size_t)t + q], blo[3 * (size_t)i + q]); tb[6 * (size_t)t + 3 + q] = f ? bhi[3 * (size_t)i + q] : fmx(tb[6 * (size_t)t + 3 + q], bhi[3 * (size_t)i + q]);
        }
    };
    bounds_of(L.tree_start[1], n);
    for (uint32_t t = 1; t < n_trees; t++) tree_bounds(t);
    for (size_t k = 0; k < sc.inst_object.size(); k++) transform_bounds(&sc.inst_i2w[16 * k], &tb[6 * (size_t)L.inst_tree[k]], &tb[6 * (size_t)L.inst_tree[k] + 3], &ib[6 * k]);
    bounds_of(0, L.tree_start[1]); tree_bounds(0);
    std::vector<uint32_t> tree_of(n), code0(n), ids(n), codes(n);
    for (uint32_t t = 0; t < n_trees; t++) for (uint32_t i = L.tree_start[t]; i < L.tree_start[t + 1]; i++) tree_of[i] = t;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t c[3];
        for (int q = 0; q < 3; q++) {
            const float glo = tb[6 * (size_t)tree_of[i] + q], ghi = tb[6 * (size_t)tree_of[i] + 3 + q];
            float o = 0.5f * (blo[3 * (size_t)i + q] + bhi[3 * (size_t)i + q]) - glo;
            if (ghi > glo) o = o / (ghi - glo);
            const float sc1024 = o * 1024.0f; uint32_t u; std::memcpy(&u, &sc1024, 4);
            c[q] = left_shift_3(u);
        }
        code0[i] = (c[2] << 2) | (c[1] << 1) | c[0]; ids[i] = i;
    }
    std::stable_sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t b) { return tree_of[a] != tree_of[b] ? tree_of[a] < tree_of[b] : code0[a] < code0[b]; });
    for (uint32_t i = 0; i < n; i++) codes[i] = code0[ids[i]];
    std::vector<uint32_t> tl_first;
    for (uint32_t i = 0; i < n; i++) if (i == 0 || tree_of[i] != tree_of[i - 1] || (codes[i] >> 18) != (codes[i - 1] >> 18)) tl_first.push_back(i);
    const uint32_t nt = (uint32_t)tl_first.size();
    tl_first.push_back(n);
    std::vector<Emit> em; em.reserve(nt);
    std::vector<StitchTreelet> tl(nt);
    for (uint32_t t = 0; t < nt; t++) {
        em.push_back(Emit{codes, ids, blo, bhi, (uint32_t)(max_prims & 0xff)});
        Emit& e = em.back();
        const int root = e.emit(tl_first[t], tl_first[t + 1] - tl_first[t], 29 - 12, 0);
        tl[t] = StitchTreelet{tl_first[t], tl_first[t + 1] - tl_first[t], e.interior, e.leaves, e.max_leaf, e.depth, {0, 0, 0}, {0, 0, 0}};
        for (int q = 0; q < 3; q++) { tl[t].lo[q] = e.nodes[(size_t)root].lo[q]; tl[t].hi[q] = e.nodes[(size_t)root].hi[q]; }
    }
    // ---- the host's share ----
    StitchPlan plan;
    const int prc = plan_hlbvh_forest(tl.data(), nt, L.tree_start.data(), n_trees, plan);
    EXPECT(prc == 0, "plan returns %d", prc);
    if (prc != 0) return;
    if (want_single_treelets) for (uint32_t t = 0; t < n_trees; t++) EXPECT(plan.tl0[t + 1] - plan.tl0[t] == 1, "tree %u has %u treelets, the case wants one", t, plan.tl0[t + 1] - plan.tl0[t]);
    if (want_lone_object) { bool lone = false; for (uint32_t t = 1; t < n_trees; t++) lone |= plan.trees[t].n_items == 1; EXPECT(lone, "no object with one primitive"); }
    std::vector<Node64> nodes(plan.interior_nodes);
    std::vector<uint32_t> rec_prim(n), rec_last(n, 0u);
    for (uint32_t t = 0; t < nt; t++) {   // K6 of bvh_device.hip
        const Emit& e = em[t];
        auto ref = [&](const TNode& c) { return c.kid[0] < 0 ? (PH_LEAF_BIT | (plan.out_base[t] + (c.first - tl[t].first))) : plan.dense_base[t] + c.dense; };
        for (const TNode& nd : e.nodes) {
            if (nd.kid[0] < 0) { rec_last[plan.out_base[t] + (nd.first - tl[t].first) + nd.count - 1] = 1u; continue; }
            const TNode& a = e.nodes[(size_t)nd.kid[0]]; const TNode& b = e.nodes[(size_t)nd.kid[1]];
            Node64 o;
            o.x0[0] = a.lo[0]; o.x0[1] = a.hi[0]; o.y0[0] = a.lo[1]; o.y0[1] = a.hi[1]; o.z0[0] = a.lo[2]; o.z0[1] = a.hi[2];
            o.x1[0] = b.lo[0]; o.x1[1] = b.hi[0]; o.y1[0] = b.lo[1]; o.y1[1] = b.hi[1]; o.z1[0] = b.lo[2]; o.z1[1] = b.hi[2];
            o.c0 = ref(a); o.c1 = ref(b); o.axis = nd.axis; o.pad = 0;
            nodes[plan.dense_base[t] + nd.dense] = o;
        }
        for (uint32_t i = tl[t].first; i < tl[t].first + tl[t].n; i++) rec_prim[plan.out_base[t] + (i - tl[t].first)] = L.items[ids[i]];
    }
    place_upper_nodes(plan, nodes.data());
    if (sc.obj_tri0.empty()) {   // one tree: this is the array the device build ships
        EXPECT(n_trees == 1, "%u trees, the case wants one", n_trees);
        walk_in_step(name, nodes, plan.trees[0].root_ref, want.nodes, want_trees[0].root_ref);
    }
    renumber_like_host(plan, nodes.data(), 0, n_trees);
    // ---- against build_forest_host ----
    EXPECT(plan.interior_nodes == want.interior_nodes && plan.leaf_nodes == want.leaf_nodes && plan.max_leaf_prims == want.max_leaf_prims && plan.max_depth == want.max_depth,
           "statistics %zu %zu %zu %d, host %zu %zu %zu %d", plan.interior_nodes, plan.leaf_nodes, plan.max_leaf_prims, plan.max_depth, want.interior_nodes, want.leaf_nodes, want.max_leaf_prims, want.max_depth);
    EXPECT(nodes.size() == want.nodes.size(), "%zu nodes, host %zu", nodes.size(), want.nodes.size());
    for (uint32_t t = 0; t < n_trees; t++) {
        const ForestTreeOut& a = plan.trees[t]; const ForestTreeOut& b = want_trees[t];
        EXPECT(a.root_ref == b.root_ref && a.n_items == b.n_items, "tree %u: root %08x items %u, host %08x %u", t, a.root_ref, a.n_items, b.root_ref, b.n_items);
        for (int q = 0; q < 3; q++) EXPECT(a.lo[q] == b.lo[q] && a.hi[q] == b.hi[q], "tree %u: bounds differ on axis %d", t, q);
    }
    for (size_t v = 0; v < std::min(nodes.size(), want.nodes.size()); v++) {
        const Node64& a = nodes[v]; const Node64& b = want.nodes[v];
        EXPECT(a.c0 == b.c0 && a.c1 == b.c1 && a.axis == b.axis, "node %zu: children %08x %08x axis %u, host %08x %08x %u", v, a.c0, a.c1, a.axis, b.c0, b.c1, b.axis);
        EXPECT(same_boxes(a, b), "node %zu: child boxes differ", v);
    }
    for (uint32_t i = 0; i < n; i++) {
        const bool inst = (rec_prim[i] & PH_ITEM_INST) != 0;
        EXPECT(want.tris[i].prim == (rec_prim[i] & ~PH_ITEM_INST) && ((want.tris[i].flags & PH_TRI_INSTANCE) != 0) == inst && ((want.tris[i].flags & PH_TRI_LAST) != 0) == (rec_last[i] != 0),
               "record %u: item %08x last %u, host prim %u flags %u", i, rec_prim[i], rec_last[i], want.tris[i].prim, want.tris[i].flags);
    }
    std::printf("%s: %u trees, %u treelets, %zu nodes, %u records, depth %d\n", name, n_trees, nt, nodes.size(), n, plan.max_depth);
}

int main() {
    {   // three trees: the scene's (lone triangles between instances) and two objects of several treelets each
        Scene s;
        const uint32_t a = s.object(700, 4.0f, 0.2f), b = s.object(90, 2.0f, 0.3f);
        for (int k = 0; k < 9; k++) { if (k % 2) s.top_tri(10.0f); s.instance(k % 3 == 2 ? b : a, k == 4); }
        for (int mp : {1, 4}) check("three trees", s, mp, false, false);
    }
    {   // every tree a single treelet
        Scene t;   // an object whose triangles share ONE centroid: equal codes, one treelet, one leaf whatever max_prims is; the scene holds its single instance: one treelet too
        t.obj_tri0.push_back(0);
        for (int k = 0; k < 12; k++) {
            const float r = 0.1f + 0.05f * (float)k;
            const uint32_t v = (uint32_t)(t.P.size() / 3);
            const float p[9] = {-r, -r, -r, r, r, r, 0.25f * r, -0.5f * r, 0.125f * r};   // box (-r .. r)^3: centroid 0 for every k
            t.P.insert(t.P.end(), p, p + 9); t.idx.push_back(v); t.idx.push_back(v + 1); t.idx.push_back(v + 2);
        }
        t.obj_tri1.push_back(12);
        t.instance(0);
        for (int mp : {1, 4}) check("single treelets, equal codes", t, mp, true, false);
    }
    {   // one object has one primitive (used directly: no aggregate), beside a larger one
        Scene s;
        const uint32_t lone = s.object(1, 1.0f, 0.5f), big = s.object(300, 3.0f, 0.2f);
        s.instance(big); s.top_tri(6.0f); s.instance(lone); s.instance(lone, true); s.top_tri(6.0f); s.instance(big);
        for (int mp : {1, 4}) check("an object of one primitive", s, mp, false, true);
    }
    {   // few, deep treelets: an object whose bound is the unit cube and whose centroids are 0.5 + j * 2^-24 per axis, j < 64 — the scaled offsets 512 + j * 2^-14 differ in the
        // low six bits of their bit patterns only (quirk B10), so the top 12 code bits agree and one treelet holds them all, split down to single primitives under max_prims 1
        Scene s;
        s.obj_tri0.push_back(0);
        auto push = [&](const float a[3], const float b[3], const float c[3]) {
            const uint32_t v = (uint32_t)(s.P.size() / 3);
            s.P.insert(s.P.end(), a, a + 3); s.P.insert(s.P.end(), b, b + 3); s.P.insert(s.P.end(), c, c + 3);
            s.idx.push_back(v); s.idx.push_back(v + 1); s.idx.push_back(v + 2);
        };
        { const float a[3] = {0, 0, 0}, b[3] = {1, 1, 1}, c[3] = {0.5f, 0.25f, 0.75f}; push(a, b, c); }
        for (int k = 0; k < 240; k++) {
            float ctr[3], a[3], b[3];
            for (int q = 0; q < 3; q++) { ctr[q] = 0.5f + (float)(int)(frand() * 64.0f) * 5.9604644775390625e-8f; a[q] = ctr[q] - 0.125f; b[q] = ctr[q] + 0.125f; }
            push(a, b, ctr);
        }
        s.obj_tri1.push_back((uint32_t)(s.idx.size() / 3));
        s.instance(0); s.top_tri(6.0f); s.instance(0, true);
        for (int mp : {1, 4}) check("deep treelets", s, mp, false, false);
    }
    for (int n : {1, 2, 3, 17, 300, 5000}) {   // no objects: one tree of scene-level triangles, as a scene without instances is built
        Scene s;
        for (int k = 0; k < n; k++) s.top_tri(10.0f);
        const std::string name = "one tree of " + std::to_string(n);
        for (int mp : {1, 4}) check(name.c_str(), s, mp, false, false);
    }
    if (g_bad) { std::printf("%d mismatches\n", g_bad); return 1; }
    std::printf("all equal\n");
    return 0;
}
