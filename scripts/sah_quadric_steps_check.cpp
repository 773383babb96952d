// Single-threaded rehearsal of the device SAH build's passes (pbrt-v3-rs_amd/csrc/bvh_sah_steps.h) on inputs whose primitive slots hold QUADRICS next to triangles, against the host
// builder (bvh_build.cpp: build_bvh, build_forest_host): the same step functions the kernels run, called in grid order by plain loops, as scripts/sah_steps_check.cpp does for
// triangles.  Node array, leaf records (all twelve words, so the leaf ends too) and statistics must be the host builder's.  A program of its own with its own main, so that the host
// side can run under the address and undefined-behaviour sanitizers.  Build and run:  bash scripts/sah_quadric_steps_check.sh
#include "../pbrt-v3-rs_amd/csrc/bvh_sah_steps.h"
#include "../pbrt-v3-rs_amd/csrc/bvh_build.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace phs;

// a list of primitive slots: a triangle (three vertices of its own) or a quadric (its world bound, idx = {0, 0, 0}); every slot has flag bits and a mesh id of its own
struct Slots {
    std::vector<float> P, qb;
    std::vector<uint32_t> idx, pq, flags, mesh;
    std::mt19937 rng;
    explicit Slots(unsigned seed) : rng(seed) {}
    float U() { return std::uniform_real_distribution<float>(-1.0f, 1.0f)(rng); }
    size_t n() const { return pq.size(); }
    void common() {
        flags.push_back((rng() & 0x7u) | ((rng() & 0xFFFu) << 16));   // bit 0 (LAST) among them: the builders clear it
        mesh.push_back((uint32_t)(rng() % 9u));
    }
    void tri() {
        const float c[3] = {U(), U(), U()};
        for (int v = 0; v < 3; v++) { for (int k = 0; k < 3; k++) P.push_back(c[k] + 0.05f * U()); idx.push_back((uint32_t)(P.size() / 3 - 1)); }
        pq.push_back(0u); common();
    }
    void quad(const float* c, const float* half) {
        for (int k = 0; k < 3; k++) qb.push_back(c[k] - half[k]);
        for (int k = 0; k < 3; k++) qb.push_back(c[k] + half[k]);
        for (int k = 0; k < 3; k++) idx.push_back(0u);
        pq.push_back((uint32_t)(qb.size() / 6)); common();
    }
    void quad() { const float c[3] = {U(), U(), U()}, h[3] = {0.16f + 0.15f * U(), 0.16f + 0.15f * U(), 0.16f + 0.15f * U()}; quad(c, h); }
};

enum Kind { QUADRICS_ONLY, FIRST_AND_LAST, SAME_CENTROID, INTERLEAVED, MIXED };

static void fill(Slots& s, Kind kind, size_t n) {
    switch (kind) {
    case QUADRICS_ONLY: for (size_t i = 0; i < n; i++) s.quad(); break;
    case FIRST_AND_LAST: s.quad(); for (size_t i = 0; i + 3 < n; i++) { if (i == n / 2) s.quad(); s.tri(); } s.quad(); break;   // n - 3 triangles, a quadric before, among and after them
    case SAME_CENTROID: {   // powers of two around one centre: every centroid is exactly the centre, the centroid bounds are a point
        const float c[3] = {0.25f, -0.5f, 0.125f};
        for (size_t i = 0; i < n; i++) { const float h[3] = {0.125f * (float)(1 + i), 0.25f, 0.5f / (float)(1u << (i % 4))}; s.quad(c, h); }
        break;
    }
    case INTERLEAVED: for (size_t i = 0; i < n; i++) { if (i & 1) s.quad(); else s.tri(); } break;
    case MIXED: for (size_t i = 0; i < n; i++) { if (s.rng() % 10u < 3u) s.quad(); else s.tri(); } break;
    }
}

// forest: the first third of the slots is the scene's own list (kind decides what they hold), the rest two object definitions of triangles, instanced twice and once
static int run(const char* name, Kind kind, size_t n, unsigned seed, int max_prims, bool forest) {
    Slots s(seed);
    const size_t n_top = forest ? n / 3 : n;
    fill(s, kind, n_top);
    for (size_t i = n_top; i < n; i++) s.tri();
    const bool no_tri = s.P.empty();
    phost::BuildInput in{};
    in.P = no_tri ? nullptr : s.P.data(); in.idx = s.idx.data(); in.n_tris = n; in.tri_flags = s.flags.data(); in.tri_mesh = s.mesh.data();
    in.prim_quadric = s.pq.data(); in.quad_bounds = s.qb.data(); in.n_quadrics = s.qb.size() / 6;
    phost::BuildOutput want;
    std::vector<uint32_t> tri0, tri1, inst_object, top_items; std::vector<float> inst_i2w;
    phost::ForestLayout layout; std::vector<phost::ForestTreeOut> want_trees;
    phost::InstancedScene isc{};
    if (forest) {
        for (size_t t = 0; t < n_top; t++) top_items.push_back((uint32_t)t);
        const size_t cut = n <= 9 ? n - 1 : n_top + (n - n_top) / 2;   // the smallest forest has an object of one triangle
        tri0 = {(uint32_t)n_top, (uint32_t)cut}; tri1 = {(uint32_t)cut, (uint32_t)n};
        for (uint32_t ob : {0u, 1u, 0u}) {
            float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) m[4 * r + q] = (r == q ? 0.5f : 0.0f) + 0.3f * s.U(); m[4 * r + 3] = s.U(); }
            inst_object.push_back(ob); inst_i2w.insert(inst_i2w.end(), m, m + 16);
            top_items.insert(top_items.begin() + (long)(s.rng() % (top_items.size() + 1)), PH_ITEM_INST | (uint32_t)(inst_object.size() - 1));
        }
        isc = phost::InstancedScene{tri0.data(), tri1.data(), tri0.size(), inst_object.data(), inst_i2w.data(), inst_object.size(), top_items.data(), top_items.size()};
        phost::forest_layout(isc, layout);
        if (phost::build_forest_host(in, isc, layout, 0, max_prims, want, want_trees) != 0) { std::printf("%s: host forest build failed\n", name); return 1; }
    } else if (phost::build_bvh(in, 0, max_prims, 1, want) != 0) { std::printf("%s: host build failed\n", name); return 1; }

    const uint32_t N = (uint32_t)(forest ? layout.items.size() : n);
    const uint32_t n_trees = forest ? (uint32_t)layout.tree_start.size() - 1u : 1u;
    const uint32_t one_tree[2] = {0u, N};
    std::vector<uint32_t> root_words(12 * (size_t)n_trees); std::vector<float> ibounds(6 * inst_object.size() + 1);
    std::vector<Elem> e_lo(N), e_hi(N); std::vector<uint32_t> seg(N), scan(N + 1), lf(N), lb(N), leaf_last(N, 0u), counters(16, 0u); std::vector<uint8_t> bkt(N);
    std::vector<SNode> nodes(2 * (size_t)N + 2); std::vector<uint32_t> scratch; std::vector<Node64> out_nodes(N); std::vector<TriRec> out_tris(N);
    Ctx c{};
    c.n = N; c.max_prims = (uint32_t)(max_prims & 0xff); c.P = in.P; c.idx = s.idx.data(); c.tri_flags = s.flags.data(); c.tri_mesh = s.mesh.data();
    c.prim_quadric = s.pq.data(); c.quad_bounds = s.qb.data();
    c.e_lo = e_lo.data(); c.e_hi = e_hi.data(); c.seg = seg.data(); c.bkt = bkt.data(); c.nodes = nodes.data(); c.counters = counters.data();
    c.scan = scan.data(); c.lf = lf.data(); c.lb = lb.data(); c.leaf_last = leaf_last.data(); c.out_nodes = out_nodes.data(); c.out_tris = out_tris.data();
    c.items = forest ? layout.items.data() : nullptr; c.inst_bounds = ibounds.data(); c.tree_start = forest ? layout.tree_start.data() : one_tree; c.n_trees = n_trees; c.root_words = root_words.data();
    for (uint32_t t = 0; t < n_trees; t++) init_bounds_words(c.root_words + 12 * t);
    const uint32_t top_end = forest ? layout.tree_start[1] : 0u;
    for (uint32_t i = top_end; i < N; i++) { const uint32_t t = tree_of(c, i); init_elem(c, i, t, c.root_words + 12 * t); }   // the objects first: the instances' bounds come from their roots
    for (size_t k = 0; k < inst_object.size(); k++) {
        const uint32_t t = layout.inst_tree[k];
        float lo[3], hi[3];
        for (int q = 0; q < 3; q++) { lo[q] = ord2f(root_words[12 * t + q]); hi[q] = ord2f(root_words[12 * t + 3 + q]); }
        phost::transform_bounds(&inst_i2w[16 * k], lo, hi, &ibounds[6 * k]);
    }
    for (uint32_t i = 0; i < top_end; i++) init_elem(c, i, 0u, c.root_words);
    for (uint32_t t = 0; t < n_trees; t++) make_root(c, t);
    std::vector<std::pair<uint32_t, uint32_t>> levels;
    uint32_t lb0 = 0, le0 = n_trees; int depth = 0;
    while (lb0 < le0) {
        levels.push_back({lb0, le0});
        c.counters[1] = 0;
        for (uint32_t v = lb0; v < le0; v++) decide_node(c, v);
        const uint32_t slots = c.counters[1];
        if (slots) {
            scratch.resize((size_t)slots * PHS_SLOT);
            for (size_t w = 0; w < scratch.size(); w++) scratch[w] = scratch_init_word((uint32_t)(w % PHS_SLOT));
            c.scratch = scratch.data();
            for (uint32_t i = 0; i < N; i++) bucket_elem(c, i, nullptr);
            for (uint32_t v = lb0; v < le0; v++) eval_node(c, v);
            uint32_t run = 0;
            for (uint32_t i = 0; i < N; i++) { scan[i] = run; run += flag_of(c, i); }
            scan[N] = run;
            for (uint32_t i = 0; i < N; i++) list_elem(c, i);
            for (uint32_t i = 0; i < N; i++) swap_pos(c, i);
        }
        for (uint32_t i = 0; i < N; i++) relabel_pos(c, i);
        if (c.counters[0] > le0) depth = (int)levels.size();
        lb0 = le0; le0 = c.counters[0];
    }
    for (size_t L = levels.size(); L-- > 0;) for (uint32_t v = levels[L].first; v < levels[L].second; v++) size_node(c, v);
    uint32_t interior = 0;
    for (uint32_t t = 0; t < n_trees; t++) { root_numbers(c, t, interior); interior += nodes[t].size; }
    for (size_t L = 0; L < levels.size(); L++) for (uint32_t v = levels[L].first; v < levels[L].second; v++) number_node(c, v);
    for (uint32_t i = 0; i < N; i++) emit_tri(c, i);

    int bad = 0;
    if (want.tris.size() != N || want.nodes.size() != interior) { std::printf("%s: sizes differ: records %u/%zu nodes %u/%zu\n", name, N, want.tris.size(), interior, want.nodes.size()); return 1; }
    if (interior != want.interior_nodes || c.counters[2] != want.leaf_nodes || c.counters[3] != want.max_leaf_prims || depth != want.max_depth) {
        std::printf("%s: statistics differ: interior %u/%zu leaves %u/%zu maxleaf %u/%zu depth %d/%d\n", name, interior, want.interior_nodes, c.counters[2], want.leaf_nodes, c.counters[3], want.max_leaf_prims, depth, want.max_depth);
        bad++;
    }
    uint32_t n_quadric_records = 0, n_last = 0;
    for (uint32_t i = 0; i < N; i++) {
        if (out_tris[i].flags & PH_TRI_QUADRIC) n_quadric_records++;
        if (out_tris[i].flags & PH_TRI_LAST) n_last++;
        if (std::memcmp(&out_tris[i], &want.tris[i], sizeof(TriRec)) != 0 && bad < 5) {
            std::printf("%s: record %u differs: prim %u/%u flags %x/%x mesh %u/%u\n", name, i, out_tris[i].prim, want.tris[i].prim, out_tris[i].flags, want.tris[i].flags, out_tris[i].mesh, want.tris[i].mesh);
            bad++;
        }
    }
    if (n_quadric_records != in.n_quadrics) { std::printf("%s: %u quadric records for %zu quadrics\n", name, n_quadric_records, in.n_quadrics); bad++; }
    if (n_last != c.counters[2]) { std::printf("%s: %u leaf ends for %u leaves\n", name, n_last, c.counters[2]); bad++; }
    for (uint32_t v = 0; v < interior && bad < 5; v++) {
        const Node64 &a = out_nodes[v], &b = want.nodes[v];
        const float* fa = a.x0; const float* fb = b.x0;
        bool same = a.c0 == b.c0 && a.c1 == b.c1 && a.axis == b.axis;
        for (int k = 0; k < 12; k++) same = same && fa[k] == fb[k];   // (== : but for the sign of a zero, bvh_sah_steps.h)
        if (!same) { std::printf("%s: node %u differs (c0 %x/%x c1 %x/%x axis %u/%u)\n", name, v, a.c0, b.c0, a.c1, b.c1, a.axis, b.axis); bad++; }
    }
    for (int k = 0; k < 3; k++) if (nodes[0].lo[k] != want.root_lo[k] || nodes[0].hi[k] != want.root_hi[k]) { std::printf("%s: root bound differs\n", name); bad++; }
    const uint32_t want_root = nodes[0].size ? 0u : (PH_LEAF_BIT | 0u);
    if (want.root_ref != want_root) { std::printf("%s: root reference %x/%x\n", name, want_root, want.root_ref); bad++; }
    uint32_t base = 0;
    for (uint32_t t = 0; forest && t < n_trees; t++) {   // every tree's root as the instance records will name it
        const uint32_t ref = nodes[t].size ? base : (PH_LEAF_BIT | layout.tree_start[t]);
        base += nodes[t].size;
        bool same = ref == want_trees[t].root_ref;
        for (int k = 0; k < 3; k++) same = same && nodes[t].lo[k] == want_trees[t].lo[k] && nodes[t].hi[k] == want_trees[t].hi[k];
        if (!same) { std::printf("%s: tree %u: root %x/%x or its bound differs\n", name, t, ref, want_trees[t].root_ref); bad++; }
    }
    if (bad) std::printf("%s (max_prims %d): %d differences\n", name, max_prims, bad);
    return bad;
}

int main() {
    struct Case { const char* name; Kind kind; size_t n; bool forest; };
    const Case cases[] = {
        {"one quadric: the root is a leaf, no vertex at all", QUADRICS_ONLY, 1, false},
        {"two quadrics", QUADRICS_ONLY, 2, false},
        {"six quadrics", QUADRICS_ONLY, 6, false},
        {"quadrics first and last among 40 triangles", FIRST_AND_LAST, 43, false},
        {"five quadrics with one centroid", SAME_CENTROID, 5, false},
        {"300 triangles + 300 quadrics interleaved", INTERLEAVED, 600, false},
        {"5000 mixed", MIXED, 5000, false},
        {"forest of 9 items", INTERLEAVED, 9, true},
        {"forest of 300 items", INTERLEAVED, 300, true},
        {"forest of 5000 items", MIXED, 5000, true},
        {"forest whose scene tree holds quadrics with one centroid", SAME_CENTROID, 15, true},
    };
    int bad = 0, n_cases = 0;
    for (const Case& cs : cases)
        for (int mp : {1, 4, 255}) { bad += run(cs.name, cs.kind, cs.n, 7919u * (unsigned)cs.n + 13u, mp, cs.forest); n_cases++; }
    std::printf("%d cases, %d differences\n", n_cases, bad);
    return bad ? 1 : 0;
}
