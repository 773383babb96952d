// CPU check of the device builders' input stage (pbrt-v3-rs_amd/csrc/device_build_input.h): check_device_build_input accepts one flat input and one forest (3 trees, 2 instances,
// one quadric slot in tree 0) and refuses each way of breaking them with -1 and a message; count_build_verts over a quadric-only, a mixed and a triangles-only input.
// Built with the address and undefined-behaviour sanitizers by device_build_input_check.sh, so a check that reads past an array it was meant to guard ends the program.
// Prints one line per case; exit status 1 on any unexpected answer.
#include "../pbrt-v3-rs_amd/csrc/device_build_input.h"
#include <cstdio>
#include <vector>

using namespace phost;

static int g_bad = 0;
static void expect(const char* what, bool ok, const std::string& detail = "") {
    std::printf("%s: %s%s%s\n", what, ok ? "ok" : "MISMATCH", detail.empty() ? "" : " - ", detail.c_str());
    if (!ok) g_bad++;
}
static void accepted(const char* what, const BuildInput& in, const ForestSpec* f) {
    std::string err;
    const int rc = check_device_build_input(in, f, err);
    expect(what, rc == 0 && err.empty(), "accepted" + (err.empty() ? std::string() : " but says: " + err));
}
static void refused(const char* what, const BuildInput& in, const ForestSpec* f) {
    std::string err;
    const int rc = check_device_build_input(in, f, err);
    expect(what, rc == -1 && !err.empty(), rc == -1 ? "refused: " + err : "answer " + std::to_string(rc));
}

int main() {
    // Seven primitive slots over five vertices.  Slots 0, 1: the scene's own triangles; slot 2: a quadric (index triple {0, 0, 0}); slots 3, 4: object A; slots 5, 6: object B.
    const std::vector<float> P(15, 0.0f);
    const std::vector<uint32_t> idx = {0, 1, 2, 1, 2, 3, 0, 0, 0, 2, 3, 4, 0, 2, 4, 1, 3, 4, 0, 1, 4};
    const std::vector<uint32_t> pq = {0, 0, 1, 0, 0, 0, 0};
    const std::vector<float> qb = {-1, -1, -1, 1, 1, 1};
    // the forest: tree 0 = {triangle 0, instance 0, the quadric, instance 1, triangle 1}, tree 1 = object A, tree 2 = object B
    const std::vector<uint32_t> items = {0, PH_ITEM_INST | 0u, 2, PH_ITEM_INST | 1u, 1, 3, 4, 5, 6};
    const std::vector<uint32_t> tree_start = {0, 5, 7, 9};
    const std::vector<uint32_t> inst_tree = {1, 2};
    const std::vector<float> i2w(32, 0.0f);

    BuildInput flat{P.data(), idx.data(), 7, nullptr};
    flat.prim_quadric = pq.data(); flat.quad_bounds = qb.data(); flat.n_quadrics = 1;
    const BuildInput in = flat;
    const ForestSpec forest{items.data(), items.size(), tree_start.data(), 3, inst_tree.data(), i2w.data(), 2};

    accepted("flat input", flat, nullptr);
    accepted("forest of 3 trees, 2 instances, a quadric in tree 0", in, &forest);
    { BuildInput e = flat; e.n_tris = 0; accepted("no primitive at all", e, nullptr); }

    { BuildInput b = flat; b.items = items.data(); b.n_items = items.size(); refused("items without a forest", b, nullptr); }
    { std::vector<uint32_t> ts = {0, 5, 5, 9}; ForestSpec f = forest; f.tree_start = ts.data(); refused("an empty tree range", in, &f); }
    { std::vector<uint32_t> ts = {0, 5, 7, 8}; ForestSpec f = forest; f.tree_start = ts.data(); refused("ranges that end before the items do", in, &f); }
    { std::vector<uint32_t> ts = {1, 5, 7, 9}; ForestSpec f = forest; f.tree_start = ts.data(); refused("ranges that begin behind the first item", in, &f); }
    { std::vector<uint32_t> it = items; it[6] = 7; ForestSpec f = forest; f.items = it.data(); refused("an item that names no triangle", in, &f); }
    { std::vector<uint32_t> it = items; it[1] = PH_ITEM_INST | 2u; ForestSpec f = forest; f.items = it.data(); refused("an item that names no instance", in, &f); }
    { std::vector<uint32_t> it = items; it[5] = PH_ITEM_INST | 0u; ForestSpec f = forest; f.items = it.data(); refused("an instance item outside tree 0", in, &f); }
    { std::vector<uint32_t> t = {0, 2}; ForestSpec f = forest; f.inst_tree = t.data(); refused("inst_tree equal to 0", in, &f); }
    { std::vector<uint32_t> t = {1, 3}; ForestSpec f = forest; f.inst_tree = t.data(); refused("inst_tree equal to n_trees", in, &f); }
    { ForestSpec f = forest; f.inst_tree = nullptr; refused("instances without their trees", in, &f); }
    { BuildInput b = in; b.quad_bounds = nullptr; refused("quadric slots without bounds (forest)", b, &forest); refused("quadric slots without bounds (flat)", b, nullptr); }
    { std::vector<uint32_t> q = pq; q[3] = 1; BuildInput b = in; b.prim_quadric = q.data(); refused("a quadric slot inside an object's tree", b, &forest); }
    { std::vector<uint32_t> q = pq; q[2] = 2; BuildInput b = in; b.prim_quadric = q.data(); refused("a slot that names no quadric (forest)", b, &forest); refused("a slot that names no quadric (flat)", b, nullptr); }

    // n_verts: a quadric slot's index triple stands for no vertex
    {
        const std::vector<uint32_t> only_q = {1, 2};
        const std::vector<uint32_t> idx_q = {0, 0, 0, 0, 0, 0};
        BuildInput q{nullptr, idx_q.data(), 2, nullptr};
        q.prim_quadric = only_q.data();
        expect("n_verts, quadrics only", count_build_verts(q) == 0, std::to_string(count_build_verts(q)));
        expect("n_verts, mixed", count_build_verts(flat) == 5, std::to_string(count_build_verts(flat)));
        const std::vector<uint32_t> idx_low = {0, 1, 2, 0, 0, 0, 1, 2, 3};   // the quadric in the middle, the highest vertex 3
        const std::vector<uint32_t> pq_low = {0, 1, 0};
        BuildInput m{P.data(), idx_low.data(), 3, nullptr};
        m.prim_quadric = pq_low.data();
        expect("n_verts, mixed, vertex 0 named by the quadric slot only", count_build_verts(m) == 4, std::to_string(count_build_verts(m)));
        BuildInput t{P.data(), idx.data(), 7, nullptr};
        expect("n_verts, triangles only", count_build_verts(t) == 5, std::to_string(count_build_verts(t)));
        const DeviceBuildItems a(flat, nullptr), b(in, &forest);
        expect("a flat input is one tree of its slots", a.n == 7 && a.n_trees == 1 && a.tree_start()[0] == 0 && a.tree_start()[1] == 7 && !a.items() && a.n_inst() == 0 && a.top_end() == 7);
        expect("a forest keeps its ranges", b.n == 9 && b.n_trees == 3 && b.tree_start() == tree_start.data() && b.items() == items.data() && b.n_inst() == 2 && b.top_end() == 5);
    }
    std::printf(g_bad ? "%d unexpected answers\n" : "all as expected\n", g_bad);
    return g_bad ? 1 : 0;
}
