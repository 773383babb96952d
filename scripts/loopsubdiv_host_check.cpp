// Stand-alone run of pbrt-v3-rs_amd/csrc/loopsubdiv_host.h (the host's share of Shape "loopsubdiv"), built under the address and undefined-behaviour sanitizers by
// scripts/loopsubdiv_host_check.sh.  CPU only.
//   loopsubdiv_host_check MESH...   each file: "n_verts n_indices n_levels" and the indices.  Prints the control mesh's arrays, the level counts and the cos / sin table
//                                   (as the bits of each f32) for tests/test_loopsubdiv_host_cpu.py to compare with the NumPy restatement's.
//   loopsubdiv_host_check           runs every refusal and prints its sentence.
#include "../pbrt-v3-rs_amd/csrc/loopsubdiv_host.h"
#include <cstdio>
#include <cstring>
#include <fstream>

static void print_ints(const char* name, const std::vector<int32_t>& v) {
    std::printf("%s", name);
    for (int32_t x : v) std::printf(" %d", x);
    std::printf("\n");
}

static int dump(const char* path) {
    std::ifstream in(path);
    unsigned long long nv = 0, ni = 0; int levels = 0;
    if (!(in >> nv >> ni >> levels)) { std::printf("cannot read %s\n", path); return 1; }
    std::vector<uint32_t> idx(ni);
    for (auto& x : idx) if (!(in >> x)) { std::printf("short file %s\n", path); return 1; }
    std::vector<float> P(3 * (nv ? nv : 1), 0.0f);
    ploop::Control c;
    const std::string bad = ploop::build_control(P.data(), nv, idx.data(), ni, levels, c);
    std::printf("mesh %s\n", path);
    if (!bad.empty()) { std::printf("refused %s\n", bad.c_str()); return 0; }
    print_ints("fv", c.fv); print_ints("ff", c.ff); print_ints("start_face", c.start_face);
    std::vector<int32_t> b, r, val;
    for (uint32_t i = 0; i < c.n_verts; i++) { b.push_back((c.vflags[i] & ploop::V_BOUNDARY) ? 1 : 0); r.push_back((c.vflags[i] & ploop::V_REGULAR) ? 1 : 0); val.push_back((int32_t)c.valence[i]); }
    print_ints("boundary", b); print_ints("regular", r); print_ints("valence", val);
    std::printf("counts %llu %llu %llu %llu %u\n", (unsigned long long)c.n_edges, (unsigned long long)c.out_verts, (unsigned long long)c.out_faces, (unsigned long long)c.trig.size(), c.max_valence);
    for (size_t n = 0; n < c.interior_off.size(); n++)
        for (int side = 0; side < 2; side++) {
            const int32_t off = side ? c.boundary_off[n] : c.interior_off[n];
            if (off < 0) continue;
            const size_t len = side ? n : 2 * n;
            if ((size_t)off + len > c.trig.size()) { std::printf("table entry out of range\n"); return 1; }
            std::printf("%s %zu", side ? "trig_boundary" : "trig_interior", n);
            for (size_t k = 0; k < len; k++) { uint32_t u; std::memcpy(&u, &c.trig[off + k], 4); std::printf(" %08x", u); }
            std::printf("\n");
        }
    return 0;
}

static int failures = 0;
static void refusal(const char* name, const float* P, uint64_t nv, const std::vector<uint32_t>& idx, int levels, const char* must_contain) {
    ploop::Control c;
    const std::string bad = ploop::build_control(P, nv, idx.empty() ? nullptr : idx.data(), idx.size(), levels, c);
    const bool ok = !bad.empty() && bad.find(must_contain) != std::string::npos && bad.find('\n') == std::string::npos;
    std::printf("refusal %s: %s%s\n", name, bad.c_str(), ok ? "" : "   <-- WRONG");
    if (!ok) failures++;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int i = 1; i < argc; i++) if (dump(argv[i])) return 1;
        std::printf("loopsubdiv_host_check: ok\n");
        return 0;
    }
    const float P[3 * 8] = {0};
    refusal("no indices", P, 3, {}, 3, "Vertex indices 'indices' not provided for LoopSubDiv shape.");
    refusal("no P", nullptr, 0, {0, 1, 2}, 3, "Vertex positions 'P' not provided for LoopSubDiv shape.");
    refusal("index out of bounds", P, 3, {0, 1, 3}, 1, "Vertex index 3 is out of bounds");
    refusal("repeated vertex", P, 3, {0, 1, 1}, 1, "Face 0 names a vertex twice.");
    refusal("unused vertex", P, 4, {0, 1, 2}, 1, "Start face for vertex 3 is not set. Check input mesh to ensure all vertices used.");
    refusal("three faces on an edge", P, 5, {0, 1, 2, 1, 0, 3, 0, 1, 4}, 1, "is in more than two faces.");
    refusal("same direction", P, 4, {0, 1, 2, 0, 1, 3}, 1, "in the same direction.");
    refusal("negative levels", P, 3, {0, 1, 2}, -1, "nlevels -1 is negative.");
    refusal("counts beyond 32 bits", P, 3, {0, 1, 2}, 16, "does not fit 32-bit indices.");
    refusal("counts beyond 3 * index in an int", P, 4, {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2}, 14, "The mesh after 14 levels does not fit 32-bit indices.");
    refusal("fewer than three indices", P, 3, {0, 1}, 1, "name no whole face");
    {   // accepted: a bow-tie, and indices beyond the last multiple of 3
        ploop::Control c;
        const std::vector<uint32_t> bow = {0, 1, 2, 0, 3, 4, 9};
        const std::string bad = ploop::build_control(P, 5, bow.data(), bow.size(), 2, c);
        const bool ok = bad.empty() && c.n_faces == 2 && c.out_faces == 32 && c.start_face[0] == 1 && c.valence[0] == 2 && (c.vflags[0] & ploop::V_BOUNDARY);
        std::printf("accepted bow-tie: %s\n", ok ? "yes" : ("NO " + bad).c_str());
        if (!ok) failures++;
    }
    {   // the largest mesh accepted: every count times 3 still fits an int (the kernels' index arithmetic)
        ploop::Control c;
        const std::vector<uint32_t> tet = {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2};
        const std::string bad = ploop::build_control(P, 4, tet.data(), tet.size(), 13, c);
        const bool ok = bad.empty() && c.out_faces == 268435456ull && 3 * c.out_faces <= 0x7FFFFFFFull && 3 * c.out_verts <= 0x7FFFFFFFull;
        std::printf("accepted 13 levels: %s\n", ok ? "yes" : ("NO " + bad).c_str());
        if (!ok) failures++;
    }
    if (failures) { std::printf("%d WRONG\n", failures); return 1; }
    std::printf("loopsubdiv_host_check: ok\n");
    return 0;
}
