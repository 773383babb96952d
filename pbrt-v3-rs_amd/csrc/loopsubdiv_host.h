// The host's share of LoopSubDiv::subdivide (shapes/src/loopsubdiv.rs:321-400): the control mesh's face, vertex and neighbour pointers, each vertex's boundary / regular
// flags, the refusals, the level counts, and the table of cos / sin the normal pass reads (:605-607, :624-628).  Plain C++, no HIP: the library (loopsubdiv.hip), the front
// end (its --check calls nothing in the library) and the stand-alone checker (scripts/loopsubdiv_host_check.cpp) all include it.
//
// What the reference leaves to a panic, or to a walk that would not end, is refused here with one sentence, before anything is built:
//   no indices / no P (from_props, :674-679) · an index >= n_verts · a face with a repeated vertex · a vertex no face uses (:377-382) · an edge in more than two faces ·
//   an edge its two faces run through in the same direction · n_levels < 0 · final counts beyond 32-bit indices.
// With those gone every ring walk ends: across an edge (v, next) the neighbour holds it as (next, v), so next_face and prev_face around v are inverse to each other and a walk
// either returns to its start or meets -1.  A vertex whose faces form several fans (a bow-tie) is accepted as the reference accepts it: its ring is its start_face's fan.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace ploop {

enum : uint32_t { V_BOUNDARY = 1u, V_REGULAR = 2u };   // per-vertex flag word (SDVertex::boundary, ::regular)

inline int next3(int i) { return (i + 1) % 3; }   // next / prev (:759-768)
inline int prev3(int i) { return (i + 2) % 3; }

struct Control {
    uint32_t n_verts = 0, n_faces = 0;
    uint64_t n_edges = 0;
    std::vector<int32_t> fv, ff;        // 3 per face: SDFace::v, SDFace::f (-1: no neighbour)
    std::vector<int32_t> start_face;    // per vertex: the LAST face that names it (:343-344)
    std::vector<uint32_t> vflags;       // per vertex: V_BOUNDARY | V_REGULAR (:391-399)
    std::vector<uint32_t> valence;      // per vertex: SDVertex::valence (:52-87)
    uint32_t max_valence = 0;           // valence never grows under refinement: a new edge vertex has 6 inside, 4 on the boundary
    // trig[]: for an interior valence n that occurs (and for 6, the valence of every new interior vertex) 2 n floats at interior_off[n]: cos, sin of TWO_PI * j / n, j = 0..n-1;
    // for a boundary valence n > 4 that occurs n floats at boundary_off[n]: sin(theta), cos(theta), then sin(k * theta), k = 1..n-2, theta = PI / (n - 1).  -1: not in the table
    std::vector<float> trig;
    std::vector<int32_t> interior_off, boundary_off;   // max_valence + 1 entries each (at least 7)
    uint64_t out_verts = 0, out_faces = 0;             // V_L, F 4^L
};

inline int vnum(const int32_t* v, int32_t vert) { return v[0] == vert ? 0 : v[1] == vert ? 1 : v[2] == vert ? 2 : -1; }   // SDFace::vnum (:232-239)

// SDVertex::valence (:52-87) on the arrays above
inline uint32_t valence_of(const Control& c, int32_t vi, bool boundary) {
    const int32_t start = c.start_face[vi];
    int32_t f = start;
    uint32_t nf = 1;
    if (!boundary) {
        while (f != -1) {
            f = c.ff[3 * f + vnum(&c.fv[3 * f], vi)];
            if (f == start) break;
            nf++;
        }
        return nf;
    }
    while (f != -1) {
        f = c.ff[3 * f + vnum(&c.fv[3 * f], vi)];
        if (f != -1) nf++; else break;
    }
    f = start;
    while (f != -1) {
        f = c.ff[3 * f + prev3(vnum(&c.fv[3 * f], vi))];
        if (f != -1) nf++; else break;
    }
    return nf + 1;
}

// V' = V + E, E' = 2E + 3F, F' = 4F, n_levels times; false when a count leaves what the library indexes with.  The kernels (loopsubdiv.hip) form 3 * vertex and 3 * face
// in signed 32-bit arithmetic, as the scene's own arrays do, so every level's V and F — and with them the 3 F face-edges the scan runs over and the V + E of the next
// level — stay at or below kMaxCount = 0x7FFFFFFF / 3
constexpr uint64_t kMaxCount = 0x7FFFFFFFull / 3ull;
inline bool level_counts(uint64_t v, uint64_t e, uint64_t f, int n_levels, uint64_t& out_v, uint64_t& out_f) {
    if (v > kMaxCount || f > kMaxCount) return false;
    for (int l = 0; l < n_levels; l++) {
        const uint64_t nv = v + e, ne = 2 * e + 3 * f, nf = 4 * f;
        v = nv; e = ne; f = nf;
        if (v > kMaxCount || f > kMaxCount) return false;   // (e < 3 f + v bounds the edges along with them; nothing indexes by edge)
    }
    out_v = v; out_f = f;
    return true;
}

// The cos / sin table in f32, with the arguments computed as the reference's lines compute them; cosf / sinf are what its f32::cos / f32::sin call
inline void build_trig(Control& c) {
    const float kPi = 3.14159265358979323846f, kTwoPi = kPi * 2.0f;   // PI, TWO_PI (core/src/pbrt/common.rs:22,34)
    const uint32_t top = c.max_valence < 6u ? 6u : c.max_valence;
    std::vector<uint8_t> inner(top + 1, 0), bound(top + 1, 0);
    inner[6] = 1;
    for (uint32_t i = 0; i < c.n_verts; i++) ((c.vflags[i] & V_BOUNDARY) ? bound : inner)[c.valence[i]] = 1;
    c.interior_off.assign(top + 1, -1); c.boundary_off.assign(top + 1, -1);
    c.trig.clear();
    for (uint32_t n = 1; n <= top; n++) {
        if (inner[n]) {
            c.interior_off[n] = (int32_t)c.trig.size();
            for (uint32_t j = 0; j < n; j++) {
                const float theta = kTwoPi * (float)j / (float)n;   // :605
                c.trig.push_back(cosf(theta)); c.trig.push_back(sinf(theta));
            }
        }
        if (bound[n] && n > 4u) {
            c.boundary_off[n] = (int32_t)c.trig.size();
            const float theta = kPi / (float)(n - 1u);              // :624
            c.trig.push_back(sinf(theta)); c.trig.push_back(cosf(theta));
            for (uint32_t k = 1; k + 1 < n; k++) c.trig.push_back(sinf((float)k * theta));   // :627
        }
    }
}

// Builds `c` from the control mesh; returns "" or the one sentence of the refusal (c is then unspecified).  P is looked at only for being there.
inline std::string build_control(const float* P, uint64_t n_verts, const uint32_t* indices, uint64_t n_indices, int n_levels, Control& c) {
    if (!indices || n_indices == 0) return "Vertex indices 'indices' not provided for LoopSubDiv shape.";
    if (!P || n_verts == 0) return "Vertex positions 'P' not provided for LoopSubDiv shape.";
    if (n_levels < 0) return "nlevels " + std::to_string(n_levels) + " is negative.";
    const uint64_t n_faces = n_indices / 3;   // indices beyond the last multiple of 3 are ignored (:332)
    if (n_faces == 0) return "Vertex indices 'indices' name no whole face (" + std::to_string(n_indices) + " given, 3 make a face).";
    if (n_verts > kMaxCount || n_faces > kMaxCount) return "The control mesh does not fit 32-bit indices.";
    for (uint64_t i = 0; i < 3 * n_faces; i++)
        if (indices[i] >= n_verts) return "Vertex index " + std::to_string(indices[i]) + " is out of bounds (" + std::to_string(n_verts) + " vertices).";
    c = Control();
    c.n_verts = (uint32_t)n_verts; c.n_faces = (uint32_t)n_faces;
    c.fv.resize(3 * n_faces); c.ff.assign(3 * n_faces, -1);
    c.start_face.assign(n_verts, -1);
    // face to vertex pointers; start_face ends up the last face that names the vertex (:335-346)
    for (uint64_t i = 0; i < n_faces; i++) {
        const uint32_t a = indices[3 * i], b = indices[3 * i + 1], d = indices[3 * i + 2];
        if (a == b || b == d || a == d) return "Face " + std::to_string(i) + " names a vertex twice.";
        for (int j = 0; j < 3; j++) { c.fv[3 * i + j] = (int32_t)indices[3 * i + j]; c.start_face[indices[3 * i + j]] = (int32_t)i; }
    }
    for (uint64_t i = 0; i < n_verts; i++)
        if (c.start_face[i] == -1) return "Start face for vertex " + std::to_string(i) + " is not set. Check input mesh to ensure all vertices used.";
    // neighbour pointers (:348-370): the first face that meets an edge in (face, edge) order owns it; the second closes it
    struct Seen { int32_t face; int32_t edge; uint32_t count; };
    std::unordered_map<uint64_t, Seen> edges;
    edges.reserve(3 * n_faces);
    for (uint64_t i = 0; i < n_faces; i++)
        for (int k = 0; k < 3; k++) {
            const uint32_t v0 = (uint32_t)c.fv[3 * i + k], v1 = (uint32_t)c.fv[3 * i + next3(k)];
            const uint32_t lo = v0 < v1 ? v0 : v1, hi = v0 < v1 ? v1 : v0;
            const uint64_t key = ((uint64_t)lo << 32) | hi;
            auto it = edges.find(key);
            if (it == edges.end()) { edges.emplace(key, Seen{(int32_t)i, k, 1u}); continue; }
            Seen& e = it->second;
            if (e.count >= 2u) return "The edge between vertices " + std::to_string(lo) + " and " + std::to_string(hi) + " is in more than two faces.";
            if (c.fv[3 * e.face + e.edge] == (int32_t)v0)
                return "Faces " + std::to_string(e.face) + " and " + std::to_string(i) + " run through the edge between vertices " + std::to_string(lo) + " and " + std::to_string(hi) + " in the same direction.";
            e.count = 2u;
            c.ff[3 * e.face + e.edge] = (int32_t)i;
            c.ff[3 * i + k] = e.face;
        }
    c.n_edges = edges.size();
    if (!level_counts(n_verts, c.n_edges, n_faces, n_levels, c.out_verts, c.out_faces))
        return "The mesh after " + std::to_string(n_levels) + " levels does not fit 32-bit indices.";
    // boundary / regular (:372-400)
    c.vflags.assign(n_verts, 0u); c.valence.assign(n_verts, 0u);
    for (uint64_t i = 0; i < n_verts; i++) {
        const int32_t start = c.start_face[i];
        int32_t f = start;
        do { f = c.ff[3 * f + vnum(&c.fv[3 * f], (int32_t)i)]; } while (f != -1 && f != start);
        const bool boundary = f == -1;
        // the reference takes the valence for `regular` while `boundary` is still false (:391-392): at a boundary vertex that counts the faces from start_face on, plus one.
        // Nothing reads a boundary vertex's `regular`, and the interior's 1/16 equals beta(6) bit for bit, so the flag is kept only to be the reference's
        const uint32_t val_reg = valence_of(c, (int32_t)i, false);
        const uint32_t val = boundary ? valence_of(c, (int32_t)i, true) : val_reg;
        c.valence[i] = val;
        c.vflags[i] = (boundary ? V_BOUNDARY : 0u) | (((!boundary && val_reg == 6u) || (boundary && val_reg == 4u)) ? V_REGULAR : 0u);
        if (val > c.max_valence) c.max_valence = val;
    }
    build_trig(c);
    return "";
}

}  // namespace ploop
