// Host-side set-up of the reference's Curve shape (shapes/src/curve.rs), in the reference's f32 expression order (compiled with -ffp-contract=off): plain C++, no HIP,
// so that scripts/curve_host_check.cpp can run it under the sanitizers.
//   curve_data           CurveData::new (:743-762)
//   segment_object_bound Curve::object_bound (:660-674) of the segment [u_min, u_max]
//   segment_range        the u range of segment i of Curve::create_segments (:117-132)
//   from_props_segments  the conversion half of Curve::from_props (:149-316): degree elevation, the b-spline blossoming, the per-segment widths
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "scene_types.h"

namespace pcurve {

inline float lerp(float t, float a, float b) { return (1.0f - t) * a + t * b; }   // common.rs:167-173
inline float pmax(float a, float b) { return a > b ? a : b; }
inline float pmin(float a, float b) { return a < b ? a : b; }
struct P3 { float x, y, z; };
inline P3 lerp3(float t, P3 a, P3 b) { return {(1.0f - t) * a.x + t * b.x, (1.0f - t) * a.y + t * b.y, (1.0f - t) * a.z + t * b.z}; }
inline P3 ld(const float* p) { return {p[0], p[1], p[2]}; }

// CurveData::new: the normals normalised (zero without any), normal_angle = acos(clamp(n0 . n1, 0, 1)), inv_sin_normal_angle = 1 / sin(normal_angle); acos and sin in f64, rounded once
inline void curve_data(int type, const float cp[12], const float width[2], const float* n /* 6 or null */, CurveRec& c) {
    c = CurveRec{};
    for (int k = 0; k < 12; k++) c.cp[k] = cp[k];
    c.width[0] = width[0]; c.width[1] = width[1];
    c.type = (uint32_t)type;
    if (n) {
        for (int e = 0; e < 2; e++) {
            const float* v = n + 3 * e;
            const float inv = 1.0f / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);   // Normal3::normalize: n / length, as a product with the inverse (normal.rs:73-78, :286-291)
            c.n[3 * e] = inv * v[0]; c.n[3 * e + 1] = inv * v[1]; c.n[3 * e + 2] = inv * v[2];
        }
    }
    const float d = c.n[0] * c.n[3] + c.n[1] * c.n[4] + c.n[2] * c.n[5];
    const float cl = d < 0.0f ? 0.0f : (d > 1.0f ? 1.0f : d);
    c.normal_angle = (float)std::acos((double)cl);
    c.inv_sin_normal_angle = 1.0f / (float)std::sin((double)c.normal_angle);
}

inline P3 blossom(const float* p, float u0, float u1, float u2) {   // blossom_bezier (:771-775)
    const P3 a0 = lerp3(u0, ld(p), ld(p + 3)), a1 = lerp3(u0, ld(p + 3), ld(p + 6)), a2 = lerp3(u0, ld(p + 6), ld(p + 9));
    const P3 b0 = lerp3(u1, a0, a1), b1 = lerp3(u1, a1, a2);
    return lerp3(u2, b0, b1);
}
inline void segment_range(int i, int split_depth, float& u_min, float& u_max) {
    const float f = 1.0f / (float)(1u << split_depth);
    u_min = (float)i * f; u_max = (float)(i + 1) * f;
}
// the union of the boxes of blossomed points (0, 1) and (2, 3), expanded by half the larger end width of the segment
inline void segment_object_bound(const CurveRec& c, float u_min, float u_max, float lo[3], float hi[3]) {
    const P3 q[4] = {blossom(c.cp, u_min, u_min, u_min), blossom(c.cp, u_min, u_min, u_max), blossom(c.cp, u_min, u_max, u_max), blossom(c.cp, u_max, u_max, u_max)};
    const float w0 = lerp(u_min, c.width[0], c.width[1]), w1 = lerp(u_max, c.width[0], c.width[1]);
    const float delta = pmax(w0, w1) * 0.5f;
    const float a[4][3] = {{q[0].x, q[0].y, q[0].z}, {q[1].x, q[1].y, q[1].z}, {q[2].x, q[2].y, q[2].z}, {q[3].x, q[3].y, q[3].z}};
    for (int k = 0; k < 3; k++) {
        const float lo01 = pmin(a[0][k], a[1][k]), hi01 = pmax(a[0][k], a[1][k]), lo23 = pmin(a[2][k], a[3][k]), hi23 = pmax(a[2][k], a[3][k]);
        lo[k] = pmin(lo01, lo23) - delta; hi[k] = pmax(hi01, hi23) + delta;
    }
}

// One cubic Bezier segment of a Shape "curve": what Curve::from_props hands Curve::create_segments
struct PropSegment { float cp[12]; float width[2]; };
// The conversion loop of Curve::from_props (:231-314).  degree 2 or 3, bspline or bezier, n_cp control points (3 floats each).  An empty string = fine; else the reference's panic as one sentence.
inline std::string from_props_segments(int degree, bool bspline, const float* P, size_t n_cp, float width0, float width1, std::vector<PropSegment>& out) {
    out.clear();
    if (degree != 2 && degree != 3) return "Invalid degree " + std::to_string(degree) + ": only degree 2 and 3 curves are supported.";
    const size_t deg = (size_t)degree;
    size_t n_segments;
    if (!bspline) {
        if (n_cp < deg + 1 || ((n_cp - 1 - deg) % deg) != 0)
            return "Invalid number of control points " + std::to_string(n_cp) + ": for the degree " + std::to_string(degree) + " Bezier basis " + std::to_string(degree + 1) + " + n * " +
                   std::to_string(degree) + " are required, for n >= 0.";
        n_segments = (n_cp - 1) / deg;
    } else {
        if (n_cp < deg + 1)
            return "Invalid number of control points " + std::to_string(n_cp) + ": for the degree " + std::to_string(degree) + " b-spline basis, must have >= " + std::to_string(degree + 1) + ".";
        n_segments = n_cp - deg;
    }
    size_t cp_base = 0;
    auto at = [&](size_t i) { return ld(P + 3 * (cp_base + i)); };
    for (size_t seg = 0; seg < n_segments; seg++) {
        P3 b[4];
        if (!bspline) {
            if (degree == 2) { b[0] = at(0); b[1] = lerp3(2.0f / 3.0f, at(0), at(1)); b[2] = lerp3(1.0f / 3.0f, at(1), at(2)); b[3] = at(2); }
            else for (int i = 0; i < 4; i++) b[i] = at((size_t)i);
            cp_base += deg;
        } else {
            if (degree == 2) {
                const P3 p01 = at(0), p12 = at(1), p23 = at(2);
                const P3 p11 = lerp3(0.5f, p01, p12), p22 = lerp3(0.5f, p12, p23);
                b[0] = p11; b[1] = lerp3(2.0f / 3.0f, p11, p12); b[2] = lerp3(1.0f / 3.0f, p12, p22); b[3] = p22;
            } else {
                const P3 p012 = at(0), p123 = at(1), p234 = at(2), p345 = at(3);
                const P3 p122 = lerp3(2.0f / 3.0f, p012, p123), p223 = lerp3(1.0f / 3.0f, p123, p234), p233 = lerp3(2.0f / 3.0f, p123, p234), p334 = lerp3(1.0f / 3.0f, p234, p345);
                b[0] = lerp3(0.5f, p122, p223); b[1] = p223; b[2] = p233; b[3] = lerp3(0.5f, p233, p334);
            }
            cp_base += 1;
        }
        PropSegment s;
        for (int i = 0; i < 4; i++) { s.cp[3 * i] = b[i].x; s.cp[3 * i + 1] = b[i].y; s.cp[3 * i + 2] = b[i].z; }
        s.width[0] = lerp((float)seg / (float)n_segments, width0, width1);
        s.width[1] = lerp((float)(seg + 1) / (float)n_segments, width0, width1);
        out.push_back(s);
    }
    return std::string();
}

}  // namespace pcurve
