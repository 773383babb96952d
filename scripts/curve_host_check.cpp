// The host-side set-up of the Curve shape (pbrt-v3-rs_amd/csrc/curve_host.h) on cases worked out by hand from shapes/src/curve.rs: CurveData::new (:743-762), the segment
// ranges of Curve::create_segments (:117-132), Curve::object_bound (:660-674) and the conversion loop of Curve::from_props (:231-314: degree elevation, b-spline
// blossoming, per-segment widths, the panics as sentences).  Needs neither the built library nor a device.  Prints one line per failure; the exit status is 1 if anything
// failed.  tests/test_curve_capi.py compiles it with -fsanitize=address,undefined and runs it:
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I pbrt-v3-rs_amd/csrc scripts/curve_host_check.cpp -o curve_host_check && ./curve_host_check
#include "curve_host.h"
#include <cstdio>

static int fails = 0;
static void near(const char* what, float got, double want, double tol = 1e-6) {
    if (!(std::fabs((double)got - want) <= tol)) { std::printf("FAIL %s: %.9g, expected %.9g\n", what, got, want); fails++; }
}
static void check(const char* what, bool ok) { if (!ok) { std::printf("FAIL %s\n", what); fails++; } }

int main() {
    const float cp[12] = {0, 0, 0, 1, 2, 0, 2, -1, 1, 3, 0, 0};
    const float width[2] = {0.2f, 0.6f};
    CurveRec c;
    pcurve::curve_data(PH_CURVE_FLAT, cp, width, nullptr, c);
    check("no normals: n = 0", c.n[0] == 0 && c.n[4] == 0 && c.type == PH_CURVE_FLAT);
    near("no normals: normal_angle = acos(0)", c.normal_angle, 1.5707963267948966);
    near("no normals: 1 / sin", c.inv_sin_normal_angle, 1.0);
    const float n[6] = {0, 0, 2, 0, 3, 3};
    pcurve::curve_data(PH_CURVE_RIBBON, cp, width, n, c);
    near("ribbon: n0 normalised", c.n[2], 1.0); near("ribbon: n1 normalised", c.n[4], 0.7071067811865476);
    near("ribbon: normal_angle", c.normal_angle, 0.7853981633974483); near("ribbon: 1 / sin", c.inv_sin_normal_angle, 1.4142135623730951, 1e-5);
    // the ranges: 2^split_depth equal parts, exact
    for (int sd = 0; sd <= 16; sd += 4) {
        const int k = 1 << sd;
        float a, b, a2, b2;
        pcurve::segment_range(0, sd, a, b); pcurve::segment_range(k - 1, sd, a2, b2);
        check("segment ranges start at 0 and end at 1", a == 0.0f && b2 == 1.0f && b == 1.0f / (float)k);
    }
    // object_bound of the whole curve: the hull of the control points, expanded by half the larger width
    float lo[3], hi[3];
    pcurve::segment_object_bound(c, 0.0f, 1.0f, lo, hi);
    near("bound lo x", lo[0], -0.3); near("bound lo y", lo[1], -1.3); near("bound lo z", lo[2], -0.3);
    near("bound hi x", hi[0], 3.3); near("bound hi y", hi[1], 2.3); near("bound hi z", hi[2], 1.3);
    // a segment's bound: blossomed points; at u in [0, 0.5] the first is cp[0] and the width is lerp(0.5) = 0.4
    pcurve::segment_object_bound(c, 0.0f, 0.5f, lo, hi);
    near("half bound lo x", lo[0], 0.0 - 0.2); near("half bound hi x", hi[0], 1.5 + 0.2);   // B(0.5).x = (0 + 3 + 6 + 3) / 8 = 1.5
    // from_props: 7 control points, degree 3 Bezier: two segments sharing a point, widths interpolated over the segment index
    const float P7[21] = {0, 0, 0, 1, 1, 0, 2, -1, 0, 3, 0, 0, 4, 1, 0, 5, -1, 0, 6, 0, 0};
    std::vector<pcurve::PropSegment> segs;
    check("bezier 7 points", pcurve::from_props_segments(3, false, P7, 7, 0.0f, 1.0f, segs).empty() && segs.size() == 2);
    if (segs.size() == 2) {
        check("bezier: shared end point", segs[0].cp[9] == 3 && segs[1].cp[0] == 3 && segs[1].cp[9] == 6);
        near("bezier: width at the joint", segs[0].width[1], 0.5); near("bezier: width at the joint", segs[1].width[0], 0.5); near("bezier: last width", segs[1].width[1], 1.0);
    }
    check("bspline degree 3: n - 3 segments", pcurve::from_props_segments(3, true, P7, 7, 1.0f, 1.0f, segs).empty() && segs.size() == 4);
    if (segs.size() == 4) for (int s = 0; s < 3; s++) for (int k = 0; k < 3; k++) near("bspline: segments join", segs[s].cp[9 + k], segs[s + 1].cp[k]);
    check("bspline degree 2: n - 2 segments", pcurve::from_props_segments(2, true, P7, 7, 1.0f, 1.0f, segs).empty() && segs.size() == 5);
    if (segs.size() == 5) { near("bspline 2: first point = the midpoint", segs[0].cp[0], 0.5); near("bspline 2: first point = the midpoint", segs[0].cp[1], 0.5); }
    check("bezier degree 2: 3 + 2n points", pcurve::from_props_segments(2, false, P7, 7, 1.0f, 1.0f, segs).empty() && segs.size() == 3);
    if (segs.size() == 3) { near("degree elevation", segs[0].cp[3], 2.0 / 3.0); near("degree elevation", segs[0].cp[6], 1.0 + 1.0 / 3.0); }
    // the panics, as sentences
    check("degree 4", pcurve::from_props_segments(4, false, P7, 7, 1, 1, segs).find("Invalid degree 4") == 0 && segs.empty());
    check("bezier 5 points", pcurve::from_props_segments(3, false, P7, 5, 1, 1, segs).find("Invalid number of control points 5") == 0);
    check("bezier 2 points", !pcurve::from_props_segments(3, false, P7, 2, 1, 1, segs).empty());
    check("bezier 0 points", !pcurve::from_props_segments(3, false, P7, 0, 1, 1, segs).empty());
    check("bspline 3 points", pcurve::from_props_segments(3, true, P7, 3, 1, 1, segs).find("Invalid number of control points 3") == 0);
    if (fails) { std::printf("curve_host_check: %d failures\n", fails); return 1; }
    std::printf("curve_host_check: ok\n");
    return 0;
}
