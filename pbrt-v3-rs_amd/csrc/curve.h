// The reference's Curve shape on the device (shapes/src/curve.rs) as it RUNS, quirks included.  Two entry points, both out of line like the quadrics':
//   curve_test     — Curve::intersect (curve.rs:543-645) with recursive_intersect (:339-536) up to the accept decision, for closest-hit rays (is_shadow_ray = false) and
//                    shadow rays (true): what quadric_test hands a leaf record to whose QuadricRec names a curve segment;
//   curve_surface  — the tail of the accepting leaf evaluation (:496-534) from (ray, t, u, v): the SurfaceInteraction carried to world space, for the shade and texture passes.
// The test is a pure function of (segment, ray, ray.t_max, is_shadow_ray), and its answer DEPENDS on ray.t_max (the culling boxes' z_max): the shade pass cannot repeat it, so an
// accepted hit retires with the u and v its leaf evaluation computed (HitOut's barycentric slots), and curve_surface rebuilds the rest — everything else depends on the ray alone.
// No recursion on the device: the walk keeps one path word (two bits per level) and re-subdivides from the segment's root along it where the reference returns from a recursive
// call; the same operations on the same operands give the same bits.  No frames in scratch: the only scratch is the 4x4 Gauss-Jordan of Transform::look_at.
// Expression order is the reference's, f32 without contraction; sin / cos are evaluated in f64 and rounded once.
#pragma once
#include "dmath.h"
#include "scene_types.h"

namespace ph {

// What the shade and texture passes read of a hit on an analytic shape (quadric.h: quadric_surface; here: curve_surface), in world space
struct QSurf { f3 p, p_error, wo, n, dpdu, dpdv, dndu, dndv; float u, v; uint32_t hit; };
// What the traversal kernel's leaf step gets back from an analytic shape's test (quadric.h: quadric_test): u, v are a curve's, zero for a quadric
struct QTest { float t, u, v; uint32_t hit; };

// the CurveRec of a curve segment: behind the last QuadricRec of the quadrics' buffer (scene_types.h)
PH_DEV const CurveRec& ph_curve_rec(const DeviceScene* dsc, const QuadricRec& q) { return reinterpret_cast<const CurveRec*>(dsc->quadrics + q.curves_at)[q.curve]; }

PH_DEV float c_lerp(float t, float a, float b) { return (1.0f - t) * a + t * b; }      // lerp (common.rs:167-173)
PH_DEV f3 c_lerp3(float t, f3 a, f3 b) { return (1.0f - t) * a + t * b; }
struct cp4 { f3 p[4]; };
PH_DEV f3 c_blossom(const float* p, float u0, float u1, float u2) {   // blossom_bezier (curve.rs:771-775)
    const f3 p0 = ld3(p), p1 = ld3(p + 3), p2 = ld3(p + 6), p3 = ld3(p + 9);
    const f3 a0 = c_lerp3(u0, p0, p1), a1 = c_lerp3(u0, p1, p2), a2 = c_lerp3(u0, p2, p3);
    const f3 b0 = c_lerp3(u1, a0, a1), b1 = c_lerp3(u1, a1, a2);
    return c_lerp3(u2, b0, b1);
}
PH_DEV cp4 c_segment_cp(const CurveRec& c, float u_min, float u_max) {   // Curve::blossom_bezier (:319-326)
    cp4 r;
    r.p[0] = c_blossom(c.cp, u_min, u_min, u_min); r.p[1] = c_blossom(c.cp, u_min, u_min, u_max);
    r.p[2] = c_blossom(c.cp, u_min, u_max, u_max); r.p[3] = c_blossom(c.cp, u_max, u_max, u_max);
    return r;
}
// eval_bezier (:797-812): the point and the derivative, which falls back to cp[3] - cp[0] where it is zero
PH_DEV f3 c_eval_bezier(f3 c0, f3 c1, f3 c2, f3 c3, float u, f3& deriv) {
    const f3 a0 = c_lerp3(u, c0, c1), a1 = c_lerp3(u, c1, c2), a2 = c_lerp3(u, c2, c3);
    const f3 b0 = c_lerp3(u, a0, a1), b1 = c_lerp3(u, a1, a2);
    deriv = (length_squared(b1 - b0) > 0.0f) ? 3.0f * (b1 - b0) : c3 - c0;
    return c_lerp3(u, b0, b1);
}
// one half of subdivide_bezier (:781-791): points 0 - 3 (half 0) or 3 - 6 (half 1) of the seven
PH_DEV cp4 c_half(const cp4& c, uint32_t half) {
    cp4 r;
    const f3 mid = (c.p[0] + 3.0f * c.p[1] + 3.0f * c.p[2] + c.p[3]) / 8.0f;
    if (half == 0u) { r.p[0] = c.p[0]; r.p[1] = (c.p[0] + c.p[1]) / 2.0f; r.p[2] = (c.p[0] + 2.0f * c.p[1] + c.p[2]) / 4.0f; r.p[3] = mid; }
    else { r.p[0] = mid; r.p[1] = (c.p[1] + 2.0f * c.p[2] + c.p[3]) / 4.0f; r.p[2] = (c.p[2] + c.p[3]) / 2.0f; r.p[3] = c.p[3]; }
    return r;
}
// the culling box of the root (:588-612) and of a half (:364-411): true = the ray's box misses it
PH_DEV bool c_culled(const cp4& c, float max_width, float z_max) {
    const float hw = 0.5f * max_width;
    if (pmaxf(pmaxf(c.p[0].y, c.p[1].y), pmaxf(c.p[2].y, c.p[3].y)) + hw < 0.0f || pminf(pminf(c.p[0].y, c.p[1].y), pminf(c.p[2].y, c.p[3].y)) - hw > 0.0f) return true;
    if (pmaxf(pmaxf(c.p[0].x, c.p[1].x), pmaxf(c.p[2].x, c.p[3].x)) + hw < 0.0f || pminf(pminf(c.p[0].x, c.p[1].x), pminf(c.p[2].x, c.p[3].x)) - hw > 0.0f) return true;
    if (pmaxf(pmaxf(c.p[0].z, c.p[1].z), pmaxf(c.p[2].z, c.p[3].z)) + hw < 0.0f || pminf(pminf(c.p[0].z, c.p[1].z), pminf(c.p[2].z, c.p[3].z)) - hw > z_max) return true;
    return false;
}

// Matrix4x4::inverse (matrix4x4.rs:67-143): Gauss-Jordan with full pivoting, the pivot search's ties and NaNs as the reference resolves them (`>=`, big starts at 0)
PH_DEV void c_m4_inverse(const float* a, float* out) {
    int indxc[4], indxr[4], ipiv[4] = {0, 0, 0, 0};
    float m[4][4];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) m[i][j] = a[4 * i + j];
    for (int i = 0; i < 4; i++) {
        int irow = 0, icol = 0; float big = 0.0f;
        for (int j = 0; j < 4; j++) {
            if (ipiv[j] != 1) {
                for (int k = 0; k < 4; k++) {
                    if (ipiv[k] == 0) { const float v = pabs(m[j][k]); if (v >= big) { big = v; irow = j; icol = k; } }
                }
            }
        }
        ipiv[icol] += 1;
        if (irow != icol) for (int k = 0; k < 4; k++) { const float t = m[irow][k]; m[irow][k] = m[icol][k]; m[icol][k] = t; }
        indxr[i] = irow; indxc[i] = icol;
        const float pivinv = ph_div(1.0f, m[icol][icol]);
        m[icol][icol] = 1.0f;
        for (int j = 0; j < 4; j++) m[icol][j] *= pivinv;
        for (int j = 0; j < 4; j++) {
            if (j != icol) {
                const float save = m[j][icol];
                m[j][icol] = 0.0f;
                for (int k = 0; k < 4; k++) m[j][k] -= m[icol][k] * save;
            }
        }
    }
    for (int j = 3; j >= 0; j--) {
        if (indxr[j] != indxc[j]) for (int k = 0; k < 4; k++) { const float t = m[k][indxr[j]]; m[k][indxr[j]] = m[k][indxc[j]]; m[k][indxc[j]] = t; }
    }
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) out[4 * i + j] = m[i][j];
}
PH_DEV f3 c_xf_point(const float* m, f3 p) {   // transform_point (transform.rs:288-302)
    const float xp = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    const float yp = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    const float zp = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    const float wp = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    return (wp == 1.0f) ? mk3(xp, yp, zp) : mk3(xp, yp, zp) / wp;
}
PH_DEV f3 c_xf_vec(const float* m, f3 v) { return mk3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z); }   // transform_vector (:373-380)
PH_DEV f3 c_xf_normal(const float* mi, f3 n) { return mk3(mi[0] * n.x + mi[4] * n.y + mi[8] * n.z, mi[1] * n.x + mi[5] * n.y + mi[9] * n.z, mi[2] * n.x + mi[6] * n.y + mi[10] * n.z); }   // transform_normal (:439-448)

// What Curve::intersect sets up before the culling (:546-583) — it depends on the segment and the ray alone, so curve_surface repeats it bit for bit:
// the object-space ray of transform_ray_with_error (transform.rs:481-513: the origin pushed along d by its error bound, t_max kept), the segment's four control points, and
// object_to_ray = Transform::look_at(o, o + d, dx): r2o = the matrix LookAt writes down (ray_to_object's m), o2r = its Gauss-Jordan inverse (object_to_ray's m).
struct CFrame { f3 o, d; cp4 cp_obj; float r2o[16], o2r[16]; bool ok; };
PH_DEV void c_frame(const QuadricRec& q, const CurveRec& cv, f3 ro, f3 rd, CFrame& f) {
    const float* c = q.w2o;
    const float x = ro.x, y = ro.y, z = ro.z;
    const float opx = (c[0] * x + c[1] * y) + (c[2] * z + c[3]);
    const float opy = (c[4] * x + c[5] * y) + (c[6] * z + c[7]);
    const float opz = (c[8] * x + c[9] * y) + (c[10] * z + c[11]);
    const float opw = (c[12] * x + c[13] * y) + (c[14] * z + c[15]);
    const float xs = pabs(c[0] * x) + pabs(c[1] * y) + pabs(c[2] * z) + pabs(c[3]);
    const float ys = pabs(c[4] * x) + pabs(c[5] * y) + pabs(c[6] * z) + pabs(c[7]);
    const float zs = pabs(c[8] * x) + pabs(c[9] * y) + pabs(c[10] * z) + pabs(c[11]);
    const f3 o_err = kGamma3 * mk3(xs, ys, zs);
    f3 o = (opw == 1.0f) ? mk3(opx, opy, opz) : mk3(opx, opy, opz) / opw;
    const f3 d = c_xf_vec(c, rd);
    const float l2 = length_squared(d);
    if (l2 > 0.0f) { const float dt = ph_div(dot(vabs(d), o_err), l2); o = o + d * dt; }
    f.o = o; f.d = d;
    f.cp_obj = c_segment_cp(cv, q.z_min, q.z_max);
    f3 dx = cross(d, f.cp_obj.p[3] - f.cp_obj.p[0]);
    if (length_squared(dx) == 0.0f) { f3 dy; coordinate_system(d, dx, dy); }   // the ray runs along the chord (:569-575)
    // Transform::look_at (transform.rs:191-214)
    const f3 dir = normalize((o + d) - o);
    f3 right = cross(normalize(dx), dir);
    f.ok = !(length(right) == 0.0f);   // the reference panics here; the library reports a miss
    right = normalize(right);
    const f3 new_up = cross(dir, right);
    float* m = f.r2o;
    m[0] = right.x; m[1] = new_up.x; m[2] = dir.x; m[3] = o.x;
    m[4] = right.y; m[5] = new_up.y; m[6] = dir.y; m[7] = o.y;
    m[8] = right.z; m[9] = new_up.z; m[10] = dir.z; m[11] = o.z;
    m[12] = 0.0f; m[13] = 0.0f; m[14] = 0.0f; m[15] = 1.0f;
    c_m4_inverse(m, f.o2r);
}

// log2int of an f32 (core/src/pbrt/log2int.rs:12-26) as it runs: exponent PLUS the mantissa's lowest bit; 0 below 1; +inf and every NaN fail `< 1` and give 128 or more
PH_DEV uint32_t c_log2int(float v) {
    if (v < 1.0f) return 0u;
    const uint32_t bits = __float_as_uint(v);
    return ((bits >> 23) - 127u) + (bits & 1u);
}

struct CHit { float t, u, v; };
// The leaf evaluation of recursive_intersect (:437-501) up to the accept decision.  dpdu == 0 fires the reference's assert!: a miss here
PH_DEV bool c_leaf(const CurveRec& cv, const cp4& c, float u0, float u1, f3 ray_d, float ray_length, float z_max, CHit& h) {
    float edge = (c.p[1].y - c.p[0].y) * -c.p[0].y + c.p[0].x * (c.p[0].x - c.p[1].x);
    if (edge < 0.0f) return false;
    edge = (c.p[2].y - c.p[3].y) * -c.p[3].y + c.p[3].x * (c.p[3].x - c.p[2].x);
    if (edge < 0.0f) return false;
    const float sx = c.p[3].x - c.p[0].x, sy = c.p[3].y - c.p[0].y;
    const float denom = sx * sx + sy * sy;
    if (denom == 0.0f) return false;
    const float w = ph_div(-c.p[0].x * sx + -c.p[0].y * sy, denom);
    const float u = pclampf(c_lerp(w, u0, u1), u0, u1);
    float hit_width = c_lerp(u, cv.width[0], cv.width[1]);
    if (cv.type == PH_CURVE_RIBBON) {
        const float sin0 = d_sin((1.0f - u) * cv.normal_angle) * cv.inv_sin_normal_angle;
        const float sin1 = d_sin(u * cv.normal_angle) * cv.inv_sin_normal_angle;
        const f3 n_hit = sin0 * ld3(cv.n) + sin1 * ld3(cv.n + 3);
        hit_width *= ph_div(abs_dot(n_hit, ray_d), ray_length);
    }
    f3 dpcdw;
    const f3 pc = c_eval_bezier(c.p[0], c.p[1], c.p[2], c.p[3], pclampf(w, 0.0f, 1.0f), dpcdw);
    const float pt_curve_dist2 = pc.x * pc.x + pc.y * pc.y;
    if (pt_curve_dist2 > hit_width * hit_width * 0.25f) return false;
    if (pc.z < 0.0f || pc.z > z_max) return false;
    const float pt_curve_dist = ph_sqrt(pt_curve_dist2);
    const float edge_func = dpcdw.x * -pc.y + pc.x * dpcdw.y;
    const float v = (edge_func > 0.0f) ? 0.5f + ph_div(pt_curve_dist, hit_width) : 0.5f - ph_div(pt_curve_dist, hit_width);
    f3 dpdu;
    c_eval_bezier(ld3(cv.cp), ld3(cv.cp + 3), ld3(cv.cp + 6), ld3(cv.cp + 9), u, dpdu);
    if (dpdu.x == 0.0f && dpdu.y == 0.0f && dpdu.z == 0.0f) return false;
    h.t = ph_div(pc.z, ray_length); h.u = u; h.v = v;
    return true;
}

// Curve::intersect(r, is_shadow_ray) up to the accept decision.  recursive_intersect as it runs:
//   - `hit = self.recursive_intersect(..)` is unconditional (:413): a half that is not culled REPLACES what the half before it found, hit or miss.  A closest-hit ray's answer is
//     therefore that of ONE root-to-leaf path — at every level the second half if its box is met, else the first if its box is met, else a miss — and the evaluations the
//     reference makes and throws away are not made here (they are pure).  A shadow ray returns at the first hit (:429-431), so it walks the halves in order.
//   - `cps += 3` is skipped by `continue` (:381, :395, :410, :433): with the first half culled, the second is tested — box and all — on the FIRST half's control points under its own
//     u range.  One bit per level of `cp_sel` keeps which points a level took, one bit of `u_sel` which range.
//   - the boxes' z_max is ray_length * ray.t_max (:398): the caller's t_max decides which path is walked.
PH_DEV bool curve_core(const QuadricRec& q, const CurveRec& cv, f3 ro, f3 rd, float ray_t_max, bool shadow, CHit& h) {
    CFrame f;
    c_frame(q, cv, ro, rd, f);
    if (!f.ok) return false;
    cp4 root;
#pragma unroll
    for (int k = 0; k < 4; k++) root.p[k] = c_xf_point(f.o2r, f.cp_obj.p[k]);
    const float w0 = cv.width[0], w1 = cv.width[1];
    const float ray_length = length(f.d), z_max = ray_length * ray_t_max;
    if (c_culled(root, pmaxf(c_lerp(q.z_min, w0, w1), c_lerp(q.z_max, w0, w1)), z_max)) return false;
    float l0 = 0.0f;
#pragma unroll
    for (int i = 0; i < 2; i++)
        l0 = pmaxf(l0, pmaxf(pmaxf(pabs(root.p[i].x - 2.0f * root.p[i + 1].x + root.p[i + 2].x), pabs(root.p[i].y - 2.0f * root.p[i + 1].y + root.p[i + 2].y)),
                             pabs(root.p[i].z - 2.0f * root.p[i + 1].z + root.p[i + 2].z)));
    const float eps = pmaxf(w0, w1) * 0.05f;
    const uint32_t r0 = c_log2int(ph_div(1.41421356237f * 6.0f * l0, 8.0f * eps)) / 2u;
    const int max_depth = (int)(r0 > 10u ? 10u : r0);   // clamp(r0, 0, 10) of a u32

    // level k = the split made k levels below the root; bit k of cp_sel / u_sel = the half whose points / whose u range the walk took there; bit k of pend = (shadow rays) the second
    // half of level k passed its box and has not been walked yet
    uint32_t cp_sel = 0u, u_sel = 0u, pend = 0u;
    int lvl = 0;
    cp4 c = root;
    float u0 = q.z_min, u1 = q.z_max;
#pragma unroll 1
    for (;;) {
        bool back = false;
        if (lvl == max_depth) {
            if (c_leaf(cv, c, u0, u1, f.d, ray_length, z_max, h)) return true;
            back = true;
        } else {
            const float um = ph_div(u0 + u1, 2.0f);
            const cp4 first = c_half(c, 0u);
            const bool cull1 = c_culled(first, pmaxf(c_lerp(u0, w0, w1), c_lerp(um, w0, w1)), z_max);
            const cp4 second = cull1 ? first : c_half(c, 1u);
            const bool cull2 = c_culled(second, pmaxf(c_lerp(um, w0, w1), c_lerp(u1, w0, w1)), z_max);
            const uint32_t bit = 1u << lvl;
            if (shadow ? cull1 : !cull2) {   // on to the second half (or nowhere)
                if (cull2) back = true;
                else { c = second; u0 = um; u_sel |= bit; if (!cull1) cp_sel |= bit; lvl++; }
            } else {
                if (cull1) back = true;   // (closest-hit: both culled)
                else { c = first; u1 = um; if (shadow && !cull2) pend |= bit; lvl++; }
            }
        }
        if (back) {
            if (!pend) return false;
            // back to the deepest level whose second half waits: subdivide again from the root along the path (the operations of the first descent, so its bits)
            const int k = 31 - __clz((int)pend);
            const uint32_t bit = 1u << k, below = bit - 1u;
            pend &= ~bit; cp_sel = (cp_sel & below) | bit; u_sel = (u_sel & below) | bit;
            c = root; u0 = q.z_min; u1 = q.z_max;
#pragma unroll 1
            for (int j = 0; j <= k; j++) {
                const float um = ph_div(u0 + u1, 2.0f);
                c = c_half(c, (cp_sel >> j) & 1u);
                if ((u_sel >> j) & 1u) u0 = um; else u1 = um;
            }
            lvl = k + 1;
        }
    }
}

// the traversal kernel's leaf test for a curve segment (a curve may be hit at t == 0: pc.z >= 0 passes, :480)
static __device__ __noinline__ QTest curve_test(const DeviceScene* dsc, uint32_t qi, float ox, float oy, float oz, float t_max, float dx, float dy, float dz, uint32_t shadow) {
    const QuadricRec& q = dsc->quadrics[qi];
    CHit h; QTest r;
    const bool hit = curve_core(q, ph_curve_rec(dsc, q), mk3(ox, oy, oz), mk3(dx, dy, dz), t_max, shadow != 0u, h);
    r.hit = hit ? 1u : 0u; r.t = hit ? h.t : -1.0f; r.u = hit ? h.u : 0.0f; r.v = hit ? h.v : 0.0f;
    return r;
}

// Transform::rotate_axis(theta_deg, axis).transform_vector(v) (transform.rs:155-183)
PH_DEV f3 c_rotate_axis_vec(float theta_deg, f3 axis, f3 v) {
    const f3 a = normalize(axis);
    const float r = theta_deg * (kPi / 180.0f);   // f32::to_radians
    const float sin_theta = d_sin(r), cos_theta = d_cos(r);
    const float m00 = a.x * a.x + (1.0f - a.x * a.x) * cos_theta, m01 = a.x * a.y * (1.0f - cos_theta) - a.z * sin_theta, m02 = a.x * a.z * (1.0f - cos_theta) + a.y * sin_theta;
    const float m10 = a.x * a.y * (1.0f - cos_theta) + a.z * sin_theta, m11 = a.y * a.y + (1.0f - a.y * a.y) * cos_theta, m12 = a.y * a.z * (1.0f - cos_theta) - a.x * sin_theta;
    const float m20 = a.x * a.z * (1.0f - cos_theta) - a.y * sin_theta, m21 = a.y * a.z * (1.0f - cos_theta) + a.x * sin_theta, m22 = a.z * a.z + (1.0f - a.z * a.z) * cos_theta;
    return mk3(m00 * v.x + m01 * v.y + m02 * v.z, m10 * v.x + m11 * v.y + m12 * v.z, m20 * v.x + m21 * v.y + m22 * v.z);
}

// The tail of the accepting leaf evaluation (curve.rs:463-471, :496-534) from what the traversal carried over — t, u, v — and the ray: hit_width with the ribbon factor and n_hit,
// dpdu on the whole curve, dpdv per type through ray_to_object, p = ray.at(t) on the object-space ray, p_error = 2 * hit_width, SurfaceInteraction::new
// (surface_interaction.rs:69-98: n from dpdu x dpdv, flipped by reverse_orientation ^ swaps_handedness), then object_to_world.transform_surface_interaction (transform.rs:566-590).
// ray_tuv: the world-space ray's o xyz, d xyz, then t, u, v
static __device__ __noinline__ void curve_surface(const DeviceScene* dsc, uint32_t qi, const float* ray_tuv, QSurf* out) {
    const QuadricRec& q = dsc->quadrics[qi];
    const CurveRec& cv = ph_curve_rec(dsc, q);
    const float t = ray_tuv[6], u = ray_tuv[7], v = ray_tuv[8];
    CFrame f;
    c_frame(q, cv, mk3(ray_tuv[0], ray_tuv[1], ray_tuv[2]), mk3(ray_tuv[3], ray_tuv[4], ray_tuv[5]), f);
    float hit_width = c_lerp(u, cv.width[0], cv.width[1]);
    f3 n_hit = mk3(0.0f, 0.0f, 0.0f);
    if (cv.type == PH_CURVE_RIBBON) {
        const float sin0 = d_sin((1.0f - u) * cv.normal_angle) * cv.inv_sin_normal_angle;
        const float sin1 = d_sin(u * cv.normal_angle) * cv.inv_sin_normal_angle;
        n_hit = sin0 * ld3(cv.n) + sin1 * ld3(cv.n + 3);
        hit_width *= ph_div(abs_dot(n_hit, f.d), length(f.d));
    }
    f3 dpdu, dpdv;
    c_eval_bezier(ld3(cv.cp), ld3(cv.cp + 3), ld3(cv.cp + 6), ld3(cv.cp + 9), u, dpdu);
    if (cv.type == PH_CURVE_RIBBON) dpdv = normalize(cross(n_hit, dpdu)) * hit_width;
    else {
        const f3 dpdu_plane = c_xf_vec(f.o2r, dpdu);
        f3 dpdv_plane = normalize(mk3(-dpdu_plane.y, dpdu_plane.x, 0.0f)) * hit_width;
        if (cv.type == PH_CURVE_CYLINDER) dpdv_plane = c_rotate_axis_vec(-c_lerp(v, -90.0f, 90.0f), dpdu_plane, dpdv_plane);
        dpdv = c_xf_vec(f.r2o, dpdv_plane);
    }
    const f3 p = f.o + f.d * t;
    const float pe1 = 2.0f * hit_width;
    QSurf s;
    s.hit = 1u;
    f3 n = normalize(cross(dpdu, dpdv));
    if (q.flip) n = n * -1.0f;
    f3 wo = -f.d;
    const float l2 = length_squared(wo);
    wo = (l2 == 0.0f) ? wo : wo / ph_sqrt(l2);   // Hit::new (interaction/mod.rs:137-156)
    {   // transform_point_with_abs_error (transform.rs:338-370)
        const float* m = q.o2w;
        const float x = p.x, y = p.y, z = p.z;
        const float xp = (m[0] * x + m[1] * y) + (m[2] * z + m[3]);
        const float yp = (m[4] * x + m[5] * y) + (m[6] * z + m[7]);
        const float zp = (m[8] * x + m[9] * y) + (m[10] * z + m[11]);
        const float wp = (m[12] * x + m[13] * y) + (m[14] * z + m[15]);
        const float g3 = kGamma3;
        s.p_error = mk3((g3 + 1.0f) * (pabs(m[0]) * pe1 + pabs(m[1]) * pe1 + pabs(m[2]) * pe1) + g3 * (pabs(m[0] * x) + pabs(m[1] * y) + pabs(m[2] * z) + pabs(m[3])),
                        (g3 + 1.0f) * (pabs(m[4]) * pe1 + pabs(m[5]) * pe1 + pabs(m[6]) * pe1) + g3 * (pabs(m[4] * x) + pabs(m[5] * y) + pabs(m[6] * z) + pabs(m[7])),
                        (g3 + 1.0f) * (pabs(m[8]) * pe1 + pabs(m[9]) * pe1 + pabs(m[10]) * pe1) + g3 * (pabs(m[8] * x) + pabs(m[9] * y) + pabs(m[10] * z) + pabs(m[11])));
        s.p = (wp == 1.0f) ? mk3(xp, yp, zp) : mk3(xp, yp, zp) / wp;
    }
    s.wo = normalize(c_xf_vec(q.o2w, wo));
    s.n = normalize(c_xf_normal(q.w2o, n));
    s.dpdu = c_xf_vec(q.o2w, dpdu); s.dpdv = c_xf_vec(q.o2w, dpdv);
    s.dndu = mk3(0.0f, 0.0f, 0.0f); s.dndv = s.dndu;   // Normal3f::ZERO through transform_normal
    s.u = u; s.v = v;
    *out = s;
}

}  // namespace ph
