// The reference's six quadric shapes on the device: Sphere, Cylinder, Disk, Cone, Paraboloid, Hyperboloid (shapes/src/*.rs) with the running error bounds of
// EFloat (core/src/efloat.rs).  Two entry points, both out of line (real calls in the ISA: s_swappc_b64).  That keeps the interval arithmetic, the f64 square root and the f64 atan2 out of the callers' instruction
// streams; it does NOT keep their registers out of the callers' budgets — a kernel is allocated what its callees need (quadric_test: 136 VGPRs):
//   quadric_test     — Shape::intersect / intersect_p up to the accept decision (the two run the same tests): what the traversal kernel's QUADRIC instantiations call at a leaf;
//   quadric_surface  — the same test on the same ray, then the tail of ::intersect: the SurfaceInteraction carried to world space (transform.rs:566-590), for the shade and texture passes.
// Repeating the test in the shade pass gives the bits the traversal saw: the roots do not depend on ray.t_max, and every ray.t_max comparison the traversal's (shorter) t_max passed
// is passed by the ray's own.  Expression order is the reference's, f32 without contraction; phi is atan2 evaluated in f64 and rounded once.
// Both entry points hand a record of kind PH_Q_CURVE — one segment of a Curve — on to curve.h, for which none of the above holds: its test depends on ray.t_max.
#pragma once
#include "dmath.h"
#include "scene_types.h"
#include "curve.h"

namespace ph {

// ---- EFloat (efloat.rs), release build: value + interval --------------------------------------------------------------------------------------------
struct ef { float v, lo, hi; };
PH_DEV ef ef_raw(float v, float lo, float hi) { ef r; r.v = v; r.lo = lo; r.hi = hi; return r; }
PH_DEV ef ef_mk(float v, float err) {   // EFloat::new (:14-33)
    if (err == 0.0f) return ef_raw(v, v, v);
    return ef_raw(v, next_float_down(v - err), next_float_up(v + err));
}
PH_DEV ef ef_c(float v) { return ef_raw(v, v, v); }
PH_DEV float ef_abs_err(ef a) { return next_float_up(pmaxf(pabs(a.hi - a.v), pabs(a.v - a.lo))); }   // get_absolute_error (:96-98)
PH_DEV ef operator+(ef a, ef b) { return ef_raw(a.v + b.v, next_float_down(a.lo + b.lo), next_float_up(a.hi + b.hi)); }   // :150-163
PH_DEV ef operator-(ef a, ef b) { return ef_raw(a.v - b.v, next_float_down(a.lo - b.hi), next_float_up(a.hi - b.lo)); }   // :180-192
PH_DEV ef operator*(ef a, ef b) {                                                                                           // :209-228 (f32::min / max: a NaN operand is ignored)
    const float p0 = a.lo * b.lo, p1 = a.hi * b.lo, p2 = a.lo * b.hi, p3 = a.hi * b.hi;
    return ef_raw(a.v * b.v, next_float_down(fminf(fminf(p0, p1), fminf(p2, p3))), next_float_up(fmaxf(fmaxf(p0, p1), fmaxf(p2, p3))));
}
PH_DEV ef operator/(ef a, ef b) {                                                                                           // :245-270
    if (b.lo < 0.0f && b.hi > 0.0f) return ef_raw(ph_div(a.v, b.v), -kInf, kInf);   // the divisor straddles zero
    const float d0 = ph_div(a.lo, b.lo), d1 = ph_div(a.hi, b.lo), d2 = ph_div(a.lo, b.hi), d3 = ph_div(a.hi, b.hi);
    return ef_raw(ph_div(a.v, b.v), next_float_down(fminf(fminf(d0, d1), fminf(d2, d3))), next_float_up(fmaxf(fmaxf(d0, d1), fmaxf(d2, d3))));
}
// Quadratic::solve_efloat (:301-327): discriminant in f64 from the values, roots with intervals, ordered by value
PH_DEV bool quadratic_ef(ef a, ef b, ef c, ef& t0, ef& t1) {
    const double discrim = (double)b.v * (double)b.v - 4.0 * (double)a.v * (double)c.v;
    if (discrim < 0.0) return false;
    const float root = (float)sqrt(discrim);
    const ef ef_root = ef_mk(root, kMachEps * root);
    const ef q = b.v < 0.0f ? ef_c(-0.5f) * (b - ef_root) : ef_c(-0.5f) * (b + ef_root);
    t0 = q / a; t1 = c / q;
    if (t0.v > t1.v) { const ef t = t0; t0 = t1; t1 = t; }
    return true;
}

struct QHit { float t; f3 p; float phi, v; f3 perr; };   // object space; v: the hyperboloid's v, the disk's dist2

// Sphere / Cylinder / Cone / Paraboloid / Hyperboloid / Disk ::intersect and ::intersect_p up to the accept decision
// (sphere.rs:59-171, cylinder.rs:64-144, cone.rs:66-130, paraboloid.rs:66-130, hyperboloid.rs:124-190, disk.rs:64-104)
PH_DEV bool quadric_core(const QuadricRec& q, f3 ro, f3 rd, float ray_t_max, QHit& h) {
    // transform_ray_with_error (transform.rs:481-510): the origin is pushed along d by its error bound, t_max is NOT shortened
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
    const float g3 = kGamma3;
    const f3 d_err = mk3(g3 * (pabs(c[0] * rd.x) + pabs(c[1] * rd.y) + pabs(c[2] * rd.z)), g3 * (pabs(c[4] * rd.x) + pabs(c[5] * rd.y) + pabs(c[6] * rd.z)),
                         g3 * (pabs(c[8] * rd.x) + pabs(c[9] * rd.y) + pabs(c[10] * rd.z)));
    const f3 d = mk3(c[0] * rd.x + c[1] * rd.y + c[2] * rd.z, c[4] * rd.x + c[5] * rd.y + c[6] * rd.z, c[8] * rd.x + c[9] * rd.y + c[10] * rd.z);
    const float l2 = length_squared(d);
    if (l2 > 0.0f) { const float dt = ph_div(dot(vabs(d), o_err), l2); o = o + d * dt; }
    const uint32_t kind = q.kind;
    if (kind == PH_Q_DISK) {   // no EFloat here (disk.rs:64-104)
        if (d.z == 0.0f) return false;
        const float t = ph_div(q.height - o.z, d.z);
        if (t <= 0.0f || t >= ray_t_max) return false;
        const f3 p = o + d * t;
        const float dist2 = p.x * p.x + p.y * p.y;
        if (dist2 > q.radius * q.radius || dist2 < q.inner_radius * q.inner_radius) return false;
        float phi = d_atan2(p.y, p.x);
        if (phi < 0.0f) phi += kTwoPi;
        if (phi > q.phi_max) return false;
        h.t = t; h.p = p; h.phi = phi; h.v = dist2; h.perr = mk3(0.0f, 0.0f, 0.0f);
        return true;
    }
    const ef ox = ef_mk(o.x, o_err.x), oy = ef_mk(o.y, o_err.y), oz = ef_mk(o.z, o_err.z), dx = ef_mk(d.x, d_err.x), dy = ef_mk(d.y, d_err.y), dz = ef_mk(d.z, d_err.z);
    ef a, b, cc;
    if (kind == PH_Q_SPHERE) {
        a = dx * dx + dy * dy + dz * dz;
        b = ef_c(2.0f) * (dx * ox + dy * oy + dz * oz);
        cc = ox * ox + oy * oy + oz * oz - ef_c(q.radius) * ef_c(q.radius);
    } else if (kind == PH_Q_HYPERBOLOID) {
        const ef ah = ef_c(q.ah), ch = ef_c(q.ch);
        a = ah * dx * dx + ah * dy * dy - ch * dz * dz;
        b = ef_c(2.0f) * (ah * dx * ox + ah * dy * oy - ch * dz * oz);
        cc = ah * ox * ox + ah * oy * oy - ch * oz * oz - ef_c(1.0f);
    } else if (kind == PH_Q_CYLINDER) {
        a = dx * dx + dy * dy;
        b = ef_c(2.0f) * (dx * ox + dy * oy);
        cc = ox * ox + oy * oy - ef_c(q.radius) * ef_c(q.radius);
    } else if (kind == PH_Q_CONE) {
        ef k = ef_c(q.radius) / ef_c(q.height);
        k = k * k;
        a = dx * dx + dy * dy - k * dz * dz;
        b = ef_c(2.0f) * (dx * ox + dy * oy - k * dz * (oz - ef_c(q.height)));
        cc = ox * ox + oy * oy - k * (oz - ef_c(q.height)) * (oz - ef_c(q.height));
    } else {
        const ef k = ef_c(q.z_max) / (ef_c(q.radius) * ef_c(q.radius));
        a = k * (dx * dx + dy * dy);
        b = ef_c(2.0f) * k * (dx * ox + dy * oy) - dz;
        cc = k * (ox * ox + oy * oy) - oz;
    }
    ef t0, t1;
    if (!quadratic_ef(a, b, cc, t0, t1)) return false;
    if (t0.hi > ray_t_max || t1.lo <= 0.0f) return false;
    ef t_hit = t0;
    if (t_hit.lo <= 0.0f) { t_hit = t1; if (t_hit.hi > ray_t_max) return false; }
    f3 p_hit = mk3(0.0f, 0.0f, 0.0f); float phi = 0.0f, v = 0.0f;
    // two passes at most: the first root, then — if it was clipped away — the second
#pragma unroll 1
    for (int pass = 0;; pass++) {
        p_hit = o + d * t_hit.v;   // ray.at(t)
        float ay = p_hit.y, ax = p_hit.x;
        if (kind == PH_Q_SPHERE) {
            p_hit = p_hit * ph_div(q.radius, length(p_hit));   // refine (sphere.rs:104-107)
            if (p_hit.x == 0.0f && p_hit.y == 0.0f) p_hit.x = 1e-5f * q.radius;
            ay = p_hit.y; ax = p_hit.x;
        } else if (kind == PH_Q_CYLINDER) {   // refine (cylinder.rs:107-109)
            const float hit_rad = ph_sqrt(p_hit.x * p_hit.x + p_hit.y * p_hit.y);
            p_hit.x *= ph_div(q.radius, hit_rad); p_hit.y *= ph_div(q.radius, hit_rad);
            ay = p_hit.y; ax = p_hit.x;
        } else if (kind == PH_Q_HYPERBOLOID) {
            v = ph_div(p_hit.z - q.p1[2], q.p2[2] - q.p1[2]);
            const f3 pr = (1.0f - v) * mk3(q.p1[0], q.p1[1], q.p1[2]) + v * mk3(q.p2[0], q.p2[1], q.p2[2]);
            ay = pr.x * p_hit.y - p_hit.x * pr.y; ax = p_hit.x * pr.x + p_hit.y * pr.y;
        }
        phi = d_atan2(ay, ax);
        if (phi < 0.0f) phi += kTwoPi;
        bool clipped;
        if (kind == PH_Q_SPHERE) clipped = (q.z_min > -q.radius && p_hit.z < q.z_min) || (q.z_max < q.radius && p_hit.z > q.z_max) || phi > q.phi_max;
        else if (kind == PH_Q_CONE) clipped = p_hit.z < 0.0f || p_hit.z > q.height || phi > q.phi_max;
        else clipped = p_hit.z < q.z_min || p_hit.z > q.z_max || phi > q.phi_max;
        if (!clipped) break;
        if (pass == 1) return false;
        if (t_hit.v == t1.v) return false;   // EFloat == compares the values (efloat.rs:143-147)
        if (t1.hi > ray_t_max) return false;
        t_hit = t1;
    }
    h.t = t_hit.v; h.p = p_hit; h.phi = phi; h.v = v;
    if (kind == PH_Q_SPHERE) h.perr = kGamma5 * vabs(p_hit);                                               // sphere.rs:228
    else if (kind == PH_Q_CYLINDER) h.perr = kGamma3 * vabs(mk3(p_hit.x, p_hit.y, 0.0f));                  // cylinder.rs:184
    else { const ef px = ox + t_hit * dx, py = oy + t_hit * dy, pz = oz + t_hit * dz; h.perr = mk3(ef_abs_err(px), ef_abs_err(py), ef_abs_err(pz)); }   // cone.rs:176-183 and its kin
    return true;
}

// the traversal kernel's leaf test: hit or miss, the hit's t and (a curve's) u, v.  Arguments in registers, the record through DeviceScene::self.  A record that names a curve
// segment goes on to curve_test (curve.h), the one test that reads `shadow`: Curve::intersect_p is not Curve::intersect cut short
static __device__ __noinline__ QTest quadric_test(const DeviceScene* dsc, uint32_t qi, float ox, float oy, float oz, float t_max, float dx, float dy, float dz, uint32_t shadow) {
    if (dsc->quadrics[qi].kind == PH_Q_CURVE) return curve_test(dsc, qi, ox, oy, oz, t_max, dx, dy, dz, shadow);
    QHit h; QTest r;
    r.hit = quadric_core(dsc->quadrics[qi], mk3(ox, oy, oz), mk3(dx, dy, dz), t_max, h) ? 1u : 0u;
    r.t = r.hit ? h.t : -1.0f; r.u = 0.0f; r.v = 0.0f;
    return r;
}

// (QSurf, what the shade and texture passes read of the hit in world space: curve.h)
PH_DEV f3 q_xf_vec(const float* m, f3 v) { return mk3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z); }   // transform_vector
PH_DEV f3 q_xf_normal(const float* mi, f3 n) { return mk3(mi[0] * n.x + mi[4] * n.y + mi[8] * n.z, mi[1] * n.x + mi[5] * n.y + mi[9] * n.z, mi[2] * n.x + mi[6] * n.y + mi[10] * n.z); }   // transform_normal
// tails of the six ::intersect (sphere.rs:173-241, cylinder.rs:146-196, cone.rs:132-190, paraboloid.rs:132-200, disk.rs:106-140, hyperboloid.rs:192-262): parametric form, dn/du and
// dn/dv from the fundamental forms, SurfaceInteraction::new (surface_interaction.rs:69-98), then object_to_world.transform_surface_interaction (transform.rs:566-590)
static __device__ __noinline__ void quadric_surface(const DeviceScene* dsc, uint32_t qi, const float* ray_o_d /* o xyz, d xyz; for a curve segment then the hit's t, u, v */, QSurf* out) {
    const QuadricRec& q = dsc->quadrics[qi];
    if (q.kind == PH_Q_CURVE) { curve_surface(dsc, qi, ray_o_d, out); return; }
    const f3 ro = mk3(ray_o_d[0], ray_o_d[1], ray_o_d[2]), rd = mk3(ray_o_d[3], ray_o_d[4], ray_o_d[5]);
    QHit h;
    QSurf s;
    s.hit = quadric_core(q, ro, rd, kInf, h) ? 1u : 0u;
    if (!s.hit) { h.t = 0.0f; h.p = mk3(0.0f, 0.0f, 1.0f); h.phi = 0.0f; h.v = 1.0f; h.perr = mk3(0.0f, 0.0f, 0.0f); }   // (never for a hit the traversal reported)
    f3 p = h.p; const float phi = h.phi;
    const uint32_t kind = q.kind;
    const float u = ph_div(phi, q.phi_max);
    float v = 0.0f;
    f3 dpdu = mk3(-q.phi_max * p.y, q.phi_max * p.x, 0.0f), dpdv, dndu = mk3(0.0f, 0.0f, 0.0f), dndv = mk3(0.0f, 0.0f, 0.0f);
    if (kind == PH_Q_DISK) {
        const float r_hit = ph_sqrt(h.v);
        v = ph_div(q.radius - r_hit, q.radius - q.inner_radius);
        dpdv = mk3(p.x, p.y, 0.0f) * (q.inner_radius - q.radius) / r_hit;
        p.z = q.height;   // refine (disk.rs:118)
    } else {
        f3 d2p_duu = (-q.phi_max * q.phi_max) * mk3(p.x, p.y, 0.0f), d2p_duv = mk3(0.0f, 0.0f, 0.0f), d2p_dvv = mk3(0.0f, 0.0f, 0.0f);
        if (kind == PH_Q_SPHERE) {
            const float theta = d_acos(pclampf(ph_div(p.z, q.radius), -1.0f, 1.0f));
            v = ph_div(theta - q.theta_min, q.theta_max - q.theta_min);
            const float z_radius = ph_sqrt(p.x * p.x + p.y * p.y);
            const float inv_z_radius = ph_div(1.0f, z_radius);
            const float cos_phi = p.x * inv_z_radius, sin_phi = p.y * inv_z_radius;
            dpdv = (q.theta_max - q.theta_min) * mk3(p.z * cos_phi, p.z * sin_phi, -q.radius * d_sin(theta));
            d2p_duv = ((q.theta_max - q.theta_min) * p.z * q.phi_max) * mk3(-sin_phi, cos_phi, 0.0f);
            d2p_dvv = (-(q.theta_max - q.theta_min) * (q.theta_max - q.theta_min)) * mk3(p.x, p.y, p.z);
        } else if (kind == PH_Q_HYPERBOLOID) {
            v = h.v;
            const float cos_phi = d_cos(phi), sin_phi = d_sin(phi);
            dpdv = mk3((q.p2[0] - q.p1[0]) * cos_phi - (q.p2[1] - q.p1[1]) * sin_phi, (q.p2[0] - q.p1[0]) * sin_phi + (q.p2[1] - q.p1[1]) * cos_phi, q.p2[2] - q.p1[2]);
            d2p_duv = q.phi_max * mk3(-dpdv.y, dpdv.x, 0.0f);
        } else if (kind == PH_Q_CYLINDER) {
            v = ph_div(p.z - q.z_min, q.z_max - q.z_min);
            dpdv = mk3(0.0f, 0.0f, q.z_max - q.z_min);
        } else if (kind == PH_Q_CONE) {
            v = ph_div(p.z, q.height);
            dpdv = mk3(ph_div(-p.x, 1.0f - v), ph_div(-p.y, 1.0f - v), q.height);
            d2p_duv = ph_div(q.phi_max, 1.0f - v) * mk3(p.y, -p.x, 0.0f);
        } else {
            v = ph_div(p.z - q.z_min, q.z_max - q.z_min);
            dpdv = (q.z_max - q.z_min) * mk3(ph_div(p.x, 2.0f * p.z), ph_div(p.y, 2.0f * p.z), 1.0f);
            d2p_duv = ((q.z_max - q.z_min) * q.phi_max) * mk3(ph_div(-p.y, 2.0f * p.z), ph_div(p.x, 2.0f * p.z), 0.0f);
            d2p_dvv = (-(q.z_max - q.z_min) * (q.z_max - q.z_min)) * mk3(ph_div(p.x, 4.0f * p.z * p.z), ph_div(p.y, 4.0f * p.z * p.z), 0.0f);
        }
        const f3 nn = normalize(cross(dpdu, dpdv));
        const float e1 = dot(dpdu, dpdu), f1 = dot(dpdu, dpdv), g1 = dot(dpdv, dpdv);
        const float e2 = dot(nn, d2p_duu), f2 = dot(nn, d2p_duv), g2 = dot(nn, d2p_dvv);
        const float inv_egf_1 = ph_div(1.0f, e1 * g1 - f1 * f1);
        dndu = ((f2 * f1 - e2 * g1) * inv_egf_1) * dpdu + ((e2 * f1 - f2 * e1) * inv_egf_1) * dpdv;
        dndv = ((g2 * f1 - f2 * g1) * inv_egf_1) * dpdu + ((f2 * f1 - g2 * e1) * inv_egf_1) * dpdv;
    }
    // SurfaceInteraction::new with wo = -ray.d of the OBJECT-space ray, then transform_surface_interaction
    f3 n = normalize(cross(dpdu, dpdv));
    if (q.flip) n = n * -1.0f;
    f3 wo = -q_xf_vec(q.w2o, rd);
    const float l2 = length_squared(wo);
    wo = (l2 == 0.0f) ? wo : wo / ph_sqrt(l2);   // Hit::new (interaction/mod.rs:137-156)
    {   // transform_point_with_abs_error (transform.rs:338-370)
        const float* m = q.o2w;
        const f3 pe = h.perr;
        const float x = p.x, y = p.y, z = p.z;
        const float xp = (m[0] * x + m[1] * y) + (m[2] * z + m[3]);
        const float yp = (m[4] * x + m[5] * y) + (m[6] * z + m[7]);
        const float zp = (m[8] * x + m[9] * y) + (m[10] * z + m[11]);
        const float wp = (m[12] * x + m[13] * y) + (m[14] * z + m[15]);
        const float g3 = kGamma3;
        s.p_error = mk3((g3 + 1.0f) * (pabs(m[0]) * pe.x + pabs(m[1]) * pe.y + pabs(m[2]) * pe.z) + g3 * (pabs(m[0] * x) + pabs(m[1] * y) + pabs(m[2] * z) + pabs(m[3])),
                        (g3 + 1.0f) * (pabs(m[4]) * pe.x + pabs(m[5]) * pe.y + pabs(m[6]) * pe.z) + g3 * (pabs(m[4] * x) + pabs(m[5] * y) + pabs(m[6] * z) + pabs(m[7])),
                        (g3 + 1.0f) * (pabs(m[8]) * pe.x + pabs(m[9]) * pe.y + pabs(m[10]) * pe.z) + g3 * (pabs(m[8] * x) + pabs(m[9] * y) + pabs(m[10] * z) + pabs(m[11])));
        s.p = (wp == 1.0f) ? mk3(xp, yp, zp) : mk3(xp, yp, zp) / wp;
    }
    s.wo = normalize(q_xf_vec(q.o2w, wo));
    s.n = normalize(q_xf_normal(q.w2o, n));
    s.dpdu = q_xf_vec(q.o2w, dpdu); s.dpdv = q_xf_vec(q.o2w, dpdv);
    s.dndu = q_xf_normal(q.w2o, dndu); s.dndv = q_xf_normal(q.w2o, dndv);
    s.u = u; s.v = v;
    *out = s;
}

}  // namespace ph
