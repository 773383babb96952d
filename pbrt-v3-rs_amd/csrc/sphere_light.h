// Light::sample_li and Light::pdf_li where the light may be a DiffuseAreaLight whose shape is a quadric — a sphere (pbrt_hip_add_sphere_light), a disk or a cylinder
// (pbrt_hip_add_quadric_light): what the Whitted state kernel (whitted.h), the path integrator's sphere-light shade pass and light-distribution pass (wavefront.hip, spatial.h)
// and the light probes (probe.hip) call.  The reference's other three quadrics have no Shape::sample (todo!()) and cannot be lights.
#pragma once
#include "pt_device.h"

namespace ph {

// ---------------------------------------------------------------------------------------------------------------------------
// DiffuseAreaLight::sample_li (lights/src/diffuse.rs:114-129) on a Sphere: Sphere::sample_solid_angle (shapes/src/sphere.rs:344-410) — uniform over the cone the sphere
// subtends from the reference point, or uniform over the FULL sphere's area (Sphere::sample) where the point lies inside it — and the light's tail.  The z and phi cuts
// of a partial sphere enter through `area` alone: a sample may land on the part that is cut away, as in the reference.  `rev` = the shape's reverse_orientation (not
// QuadricRec::flip: the reference flips the sampled normal for reverse_orientation only, whatever the transform's handedness).
PH_DEV LiSample sphere_light_sample_li(const LightRec& l, const QuadricRec& q, bool rev, const SurfHit& hit, f2 u) {
    LiSample r;
    r.valid = false; r.pdf = 0.0f; r.wi = mk3(0, 0, 0); r.value = mks1(0.0f);
    r.vp = mk3(0, 0, 0); r.vperr = mk3(0, 0, 0); r.vn = mk3(0, 0, 0);
    const float* m = q.o2w;   // p_center = object_to_world.transform_point(Point3f::ZERO) (transform.rs:288-302)
    const float xc = m[0] * 0.0f + m[1] * 0.0f + m[2] * 0.0f + m[3], yc = m[4] * 0.0f + m[5] * 0.0f + m[6] * 0.0f + m[7];
    const float zc = m[8] * 0.0f + m[9] * 0.0f + m[10] * 0.0f + m[11], wc_ = m[12] * 0.0f + m[13] * 0.0f + m[14] * 0.0f + m[15];
    const f3 p_center = (wc_ == 1.0f) ? mk3(xc, yc, zc) : mk3(xc, yc, zc) / wc_;
    f3 p, n, p_error;
    float pdf;
    const float phi = kTwoPi * u.y;
    float sin_phi_, cos_phi_;
    d_sincos(phi, sin_phi_, cos_phi_);
    const f3 p_origin = offset_origin(hit.p, hit.p_error, hit.n, p_center - hit.p);
    if (distance_squared(p_origin, p_center) <= q.radius * q.radius) {   // inside: Sphere::sample, then the area pdf as a solid-angle one (shape.rs:64-84)
        const float z = 1.0f - 2.0f * u.x, rr = ph_sqrt(pmaxf(0.0f, 1.0f - z * z));   // uniform_sample_sphere
        f3 p_obj = q.radius * mk3(rr * cos_phi_, rr * sin_phi_, z);
        n = normalize(q_xf_normal(q.w2o, p_obj));
        if (rev) n = n * -1.0f;
        p_obj = p_obj * ph_div(q.radius, length(p_obj));
        f3 pe;
        p = xf_point_abs_err(q.o2w, p_obj, kGamma5 * vabs(p_obj), pe); p_error = pe;
        pdf = ph_div(1.0f, l.area);
        f3 wi = p - hit.p;
        if (length_squared(wi) == 0.0f) pdf = 0.0f;
        else { wi = normalize(wi); pdf *= ph_div(distance_squared(hit.p, p), abs_dot(n, -wi)); }
        if (__builtin_isinf(pdf)) pdf = 0.0f;
    } else {
        const float dc = length(hit.p - p_center), inv_dc = ph_div(1.0f, dc);
        const f3 wc = (p_center - hit.p) * inv_dc;
        f3 wc_x, wc_y;
        coordinate_system(wc, wc_x, wc_y);
        const float sin_theta_max = q.radius * inv_dc, sin_theta_max2 = sin_theta_max * sin_theta_max, inv_sin_theta_max = ph_div(1.0f, sin_theta_max);
        const float cos_theta_max = ph_sqrt(pmaxf(0.0f, 1.0f - sin_theta_max2));
        float cos_theta = (cos_theta_max - 1.0f) * u.x + 1.0f, sin_theta2 = 1.0f - cos_theta * cos_theta;
        if (sin_theta_max2 < 0.00068523f) { sin_theta2 = sin_theta_max2 * u.x; cos_theta = ph_sqrt(1.0f - sin_theta2); }   // sin^2(1.5 deg): the Taylor form
        const float cos_alpha = sin_theta2 * inv_sin_theta_max + cos_theta * ph_sqrt(pmaxf(0.0f, 1.0f - sin_theta2 * inv_sin_theta_max * inv_sin_theta_max));
        const float sin_alpha = ph_sqrt(pmaxf(0.0f, 1.0f - cos_alpha * cos_alpha));
        const f3 n_world = (sin_alpha * cos_phi_) * (-wc_x) + (sin_alpha * sin_phi_) * (-wc_y) + cos_alpha * (-wc);   // spherical_direction_in_coord_frame
        p = p_center + q.radius * n_world;
        p_error = kGamma5 * vabs(p);
        n = n_world;
        if (rev) n = n * -1.0f;
        pdf = ph_div(1.0f, kTwoPi * (1.0f - cos_theta_max));   // uniform_cone_pdf
    }
    f3 wi2 = p - hit.p;
    const float l2 = length_squared(wi2);
    if (pdf == 0.0f || l2 == 0.0f) return r;
    wi2 = wi2 / ph_sqrt(l2);
    r.wi = wi2; r.pdf = pdf; r.value = area_L(l, n, -wi2); r.vp = p; r.vperr = p_error; r.vn = n; r.valid = true;
    return r;
}
// ---------------------------------------------------------------------------------------------------------------------------
// DiffuseAreaLight::pdf_li (diffuse.rs:131-141) on a Sphere: Sphere::pdf_solid_angle (shapes/src/sphere.rs:462-475).  `qi`: the sphere's record in DeviceScene::quadrics.
// Outside, the pdf of the cone the FULL sphere subtends from hit.p: it does not depend on wi and is not zero for a direction that misses the sphere, so estimate_direct traces the
// BSDF-sampled ray in every case.  `radius` is the object-space radius against a world-space distance, whatever the transform scales, as in the reference.
// Inside (the offset reference point lies in or on the sphere) the reference writes `Shape::pdf_solid_angle(self, hit, wi)` inside `impl Shape for Sphere`, which resolves to this very
// function: it recurses until its stack ends and has no answer.  A DOCUMENTED DEPARTURE from a reference that crashes: what is built here is the counterpart of
// sample_solid_angle's inside branch and what upstream pbrt-v3 does, the trait's default (core/src/geometry/shape.rs:86-107) — hit.spawn_ray(wi) against the sphere, test_alpha = false,
// z and phi cuts included, then distance^2 / (|n . -wi| * area), 0 for a miss and for an infinite value.  The intersection is the shape's own leaf test and surface tail (quadric.h:
// quadric_surface, what make_surface_hit_q calls), so the point and the normal are the ones a traced ray would report.
// Shape::pdf_solid_angle, the trait's default (core/src/geometry/shape.rs:86-107), on quadric `qi`: the sphere's inside case below, and a disk's or a cylinder's pdf_li at every
// reference point (neither shape overrides it).
PH_DEV float quadric_pdf_solid_angle(const DeviceScene& sc, const LightRec& l, uint32_t qi, const SurfHit& hit, f3 wi) {
    const RayIn ray = spawn_ray(hit, wi);
    float rod[6] = {ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz};
    QSurf qs;
    quadric_surface(sc.self, qi, rod, &qs);
    if (!qs.hit) return 0.0f;
    const float pdf = ph_div(distance_squared(hit.p, qs.p), abs_dot(qs.n, -wi) * l.area);
    return __builtin_isinf(pdf) ? 0.0f : pdf;
}
PH_DEV float sphere_light_pdf_li(const DeviceScene& sc, const LightRec& l, uint32_t qi, const SurfHit& hit, f3 wi) {
    const QuadricRec& q = sc.quadrics[qi];
    const float* m = q.o2w;   // p_center = object_to_world.transform_point(Point3f::ZERO) (transform.rs:288-302)
    const float xc = m[0] * 0.0f + m[1] * 0.0f + m[2] * 0.0f + m[3], yc = m[4] * 0.0f + m[5] * 0.0f + m[6] * 0.0f + m[7];
    const float zc = m[8] * 0.0f + m[9] * 0.0f + m[10] * 0.0f + m[11], wc_ = m[12] * 0.0f + m[13] * 0.0f + m[14] * 0.0f + m[15];
    const f3 p_center = (wc_ == 1.0f) ? mk3(xc, yc, zc) : mk3(xc, yc, zc) / wc_;
    const f3 p_origin = offset_origin(hit.p, hit.p_error, hit.n, p_center - hit.p);
    if (distance_squared(p_origin, p_center) <= q.radius * q.radius) return quadric_pdf_solid_angle(sc, l, qi, hit, wi);
    const float sin_theta_max2 = ph_div(q.radius * q.radius, distance_squared(hit.p, p_center));
    const float cos_theta_max = ph_sqrt(pmaxf(0.0f, 1.0f - sin_theta_max2));
    return ph_div(1.0f, kTwoPi * (1.0f - cos_theta_max));   // uniform_cone_pdf
}
// ---------------------------------------------------------------------------------------------------------------------------
// Disk::sample (shapes/src/disk.rs:214-234) and Cylinder::sample (shapes/src/cylinder.rs:322-348), out of line like the shapes' intersection (quadric.h): the callers are at their
// register budgets already.  out[0..3] the world-space point, [3..6] its error bound, [6..9] the normal, flipped for reverse_orientation only.  The disk's sample ignores
// inner_radius and phi_max, the cylinder's normal comes from the point before its re-projection: as in the reference.  Sine and cosine in f64, rounded once.
static __device__ __noinline__ void quadric_shape_sample(const DeviceScene* dsc, uint32_t qi, uint32_t rev, float u0, float u1, float* out) {
    const QuadricRec& q = dsc->quadrics[qi];
    f3 p_obj, p_obj_error, n_obj;
    if (q.kind == PH_Q_DISK) {
        const f2 pd = concentric_sample_disk(mk2(u0, u1));
        p_obj = mk3(pd.x * q.radius, pd.y * q.radius, q.height);
        n_obj = mk3(0.0f, 0.0f, 1.0f);
        p_obj_error = mk3(0.0f, 0.0f, 0.0f);
    } else {
        const float z = (1.0f - u0) * q.z_min + u0 * q.z_max;   // lerp (core/src/pbrt/common.rs:167-173)
        const float phi = u1 * q.phi_max;
        float sin_phi_, cos_phi_;
        d_sincos(phi, sin_phi_, cos_phi_);
        p_obj = mk3(q.radius * cos_phi_, q.radius * sin_phi_, z);
        n_obj = mk3(p_obj.x, p_obj.y, 0.0f);
        const float hit_rad = ph_sqrt(p_obj.x * p_obj.x + p_obj.y * p_obj.y);
        p_obj.x *= ph_div(q.radius, hit_rad); p_obj.y *= ph_div(q.radius, hit_rad);
        p_obj_error = kGamma3 * vabs(mk3(p_obj.x, p_obj.y, 0.0f));
    }
    f3 n = normalize(q_xf_normal(q.w2o, n_obj));
    if (rev) n = n * -1.0f;
    f3 pe;
    const f3 p = xf_point_abs_err(q.o2w, p_obj, p_obj_error, pe);
    out[0] = p.x; out[1] = p.y; out[2] = p.z; out[3] = pe.x; out[4] = pe.y; out[5] = pe.z; out[6] = n.x; out[7] = n.y; out[8] = n.z;
}
// DiffuseAreaLight::sample_li (diffuse.rs:114-129) on a Disk or a Cylinder: the trait's default Shape::sample_solid_angle (core/src/geometry/shape.rs:64-80) over the shape's
// sample — uniform over the FULL shape's area at every reference point, the cuts enter through `area` alone — and the light's tail.
PH_DEV LiSample quadric_light_sample_li(const DeviceScene& sc, const LightRec& l, uint32_t qi, bool rev, const SurfHit& hit, f2 u) {
    LiSample r;
    r.valid = false; r.pdf = 0.0f; r.wi = mk3(0, 0, 0); r.value = mks1(0.0f);
    r.vp = mk3(0, 0, 0); r.vperr = mk3(0, 0, 0); r.vn = mk3(0, 0, 0);
    float s[9];
    quadric_shape_sample(sc.self, qi, rev ? 1u : 0u, u.x, u.y, s);
    const f3 p = mk3(s[0], s[1], s[2]), p_error = mk3(s[3], s[4], s[5]), n = mk3(s[6], s[7], s[8]);
    float pdf = ph_div(1.0f, l.area);
    f3 wi = p - hit.p;
    if (length_squared(wi) == 0.0f) pdf = 0.0f;
    else {
        wi = normalize(wi);
        pdf *= ph_div(distance_squared(hit.p, p), abs_dot(n, -wi));
        if (__builtin_isinf(pdf)) pdf = 0.0f;
    }
    f3 wi2 = p - hit.p;
    const float l2 = length_squared(wi2);
    if (pdf == 0.0f || l2 == 0.0f) return r;
    wi2 = wi2 / ph_sqrt(l2);
    r.wi = wi2; r.pdf = pdf; r.value = area_L(l, n, -wi2); r.vp = p; r.vperr = p_error; r.vn = n; r.valid = true;
    return r;
}
// Light::sample_li as the Whitted light loop calls it.  Only the QUADRIC instantiation knows that an area light's shape may be a sphere, a disk or a cylinder: the light's
// primitive slot then leads to a PH_MESH_QUADRIC record whose vert_base is the QuadricRec.  light_sample_li itself (pt_device.h) stays as the path integrator's kernels inline it.
template <bool QUADRIC> PH_DEV LiSample wh_light_sample_li(const DeviceScene& sc, const LightRec& l, const SurfHit& hit, f2 u) {
    if (QUADRIC && l.type == PH_L_AREA) {
        const MeshRec m = sc.meshes[sc.tri_mesh[l.prim]];
        if (m.flags & PH_MESH_QUADRIC) {
            const QuadricRec& q = sc.quadrics[m.vert_base];
            if (q.kind == PH_Q_SPHERE) return sphere_light_sample_li(l, q, (m.flags & PH_MESH_REV) != 0u, hit, u);
            return quadric_light_sample_li(sc, l, m.vert_base, (m.flags & PH_MESH_REV) != 0u, hit, u);   // a disk or a cylinder (pbrt_hip_add_quadric_light)
        }
    }
    return light_sample_li<true>(sc, l, hit, u);
}
// Light::pdf_li as the path integrator's sphere-light shade pass calls it (wavefront.hip, ShadeRowSphereLights): the sphere's own pdf where the light's shape is one, the trait's
// default where it is a disk or a cylinder, else
// light_pdf_li as every other shade kernel inlines it.  Its sample_li is wh_light_sample_li<true> above: the same function the Whitted light loop calls.
PH_DEV float sl_light_pdf_li(const DeviceScene& sc, const LightRec& l, const SurfHit& hit, f3 wi) {
    if (l.type == PH_L_AREA) {
        const MeshRec m = sc.meshes[sc.tri_mesh[l.prim]];
        if (m.flags & PH_MESH_QUADRIC)
            return sc.quadrics[m.vert_base].kind == PH_Q_SPHERE ? sphere_light_pdf_li(sc, l, m.vert_base, hit, wi) : quadric_pdf_solid_angle(sc, l, m.vert_base, hit, wi);
    }
    return light_pdf_li<true>(sc, l, hit, wi);
}

}  // namespace ph
