// What the recursive integrators add to a vertex beyond the texture pass's record: the shading dn/du, dn/dv of a triangle hit, and the ray differentials of a specularly
// reflected or refracted ray (core/src/integrator/sampler_integrator.rs:79-238).  PH_DEV functions only: the Whitted kernels (whitted.h) and the surface probe (probe.hip) call them.
#pragma once
#include "texture.h"

namespace ph {

// dn/du, dn/dv of a triangle's shading geometry (triangle.rs:681-715; zero without per-vertex normals), in world space for an instanced hit (transform.rs:566-590)
PH_DEV void tri_shading_dn(const DeviceScene& sc, uint32_t tri_index, uint32_t inst, f3& dndu, f3& dndv) {
    dndu = mk3(0.0f, 0.0f, 0.0f); dndv = dndu;
    const float4* tp = reinterpret_cast<const float4*>(sc.tris + tri_index);
    const uint32_t prim = __float_as_uint(tp[0].w);
    const MeshRec m = sc.meshes[__float_as_uint(tp[2].w)];
    if (!(m.flags & PH_MESH_N)) return;
    const uint32_t i0 = sc.idx[3 * prim], i1 = sc.idx[3 * prim + 1], i2 = sc.idx[3 * prim + 2];
    const f3 n0 = ld3(sc.N + 3 * (size_t)i0), n1 = ld3(sc.N + 3 * (size_t)i1), n2 = ld3(sc.N + 3 * (size_t)i2);
    f2 uv0 = mk2(0.0f, 0.0f), uv1 = mk2(1.0f, 0.0f), uv2 = mk2(1.0f, 1.0f);
    if (m.flags & PH_MESH_UV) {
        uv0 = mk2(sc.UV[2 * (size_t)i0], sc.UV[2 * (size_t)i0 + 1]); uv1 = mk2(sc.UV[2 * (size_t)i1], sc.UV[2 * (size_t)i1 + 1]);
        uv2 = mk2(sc.UV[2 * (size_t)i2], sc.UV[2 * (size_t)i2 + 1]);
    }
    const f2 duv02 = mk2(uv0.x - uv2.x, uv0.y - uv2.y), duv12 = mk2(uv1.x - uv2.x, uv1.y - uv2.y);
    const f3 dn1 = n0 - n2, dn2 = n1 - n2;
    const float determinant = duv02.x * duv12.y - duv02.y * duv12.x;
    if (fabsf(determinant) < 1e-8f) {
        const f3 dn = cross(n2 - n0, n1 - n0);
        if (length_squared(dn) != 0.0f) coordinate_system(dn, dndu, dndv);
    } else {
        const float invdet = ph_div(1.0f, determinant);
        dndu = (duv12.y * dn1 - duv02.y * dn2) * invdet;
        dndv = (-duv12.x * dn1 + duv02.x * dn2) * invdet;
    }
    if (inst != 0u) {
        const InstRec& I = sc.instances[inst - 1u];
        if (!(I.flags & PH_INST_IDENTITY)) { dndu = xf_normal(I.w2i, dndu); dndv = xf_normal(I.w2i, dndv); }
    }
}

// The differentials of the ray specular_reflect / specular_transmit spawn (sampler_integrator.rs:96-119, :171-230) at a vertex {p, wo, ns} whose parent ray had the
// offset directions prx_d, pry_d: the vertex's dp/dx, dp/dy, du/dx .. dv/dy (compute_differentials) and shading dn/du, dn/dv; wi = the sampled direction;
// bsdf_eta = the BSDF's eta (read for a refracted ray only).
PH_DEV RayDiff specular_ray_differentials(f3 p, f3 wo, f3 ns, f3 wi, f3 dpdx, f3 dpdy, f3 dndu, f3 dndv, float dudx, float dvdx, float dudy, float dvdy, f3 prx_d, f3 pry_d,
                                          float bsdf_eta, bool transmit) {
    RayDiff r;
    r.rx_o = p + dpdx; r.ry_o = p + dpdy;
    f3 dndx = dndu * dudx + dndv * dvdx;
    f3 dndy = dndu * dudy + dndv * dvdy;
    const f3 dwodx = -prx_d - wo, dwody = -pry_d - wo;
    if (!transmit) {
        const float ddndx = dot(dwodx, ns) + dot(wo, dndx), ddndy = dot(dwody, ns) + dot(wo, dndy);
        r.rx_d = wi - dwodx + 2.0f * (dot(wo, ns) * dndx + ddndx * ns);
        r.ry_d = wi - dwody + 2.0f * (dot(wo, ns) * dndy + ddndy * ns);
    } else {
        float eta = ph_div(1.0f, bsdf_eta);
        f3 nn = ns;
        if (dot(wo, nn) < 0.0f) { eta = ph_div(1.0f, eta); nn = -nn; dndx = -dndx; dndy = -dndy; }
        const float ddndx = dot(dwodx, nn) + dot(wo, dndx), ddndy = dot(dwody, nn) + dot(wo, dndy);
        const float mu = eta * dot(wo, nn) - abs_dot(wi, nn);
        const float dmudx = (eta - ph_div(eta * eta * dot(wo, nn), abs_dot(wi, nn))) * ddndx;
        const float dmudy = (eta - ph_div(eta * eta * dot(wo, nn), abs_dot(wi, nn))) * ddndy;
        r.rx_d = wi - eta * dwodx + (mu * dndx + dmudx * nn);
        r.ry_d = wi - eta * dwody + (mu * dndy + dmudy * nn);
    }
    return r;
}

}  // namespace ph
