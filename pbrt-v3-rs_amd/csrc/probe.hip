// Test hooks (include/pbrt_hip.h: pbrt_hip_bsdf_probe_batch, pbrt_hip_sampler_value_batch, pbrt_hip_light_probe_batch, pbrt_hip_sphere_light_probe_batch, pbrt_hip_raysort_probe, pbrt_hip_texture_probe_batch,
// pbrt_hip_bump_probe_batch, pbrt_hip_traverse_probe, pbrt_hip_surface_probe_batch, pbrt_hip_spatial_probe_begin / _batch / _voxel): the device's BSDF, sampler, light, texture and hit-to-interaction code,
// the spatial light distribution, the ray binning between wavefront rounds and the traversal kernel's queue on explicit inputs.
// Each kernel only unpacks its arguments and calls the PH_DEV functions the render kernels call (pt_device.h, bsdf_general.h, wf_device.h, texture.h, sphere_light.h, shading_diff.h, spatial.h); no formula lives here.
// Each entry point makes its checks, then upload_scene, then names its device arrays on a ProbeStage (probe_stage.h), launches and returns the stage's finish().
#define PH_OUTLINE_MATH 1
#include "scene_host.h"
#include "pt_device.h"
#include "bsdf_general.h"
#include "wf_device.h"
#include "texture.h"
#include "sphere_light.h"
#include "shading_diff.h"
#include "spatial.h"
#include "film_plan.h"
#include "probe_stage.h"
#include <cstring>
#include <type_traits>
#include <vector>

namespace ph {

struct ProbeFrame { float ns[3], ng[3], ss[3]; };
#define PH_PROBE_BLOCK 128

// GEN = true: GBsdf as shade_kernel<true> makes it (make_gbsdf); GEN = false: the one-lobe Bsdf of shade_kernel<false> (make_bsdf), which has no flags and no sampled type:
// the host admits only flags the lobe matches, and a sample that succeeded reports the lobe's type as BsdfOps<false>::sample_all does
template <bool GEN>
__global__ __launch_bounds__(PH_PROBE_BLOCK) void bsdf_probe_kernel(DeviceScene sc, uint32_t material, int op, uint32_t n, const float* wo_in, const float* wi_in, const float* u_in,
                                                                   const uint32_t* flags_in, ProbeFrame fr, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SurfHit si;
    si.p = mk3(0.0f, 0.0f, 0.0f); si.p_error = si.p; si.wo = si.p; si.time = 0.0f; si.prim = 0u;
    si.ns = ld3(fr.ns); si.n = ld3(fr.ng); si.dpdu_s = ld3(fr.ss);
    const f3 wo = ld3(wo_in + 3 * (size_t)i), wi = ld3(wi_in + 3 * (size_t)i);
    const f2 u = mk2(u_in[2 * (size_t)i], u_in[2 * (size_t)i + 1]);
    const uint32_t flags = flags_in[i];
    float* o = out + 8 * (size_t)i;
    for (int k = 0; k < 8; k++) o[k] = 0.0f;
    if (GEN) {
        const GBsdf b = make_gbsdf(sc, si, material);
        if (op == 0) {
            const spec f = bsdf_f(b, wo, wi, flags);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = bsdf_pdf(b, wo, wi, flags);
        } else if (op == 1) {
            spec f; float pdf; f3 w; uint32_t st;
            bsdf_sample_f(b, wo, u, flags, f, pdf, w, st);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = pdf; o[4] = w.x; o[5] = w.y; o[6] = w.z; o[7] = (float)st;
        } else {
            o[0] = (float)bsdf_num_components(b, flags); o[1] = (float)b.n; o[2] = b.eta;
        }
    } else {
        const Bsdf b = make_bsdf(sc, si, material);
        if (op == 0) {
            const spec f = bsdf_f(b, wo, wi);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = bsdf_pdf(b, wo, wi);
        } else if (op == 1) {
            spec f; float pdf; f3 w;
            bsdf_sample_f(b, wo, u, f, pdf, w);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = pdf; o[4] = w.x; o[5] = w.y; o[6] = w.z; o[7] = pdf == 0.0f ? 0.0f : (float)(BX_REFL | BX_DIFF);
        } else {
            o[0] = b.has_bxdf ? 1.0f : 0.0f; o[1] = o[0]; o[2] = 1.0f;
        }
    }
}

// cursor_for + sampler_dim as the render kernels pair them; use_lds: the block stages the first PH_LDS_DIMS Halton dimensions like shade_kernel does
__global__ __launch_bounds__(256) void sampler_value_kernel(DeviceScene sc, SamplerRec sp, uint32_t n, const int* xy, const uint32_t* sample, const uint32_t* dim, int use_lds, float* out) {
    __shared__ HaltonLds halton_lds;
    const HaltonLds* hl = nullptr;
    if (use_lds && sp.kind == 0) { halton_lds_fill(&halton_lds, sc); hl = &halton_lds; }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SamplerCursor c = cursor_for(sc, sp, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], sample[i], dim[i], hl);
    out[i] = sampler_dim(sc, sp, c, c.dim);
}

// What the two light probe kernels share.  The reference point: a SurfHit that holds what the light code reads (p, p_error, n, time), from 10 floats ...
PH_DEV SurfHit light_probe_ref(const float* rf) {
    SurfHit hit;
    hit.p = ld3(rf); hit.p_error = ld3(rf + 3); hit.n = ld3(rf + 6); hit.time = rf[9];
    hit.wo = mk3(0.0f, 0.0f, 0.0f); hit.ns = hit.n; hit.dpdu_s = hit.wo; hit.prim = 0u;
    return hit;
}
// ... and op 0's part of the output row: the LiSample, then the shadow ray shade_kernel makes next if it is valid
PH_DEV void put_li_sample(float* o, const SurfHit& hit, const LiSample& r) {
    o[0] = r.wi.x; o[1] = r.wi.y; o[2] = r.wi.z; o[3] = r.pdf; o[4] = r.value.r; o[5] = r.value.g; o[6] = r.value.b; o[7] = r.valid ? 1.0f : 0.0f;
    o[8] = r.vp.x; o[9] = r.vp.y; o[10] = r.vp.z; o[11] = r.vperr.x; o[12] = r.vperr.y; o[13] = r.vperr.z; o[14] = r.vn.x; o[15] = r.vn.y; o[16] = r.vn.z;
    if (!r.valid) return;
    const RayIn sr = spawn_ray_to_hit(hit, r.vp, r.vperr, r.vn);
    o[17] = sr.ox; o[18] = sr.oy; o[19] = sr.oz; o[20] = sr.dx; o[21] = sr.dy; o[22] = sr.dz; o[23] = sr.t_max;
}
// VARIANT 0: light_le / light_sample_li / light_pdf_li<true>, as the textured shade kernels and spatial_compute_kernel instantiate them; 1: the <false> instantiations of the
// texture-free kernels; 2: wh_light_sample_li<true>, the Whitted light loop's (op 0 only).
// PBRT_HIP_LIGHT_PROBE_STRIDE floats out per probe, zeroed first (include/pbrt_hip.h gives the layout)
template <int VARIANT>
__global__ __launch_bounds__(PH_PROBE_BLOCK) void light_probe_kernel(DeviceScene sc, uint32_t light, int op, uint32_t n, const float* ref_in, const float* u_in, const float* wi_in, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr bool MAP = VARIANT != 1;
    const SurfHit hit = light_probe_ref(ref_in + 10 * (size_t)i);
    const f2 u = mk2(u_in[2 * (size_t)i], u_in[2 * (size_t)i + 1]);
    const f3 wi = ld3(wi_in + 3 * (size_t)i);
    const LightRec& l = sc.lights[light];
    float* o = out + PBRT_HIP_LIGHT_PROBE_STRIDE * (size_t)i;
    for (int k = 0; k < PBRT_HIP_LIGHT_PROBE_STRIDE; k++) o[k] = 0.0f;
    if (op == 0) {
        const LiSample r = VARIANT == 2 ? wh_light_sample_li<true>(sc, l, hit, u) : light_sample_li<MAP>(sc, l, hit, u);
        put_li_sample(o, hit, r);
    } else if (op == 1) {
        o[0] = light_pdf_li<MAP>(sc, l, hit, wi);
    } else {
        const spec le = light_le<MAP>(sc, l, wi);
        o[0] = le.r; o[1] = le.g; o[2] = le.b;
    }
}
// Light::sample_li (op 0) and Light::pdf_li (op 1) of a light whose shape is a quadric (sphere, disk, cylinder) as the path integrator's sphere-light shade pass calls them (wavefront.hip, ShadeRowSphereLights): wh_light_sample_li<true> and
// sl_light_pdf_li (sphere_light.h).  Inputs and output layout are light_probe_kernel's.
__global__ __launch_bounds__(PH_PROBE_BLOCK) void sphere_light_probe_kernel(DeviceScene sc, uint32_t light, int op, uint32_t n, const float* ref_in, const float* u_in, const float* wi_in, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SurfHit hit = light_probe_ref(ref_in + 10 * (size_t)i);
    const LightRec& l = sc.lights[light];
    float* o = out + PBRT_HIP_LIGHT_PROBE_STRIDE * (size_t)i;
    for (int k = 0; k < PBRT_HIP_LIGHT_PROBE_STRIDE; k++) o[k] = 0.0f;
    if (op == 0) {
        const LiSample r = wh_light_sample_li<true>(sc, l, hit, mk2(u_in[2 * (size_t)i], u_in[2 * (size_t)i + 1]));
        put_li_sample(o, hit, r);
    } else {
        o[0] = sl_light_pdf_li(sc, l, hit, ld3(wi_in + 3 * (size_t)i));
    }
}

// curve_test, then — closest-hit mode, on a hit — curve_surface (curve.h) for quadric slot `qi` (a curve segment), each ray with its own t_max: the two calls the traversal kernel's leaf
// step and make_surface_hit_q make, with the hit's t, u, v carried from one to the other as HitOut carries them
__global__ __launch_bounds__(PH_PROBE_BLOCK) void curve_probe_kernel(DeviceScene sc, uint32_t qi, uint32_t shadow, uint32_t n, const RayIn* rays, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RayIn ray = load_ray(rays + i);
    float* o = out + PBRT_HIP_CURVE_PROBE_STRIDE * (size_t)i;
    for (int k = 0; k < PBRT_HIP_CURVE_PROBE_STRIDE; k++) o[k] = 0.0f;
    const QTest qt = curve_test(sc.self, qi, ray.ox, ray.oy, ray.oz, ray.t_max, ray.dx, ray.dy, ray.dz, shadow);
    if (!qt.hit) return;
    o[0] = 1.0f;
    if (shadow) return;
    o[1] = qt.t; o[2] = qt.u; o[3] = qt.v;
    float rtuv[9] = {ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, qt.t, qt.u, qt.v};
    QSurf qs;
    curve_surface(sc.self, qi, rtuv, &qs);
    o[4] = qs.p.x; o[5] = qs.p.y; o[6] = qs.p.z; o[7] = qs.p_error.x; o[8] = qs.p_error.y; o[9] = qs.p_error.z;
    o[10] = qs.dpdu.x; o[11] = qs.dpdu.y; o[12] = qs.dpdu.z; o[13] = qs.dpdv.x; o[14] = qs.dpdv.y; o[15] = qs.dpdv.z; o[16] = qs.n.x; o[17] = qs.n.y; o[18] = qs.n.z;
}

// The hit-to-interaction stage on explicit hits (include/pbrt_hip.h: pbrt_hip_surface_probe_batch gives the layouts).  VARIANT 0: make_surface_hit (by prim), 1: make_surface_hit_any
// (leaf record, instances), 2: make_surface_hit_q<true> (scenes with quadric shapes); everything after the interaction is the texture pass's / the Whitted kernels' own sequence of calls:
// hit_tex_ctx or tex_ctx_from, camera_ray_differentials, tri_shading_dn, hit_bump or bump_shading, spawn_ray, spawn_ray_to_hit, specular_ray_differentials.  The camera travels by value.
PH_DEV void put3(float* o, f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
PH_DEV void put_ray(float* o, const RayIn& r) { o[0] = r.ox; o[1] = r.oy; o[2] = r.oz; o[3] = r.t_max; o[4] = r.dx; o[5] = r.dy; o[6] = r.dz; o[7] = r.time; }
template <int VARIANT>
__global__ __launch_bounds__(PH_TEX_LDS_THREADS) void surface_probe_kernel(DeviceScene sc, CameraRec cam, uint32_t spp, int op, uint32_t tex, uint32_t camera_ray, uint32_t n, const RayIn* rays,
                                                                            const PbrtHipHit* hits, const float* aux, float* out) {
    if (op == 2) noise_lds_fill();   // (the one op that evaluates a texture; uniform over the grid)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RayIn ray = load_ray(rays + i);
    const float4* hp = reinterpret_cast<const float4*>(hits + i);
    const float4 h0 = hp[0], h1 = hp[1];
    const uint32_t prim = __float_as_uint(h0.y), tri_index = __float_as_uint(h1.y), inst = __float_as_uint(h1.z);
    const f3 ro = mk3(ray.ox, ray.oy, ray.oz), rd = mk3(ray.dx, ray.dy, ray.dz), bary = mk3(h0.z, h0.w, h1.x);
    const float* a = aux + PBRT_HIP_SURFACE_PROBE_AUX * (size_t)i;
    float* o = out + PBRT_HIP_SURFACE_PROBE_STRIDE * (size_t)i;
    for (int k = 0; k < PBRT_HIP_SURFACE_PROBE_STRIDE; k++) o[k] = 0.0f;
    MeshRec m;
    QSurf qs; qs.hit = 0u;
    SurfHit si;
    if (VARIANT == 0) { si = make_surface_hit(sc, rd, ray.time, prim, bary.x, bary.y, bary.z); m = sc.meshes[sc.tri_mesh[prim]]; }
    else if (VARIANT == 1) si = make_surface_hit_any(sc, rd, ray.time, tri_index, inst, bary.x, bary.y, bary.z, m);
    else si = make_surface_hit_q<true>(sc, ro, rd, ray.time, tri_index, inst, bary.x, bary.y, bary.z, m, &qs, h0.x);
    const bool on_quadric = VARIANT == 2 && (m.flags & PH_MESH_QUADRIC) != 0u;
    const f2 p_film = mk2(a[0], a[1]), lens = mk2(a[2], a[3]);
    const f3 wi = ld3(a + 4);
    if (op == 0) {
        put3(o, si.p); put3(o + 3, si.p_error); put3(o + 6, si.wo); put3(o + 9, si.n); put3(o + 12, si.ns); put3(o + 15, si.dpdu_s);
        o[18] = si.time; o[19] = __uint_as_float(si.prim);
    } else if (op == 1 || op == 2) {
        const TexCtx ctx = on_quadric ? tex_ctx_from(&cam, spp, mk2(qs.u, qs.v), qs.dpdu, qs.dpdv, si.p, si.n, ro, rd, p_film, lens, camera_ray)
                                      : hit_tex_ctx(sc.self, &cam, spp, tri_index, inst, bary, si.p, si.n, ro, rd, p_film, lens, camera_ray);
        if (op == 1) {
            f3 dpdu, dpdv, dndu, dndv;
            if (on_quadric) { dpdu = qs.dpdu; dpdv = qs.dpdv; dndu = qs.dndu; dndv = qs.dndv; }
            else {   // the geometric dp/du, dp/dv as whitted_vertex_kernel takes them: tri_dpdu on the leaf record, carried to world space for an instance
                const float4* tp = reinterpret_cast<const float4*>(sc.tris + tri_index);
                const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                const uint32_t rprim = __float_as_uint(ta.w);
                TriVerts t;
                t.p0 = mk3(ta.x, ta.y, ta.z); t.p1 = mk3(tb.x, tb.y, tb.z); t.p2 = mk3(tc.x, tc.y, tc.z);
                t.i0 = t.i1 = t.i2 = 0;
                if (m.flags & PH_MESH_UV) { t.i0 = sc.idx[3 * rprim]; t.i1 = sc.idx[3 * rprim + 1]; t.i2 = sc.idx[3 * rprim + 2]; }
                tri_dpdu(sc, m, t, dpdu, dpdv);
                if (inst != 0u) {
                    const InstRec& I = sc.instances[inst - 1u];
                    if (!(I.flags & PH_INST_IDENTITY)) { dpdu = xf_vec(I.i2w, dpdu); dpdv = xf_vec(I.i2w, dpdv); }
                }
                tri_shading_dn(sc, tri_index, inst, dndu, dndv);
            }
            o[0] = ctx.uv.x; o[1] = ctx.uv.y; put3(o + 2, dpdu); put3(o + 5, dpdv);
            o[8] = ctx.dudx; o[9] = ctx.dvdx; o[10] = ctx.dudy; o[11] = ctx.dvdy; put3(o + 12, ctx.dpdx); put3(o + 15, ctx.dpdy);
            if (camera_ray) {
                const RayDiff rdf = camera_ray_differentials(cam, p_film, lens, ro, rd, spp);
                put3(o + 18, rdf.rx_o); put3(o + 21, rdf.ry_o); put3(o + 24, rdf.rx_d); put3(o + 27, rdf.ry_d);
            }
            put3(o + 30, dndu); put3(o + 33, dndv);
        } else {
            BumpOut bo;
            if (on_quadric) {
                if (camera_ray) bump_shading<false, false>(sc.self, tex, ctx, si.p, si.n, si.ns, si.dpdu_s, qs.dpdv, qs.dndu, qs.dndv, &bo);
                else bump_shading<false, true>(sc.self, tex, ctx, si.p, si.n, si.ns, si.dpdu_s, qs.dpdv, qs.dndu, qs.dndv, &bo);
            } else {
                BumpIn bi; bi.tex = tex; bi.tri_index = tri_index; bi.inst = inst; bi.bary = bary;
                bi.p = si.p; bi.n = si.n; bi.ns = si.ns; bi.dpdu_s = si.dpdu_s; bi.c = ctx;
                if (camera_ray) hit_bump<false, false>(sc.self, &bi, &bo);   // the texture pass's instantiation for camera rays ...
                else hit_bump<false, true>(sc.self, &bi, &bo);               // ... and for every later round
            }
            put3(o, bo.ns); put3(o + 3, bo.dpdu_s);
        }
    } else if (op == 3) {
        put_ray(o, spawn_ray(si, wi));
        put_ray(o + 8, spawn_ray_to_hit(si, ld3(a + 7), ld3(a + 10), ld3(a + 13)));
    } else {
        const RayDiff r = specular_ray_differentials(si.p, si.wo, si.ns, wi, ld3(a + 26), ld3(a + 29), ld3(a + 32), ld3(a + 35), a[22], a[23], a[24], a[25], ld3(a + 16), ld3(a + 19), a[38],
                                                     a[39] != 0.0f);
        put3(o, r.rx_o); put3(o + 3, r.ry_o); put3(o + 6, r.rx_d); put3(o + 9, r.ry_d);
    }
}

// the 15 floats of pbrt_hip_texture_eval_batch.  NODIFF: the context of every ray but a camera ray, as tex_ctx_from and alpha_accept make it — the nine derivative fields are zero
// (the NODIFF evaluator skips only the image maps' filtered look-up; the procedural classes and bump_shading read the fields)
template <bool NODIFF>
PH_DEV TexCtx probe_tex_ctx(const float* q) {
    TexCtx c; c.uv = mk2(q[0], q[1]); c.p = mk3(q[6], q[7], q[8]);
    c.dudx = c.dvdx = c.dudy = c.dvdy = 0.0f; c.dpdx = mk3(0.0f, 0.0f, 0.0f); c.dpdy = c.dpdx;
    if (!NODIFF) { c.dudx = q[2]; c.dvdx = q[3]; c.dudy = q[4]; c.dvdy = q[5]; c.dpdx = mk3(q[9], q[10], q[11]); c.dpdy = mk3(q[12], q[13], q[14]); }
    return c;
}
// VARIANT 0 .. 3: tex_eval<SIMPLE, NODIFF> with SIMPLE = VARIANT >> 1, NODIFF = VARIANT & 1, the four instantiations of the texture pass and the alpha test; 4: alpha_prog_r, the lean
// alpha test's evaluator (red channel).  One kernel per variant: each instantiation of the evaluator owns an LDS value stack
template <int VARIANT>
__global__ __launch_bounds__(PH_TEX_LDS_THREADS) void texture_probe_kernel(DeviceScene sc, uint32_t tex, uint32_t n, const float* in, float* out) {
    noise_lds_fill();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TexCtx c = probe_tex_ctx<(VARIANT & 1) != 0 || VARIANT == 4>(in + 15 * (size_t)i);
    spec v;
    if (VARIANT == 4) v = mks(alpha_prog_r(sc, tex, c.uv), 0.0f, 0.0f);
    else v = tex_eval<(VARIANT & 2) != 0, (VARIANT & 1) != 0>(sc.self, tex, c);
    out[3 * (size_t)i] = v.r; out[3 * (size_t)i + 1] = v.g; out[3 * (size_t)i + 2] = v.b;
}
// bump_shading<SIMPLE, NODIFF> on an explicit context and shading frame: in = 15 context floats, then n, ns, dpdu_s, dpdv_s, dndu, dndv; out = the new ns and dpdu_s
template <int VARIANT>
__global__ __launch_bounds__(PH_TEX_LDS_THREADS) void bump_probe_kernel(DeviceScene sc, uint32_t tex, uint32_t n, const float* in, float* out) {
    noise_lds_fill();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in + 33 * (size_t)i;
    const TexCtx c = probe_tex_ctx<(VARIANT & 1) != 0>(q);
    BumpOut b;
    bump_shading<(VARIANT & 2) != 0, (VARIANT & 1) != 0>(sc.self, tex, c, c.p, ld3(q + 15), ld3(q + 18), ld3(q + 21), ld3(q + 24), ld3(q + 27), ld3(q + 30), &b);
    float* o = out + 6 * (size_t)i;
    o[0] = b.ns.x; o[1] = b.ns.y; o[2] = b.ns.z; o[3] = b.dpdu_s.x; o[4] = b.dpdu_s.y; o[5] = b.dpdu_s.z;
}

// The film probe's stand-in for an integrator: the records of one band, [sample][pixel of the band], from the caller's arrays [sample][pixel of the rank]; a NaN p_film.x stays
// the "no sample taken" mark.  The rounded-up mark is raygen's own (film_plan.h).
__global__ __launch_bounds__(256) void film_probe_fill_kernel(uint32_t band_px, uint32_t px0, uint32_t rank_px, uint32_t spp, const int2* px_xy, const float* L, const float* p_film,
                                                              float4* rec_L, float* rec_py, uint8_t* px_rounded) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (uint64_t)band_px * spp) return;
    const uint32_t s = (uint32_t)(gid / band_px), pix = (uint32_t)(gid % band_px);
    const size_t src = (size_t)s * rank_px + px0 + pix, dst = (size_t)s * band_px + pix;
    const float px = p_film[2 * src], py = p_film[2 * src + 1];
    if (px != px) { rec_L[dst] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u)); rec_py[dst] = 0.0f; return; }
    rec_L[dst] = make_float4(L[3 * src], L[3 * src + 1], L[3 * src + 2], px);
    rec_py[dst] = py;
    const int2 xy = px_xy[pix];
    phfilm::mark_rounded_up(px_rounded, pix, xy.x, xy.y, px, py);
}

// The spatial light distribution on explicit points (spatial.h).  The claim pass: spatial_voxel_of + spatial_claim as spatial_mark_kernel pairs them, the voxel written out as
// lookup's three coordinates (v = (x * nv[1] + y) * nv[2] + z taken apart as spatial_compute_kernel does).  Between the two runs the render's own spatial_compute_kernel.
__global__ __launch_bounds__(256) void spatial_probe_mark_kernel(SpatialRec sr, uint32_t n, const float* p_in, int32_t* out_pi) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t v = spatial_voxel_of(sr, ld3(p_in + 3 * (size_t)i));
        spatial_claim(sr, v);
        int32_t* o = out_pi + 3 * (size_t)i;
        o[2] = (int32_t)(v % (uint32_t)sr.nv[2]);
        o[1] = (int32_t)((v / (uint32_t)sr.nv[2]) % (uint32_t)sr.nv[1]);
        o[0] = (int32_t)(v / ((uint32_t)sr.nv[2] * (uint32_t)sr.nv[1]));
    }
}
// The pick: spatial_pick_light as shade_kernel calls it in the rows compiled for the spatial distribution; sr.enabled = 0 reads the scene-wide table (strategies 0 and 1)
__global__ __launch_bounds__(256) void spatial_probe_pick_kernel(DeviceScene sc, SpatialRec sr, uint32_t n, const float* p_in, const float* u_in, uint32_t* out_light, float* out_pdf) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const LightPick pick = spatial_pick_light<true>(sc, sr, ld3(p_in + 3 * (size_t)i), u_in[i]);
        out_light[i] = pick.light_num; out_pdf[i] = pick.pdf;
    }
}

}  // namespace ph

using namespace phost;

namespace {
// f(std::integral_constant<int, V>()) for the V of 0 .. N - 1 that `variant` is, so that a kernel template takes it: [&](auto v) { ... kernel<v()> ... }.  The caller has refused every other value.
template <int N, class F> void with_variant(int variant, F&& f) {
    if constexpr (N > 1) if (variant < N - 1) return with_variant<N - 1>(variant, f);
    f(std::integral_constant<int, N - 1>());
}
// a caller's rays as the kernels read them (load_ray): PbrtHipRay and ph::RayIn are one layout under two names
static_assert(sizeof(PbrtHipRay) == sizeof(ph::RayIn), "PbrtHipRay is ph::RayIn's layout");
const ph::RayIn* device_rays(const PbrtHipRay* rays) { return reinterpret_cast<const ph::RayIn*>(rays); }
dim3 probe_grid(uint64_t n) { return dim3((uint32_t)((n + PH_PROBE_BLOCK - 1) / PH_PROBE_BLOCK)); }   // of blocks of PH_PROBE_BLOCK threads, one thread per probe
bool material_reads_a_texture(const MaterialRec& m) {
    return m.textured || m.kd_tex1 || m.bump_tex1 || m.sigma_tex1 || m.opacity_tex1 || m.amount_tex1 || m.rt_mode || m.refl_tex1 || m.trans_tex1 || m.index_tex1;
}
}  // namespace

// the two texture probes share their checks and their launch: `in_stride` floats in and `out_stride` floats out per probe
namespace {
template <class Launch>
int texture_probe_common(PbrtHipScene* s, const char* who, uint32_t tex, int variant, int n_variants, uint64_t n, const float* in, size_t in_stride, float* out, size_t out_stride, Launch launch) {
    const std::string w(who);
    if (!s || (n && (!in || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, w + ": null argument");
    if (tex >= s->textures.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, w + ": unknown texture");
    if (variant < 0 || variant >= n_variants) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, w + ": unknown variant");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, w + ": too many probes");
    if (variant >= 2 && !tex_prog_is_simple(s->textures[tex].prog))
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, w + ": variants 2 and above are the code of programs made of constants, uv-mapped image maps, scale and mix; this texture holds another operation");
    if (n == 0) return PBRT_HIP_OK;
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;   // textures do not need the accelerator: an empty one is fine
    ProbeStage st(s);
    const float* d_in = st.in(in, n * in_stride);
    float* d_out = st.out(out, n * out_stride);
    if (!st.ok()) return st.finish();
    launch(probe_grid(n), dim3(PH_PROBE_BLOCK), d_in, d_out);
    return st.finish();
}
// what the two light probes do once each has made its own checks: `launch` starts the kernel on the staged ref (10 floats a probe), u (2), wi (3) and out (PBRT_HIP_LIGHT_PROBE_STRIDE)
template <class Launch>
int light_probe_common(PbrtHipScene* s, uint64_t n, const float* ref, const float* u, const float* wi, float* out, Launch launch) {
    if (n == 0) return PBRT_HIP_OK;
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;
    ProbeStage st(s);
    const float* d_ref = st.in(ref, n * 10), *d_u = st.in(u, n * 2), *d_wi = st.in(wi, n * 3);
    float* d_out = st.out(out, n * PBRT_HIP_LIGHT_PROBE_STRIDE);
    if (!st.ok()) return st.finish();
    launch(probe_grid(n), dim3(PH_PROBE_BLOCK), d_ref, d_u, d_wi, d_out);
    return st.finish();
}
}  // namespace
static_assert(PH_PROBE_BLOCK <= PH_TEX_LDS_THREADS, "the texture probes evaluate textures: their blocks must fit the evaluator's LDS stack");

extern "C" {

int pbrt_hip_bsdf_probe_batch(PbrtHipScene* s, uint32_t material, int op, int path, uint64_t n, const float* wo, const float* wi, const float* u, const uint32_t* flags, const float* frame,
                              float* out) {
    return ph_guard(s, "pbrt_hip_bsdf_probe_batch", [&]() -> int {
    if (!s || (n && (!wo || !wi || !u || !flags || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: null argument");
    if (material >= s->mats.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: unknown material");
    if (op < 0 || op > 2 || path < 0 || path > 1) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: op must be 0, 1 or 2 and path 0 or 1");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: too many probes");
    const MaterialRec& m = s->mats.items[material].rec;
    if (material_reads_a_texture(m)) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "bsdf_probe_batch: the material takes a parameter from a texture (its BSDF differs from hit to hit)");
    if (path == 1) {
        if (s->mats.items[material].spec.kind != phost::MaterialKind::Matte) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "bsdf_probe_batch: path 1 is the one-lobe BSDF of MatteMaterial; this material is not matte");
        for (uint64_t i = 0; i < n; i++)
            if ((flags[i] & 5u) != 5u) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: path 1 has no flags; every flags[i] must hold REFLECTION | DIFFUSE");
    }
    if (n == 0) return PBRT_HIP_OK;
    ph::ProbeFrame fr = {{0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, 1.0f}, {1.0f, 0.0f, 0.0f}};
    if (frame) { std::memcpy(fr.ns, frame, 12); std::memcpy(fr.ng, frame + 3, 12); std::memcpy(fr.ss, frame + 6, 12); }
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;   // materials and lobes; an empty accelerator is fine
    ProbeStage st(s);
    const float* d_wo = st.in(wo, n * 3), *d_wi = st.in(wi, n * 3), *d_u = st.in(u, n * 2);
    const uint32_t* d_flags = st.in(flags, n);
    float* d_out = st.out(out, n * 8);
    if (!st.ok()) return st.finish();
    with_variant<2>(path, [&](auto v) {   // path 0 is GEN = true
        hipLaunchKernelGGL(ph::bsdf_probe_kernel<v() == 0>, probe_grid(n), dim3(PH_PROBE_BLOCK), 0, s->stream, s->ds, material, op, (uint32_t)n, d_wo, d_wi, d_u, d_flags, fr, d_out);
    });
    return st.finish();
    });
}

int pbrt_hip_sampler_value_batch(PbrtHipScene* s, uint64_t n, const int* xy, const uint32_t* sample, const uint32_t* dim, int use_lds, float* out) {
    return ph_guard(s, "pbrt_hip_sampler_value_batch", [&]() -> int {
    if (!s || (n && (!xy || !sample || !dim || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: null argument");
    if (!s->have_sampler) return set_err(s, PBRT_HIP_ERR_STATE, "sampler_value_batch: set_sampler first");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: too many values");
    const SamplerRec& sp = s->sampler;
    if (sp.kind == 0) {
        for (uint64_t i = 0; i < n; i++)
            if (dim[i] >= 1000u) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: the Halton tables hold 1000 dimensions (PRIME_TABLE_SIZE)");
    } else {
        if (s->sobol32.empty()) return set_err(s, PBRT_HIP_ERR_STATE, "sampler_value_batch: sobol tables not set");
        const int m = sp.log2_resolution;
        const uint64_t n_dims = s->sobol32.size() / 52;
        if (m > (int)(s->vdc.size() / 52) || m > 26) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "sampler_value_batch: sample-bounds resolution exceeds the Sobol tables given");
        for (uint64_t i = 0; i < n; i++) {
            if (dim[i] >= n_dims) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "sampler_value_batch: dimension beyond the Sobol tables given");
            // the index of (pixel, sample) must stay below 2^52, the columns a generator matrix has: sample < 2^(52 - 2m), pixel inside the power-of-two square
            if (2 * m > 20 && ((uint64_t)sample[i] >> (52 - 2 * m)) != 0) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "sampler_value_batch: sample number beyond the 52 columns of the Sobol matrices");
            const int64_t dx = (int64_t)xy[2 * i] - sp.bounds[0], dy = (int64_t)xy[2 * i + 1] - sp.bounds[1];
            if (dx < 0 || dy < 0 || dx >= sp.resolution || dy >= sp.resolution) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: pixel outside the Sobol sampler's square");
        }
    }
    if (n == 0) return PBRT_HIP_OK;
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;   // the sampler tables; an empty accelerator is fine
    ProbeStage st(s);
    const int* d_xy = st.in(xy, n * 2);
    const uint32_t* d_sample = st.in(sample, n), *d_dim = st.in(dim, n);
    float* d_out = st.out(out, n);
    if (!st.ok()) return st.finish();
    hipLaunchKernelGGL(ph::sampler_value_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s->stream, s->ds, s->sampler, (uint32_t)n, d_xy, d_sample, d_dim, use_lds ? 1 : 0, d_out);
    return st.finish();
    });
}

int pbrt_hip_light_probe_batch(PbrtHipScene* s, uint32_t light, int op, int variant, uint64_t n, const float* ref, const float* u, const float* wi, float* out) {
    return ph_guard(s, "pbrt_hip_light_probe_batch", [&]() -> int {
    if (!s || (n && (!ref || !u || !wi || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "light_probe_batch: null argument");
    if (light >= s->lights.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "light_probe_batch: unknown light");
    if (op < 0 || op > 2 || variant < 0 || variant > 2) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "light_probe_batch: op must be 0, 1 or 2 and variant 0, 1 or 2");
    if (variant == 2 && op != 0) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "light_probe_batch: variant 2 is the Whitted light loop's sample_li; it has op 0 only");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "light_probe_batch: too many probes");
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, "light_probe_batch: build_accel first (the world radius and the degenerate-triangle flags come from it)");
    const LightRec& l = s->lights[light];
    if (l.type == PH_L_AREA) {
        if (l.prim >= s->tri_mesh.size()) return set_err(s, PBRT_HIP_ERR_STATE, "light_probe_batch: the area light has no shape yet");
        if ((s->meshes[s->tri_mesh[l.prim]].flags & PH_MESH_QUADRIC) && variant != 2)
            return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "light_probe_batch: a light whose shape is a quadric (a spherical, disk or cylinder area light) is sampled by variant 2, the Whitted light loop's sample_li, alone");
    }
    if (variant == 1 && l.map_mip1) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "light_probe_batch: variant 1 is the code of scenes without textures; this light holds a radiance, projection or goniometric map");
    return light_probe_common(s, n, ref, u, wi, out, [&](dim3 grid, dim3 block, const float* d_ref, const float* d_u, const float* d_wi, float* d_out) {
        with_variant<3>(variant, [&](auto v) { hipLaunchKernelGGL(ph::light_probe_kernel<v()>, grid, block, 0, s->stream, s->ds, light, op, (uint32_t)n, d_ref, d_u, d_wi, d_out); });
    });
    });
}

int pbrt_hip_sphere_light_probe_batch(PbrtHipScene* s, uint32_t light, int op, uint64_t n, const float* ref, const float* u, const float* wi, float* out) {
    return ph_guard(s, "pbrt_hip_sphere_light_probe_batch", [&]() -> int {
    if (!s || (n && (!ref || !u || !wi || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sphere_light_probe_batch: null argument");
    if (light >= s->lights.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sphere_light_probe_batch: unknown light");
    if (op < 0 || op > 1) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sphere_light_probe_batch: op must be 0 (sample_li) or 1 (pdf_li)");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sphere_light_probe_batch: too many probes");
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, "sphere_light_probe_batch: build_accel first");
    const LightRec& l = s->lights[light];
    if (l.type != PH_L_AREA || l.prim >= s->tri_mesh.size() || !(s->meshes[s->tri_mesh[l.prim]].flags & PH_MESH_QUADRIC))
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "sphere_light_probe_batch: the light's shape is not a quadric (a spherical, disk or cylinder area light: pbrt_hip_add_sphere_light, pbrt_hip_add_quadric_light); pbrt_hip_light_probe_batch probes the others");
    return light_probe_common(s, n, ref, u, wi, out, [&](dim3 grid, dim3 block, const float* d_ref, const float* d_u, const float* d_wi, float* d_out) {
        hipLaunchKernelGGL(ph::sphere_light_probe_kernel, grid, block, 0, s->stream, s->ds, light, op, (uint32_t)n, d_ref, d_u, d_wi, d_out);
    });
    });
}

namespace {
// what the three spatial probe calls refuse alike; a scene the path integrator refuses (refuse_sphere_lights) has no distribution pass either
int spatial_probe_refusals(PbrtHipScene* s, const char* who, size_t min_lights) {
    const std::string w(who);
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, w + ": build_accel first (the world bound comes from the tree)");
    if (s->lights.size() < min_lights)
        return set_err(s, PBRT_HIP_ERR_STATE, w + (min_lights > 1 ? ": fewer than two lights (a render builds no voxel tables for such a scene: light_distrib/mod.rs:59-64)" : ": the scene holds no light"));
    if (s->sphere_lights != 0 && !s->path_sphere_lights)
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, w + ": the scene holds a sphere light (pbrt_hip_add_sphere_light), which the path integrator samples only after pbrt_hip_set_path_sphere_lights");
    return PBRT_HIP_OK;
}
}  // namespace

int pbrt_hip_spatial_probe_begin(PbrtHipScene* s, int out_nv[3], uint32_t* out_capacity) {
    return ph_guard(s, "pbrt_hip_spatial_probe_begin", [&]() -> int {
    if (!s || !out_nv || !out_capacity) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "spatial_probe_begin: null argument");
    int rc;
    if ((rc = spatial_probe_refusals(s, "spatial_probe_begin", 2))) return rc;
    PH_CHECK(s, hipSetDevice(s->device));
    if ((rc = upload_scene(s))) return rc;
    ph::SpatialRec sr;
    if ((rc = spatial_probe_begin(s, &sr))) return rc;
    PH_CHECK(s, hipStreamSynchronize(s->stream));
    for (int i = 0; i < 3; i++) out_nv[i] = sr.nv[i];
    *out_capacity = sr.capacity;
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_spatial_probe_batch(PbrtHipScene* s, uint64_t n, const float* p, const float* u, int strategy, int32_t* out_pi, uint32_t* out_light, float* out_pick_pdf, uint32_t out_counters[4]) {
    return ph_guard(s, "pbrt_hip_spatial_probe_batch", [&]() -> int {
    if (!s || (n && (!p || !u || !out_light || !out_pick_pdf || (strategy == 2 && !out_pi)))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "spatial_probe_batch: null argument");
    if (strategy < 0 || strategy > 2) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "spatial_probe_batch: strategy must be 0 (uniform), 1 (power) or 2 (spatial)");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "spatial_probe_batch: too many points");
    int rc;
    if ((rc = spatial_probe_refusals(s, "spatial_probe_batch", 1))) return rc;
    PH_CHECK(s, hipSetDevice(s->device));
    if ((rc = upload_scene(s))) return rc;
    if ((rc = upload_light_distribution(s, strategy == 2 ? 0 : strategy))) return rc;   // as render_tiles does
    ph::SpatialRec sr{};
    if (strategy == 2 && (rc = spatial_probe_tables(s, &sr))) return rc;
    if (strategy == 2 && sr.stride != 2 * s->lights.size() + 2)   // (a slot holds func[n], cdf[n + 1], func_int of the lights there were at _begin)
        return set_err(s, PBRT_HIP_ERR_STATE, "spatial_probe_batch: the scene's lights changed since pbrt_hip_spatial_probe_begin; call it again");
    uint32_t ctr[4] = {0, 0, 0, 0};
    if (n) {
        ProbeStage st(s);
        const float* d_p = st.in(p, n * 3), *d_u = st.in(u, n);
        int32_t* d_pi = st.out(strategy == 2 ? out_pi : nullptr, n * 3);   // (strategies 0 and 1 write no voxel: nothing comes down)
        uint32_t* d_light = st.out(out_light, n);
        float* d_pdf = st.out(out_pick_pdf, n);
        if (!st.ok()) return st.finish();
        const dim3 grid((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), block(256);
        if (strategy == 2) {
            hipLaunchKernelGGL(ph::spatial_probe_mark_kernel, grid, block, 0, s->stream, sr, (uint32_t)n, d_p, d_pi);
            PH_CHECK(s, hipGetLastError());
            spatial_probe_compute(s, sr);
            PH_CHECK(s, hipGetLastError());
        }
        hipLaunchKernelGGL(ph::spatial_probe_pick_kernel, grid, block, 0, s->stream, s->ds, sr, (uint32_t)n, d_p, d_u, d_light, d_pdf);
        if ((rc = st.finish())) return rc;
    }
    if (strategy == 2) PH_CHECK(s, hipMemcpy(ctr, sr.counters, sizeof ctr, hipMemcpyDeviceToHost));
    if (out_counters) std::memcpy(out_counters, ctr, sizeof ctr);
    if (ctr[ph::SP_OVERFLOW])
        return set_err(s, PBRT_HIP_ERR_OOM, "spatial_probe_batch: SpatialLightDistribution pool exhausted (" + std::to_string(ctr[ph::SP_CLAIMED]) + " voxels x " + std::to_string(s->lights.size()) + " lights)");
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_spatial_probe_voxel(PbrtHipScene* s, const int pi[3], float* func, float* cdf, float* func_int) {
    return ph_guard(s, "pbrt_hip_spatial_probe_voxel", [&]() -> int {
    if (!s || !pi || !func || !cdf || !func_int) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "spatial_probe_voxel: null argument");
    ph::SpatialRec sr{};
    int rc;
    if ((rc = spatial_probe_tables(s, &sr))) return rc;
    if (sr.stride != 2 * s->lights.size() + 2)
        return set_err(s, PBRT_HIP_ERR_STATE, "spatial_probe_voxel: the scene's lights changed since pbrt_hip_spatial_probe_begin; call it again");
    for (int i = 0; i < 3; i++)
        if (pi[i] < 0 || pi[i] >= sr.nv[i]) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "spatial_probe_voxel: voxel outside the grid");
    PH_CHECK(s, hipSetDevice(s->device));
    PH_CHECK(s, hipStreamSynchronize(s->stream));
    const size_t v = ((size_t)pi[0] * (size_t)sr.nv[1] + (size_t)pi[1]) * (size_t)sr.nv[2] + (size_t)pi[2];
    int32_t slot = -1;
    PH_CHECK(s, hipMemcpy(&slot, sr.vox_slot + v, 4, hipMemcpyDeviceToHost));
    if (slot < 0 || (uint32_t)slot >= sr.capacity) return set_err(s, PBRT_HIP_ERR_STATE, "spatial_probe_voxel: no distribution was computed for this voxel");
    const size_t n = s->lights.size();
    const float* base = sr.pool + (size_t)slot * sr.stride;
    PH_CHECK(s, hipMemcpy(func, base, n * 4, hipMemcpyDeviceToHost));
    PH_CHECK(s, hipMemcpy(cdf, base + n, (n + 1) * 4, hipMemcpyDeviceToHost));
    PH_CHECK(s, hipMemcpy(func_int, base + 2 * n + 1, 4, hipMemcpyDeviceToHost));
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_curve_probe_batch(PbrtHipScene* s, uint32_t prim, int shadow, uint64_t n, const PbrtHipRay* rays, float* out) {
    return ph_guard(s, "pbrt_hip_curve_probe_batch", [&]() -> int {
    if (!s || (n && (!rays || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "curve_probe_batch: null argument");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "curve_probe_batch: too many rays");
    if (prim >= s->prim_quadric.size() || s->prim_quadric[prim] == 0u || s->quadrics[s->prim_quadric[prim] - 1u].kind != PH_Q_CURVE)
        return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "curve_probe_batch: the primitive is not a curve segment (pbrt_hip_add_curve)");
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, "curve_probe_batch: build_accel first");
    if (n == 0) return PBRT_HIP_OK;
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;
    ProbeStage st(s);
    const ph::RayIn* d_rays = st.in(device_rays(rays), n);
    float* d_out = st.out(out, n * PBRT_HIP_CURVE_PROBE_STRIDE);
    if (!st.ok()) return st.finish();
    hipLaunchKernelGGL(ph::curve_probe_kernel, probe_grid(n), dim3(PH_PROBE_BLOCK), 0, s->stream, s->ds, s->prim_quadric[prim] - 1u, shadow ? 1u : 0u, (uint32_t)n, d_rays, d_out);
    return st.finish();
    });
}

int pbrt_hip_surface_probe_batch(PbrtHipScene* s, int op, int variant, uint32_t texture, int camera_ray, uint64_t n, const PbrtHipRay* rays, const PbrtHipHit* hits, const float* aux,
                                 float* out) {
    return ph_guard(s, "pbrt_hip_surface_probe_batch", [&]() -> int {
    if (!s || (n && (!rays || !hits || !aux || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: null argument");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: too many probes");
    if (op < 0 || op > 4 || variant < 0 || variant > 2) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: op must be 0 .. 4 and variant 0, 1 or 2");
    if (op == 2 && texture >= s->textures.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: unknown texture");
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, "surface_probe_batch: build_accel first (the leaf records and a hit's pad[0] come from it)");
    const bool cam_ray = camera_ray != 0 && (op == 1 || op == 2);
    if (cam_ray && !(s->have_camera && s->have_film && s->have_sampler && s->sampler.spp > 0))
        return set_err(s, PBRT_HIP_ERR_STATE, "surface_probe_batch: a camera ray's differentials need set_camera, set_film and set_sampler (its samples per pixel scale them)");
    if (variant == 2 && s->quadrics.empty())
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "surface_probe_batch: variant 2 is the code of scenes that hold a quadric shape; this scene's kernels have no such instantiation");
    if (n == 0) return PBRT_HIP_OK;
    PH_CHECK(s, hipSetDevice(s->device));
    // the leaf records, to check every hit against: the host's copy, or the device's where the tree was left there
    std::vector<TriRec> recs;
    if (int frc = s->fetch_leaf_records(recs)) return frc;
    const size_t n_recs = recs.size();
    for (uint64_t i = 0; i < n; i++) {
        const PbrtHipHit& h = hits[i];
        if (h.prim == 0xFFFFFFFFu || h.prim >= s->tri_mesh.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: a hit names no primitive");
        if (h.pad[0] >= n_recs) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: a hit's pad[0] is no leaf record");
        const TriRec& r = recs[h.pad[0]];
        if ((r.flags & PH_TRI_INSTANCE) || r.prim != h.prim) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: a hit's pad[0] is not the leaf record of its primitive");
        if (h.pad[1] > s->instances.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: a hit's pad[1] names no instance");
        if (h.pad[1]) {
            const SceneHostState::ObjectHost& ob = s->objects[s->instances[h.pad[1] - 1u].object];
            if (h.prim < ob.tri0 || h.prim >= ob.tri1) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: a hit's pad[1] names an instance of another object");
            if (variant == 0) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "surface_probe_batch: variant 0 is the interaction made from a primitive number alone; no such path exists for a hit inside an instance");
        }
        const uint32_t q1 = h.prim < s->prim_quadric.size() ? s->prim_quadric[h.prim] : 0u;
        if (((r.flags & PH_TRI_QUADRIC) != 0u) != (q1 != 0u)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "surface_probe_batch: a hit's pad[0] is not the leaf record of its primitive");
        if (q1 && variant != 2) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "surface_probe_batch: a quadric shape's or curve segment's interaction is made by variant 2 alone");
        if (q1 && op == 2 && s->quadrics[q1 - 1u].kind == PH_Q_CURVE) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "surface_probe_batch: op 2 does not take a curve segment");
    }
    int rc;
    if ((rc = upload_scene(s))) return rc;
    ProbeStage st(s);
    const ph::RayIn* d_rays = st.in(device_rays(rays), n);
    const PbrtHipHit* d_hits = st.in(hits, n);
    const float* d_aux = st.in(aux, n * PBRT_HIP_SURFACE_PROBE_AUX);
    float* d_out = st.out(out, n * PBRT_HIP_SURFACE_PROBE_STRIDE);
    if (!st.ok()) return st.finish();
    with_variant<3>(variant, [&](auto v) {
        hipLaunchKernelGGL(ph::surface_probe_kernel<v()>, probe_grid(n), dim3(PH_PROBE_BLOCK), 0, s->stream, s->ds, s->cam, cam_ray ? s->sampler.spp : 1u, op, texture, cam_ray ? 1u : 0u, (uint32_t)n,
                           d_rays, d_hits, d_aux, d_out);
    });
    return st.finish();
    });
}

int pbrt_hip_texture_probe_batch(PbrtHipScene* s, uint32_t texture, int variant, uint64_t n, const float* contexts, float* out) {
    return ph_guard(s, "pbrt_hip_texture_probe_batch", [&]() -> int {
    return texture_probe_common(s, "texture_probe_batch", texture, variant, 5, n, contexts, 15, out, 3, [&](dim3 grid, dim3 block, const float* d_in, float* d_out) {
        with_variant<5>(variant, [&](auto v) { hipLaunchKernelGGL(ph::texture_probe_kernel<v()>, grid, block, 0, s->stream, s->ds, texture, (uint32_t)n, d_in, d_out); });
    });
    });
}

int pbrt_hip_bump_probe_batch(PbrtHipScene* s, uint32_t texture, int variant, uint64_t n, const float* in, float* out) {
    return ph_guard(s, "pbrt_hip_bump_probe_batch", [&]() -> int {
    return texture_probe_common(s, "bump_probe_batch", texture, variant, 4, n, in, 33, out, 6, [&](dim3 grid, dim3 block, const float* d_in, float* d_out) {
        with_variant<4>(variant, [&](auto v) { hipLaunchKernelGGL(ph::bump_probe_kernel<v()>, grid, block, 0, s->stream, s->ds, texture, (uint32_t)n, d_in, d_out); });
    });
    });
}

int pbrt_hip_raysort_probe(PbrtHipScene* s, uint32_t n_cl, uint32_t n_sh, const uint32_t* keys_cl, const uint32_t* keys_sh, uint32_t sort_blocks, uint32_t* order_out) {
    return ph_guard(s, "pbrt_hip_raysort_probe", [&]() -> int {
    if (!s || (n_cl && !keys_cl) || (n_sh && !keys_sh) || ((n_cl || n_sh) && !order_out)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "raysort_probe: null argument");
    if (sort_blocks == 0 || sort_blocks > 65536u) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "raysort_probe: sort_blocks must be 1 .. 65536");
    const uint64_t n = (uint64_t)n_cl + n_sh;
    if (n >= 0x7FFF0000ull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "raysort_probe: more rays than a round's queues hold");
    // (a closest-hit key may carry the escape-query mark, PH_SORT_BINS, on top of its bin: mis_escape.h)
    for (uint32_t i = 0; i < n_cl; i++) if (keys_cl[i] >= PH_SORT_KEYS) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "raysort_probe: a closest-hit key is not below 4096, marked or not");
    for (uint32_t i = 0; i < n_sh; i++) if (keys_sh[i] >= PH_SORT_BINS) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "raysort_probe: a key is not below 4096");
    PH_CHECK(s, hipSetDevice(s->device));
    const uint32_t counts[2] = {n_cl, n_sh};
    ProbeStage st(s);
    const uint32_t* d_cl = st.in(keys_cl, n_cl), *d_sh = st.in(keys_sh, n_sh), *d_n = st.in(counts, 2);
    uint32_t* d_order = st.out(order_out, n);
    uint32_t* d_ws = st.work<uint32_t>(raysort_workspace_bytes(sort_blocks) / sizeof(uint32_t));
    if (!st.ok()) return st.finish();
    launch_raysort(s, d_cl, d_sh, d_n, d_n + 1, d_order, d_ws, sort_blocks);
    return st.finish();   // (`counts` and the caller's arrays are pageable: the copies have left them once the stream has been waited for)
    });
}

// The traversal kernel on an explicit queue: TravParams filled as run_round (wavefront.hip) fills them — counts in device memory, queue heads, head chunk, order — and the grid the caller
// names.  No traversal logic here: the kernel row is the scene's (launch_traverse_kernel, pick_shape).
#define PH_TRAVERSE_PROBE_HEADS 8u   // the heads buffer of a probe: what a path round uses (PathPlan::n_heads)
int pbrt_hip_traverse_probe(PbrtHipScene* s, int mode, const PbrtHipRay* rays_cl, uint32_t n_cl, const PbrtHipRay* rays_sh, uint32_t n_sh, const uint32_t* order, uint32_t n_heads,
                            uint32_t head_chunk, uint32_t blocks, PbrtHipHit* hits_out, uint8_t* occluded_out) {
    return ph_guard(s, "pbrt_hip_traverse_probe", [&]() -> int {
    if (!s) return PBRT_HIP_ERR_INVALID_ARG;
    if ((n_cl && (!rays_cl || !hits_out)) || (n_sh && (!rays_sh || !occluded_out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: null array with a non-zero count");
    if (mode < 0 || mode > 2) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: mode must be 0 (closest hit), 1 (any hit) or 2 (mixed)");
    if ((mode == 0 && n_sh) || (mode == 1 && n_cl)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: mode 0 takes closest-hit rays only (n_sh = 0), mode 1 any-hit rays only (n_cl = 0)");
    const uint64_t n = (uint64_t)n_cl + n_sh;
    if (n >= 0x7FFF0000ull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: more rays than a round's queues hold");
    if (n_heads == 0 || n_heads > PH_TRAVERSE_PROBE_HEADS) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: n_heads must be 1 .. 8");
    if (n_heads > 1 && (head_chunk == 0 || head_chunk % PH_BATCH != 0)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: with several heads head_chunk must be a non-zero multiple of 64");
    if (blocks == 0) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: blocks must be at least 1");
    if (order) {   // a permutation of 0 .. n: any other list would leave a ray untraced or trace one twice
        // An entry may carry the escape-query mark (PH_ORDER_ESCAPE, mis_escape.h) as the ray binning writes it for a marked key: only on a closest-hit position, only in mode 2
        // and only where the scene's kernel row reads it — any other kernel would take the marked entry for a queue position.  It passes through to the kernel as it is.
        const bool marks_ok = mode == 2 && ph::mis_escape_row(!s->alpha_textures ? 0 : s->alpha_lean ? 1 : 2, !s->quadrics.empty(), s->count_traversal);
        std::vector<bool> seen(n, false);
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t pos = order[i] & ~PH_ORDER_ESCAPE;
            if (pos >= n || seen[pos]) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: order is not a permutation of the queue positions");
            if ((order[i] & PH_ORDER_ESCAPE) && (!marks_ok || pos >= n_cl))
                return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: an escape-query mark on an any-hit position, outside mode 2, or in a scene whose kernel row serves none");
            seen[pos] = true;
        }
    }
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, "traverse_probe: call pbrt_hip_build_accel first");
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;
    if ((rc = ensure_traversal_workspace(s))) return rc;
    if (blocks > s->trav_blocks) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "traverse_probe: blocks exceeds the resident grid (the spill region is sized for it)");
    const uint32_t counts[2] = {n_cl, n_sh};
    ProbeStage st(s);
    const ph::RayIn* d_cl = st.in(device_rays(rays_cl), n_cl), *d_sh = st.in(device_rays(rays_sh), n_sh);
    const uint32_t* d_n = st.in(counts, 2), *d_order = st.in(order, n);
    uint32_t* d_heads = st.work<uint32_t>(PH_TRAVERSE_PROBE_HEADS * 16, 0);   // (a head is a 64-byte line)
    // results start as 0xFF bytes: a ray the queue never served is told from every answer the kernel writes
    PbrtHipHit* d_hits = st.out(hits_out, n_cl, 0xFF);
    uint8_t* d_occ = st.out(occluded_out, n_sh, 0xFF);
    if (!st.ok()) return st.finish();
    PH_CHECK(s, hipMemsetAsync(s->d_counter.p, 0, 4, s->stream));
    ph::TravParams tp{};
    tp.n = 0; tp.counter = (uint32_t*)s->d_counter.p;
    if (mode == 1) { tp.rays = d_sh; tp.out = d_occ; tp.n_ptr = d_n + 1; }
    else { tp.rays = d_cl; tp.out = d_hits; tp.n_ptr = d_n; }
    if (mode == 2) { tp.rays2 = d_sh; tp.out2 = d_occ; tp.n2_ptr = d_n + 1; }
    tp.heads = d_heads; tp.n_heads = n_heads; tp.head_chunk = head_chunk;
    tp.order = order ? d_order : nullptr;
    launch_traverse_kernel(s, mode, blocks, tp);
    if ((rc = st.finish())) return rc;   // (`counts` and the caller's arrays are pageable: the copies have left them once the stream has been waited for)
    return traversal_overflow_check(s);
    });
}

// The film side of a render on explicit samples: the rank's tile and pixel lists, the bands, the record buffers and the film pass are the render's own (samples_begin ..
// samples_to_tiles, merge_own_tiles); film_probe_fill_kernel stands where an integrator would fill the records.
namespace {
int film_probe_args(PbrtHipScene* s, const char* who, int tile_size, int tile_part, int tile_parts) {
    const std::string w(who);
    if (tile_size <= 0 || tile_parts <= 0 || tile_parts > PH_MAX_TILE_PARTS || tile_part < 0 || tile_part >= tile_parts) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, w + ": bad tile partition");
    if (!s->have_film) return set_err(s, PBRT_HIP_ERR_STATE, w + ": set_film first");
    return PBRT_HIP_OK;
}
}  // namespace

int pbrt_hip_film_probe_layout(PbrtHipScene* s, int tile_size, int tile_part, int tile_parts, uint64_t out[4], int32_t* out_px_xy, int32_t* out_tile_pb) {
    return ph_guard(s, "pbrt_hip_film_probe_layout", [&]() -> int {
    if (!s || !out) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "film_probe_layout: null argument");
    int rc;
    if ((rc = film_probe_args(s, "film_probe_layout", tile_size, tile_part, tile_parts))) return rc;
    PH_CHECK(s, hipSetDevice(s->device));
    SampleRecords rec;
    if ((rc = samples_begin(s, tile_size, tile_part, tile_parts, &rec))) return rc;
    const int2* px; size_t n_px; std::vector<int32_t> pb; uint32_t sw, sh;
    film_layout(s, &px, &n_px, &pb, &sw, &sh);
    out[0] = n_px; out[1] = pb.size() / 4; out[2] = sw; out[3] = sh;
    if (out_px_xy) for (size_t i = 0; i < n_px; i++) { out_px_xy[2 * i] = px[i].x; out_px_xy[2 * i + 1] = px[i].y; }
    if (out_tile_pb && !pb.empty()) std::memcpy(out_tile_pb, pb.data(), pb.size() * 4);
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_film_probe(PbrtHipScene* s, int tile_size, int tile_part, int tile_parts, uint64_t n_px, const float* L, const float* p_film, void* d_tile_buffer, float* out_xyz,
                        float* out_weight, float* out_tiles) {
    return ph_guard(s, "pbrt_hip_film_probe", [&]() -> int {
    if (!s || (n_px && (!L || !p_film)) || (!out_xyz != !out_weight)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "film_probe: null argument");
    if (d_tile_buffer && out_xyz) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "film_probe: the film comes from the handle's own tile buffer; merge a caller's buffers with pbrt_hip_merge_tiles_device");
    int rc;
    if ((rc = film_probe_args(s, "film_probe", tile_size, tile_part, tile_parts))) return rc;
    if (!s->have_sampler || s->sampler.spp == 0) return set_err(s, PBRT_HIP_ERR_STATE, "film_probe: set_sampler first (its samples per pixel size the records)");
    PH_CHECK(s, hipSetDevice(s->device));
    SampleRecords rec;
    if ((rc = samples_begin(s, tile_size, tile_part, tile_parts, &rec))) return rc;
    if (n_px != rec.n_px) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "film_probe: n_px is not the length of this part's pixel list (pbrt_hip_film_probe_layout)");
    const uint32_t spp = s->sampler.spp;
    {   // what the film pass rests on: a sample of pixel (x, y) lies in [x, x + 1] x [y, y + 1], the upper ends being positions rounded up; the integrators zero a non-finite radiance
        const int2* px; size_t n; std::vector<int32_t> pb; uint32_t sw, sh;
        film_layout(s, &px, &n, &pb, &sw, &sh);
        for (uint32_t k = 0; k < spp; k++)
            for (size_t i = 0; i < n; i++) {
                const size_t o = (size_t)k * n + i;
                const float x = p_film[2 * o], y = p_film[2 * o + 1];
                if (x != x) continue;   // no sample taken
                if (!(x >= (float)px[i].x && x <= (float)(px[i].x + 1) && y >= (float)px[i].y && y <= (float)(px[i].y + 1)))
                    return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "film_probe: a film position lies outside its pixel");
                if (!std::isfinite(L[3 * o]) || !std::isfinite(L[3 * o + 1]) || !std::isfinite(L[3 * o + 2])) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "film_probe: a radiance is not finite");
            }
    }
    const size_t tile_floats = tile_buffer_floats_for(s, tile_size, tile_part, tile_parts);
    void* tiles = d_tile_buffer;
    if (!tiles) {
        DevBuf& own = tile_buffer_of(s);
        if ((rc = ensure_buf(s, own, tile_floats * 4))) return rc;
        tiles = own.p;
    }
    ProbeStage st(s);
    if (rec.n_px == 0) PH_CHECK(s, hipMemsetAsync(tiles, 0, tile_floats * 4, s->stream));
    else {
        if ((rc = samples_plan_bands(s, &rec, 0, 0))) return rc;
        if ((rc = samples_alloc(s, &rec))) return rc;
        const size_t n_rec = (size_t)spp * rec.n_px;
        const float* d_L = st.in(L, n_rec * 3), *d_p = st.in(p_film, n_rec * 2);
        if (!st.ok()) return st.finish();
        for (size_t b = 0; b < rec.bands.size(); b++) {
            SampleRecords br;
            if ((rc = samples_band(s, rec, b, &br))) return rc;
            const uint64_t threads = (uint64_t)br.n_px * spp;
            hipLaunchKernelGGL(ph::film_probe_fill_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s->stream, br.n_px, br.band.px0, rec.n_px, spp, br.px_xy,
                               d_L, d_p, br.rec_L, br.rec_py, br.px_rounded);
            PH_CHECK(s, hipGetLastError());
            if ((rc = samples_to_tiles(s, br, tiles))) return rc;
        }
    }
    if (out_tiles) st.fetch(out_tiles, static_cast<const float*>(tiles), tile_floats);
    if ((rc = st.finish())) return rc;   // (the caller's arrays are pageable: the copies have left them by now)
    if (out_xyz) return merge_own_tiles(s, tile_size, tile_part, tile_parts, out_xyz, out_weight);
    return PBRT_HIP_OK;
    });
}

}  // extern "C"
