// WhittedIntegrator::li (integrators/src/whitted.rs:51-118) with SamplerIntegrator::specular_reflect / specular_transmit
// (core/src/integrator/sampler_integrator.rs:79-238) as a state machine over a pool of camera samples: the records a sample keeps between the
// rounds of the wavefront driver (whitted.hip), the per-vertex pass that evaluates textures with the ray's own differentials, and the state kernel.
//
// li is a recursion — L of a vertex waits for `f * li(child) * |wi.ns| / pdf` of its reflected and then its refracted child — and it is evaluated as
// one: every level of a sample owns a WhFrame with its partial L and the factors that wait for the child's return value.  A flattened throughput
// product would round differently.
#pragma once
#include "bsdf_general.h"
#include "texture.h"
#include "shading_diff.h"
#include "wf_device.h"
#include "sphere_light.h"
#include "film_plan.h"

namespace ph {

#define PH_WH_MAX_DEPTH 16      // frames per sample; pbrt_hip_render_whitted refuses a larger max_depth
#define PH_WH_SLICE 4           // occlusion rays a sample may send per round: the light loop of a vertex runs in slices of at most this many lights that pass f / pdf

enum : uint32_t { WH_AWAIT = 0u,   // the frame's ray is in this round's closest-hit queue
                  WH_LIGHTS = 1u,  // the light loop: next light = WhSample::light_next
                  WH_REFL = 2u,    // specular_reflect is due
                  WH_TRANS = 3u }; // specular_transmit is due (the reflected subtree has returned into WhFrame::refl)

// what the vertex pass leaves for the state kernel: the texture pass's record and the hit's differentials (surface_interaction.rs:203-278) plus the shading
// dn/du, dn/dv, which the reflected / refracted ray differentials are made of
struct alignas(16) WhVertex {
    TexOut tex;
    float dpdx[3], dudx, dpdy[3], dvdx, dndu[3], dudy, dndv[3], dvdy;
};
// one level of the recursion
struct alignas(16) WhFrame {
    RayIn ray;                                   // the ray li was called with (after a Material "none" surface: its continuation)
    float rx_o[3], ry_o[3], rx_d[3], ry_d[3];    // its differentials, if has_diff
    HitOut hit;                                  // what it hit
    float L[3]; uint32_t has_diff;
    float f[3], abs_dot;                         // of the child in flight: li(child) returns into f * . * abs_dot / pdf
    float refl[3], pdf;
    WhVertex v;
};
struct alignas(16) WhSample {
    uint32_t depth, phase, dim, slot;            // current frame, its phase, next sampler dimension, the frame's ray in this round's closest-hit queue
    uint32_t light_next, n_pend, sh_base, pad_;  // the light loop's next light; occlusion rays sent last round: rays_sh[sh_base .. sh_base + n_pend)
    float pend[PH_WH_SLICE][4];                  // their f * Li * |wi.ns| / pdf, added to the frame's L in the lights' order where the ray arrives
};
// DirectLightingIntegrator::li on the same driver (PH_WH_DIRECT): what a sample keeps of its vertex's light phase between rounds, in a buffer the Whitted mode never allocates
struct alignas(16) WhDirect {
    float acc[3]; uint32_t flags;   // uniform_sample_all_lights' local `l` / uniform_sample_one_light's estimate so far; WD_* of the non-delta light whose estimate_direct is in flight
    float f[3], weight;             // its BSDF half: f * |wi.ns| and power_heuristic(scattering_pdf, light_pdf)
    float spdf; uint32_t light, pad_[2];   // scattering_pdf, the light's index
};
enum : uint32_t { WD_SH = 1u,     // the last of this round's occlusion rays belongs to the non-delta light (the light half of its estimate_direct)
                  WD_MIS = 2u };  // the sample's closest-hit slot holds its BSDF-sampled ray
enum : int { PH_WH_WHITTED = 0, PH_WH_DIRECT = 1 };   // the state kernel's MODE
struct WhCounters { uint32_t n_cl, n_sh, n_live, head; };
struct WhDevStats { unsigned long long camera_rays; };

struct WhParams {
    CameraRec cam; SamplerRec sp;
    int32_t pixel_bounds[4];
    int32_t max_depth;
    uint32_t n_frames;           // frames per sample: max(max_depth, 1)
    uint32_t n_px, chunk_spp, s0, B;   // n_px: pixels of the band being rendered (band_plan.h); px_xy starts at the band's first pixel, the records are [sample][pixel of the band]
    uint32_t diffs;              // the scene has textures or bump maps: rays carry differentials (nothing else reads them)
    const int2* px_xy;
    float4* rec_L; float* rec_py; uint8_t* px_rounded;
    RayIn* rays_cl[2]; HitOut* hits_cl; RayIn* rays_sh[2]; uint8_t* occ;
    uint32_t* live[2];           // camera samples (chunk-local ids) still running, per round parity
    WhCounters* ctr;             // [2], per round parity
    WhDevStats* stats;
    WhSample* samples; WhFrame* frames;   // frames[pid * n_frames + depth]
};
// what the direct-lighting mode's state kernel takes besides
struct WhDirectArgs {
    WhDirect* direct;            // [sample of the chunk]
    uint32_t strategy;           // 0 uniform_sample_all_lights, 1 uniform_sample_one_light
};

PH_DEV f3 ld3f(const float* p) { return mk3(p[0], p[1], p[2]); }
PH_DEV void st3f(float* p, f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
PH_DEV spec lds3(const float* p) { return mks(p[0], p[1], p[2]); }
PH_DEV void sts3(float* p, spec v) { p[0] = v.r; p[1] = v.g; p[2] = v.b; }

// ---------------------------------------------------------------------------------------------------------------------------
// Camera samples of a chunk (get_camera_sample + generate_ray_differential + scale_differentials, sampler/mod.rs:45-53, sampler_integrator.rs:352-358): frame 0 of every sample.
__global__ __launch_bounds__(256) void whitted_raygen_kernel(DeviceScene sc, WhParams w) {
    const uint32_t pid = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = pid < w.B;
    RayIn ray;
    WhFrame* fr = nullptr;
    if (active) {
        const uint32_t pix = pid / w.chunk_spp, j = pid - pix * w.chunk_spp, s = w.s0 + j;
        const int2 xy = w.px_xy[pix];
        active = xy.x >= w.pixel_bounds[0] && xy.x < w.pixel_bounds[2] && xy.y >= w.pixel_bounds[1] && xy.y < w.pixel_bounds[3];   // sampler_integrator.rs:348-350
        const size_t gsi = (size_t)s * w.n_px + pix;
        if (active) {
            SamplerCursor c = cursor_for(sc, w.sp, xy.x, xy.y, s, 0);
            const f2 fs = get_2d(sc, w.sp, c);
            const f2 p_film = mk2((float)xy.x + fs.x, (float)xy.y + fs.y);
            const float time = get_1d(sc, w.sp, c);
            const f2 lens = get_2d(sc, w.sp, c);
            generate_camera_ray(w.cam, p_film, time, lens, ray);
            w.rec_L[gsi] = make_float4(0.0f, 0.0f, 0.0f, p_film.x);
            w.rec_py[gsi] = p_film.y;
            phfilm::mark_rounded_up(w.px_rounded, pix, xy.x, xy.y, p_film.x, p_film.y);
            fr = w.frames + (size_t)pid * w.n_frames;
            fr->ray = ray; fr->has_diff = w.diffs;
            if (w.diffs) {
                const RayDiff rd = camera_ray_differentials(w.cam, p_film, lens, mk3(ray.ox, ray.oy, ray.oz), mk3(ray.dx, ray.dy, ray.dz), w.sp.spp);
                st3f(fr->rx_o, rd.rx_o); st3f(fr->ry_o, rd.ry_o); st3f(fr->rx_d, rd.rx_d); st3f(fr->ry_d, rd.ry_d);
            }
        } else {
            w.rec_L[gsi] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u));  // NaN p_film.x marks "no sample"
            w.rec_py[gsi] = 0.0f;
        }
    }
    const uint32_t slot = wave_alloc(&w.ctr[0].n_cl, active);
    const uint32_t lslot = wave_alloc(&w.ctr[0].n_live, active);
    if (active) {
        store_ray(w.rays_cl[0] + slot, ray);
        w.live[0][lslot] = pid;
        WhSample* sm = w.samples + pid;
        sm->depth = 0u; sm->phase = WH_AWAIT; sm->dim = 5u; sm->slot = slot; sm->light_next = 0u; sm->n_pend = 0u; sm->sh_base = 0u;
    }
    const uint64_t m = __ballot(active);
    if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(&w.stats->camera_rays, (unsigned long long)__popcll(m));
}

// ---------------------------------------------------------------------------------------------------------------------------
// (dn/du, dn/dv of a triangle's shading geometry: tri_shading_dn, shading_diff.h)

// The vertex pass: one thread per running sample whose frame met a surface this round.  compute_differentials with the frame's ray differentials (camera rays AND the
// reflected / refracted rays below them carry some), Material::bump, the textured lobe colours — texture_kernel's work (wavefront.hip) with the differentials taken from
// the ray instead of the camera.  Launched only for scenes with textures or bump maps.
template <bool QUADRIC>
__global__ __launch_bounds__(PH_TEX_LDS_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void whitted_vertex_kernel(DeviceScene sc, WhParams w, int par) {
    const uint32_t n_live = w.ctr[par].n_live;
    noise_lds_fill();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_live; i += gridDim.x * blockDim.x) {
        const uint32_t pid = w.live[par][i];
        const WhSample* sm = w.samples + pid;
        if (sm->phase != WH_AWAIT) continue;
        WhFrame* fr = w.frames + (size_t)pid * w.n_frames + sm->depth;
        const float4* hp = reinterpret_cast<const float4*>(w.hits_cl + sm->slot);
        const float4 h0 = hp[0];
        if (__float_as_uint(h0.y) == 0xFFFFFFFFu) continue;
        const float4 h1 = hp[1];
        const RayIn ray = fr->ray;
        const f3 ro = mk3(ray.ox, ray.oy, ray.oz), rd = mk3(ray.dx, ray.dy, ray.dz);
        MeshRec m;
        QSurf qs; qs.hit = 0u;
        const SurfHit si = make_surface_hit_q<QUADRIC>(sc, ro, rd, ray.time, __float_as_uint(h1.y), __float_as_uint(h1.z), h0.z, h0.w, h1.x, m, &qs, h0.x);
        const bool on_quadric = QUADRIC && (m.flags & PH_MESH_QUADRIC) != 0u;
        const MaterialRec& mr = sc.materials[m.material];
        if (mr.none) continue;
        // uv and the geometric dp/du, dp/dv (triangles: triangle.rs:548-584, carried to world space for an instance)
        f2 uv; f3 dpdu, dpdv, dndu, dndv;
        const uint32_t tri_index = __float_as_uint(h1.y), inst = __float_as_uint(h1.z);
        if (on_quadric) { uv = mk2(qs.u, qs.v); dpdu = qs.dpdu; dpdv = qs.dpdv; dndu = qs.dndu; dndv = qs.dndv; }
        else {
            const float4* tp = reinterpret_cast<const float4*>(sc.tris + tri_index);
            const float4 a = tp[0], b = tp[1], c = tp[2];
            const uint32_t prim = __float_as_uint(a.w);
            TriVerts t;
            t.p0 = mk3(a.x, a.y, a.z); t.p1 = mk3(b.x, b.y, b.z); t.p2 = mk3(c.x, c.y, c.z);
            t.i0 = t.i1 = t.i2 = 0;
            f2 uv0 = mk2(0.0f, 0.0f), uv1 = mk2(1.0f, 0.0f), uv2 = mk2(1.0f, 1.0f);
            if (m.flags & PH_MESH_UV) {
                t.i0 = sc.idx[3 * prim]; t.i1 = sc.idx[3 * prim + 1]; t.i2 = sc.idx[3 * prim + 2];
                uv0 = mk2(sc.UV[2 * (size_t)t.i0], sc.UV[2 * (size_t)t.i0 + 1]); uv1 = mk2(sc.UV[2 * (size_t)t.i1], sc.UV[2 * (size_t)t.i1 + 1]);
                uv2 = mk2(sc.UV[2 * (size_t)t.i2], sc.UV[2 * (size_t)t.i2 + 1]);
            }
            tri_dpdu(sc, m, t, dpdu, dpdv);
            if (inst != 0u) {
                const InstRec& I = sc.instances[inst - 1u];
                if (!(I.flags & PH_INST_IDENTITY)) { dpdu = xf_vec(I.i2w, dpdu); dpdv = xf_vec(I.i2w, dpdv); }
            }
            uv = mk2((h0.z * uv0.x + h0.w * uv1.x) + h1.x * uv2.x, (h0.z * uv0.y + h0.w * uv1.y) + h1.x * uv2.y);
            tri_shading_dn(sc, tri_index, inst, dndu, dndv);
        }
        TexCtx ctx;
        ctx.uv = uv; ctx.dudx = ctx.dvdx = ctx.dudy = ctx.dvdy = 0.0f;
        ctx.p = si.p; ctx.dpdx = mk3(0.0f, 0.0f, 0.0f); ctx.dpdy = ctx.dpdx;
        if (fr->has_diff) {
            RayDiff rdf; rdf.rx_o = ld3f(fr->rx_o); rdf.ry_o = ld3f(fr->ry_o); rdf.rx_d = ld3f(fr->rx_d); rdf.ry_d = ld3f(fr->ry_d);
            compute_differentials(si.p, si.n, dpdu, dpdv, rdf, ctx);
        }
        WhVertex out;
        out.tex.bumped = 0u; out.tex.lambert = 0u;
        st3f(out.tex.ns, si.ns); st3f(out.tex.dpdu_s, si.dpdu_s);
        if (mr.bump_tex1) {
            BumpOut bo;
            if (on_quadric) bump_shading<false, false>(sc.self, mr.bump_tex1 - 1u, ctx, si.p, si.n, si.ns, si.dpdu_s, qs.dpdv, qs.dndu, qs.dndv, &bo);
            else {
                BumpIn bi; bi.tex = mr.bump_tex1 - 1u; bi.tri_index = tri_index; bi.inst = inst; bi.bary = mk3(h0.z, h0.w, h1.x);
                bi.p = si.p; bi.n = si.n; bi.ns = si.ns; bi.dpdu_s = si.dpdu_s; bi.c = ctx;
                hit_bump<false, false>(sc.self, &bi, &bo);
            }
            st3f(out.tex.ns, bo.ns); st3f(out.tex.dpdu_s, bo.dpdu_s);
            out.tex.bumped = 1u;
        }
        for (int k = 0; k < PH_HIT_COLS; k++) out.tex.col[k][0] = out.tex.col[k][1] = out.tex.col[k][2] = out.tex.col[k][3] = 0.0f;
        if (mr.textured) eval_lobe_colours<false, false>(sc.self, mr, sc.lobes + mr.lobe_base, mr.n_lobes, ctx, out.tex);
        st3f(out.dpdx, ctx.dpdx); st3f(out.dpdy, ctx.dpdy); out.dudx = ctx.dudx; out.dvdx = ctx.dvdx; out.dudy = ctx.dudy; out.dvdy = ctx.dvdy;
        st3f(out.dndu, dndu); st3f(out.dndv, dndv);
        float4* dst = reinterpret_cast<float4*>(&fr->v);
        const float4* src = reinterpret_cast<const float4*>(&out);
        for (uint32_t k = 0; k < sizeof(WhVertex) / 16; k++) dst[k] = src[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The BSDF as WhittedIntegrator sees it: compute_scattering_functions with allow_multiple_lobes = false.  The one difference on this path: smooth glass is
// SpecularReflection(Kr, FresnelDielectric(1, eta)) followed by SpecularTransmission(Kt, 1, eta) — each only where its colour is not black — instead of the one
// FresnelSpecular lobe (glass.rs:112-129).  `split` = the template lobe that is seen that way (the first FresnelSpecular of the hit's list), or none.
struct WhBsdf { GBsdf g; uint32_t split; };
PH_DEV WhBsdf wh_make_bsdf(const DeviceScene& sc, const SurfHit& si, uint32_t material, const TexOut* to, bool textured_scene) {
    WhBsdf b;
    b.g = make_gbsdf(sc, si, material);
    const MaterialRec& mr = *b.g.mr;
    if (textured_scene && mr.textured) {
        if (mr.rt_mode && (to->bumped & PH_TEXOUT_NULL_BSDF)) b.g.keep = 0u;   // translucent.rs:72-74: no lobes at this hit
        else b.g.keep = hit_lobe_mask(mr, b.g.lobes, b.g.n, to, b.g.eta);
        b.g.hit = to;
    }
    b.split = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < b.g.n; i++) if (lobe_in(b.g, i) && b.g.lobes[i].kind == PH_LK_FRESNEL_SPEC) { b.split = i; break; }
    return b;
}
// bsdf.f(wo, wi, ALL): specular lobes evaluate to zero whichever way smooth glass is written, so the lobe list as it stands gives the sum
PH_DEV spec wh_bsdf_f(const WhBsdf& b, f3 wo, f3 wi) { return bsdf_f(b.g, wo, wi, BX_ALL); }
// bsdf.sample_f(wo, u, SPECULAR | (REFLECTION or TRANSMISSION)) (bsdf.rs:160-292): the sampled lobe is specular, so f and pdf are its own
PH_DEV void wh_sample_specular(const WhBsdf& b, f3 wo_w, f2 u, bool transmit, spec& f_out, float& pdf_out, f3& wi_out) {
    f_out = mks1(0.0f); pdf_out = 0.0f; wi_out = mk3(0.0f, 0.0f, 0.0f);
    const uint32_t flags = BX_SPEC | (transmit ? BX_TRANS : BX_REFL);
    LobeRec half;   // the half of the split lobe that matches `flags`, if it exists at this hit
    bool half_in = false;
    if (b.split != 0xFFFFFFFFu) {
        const LobeRec g = lobe_at(b.g, b.split);
        const float* col = transmit ? g.t : g.r;
        half_in = !(col[0] == 0.0f && col[1] == 0.0f && col[2] == 0.0f);
        half = g;
        half.kind = transmit ? PH_LK_SPEC_T : PH_LK_SPEC_R; half.type = flags; half.fresnel = PH_FR_DIEL; half.n_scale = 0u;
    }
    uint32_t matching = 0;
    for (uint32_t i = 0; i < b.g.n; i++) if (i == b.split ? half_in : lobe_sel(b.g, i, flags)) matching++;
    if (matching == 0u) return;
    uint32_t comp = f2u_sat(floorf(u.x * (float)matching));
    if (comp > matching - 1u) comp = matching - 1u;
    uint32_t idx = 0, count = comp;
    for (uint32_t i = 0; i < b.g.n; i++) if (i == b.split ? half_in : lobe_sel(b.g, i, flags)) { if (count == 0u) { idx = i; break; } count--; }
    const f2 ur = mk2(pminf(u.x * (float)matching - (float)comp, kOneMinusEps), u.y);
    const f3 wo = w2l(b.g, wo_w);
    if (wo.z == 0.0f) return;
    spec f; float pdf; f3 wi;
    if (idx == b.split) (void)lobe_sample_f(half, wo, ur, f, pdf, wi);
    else (void)lobe_sample_f(lobe_at(b.g, idx), wo, ur, f, pdf, wi);
    if (pdf == 0.0f) return;
    if (matching > 1u) pdf = ph_div(pdf, (float)matching);
    f_out = f; pdf_out = pdf; wi_out = l2w(b.g, wi);
}

// ---------------------------------------------------------------------------------------------------------------------------
// estimate_direct (core/src/integrator/common.rs:146-299, specular = false, handle_media = false) for the direct-lighting mode, in the two pieces a round boundary cuts it into.
// Every expression is the path shade kernel's (wavefront.hip, "estimate_direct" and "K6").
PH_DEV bool wd_is_delta(const LightRec& l) { return l.type == PH_L_DISTANT || l.type == PH_L_POINT || l.type == PH_L_SPOT || l.type == PH_L_PROJECTION || l.type == PH_L_GONIO; }
// The sending half.  Returns through `sh` / `mis` the occlusion ray of the light sample and the BSDF-sampled ray, where estimate_direct traces them.
template <bool QUADRIC>
PH_DEV void wd_estimate_send(const DeviceScene& sc, const LightRec& light, uint32_t light_num, const SurfHit& si, const WhBsdf& bsdf, f2 u_light, f2 u_scatter,
                             bool& want_sh, RayIn& sh, float* pend, bool& want_mis, RayIn& mis, WhDirect* dl) {
    const bool is_delta = wd_is_delta(light);
    want_sh = false; want_mis = false;
    const LiSample ls = wh_light_sample_li<QUADRIC>(sc, light, si, u_light);
    if (ls.valid && ls.pdf > 0.0f && !is_black(ls.value)) {
        const spec f = bsdf_f(bsdf.g, si.wo, ls.wi, BX_ALL & ~BX_SPEC) * abs_dot(ls.wi, si.ns);
        const float scattering_pdf = bsdf_pdf(bsdf.g, si.wo, ls.wi, BX_ALL & ~BX_SPEC);
        if (!is_black(f)) {
            sh = spawn_ray_to_hit(si, ls.vp, ls.vperr, ls.vn);   // VisibilityTester::unoccluded
            want_sh = true;
            spec A;
            if (is_delta) A = f * ls.value / ls.pdf;
            else A = f * ls.value * power_heuristic1(ls.pdf, scattering_pdf) / ls.pdf;
            pend[0] = A.r; pend[1] = A.g; pend[2] = A.b;
        }
    }
    if (!is_delta) {
        spec f1; float spdf; f3 wi2; uint32_t st;
        bsdf_sample_f(bsdf.g, si.wo, u_scatter, BX_ALL & ~BX_SPEC, f1, spdf, wi2, st);   // never specular with these flags: sampled_specular = false
        const spec f = f1 * abs_dot(wi2, si.ns);
        if (!is_black(f) && spdf > 0.0f) {
            float lp;
            if constexpr (QUADRIC) lp = sl_light_pdf_li(sc, light, si, wi2);
            else lp = light_pdf_li<true>(sc, light, si, wi2);
            if (lp != 0.0f) {   // lp == 0: `return ld` with the light half only
                mis = spawn_ray(si, wi2);
                want_mis = true;
                sts3(dl->f, f); dl->weight = power_heuristic1(spdf, lp); dl->spdf = spdf; dl->light = light_num;
            }
        }
    }
}
// The receiving half, a round later: the delta lights' samples of the slice in the lights' order, then the non-delta light's two halves, each light's `ld` added to `acc`.
// The BSDF-sampled ray's hit is read where the traversal left it; WhFrame::hit stays the vertex's own.
template <bool QUADRIC>
PH_DEV void wd_estimate_receive(const DeviceScene& sc, const WhParams& w, int par, const WhSample* sm, WhDirect* dl) {
    spec acc = lds3(dl->acc);
    const uint32_t flags = dl->flags;
    const uint32_t n_delta = sm->n_pend - ((flags & WD_SH) ? 1u : 0u);
    for (uint32_t k = 0; k < n_delta; k++) if (!w.occ[sm->sh_base + k]) acc = acc + mks(sm->pend[k][0], sm->pend[k][1], sm->pend[k][2]);
    if (flags & (WD_SH | WD_MIS)) {
        spec ld = mks1(0.0f);
        if ((flags & WD_SH) && !w.occ[sm->sh_base + n_delta]) ld = ld + mks(sm->pend[n_delta][0], sm->pend[n_delta][1], sm->pend[n_delta][2]);
        if (flags & WD_MIS) {
            const RayIn mr = load_ray(w.rays_cl[par] + sm->slot);
            const float4* hp = reinterpret_cast<const float4*>(w.hits_cl + sm->slot);
            const float4 h0 = hp[0];
            const uint32_t hprim = __float_as_uint(h0.y);
            const f3 wi = mk3(mr.dx, mr.dy, mr.dz);
            const LightRec& lt = sc.lights[dl->light];
            spec li2 = mks1(0.0f);
            if (hprim != 0xFFFFFFFFu) {
                if (lt.type == PH_L_AREA && lt.prim == hprim) {   // the hit primitive's area light IS the sampled light
                    const float4 h1 = hp[1];
                    MeshRec m;
                    QSurf lqs; lqs.hit = 0u;
                    const SurfHit lh = make_surface_hit_q<QUADRIC>(sc, mk3(mr.ox, mr.oy, mr.oz), wi, mr.time, __float_as_uint(h1.y), __float_as_uint(h1.z), h0.z, h0.w, h1.x, m, &lqs, h0.x);
                    li2 = area_L(lt, lh.n, -wi);   // SurfaceInteraction::le (surface_interaction.rs:283-289)
                }
            } else li2 = light_le<true>(sc, lt, wi);
            if (!is_black(li2)) ld = ld + lds3(dl->f) * li2 * mks1(1.0f) * dl->weight / dl->spdf;   // f * li * tr * weight / scattering_pdf
        }
        acc = acc + ld;
    }
    sts3(dl->acc, acc);
    dl->flags = 0u;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Light::sample_li as the light loop calls it: wh_light_sample_li (sphere_light.h).
// The state kernel: one thread per running sample and round.  It adds last round's unoccluded light samples to their frame, then advances the sample's recursion until it
// has a closest-hit ray to send, has sent PH_WH_SLICE occlusion rays, or frame 0 has returned.  A vertex is rebuilt from the frame (ray, hit, vertex record) whenever the
// sample comes back to it: its light loop's next slice, the refracted ray once the reflected subtree has returned.
// MODE PH_WH_DIRECT: DirectLightingIntegrator::li (integrators/src/direct_lighting.rs:110-166) — the same recursion with estimate_direct in the light phase: per round a slice of
// delta lights and at most one non-delta light, whose BSDF-sampled ray takes the sample's closest-hit slot (no frame ray is in flight during a light phase).
// `x` is read by that mode only; the Whitted instantiations keep the code they had without it.
template <bool QUADRIC, int MODE>
__global__ __launch_bounds__(256) void whitted_state_kernel(DeviceScene sc, WhParams w, int par, WhDirectArgs x) {
    const uint32_t n_live = w.ctr[par].n_live;
    WhCounters* next = w.ctr + (par ^ 1);
    for (uint32_t base = blockIdx.x * blockDim.x; base < n_live; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        const bool active = i < n_live;
        bool want_cl = false, done = false;
        uint32_t n_sh = 0, pid = 0;
        RayIn ray_cl;
        RayIn ray_sh[PH_WH_SLICE];
        WhSample* sm = nullptr;
        if (active) {
            pid = w.live[par][i];
            sm = w.samples + pid;
            WhFrame* frames = w.frames + (size_t)pid * w.n_frames;
            uint32_t depth = sm->depth, phase = sm->phase, dim = sm->dim, light_next = sm->light_next;
            const uint32_t ppix = pid / w.chunk_spp;
            const int2 xy = w.px_xy[ppix];
            SamplerCursor cur = cursor_for(sc, w.sp, xy.x, xy.y, w.s0 + (pid - ppix * w.chunk_spp), dim);
            // last round's light samples: `L += f * Li * |wi.ns| / pdf` where the occlusion ray arrived (whitted.rs:88-104), in the lights' order
            if constexpr (MODE == PH_WH_DIRECT) {
                if (sm->n_pend || x.direct[pid].flags) wd_estimate_receive<QUADRIC>(sc, w, par, sm, x.direct + pid);
            } else
            if (sm->n_pend) {
                WhFrame* fr = frames + depth;
                spec L = lds3(fr->L);
                for (uint32_t k = 0; k < sm->n_pend; k++) if (!w.occ[sm->sh_base + k]) L = L + mks(sm->pend[k][0], sm->pend[k][1], sm->pend[k][2]);
                sts3(fr->L, L);
            }
            bool returning = false;
            spec Lret = mks1(0.0f);
#pragma unroll 1
            for (;;) {
                if (returning) {   // li of frame `depth` has returned Lret
                    if (depth == 0u) { done = true; break; }
                    depth--;
                    WhFrame* pf = frames + depth;
                    const spec val = lds3(pf->f) * Lret * pf->abs_dot / pf->pdf;   // sampler_integrator.rs:121-125, :232-236
                    if (!(pf->has_diff & 256u)) { sts3(pf->refl, val); phase = WH_TRANS; returning = false; }   // the reflected subtree: specular_transmit is next
                    else { Lret = lds3(pf->L) + (lds3(pf->refl) + val); continue; }                            // L += specular_reflect(..) + specular_transmit(..) (whitted.rs:110-112)
                }
                WhFrame* fr = frames + depth;
                const RayIn ray = fr->ray;
                const f3 ro = mk3(ray.ox, ray.oy, ray.oz), rd = mk3(ray.dx, ray.dy, ray.dz);
                const bool has_diff = (fr->has_diff & 1u) != 0u;
                if (phase == WH_AWAIT) {
                    const float4* hp = reinterpret_cast<const float4*>(w.hits_cl + sm->slot);
                    const float4 h0 = hp[0], h1 = hp[1];
                    float4* hd = reinterpret_cast<float4*>(&fr->hit);
                    hd[0] = h0; hd[1] = h1;
                    if (__float_as_uint(h0.y) == 0xFFFFFFFFu) {   // `L += light.le(ray)` of every light (whitted.rs:57-61): zero for all but the infinite ones
                        spec L = mks1(0.0f);
                        for (uint32_t k = 0; k < sc.n_infinite; k++) L = L + light_le<true>(sc, sc.lights[sc.infinite_lights[k]], rd);
                        Lret = L; returning = true;
                        continue;
                    }
                }
                const float4* hq = reinterpret_cast<const float4*>(&fr->hit);
                const float4 h0 = hq[0], h1 = hq[1];
                const uint32_t hprim = __float_as_uint(h0.y);
                MeshRec m;
                QSurf qs; qs.hit = 0u;
                SurfHit si = make_surface_hit_q<QUADRIC>(sc, ro, rd, ray.time, __float_as_uint(h1.y), __float_as_uint(h1.z), h0.z, h0.w, h1.x, m, &qs, h0.x);
                const MaterialRec& mr = sc.materials[m.material];
                if (mr.none) {   // bsdf.is_none(): `return self.li(&isect.spawn_ray(&ray.d), ..)` at the same depth (whitted.rs:63-66); the new ray has no differentials
                    ray_cl = spawn_ray(si, rd);
                    fr->ray = ray_cl; fr->has_diff = 0u;
                    phase = WH_AWAIT; want_cl = true;
                    break;
                }
                const bool tex_hit = w.diffs && (mr.textured != 0u || mr.bump_tex1 != 0u);
                if (tex_hit && mr.bump_tex1) { si.ns = ld3f(fr->v.tex.ns); si.dpdu_s = ld3f(fr->v.tex.dpdu_s); }   // Material::bump: the BSDF is made on the bumped frame
                const WhBsdf bsdf = wh_make_bsdf(sc, si, m.material, &fr->v.tex, tex_hit);
                const f3 wo = si.wo, ns = si.ns;
                if (phase == WH_AWAIT) {   // `L += isect.le(&wo)` (whitted.rs:84)
                    spec L = mks1(0.0f);
                    if (m.first_light >= 0) L = L + area_L(sc.lights[(uint32_t)m.first_light + (hprim - m.tri_base)], si.n, wo);
                    sts3(fr->L, L);
                    phase = WH_LIGHTS; light_next = 0u;
                    if constexpr (MODE == PH_WH_DIRECT) { WhDirect* dl = x.direct + pid; sts3(dl->acc, mks1(0.0f)); dl->flags = 0u; }
                }
                if constexpr (MODE == PH_WH_DIRECT) {
                if (phase == WH_LIGHTS) {   // uniform_sample_all_lights as it runs (common.rs:42-57: one get_2d pair and one estimate_direct per light) / uniform_sample_one_light (common.rs:111-132)
                    WhDirect* dl = x.direct + pid;
                    bool in_flight = false;   // a non-delta light's estimate_direct is: the slice ends with it
                    while (light_next < sc.n_lights && n_sh < PH_WH_SLICE && !in_flight) {
                        uint32_t k = light_next++;
                        if (x.strategy == 1u) {
                            const float nl = (float)sc.n_lights;
                            k = (uint32_t)pminf(get_1d(sc, w.sp, cur) * nl, nl - 1.0f);
                            light_next = sc.n_lights;
                        }
                        const f2 u_light = get_2d(sc, w.sp, cur);
                        const f2 u_scatter = get_2d(sc, w.sp, cur);
                        bool sh = false, mis = false;
                        wd_estimate_send<QUADRIC>(sc, sc.lights[k], k, si, bsdf, u_light, u_scatter, sh, ray_sh[n_sh], sm->pend[n_sh], mis, ray_cl, dl);
                        if (sh) n_sh++;
                        if (!wd_is_delta(sc.lights[k]) && (sh || mis)) {
                            dl->flags = (sh ? WD_SH : 0u) | (mis ? WD_MIS : 0u);
                            want_cl = mis; in_flight = true;
                        }
                    }
                    if (light_next < sc.n_lights || n_sh || in_flight) break;   // more lights, or samples in flight: they join `acc` next round, before L sees it
                    spec ld = lds3(dl->acc);
                    if (x.strategy == 1u && sc.n_lights) ld = ld / ph_div(1.0f, (float)sc.n_lights);   // `estimate / light_pdf` (common.rs:113, :132)
                    sts3(fr->L, lds3(fr->L) + ld);   // `l += light_sample` (direct_lighting.rs:143)
                    phase = WH_REFL;
                }
                } else
                if (phase == WH_LIGHTS) {   // one sample of every light, in the lights' order (whitted.rs:88-104)
                    while (light_next < sc.n_lights && n_sh < PH_WH_SLICE) {
                        const f2 u = get_2d(sc, w.sp, cur);
                        const LiSample ls = wh_light_sample_li<QUADRIC>(sc, sc.lights[light_next], si, u);
                        light_next++;
                        if (!ls.valid || is_black(ls.value) || ls.pdf == 0.0f) continue;
                        const spec f = wh_bsdf_f(bsdf, wo, ls.wi);
                        if (is_black(f)) continue;
                        ray_sh[n_sh] = spawn_ray_to_hit(si, ls.vp, ls.vperr, ls.vn);
                        const spec c = f * ls.value * abs_dot(ls.wi, ns) / ls.pdf;
                        sm->pend[n_sh][0] = c.r; sm->pend[n_sh][1] = c.g; sm->pend[n_sh][2] = c.b;
                        n_sh++;
                    }
                    if (light_next < sc.n_lights) break;   // the slice is full: the loop goes on next round
                    phase = WH_REFL;
                    if (n_sh) break;                        // this slice's samples join L next round, before anything below this vertex is added
                }
                if ((int)depth + 1 >= w.max_depth) {   // whitted.rs:108: no specular recursion at the last level
                    Lret = lds3(fr->L); returning = true;
                    continue;
                }
                // specular_reflect (phase WH_REFL) / specular_transmit (WH_TRANS)
                const bool transmit = phase == WH_TRANS;
                const f2 u = get_2d(sc, w.sp, cur);
                spec f; float pdf; f3 wi;
                wh_sample_specular(bsdf, wo, u, transmit, f, pdf, wi);
                if (pdf > 0.0f && !is_black(f) && abs_dot(wi, ns) != 0.0f) {
                    ray_cl = spawn_ray(si, wi);
                    WhFrame* cf = frames + depth + 1u;
                    cf->ray = ray_cl; cf->has_diff = 0u;
                    if (has_diff) {   // sampler_integrator.rs:96-119, :171-230
                        cf->has_diff = 1u;
                        const RayDiff cd = specular_ray_differentials(si.p, wo, ns, wi, ld3f(fr->v.dpdx), ld3f(fr->v.dpdy), ld3f(fr->v.dndu), ld3f(fr->v.dndv), fr->v.dudx, fr->v.dvdx, fr->v.dudy,
                                                                      fr->v.dvdy, ld3f(fr->rx_d), ld3f(fr->ry_d), bsdf.g.eta, transmit);   // shading_diff.h
                        st3f(cf->rx_o, cd.rx_o); st3f(cf->ry_o, cd.ry_o); st3f(cf->rx_d, cd.rx_d); st3f(cf->ry_d, cd.ry_d);
                    }
                    sts3(fr->f, f); fr->abs_dot = abs_dot(wi, ns); fr->pdf = pdf;
                    fr->has_diff = (fr->has_diff & 1u) | (transmit ? 256u : 0u);   // bit 8: the child in flight is the refracted one
                    depth++; phase = WH_AWAIT; want_cl = true;
                    break;
                }
                // the branch contributes nothing (`Spectrum::ZERO`)
                if (!transmit) { sts3(fr->refl, mks1(0.0f)); phase = WH_TRANS; continue; }
                Lret = lds3(fr->L) + (lds3(fr->refl) + mks1(0.0f)); returning = true;
            }
            sm->depth = depth; sm->phase = phase; sm->dim = cur.dim; sm->light_next = light_next; sm->n_pend = n_sh;
            if (done) {   // radiance sanitising of render_tile (sampler_integrator.rs:373-397)
                spec L = Lret;
                if (has_nans(L)) L = mks1(0.0f);
                else if (lum_y(L) < -1e-5f) L = mks1(0.0f);
                else if (__builtin_isinf(lum_y(L))) L = mks1(0.0f);
                const size_t gsi = (size_t)(w.s0 + (pid - ppix * w.chunk_spp)) * w.n_px + ppix;
                float4 rec = w.rec_L[gsi];
                rec.x = L.r; rec.y = L.g; rec.z = L.b;
                w.rec_L[gsi] = rec;
            }
        }
        const uint32_t cl_slot = wave_alloc(&next->n_cl, want_cl);
        const uint32_t lv_slot = wave_alloc(&next->n_live, active && !done);
        uint32_t sh_slot = 0;
        if (n_sh) sh_slot = atomicAdd(&next->n_sh, n_sh);
        if (active && !done) {
            w.live[par ^ 1][lv_slot] = pid;
            if (want_cl) { store_ray(w.rays_cl[par ^ 1] + cl_slot, ray_cl); sm->slot = cl_slot; }
            for (uint32_t k = 0; k < n_sh; k++) store_ray(w.rays_sh[par ^ 1] + sh_slot + k, ray_sh[k]);
            sm->sh_base = sh_slot;
        }
    }
}

}  // namespace ph
