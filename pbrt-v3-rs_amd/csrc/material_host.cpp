// Materials on the host: the BxDF list compute_scattering_functions builds (materials/src/*.rs), for constant and for textured parameters, from one description each.
#include "material_host.h"
#include "host_math.h"
#include <algorithm>

namespace phost {
namespace {
enum : uint32_t { T_REFL = 1, T_TRANS = 2, T_DIFF = 4, T_GLOSSY = 8, T_SPEC = 16 };
enum { KD = PBRT_HIP_PARAM_KD, KS = PBRT_HIP_PARAM_KS, KR = PBRT_HIP_PARAM_KR, KT = PBRT_HIP_PARAM_KT, OPACITY = PBRT_HIP_PARAM_OPACITY, AMOUNT = PBRT_HIP_PARAM_AMOUNT,
       ETA = PBRT_HIP_PARAM_ETA, K = PBRT_HIP_PARAM_K, REFLECT = PBRT_HIP_PARAM_REFLECT, TRANSMIT = PBRT_HIP_PARAM_TRANSMIT };

float roughness_to_alpha(float roughness) {  // TrowbridgeReitzDistribution::roughness_to_alpha (microfacet/trowbridge_reitz.rs:31-40); host libm logf as for the reference
    roughness = roughness > 1e-3f ? roughness : 1e-3f;
    const float x = std::log(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}
bool black(const float c[3]) { return c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f; }
bool clamp3(const float in[3], float out[3]) {  // clamp_default(); returns !is_black()
    for (int c = 0; c < 3; c++) out[c] = hm::clampf(in[c], 0.0f, hm::kInf);
    return !black(out);
}
LobeRec lobe(uint32_t kind, uint32_t type) { LobeRec l{}; l.kind = kind; l.type = type; l.eta_a = l.eta_b = 1.0f; return l; }
LobeRec dielectric(uint32_t kind, uint32_t type, float eta_a, float eta_b) { LobeRec l = lobe(kind, type); l.fresnel = PH_FR_DIEL; l.eta_a = eta_a; l.eta_b = eta_b; return l; }
void set_tr(LobeRec& l, float ax, float ay) { l.ax = 0.001f > ax ? 0.001f : ax; l.ay = 0.001f > ay ? 0.001f : ay; }  // TrowbridgeReitzDistribution::new: max(0.001, alpha)

// The description's textures, and which of them a lobe took: one that no lobe took makes derive refuse the description.
struct Textures {
    const MaterialSpec& s;
    uint32_t col_taken = 0, flt_taken = 0;
    uint32_t col(int p) { col_taken |= 1u << p; return s.col_tex1[p]; }
    uint32_t flt(int p) { flt_taken |= 1u << p; return s.flt_tex1[p]; }
    // the Trowbridge-Reitz distribution of `l`: the constants (remapped at construction, trowbridge_reitz.rs:31-40) and the float textures (remapped per hit if `remap`)
    void roughness(LobeRec& l, float ur, float vr) {
        if (s.remap) { ur = roughness_to_alpha(ur); vr = roughness_to_alpha(vr); }
        set_tr(l, ur, vr);
        l.ax_tex1 = flt(PH_FPARAM_UROUGHNESS); l.ay_tex1 = flt(PH_FPARAM_VROUGHNESS);
        if (l.ax_tex1 || l.ay_tex1) l.remap = s.remap ? 1u : 0u;
    }
};

void derive_matte(const MaterialSpec& s, Textures& tx, MaterialRec& m, std::vector<LobeRec>& lobes) {  // matte.rs:47-76
    for (int c = 0; c < 3; c++) m.kd[c] = hm::clampf(s.col[KD][c], 0.0f, hm::kInf);  // clamp_default (matte.rs:63)
    m.sigma = hm::clampf(s.sigma, 0.0f, 90.0f);                                      // matte.rs:64
    m.has_bxdf = !black(m.kd);
    if (m.sigma != 0.0f) {  // OrenNayar::new (oren_nayar.rs:28-39)
        float sg = hm::to_radians(m.sigma), s2 = sg * sg;
        m.a = 1.0f - (s2 / (2.0f * (s2 + 0.33f)));
        m.b = 0.45f * s2 / (s2 + 0.09f);
    }
    if (m.has_bxdf) {
        LobeRec l = lobe(m.sigma != 0.0f ? PH_LK_OREN : PH_LK_LAMBERT, T_REFL | T_DIFF);
        std::memcpy(l.r, m.kd, 12); l.a = m.a; l.b = m.b;
        m.kd_tex1 = l.r_tex1 = tx.col(KD);   // the one-lobe kernel reads kd_tex1
        lobes.push_back(l);
    }
}
void derive_mirror(const MaterialSpec& s, Textures& tx, std::vector<LobeRec>& lobes) {  // mirror.rs:40-62
    float r[3];
    if (clamp3(s.col[KR], r)) { LobeRec l = lobe(PH_LK_SPEC_R, T_REFL | T_SPEC); l.fresnel = PH_FR_NOOP; std::memcpy(l.r, r, 12); l.r_tex1 = tx.col(KR); lobes.push_back(l); }
}
void derive_plastic(const MaterialSpec& s, Textures& tx, MaterialRec& m, std::vector<LobeRec>& lobes) {  // plastic.rs:50-82
    float d[3], sp[3];
    if (clamp3(s.col[KD], d)) { LobeRec l = lobe(PH_LK_LAMBERT, T_REFL | T_DIFF); std::memcpy(l.r, d, 12); l.r_tex1 = tx.col(KD); lobes.push_back(l); }
    if (clamp3(s.col[KS], sp)) {
        LobeRec l = dielectric(PH_LK_MICRO_R, T_REFL | T_GLOSSY, 1.5f, 1.0f); std::memcpy(l.r, sp, 12); l.r_tex1 = tx.col(KS);
        tx.roughness(l, s.urough, s.urough);
        lobes.push_back(l);
    } else if (!lobes.empty()) m.kd_tex1 = lobes[0].r_tex1;   // a lone Lambertian lobe: the one-lobe kernel's texture
}
// glass.rs:62-141 with allow_multiple_lobes = true (path.rs:143).  With a roughness texture, which lobes a hit gets depends on `urough == 0 && vrough == 0` there: the list holds
// the smooth alternative (FresnelSpecular) and the rough one (the microfacet pair); every lobe carries the textures (the smooth one for its `== 0` test)
void derive_glass(const MaterialSpec& s, Textures& tx, MaterialRec& m, std::vector<LobeRec>& lobes) {
    float r[3], t[3];
    const bool per_hit = s.flt_tex1[PH_FPARAM_UROUGHNESS] || s.flt_tex1[PH_FPARAM_VROUGHNESS];
    const bool has_r = clamp3(s.col[KR], r) || (per_hit && s.col_tex1[KR]), has_t = clamp3(s.col[KT], t) || (per_hit && s.col_tex1[KT]);
    const bool smooth = s.urough == 0.0f && s.vrough == 0.0f;
    auto tag = [&](LobeRec& l, uint32_t alt) { if (per_hit) { l.alt = alt; l.ur_raw = s.urough; l.vr_raw = s.vrough; tx.roughness(l, s.urough, s.vrough); } };
    if ((per_hit || smooth) && (has_r || has_t)) {
        LobeRec l = lobe(PH_LK_FRESNEL_SPEC, T_REFL | T_TRANS | T_SPEC); std::memcpy(l.r, r, 12); std::memcpy(l.t, t, 12); l.eta_a = 1.0f; l.eta_b = s.index;
        l.r_tex1 = tx.col(KR); l.t_tex1 = tx.col(KT);
        tag(l, 1u);
        lobes.push_back(l);
    }
    if (per_hit || !smooth) {
        if (has_r) { LobeRec l = dielectric(PH_LK_MICRO_R, T_REFL | T_GLOSSY, 1.0f, s.index); std::memcpy(l.r, r, 12); l.r_tex1 = tx.col(KR);
                     if (per_hit) tag(l, 2u); else tx.roughness(l, s.urough, s.vrough);
                     lobes.push_back(l); }
        if (has_t) { LobeRec l = dielectric(PH_LK_MICRO_T, T_TRANS | T_GLOSSY, 1.0f, s.index); std::memcpy(l.t, t, 12); l.t_tex1 = tx.col(KT);
                     if (per_hit) tag(l, 2u); else tx.roughness(l, s.urough, s.vrough);
                     lobes.push_back(l); }
    }
    if (!lobes.empty()) m.index_tex1 = tx.flt(PH_FPARAM_INDEX);   // `let eta = self.index.evaluate(..)` (glass.rs:102): every dielectric lobe of the hit takes it
}
void derive_metal(const MaterialSpec& s, Textures& tx, std::vector<LobeRec>& lobes) {  // metal.rs:62-125
    LobeRec l = lobe(PH_LK_MICRO_R, T_REFL | T_GLOSSY); l.fresnel = PH_FR_COND;
    l.r[0] = l.r[1] = l.r[2] = 1.0f; std::memcpy(l.c_eta_t, s.col[ETA], 12); std::memcpy(l.c_k, s.col[K], 12);
    l.eta_tex1 = tx.col(ETA); l.k_tex1 = tx.col(K);
    tx.roughness(l, s.urough, s.vrough);
    lobes.push_back(l);
}
// uber.rs:116-186.  Constant opacity: each colour is `op * k.clamp_default()`, its lobe made where that is not black; a textured colour is multiplied by the opacity, then tested
// (has_pre 1).  With an opacity texture the list holds every lobe the material CAN have (uber.rs:126-160): colours, presence and BSDF::eta are decided per hit.
void derive_uber(const MaterialSpec& s, Textures& tx, MaterialRec& m, std::vector<LobeRec>& lobes) {
    float op[3], t[3], tmp[3];
    clamp3(s.col[OPACITY], op);
    const float e = s.index;
    m.opacity_tex1 = tx.col(OPACITY);
    const bool per_hit = m.opacity_tex1 != 0u;
    if (per_hit) {
        LobeRec l = dielectric(PH_LK_SPEC_T, T_TRANS | T_SPEC, 1.0f, 1.0f); l.has_pre = PH_PRE_PASSTHROUGH; lobes.push_back(l);
        m.bsdf_eta = 1.0f; m.bsdf_eta_alt = e; m.uber_eta = 1u;
        m.index_tex1 = tx.flt(PH_FPARAM_INDEX);   // `let e = self.index.evaluate(..)` (uber.rs:128)
    } else {
        for (int c = 0; c < 3; c++) tmp[c] = op[c] * -1.0f + 1.0f;  // (-op + Spectrum::ONE)
        if (clamp3(tmp, t)) { m.bsdf_eta = 1.0f; LobeRec l = dielectric(PH_LK_SPEC_T, T_TRANS | T_SPEC, 1.0f, 1.0f); std::memcpy(l.t, t, 12); lobes.push_back(l); }
        else m.bsdf_eta = e;
    }
    for (int p = KD; p <= KT; p++) {
        float base[3], v[3];
        const bool nonblack = clamp3(s.col[p], base);
        for (int c = 0; c < 3; c++) v[c] = op[c] * base[c];
        if (per_hit ? !nonblack : black(v)) continue;   // black at every hit: the lobe is never added
        LobeRec l = p == KD ? lobe(PH_LK_LAMBERT, T_REFL | T_DIFF) : p == KS ? dielectric(PH_LK_MICRO_R, T_REFL | T_GLOSSY, 1.0f, e)
                  : p == KR ? dielectric(PH_LK_SPEC_R, T_REFL | T_SPEC, 1.0f, e) : dielectric(PH_LK_SPEC_T, T_TRANS | T_SPEC, 1.0f, e);
        if (p == KS) tx.roughness(l, s.urough, s.vrough);
        const uint32_t tex1 = tx.col(p);
        (p == KT ? l.t_tex1 : l.r_tex1) = tex1;
        if (per_hit) { l.has_pre = PH_PRE_OPACITY; std::memcpy(l.pre, base, 12); }
        else {
            std::memcpy(p == KT ? l.t : l.r, v, 12);
            if (tex1) { l.has_pre = 1u; std::memcpy(l.pre, op, 12); }
        }
        lobes.push_back(l);
    }
}
void derive_substrate(const MaterialSpec& s, Textures& tx, std::vector<LobeRec>& lobes) {  // substrate.rs:55-84
    float d[3], sp[3];
    const bool db = clamp3(s.col[KD], d), sb = clamp3(s.col[KS], sp);
    if (db || sb) {
        LobeRec l = lobe(PH_LK_FRESNEL_BLEND, T_REFL | T_GLOSSY); std::memcpy(l.r, d, 12); std::memcpy(l.t, sp, 12); l.r_tex1 = tx.col(KD); l.t_tex1 = tx.col(KS);
        tx.roughness(l, s.urough, s.vrough);
        lobes.push_back(l);
    }
}
// translucent.rs:57-112.  Constant reflect / transmit: each lobe keeps that factor of its product (pre, PH_PRE_RAW_TEST) so that a Kd / Ks texture can replace the other factor per
// hit.  With a reflect / transmit texture the list holds every lobe the material CAN have (translucent.rs:76-98): a lobe's colour is the product of the hit's reflect or transmit with
// the hit's Kd or Ks, kept where neither factor is black (PH_PRE_RT); where reflect and transmit are both black the hit has no BSDF at all.
void derive_translucent(const MaterialSpec& s, Textures& tx, MaterialRec& m, std::vector<LobeRec>& lobes) {
    m.bsdf_eta = 1.5f;
    float rt[2][3];
    const bool per_hit = s.col_tex1[REFLECT] || s.col_tex1[TRANSMIT];
    const bool side_on[2] = {clamp3(s.col[REFLECT], rt[0]) || per_hit, clamp3(s.col[TRANSMIT], rt[1]) || per_hit};
    if (per_hit) {
        m.rt_mode = 1u; m.refl_tex1 = tx.col(REFLECT); m.trans_tex1 = tx.col(TRANSMIT);
        std::memcpy(m.refl_c, rt[0], 12); std::memcpy(m.trans_c, rt[1], 12);
    } else if (!side_on[0] && !side_on[1]) m.none = 1u;   // `return` before a BSDF is made (translucent.rs:72-74): every hit is passed through, as with Material "none"
    for (int p = KD; p <= KS; p++) {
        float base[3];
        if (!clamp3(s.col[p], base)) continue;   // Kd / Ks black at every hit
        for (int side = 0; side < 2; side++) {
            if (!side_on[side]) continue;
            LobeRec l;
            if (p == KD) l = side ? lobe(PH_LK_LAMBERT_T, T_TRANS | T_DIFF) : lobe(PH_LK_LAMBERT, T_REFL | T_DIFF);
            else {
                l = side ? dielectric(PH_LK_MICRO_T, T_TRANS | T_GLOSSY, 1.0f, 1.5f) : dielectric(PH_LK_MICRO_R, T_REFL | T_GLOSSY, 1.0f, 1.5f);
                tx.roughness(l, s.urough, s.urough);
                if (per_hit) l.remap = s.remap ? 1u : 0u;
            }
            (side ? l.t_tex1 : l.r_tex1) = tx.col(p);
            if (per_hit) { l.has_pre = PH_PRE_RT; std::memcpy(l.pre, base, 12); }
            else {
                float* v = side ? l.t : l.r;
                for (int c = 0; c < 3; c++) v[c] = rt[side][c] * base[c];
                l.has_pre = PH_PRE_RAW_TEST; std::memcpy(l.pre, rt[side], 12);
            }
            lobes.push_back(l);
        }
    }
}
const char* derive_mix(const MaterialSpec& s, Textures& tx, MaterialRec& m, std::vector<LobeRec>& lobes, int& code) {  // mix.rs:51-88; returns what is wrong (and `code`), or null
    code = PBRT_HIP_ERR_UNSUPPORTED;
    float sc[2][3], tmp[3];
    clamp3(s.col[AMOUNT], sc[0]);
    for (int c = 0; c < 3; c++) tmp[c] = 1.0f - sc[0][c];
    clamp3(tmp, sc[1]);
    const MaterialRec &a = s.child_rec[0], &b = s.child_rec[1];
    // mix.rs:63-76: m1 bumps `si` itself, m2 a clone of it, and the mixture's BSDF is made on `si`: the first material's bump map shapes the frame of every
    // lobe, the second one's changes nothing that is used
    m.bump_tex1 = a.bump_tex1;
    if (a.amount_tex1 || b.amount_tex1) return "add_material_mix: a sub-material is a mix whose amount is a texture; not supported";
    if (a.rt_mode || b.rt_mode) return "add_material_mix: a translucent sub-material with a reflect / transmit texture (a per-hit null BSDF) is not supported";
    if (a.index_tex1 || b.index_tex1) return "add_material_mix: a sub-material with a textured index of refraction is not supported";
    if (a.opacity_tex1 && b.opacity_tex1) return "add_material_mix: both sub-materials are uber materials with opacity textures; not supported";
    m.opacity_tex1 = a.opacity_tex1 ? a.opacity_tex1 : b.opacity_tex1;
    if (s.child_lobes[0].size() + s.child_lobes[1].size() > 8) return code = PBRT_HIP_ERR_INVALID_ARG, "add_material_mix: more than MAX_BXDFS = 8 lobes (BSDF::add asserts, bsdf.rs:119-125)";
    const uint32_t amount_tex1 = tx.col(AMOUNT);   // mix.rs:59-60
    for (int k = 0; k < 2; k++)
        for (LobeRec l : s.child_lobes[k]) {
            if (l.n_scale >= 2) return "add_material_mix: mix nested deeper than two levels";
            std::memcpy(l.n_scale == 0 ? l.scale0 : l.scale1, sc[k], 12); l.n_scale++;
            if (amount_tex1) l.amt = (k == 0 ? 1u : 2u) | ((l.n_scale - 1u) << 8);
            lobes.push_back(l);
        }
    uint32_t cols = 0, scal = 0; const LobeRec* first = nullptr;
    for (const LobeRec& l : lobes) {
        cols += lobe_tex_cols(l);
        if (l.ax_tex1 || l.ay_tex1 || l.sigma_tex1) {
            if (!first) { first = &l; scal = 1; }
            else if (l.ax_tex1 != first->ax_tex1 || l.ay_tex1 != first->ay_tex1 || l.remap != first->remap || l.sigma_tex1 != first->sigma_tex1 || l.ax != first->ax || l.ay != first->ay) scal++;
        }
    }
    if (a.textured || b.textured) {
        // the sub-materials' textures are evaluated per hit and each lobe is kept or dropped as its own material would (mix.rs:63-87); the per-hit list has
        // PH_HIT_LOBES lobe slots, PH_HIT_COLS colour slots and ONE pair of per-hit scalars (roughness or sigma)
        if (lobes.size() > PH_HIT_LOBES || cols > PH_HIT_COLS || scal > 1u)
            return "add_material_mix: a textured mix may have at most 8 lobes, 6 textured colours and one textured roughness / sigma";
        m.textured = 1u;
    }
    if (amount_tex1 && (1u + cols > PH_HIT_COLS || lobes.size() > PH_HIT_LOBES)) return "set_material_texture: a mix with a textured amount may have at most 5 more per-hit colours";
    m.amount_tex1 = amount_tex1;
    return nullptr;
}
}  // namespace

uint32_t lobe_tex_cols(const LobeRec& l) {
    if (l.has_pre == PH_PRE_RT) return 1u;   // one product colour per lobe
    return (l.r_tex1 || (l.has_pre == PH_PRE_OPACITY && l.kind != PH_LK_SPEC_T) ? 1u : 0u) + (l.t_tex1 || (l.has_pre == PH_PRE_OPACITY && l.kind == PH_LK_SPEC_T) || l.has_pre == PH_PRE_PASSTHROUGH ? 1u : 0u) +
           (l.eta_tex1 ? 1u : 0u) + (l.k_tex1 ? 1u : 0u);
}

int derive(const MaterialSpec& s, MaterialRec& rec, std::vector<LobeRec>& out_lobes, std::string& why) {
    auto refuse = [&](int code, const char* msg) { why = msg; return code; };
    MaterialRec m{}; m.bsdf_eta = 1.0f;
    std::vector<LobeRec> lobes;
    Textures tx{s};
    switch (s.kind) {
    case MaterialKind::None: m.none = 1u; break;   // Material "none" / "" (graphics_state.rs make_material -> None)
    case MaterialKind::Matte: derive_matte(s, tx, m, lobes); break;
    case MaterialKind::Mirror: derive_mirror(s, tx, lobes); break;
    case MaterialKind::Plastic: derive_plastic(s, tx, m, lobes); break;
    case MaterialKind::Glass: derive_glass(s, tx, m, lobes); break;
    case MaterialKind::Metal: derive_metal(s, tx, lobes); break;
    case MaterialKind::Uber: derive_uber(s, tx, m, lobes); break;
    case MaterialKind::Substrate: derive_substrate(s, tx, lobes); break;
    case MaterialKind::Translucent: derive_translucent(s, tx, m, lobes); break;
    case MaterialKind::Mix: { int code; if (const char* msg = derive_mix(s, tx, m, lobes, code)) return refuse(code, msg); break; }
    }
    if (s.flt_tex1[PH_FPARAM_SIGMA]) {   // matte.rs:64-70
        if (m.none || lobes.size() != 1u || !(lobes[0].kind == PH_LK_LAMBERT || lobes[0].kind == PH_LK_OREN))
            return refuse(PBRT_HIP_ERR_UNSUPPORTED, "set_material_float_texture: sigma belongs to MatteMaterial (created with a non-black Kd)");
        lobes[0].sigma_tex1 = m.sigma_tex1 = tx.flt(PH_FPARAM_SIGMA);
    }
    bool textured = false;
    for (int p = 0; p < 10; p++) {
        if (!s.col_tex1[p]) continue;
        textured = true;
        if (tx.col_taken & (1u << p)) continue;
        if (p <= KT)
            return refuse(PBRT_HIP_ERR_UNSUPPORTED, "set_material_texture: this material has no lobe fed by that parameter (matte Kd, plastic Kd / Ks, mirror Kr, substrate Kd / Ks, "
                                                    "glass Kr / Kt, uber Kd / Ks / Kr / Kt and translucent Kd / Ks take textures; create the material with a non-black placeholder for the parameter)");
        return refuse(PBRT_HIP_ERR_UNSUPPORTED, p == OPACITY ? "set_material_texture: opacity belongs to UberMaterial" : p == AMOUNT ? "set_material_texture: amount belongs to MixMaterial"
                                              : p == ETA || p == K ? "set_material_texture: eta / k belong to MetalMaterial" : "set_material_texture: reflect / transmit belong to TranslucentMaterial");
    }
    for (int p = 0; p < 4; p++) {
        if (!s.flt_tex1[p]) continue;
        textured = true;
        if (tx.flt_taken & (1u << p)) continue;
        const bool dielectric_index = s.kind == MaterialKind::Glass || s.kind == MaterialKind::Uber;
        if (p == PH_FPARAM_INDEX)
            return refuse(PBRT_HIP_ERR_UNSUPPORTED, dielectric_index ? "set_material_float_texture: this material has no lobe (black Kr and Kt)" : "set_material_float_texture: index belongs to GlassMaterial and UberMaterial");
        return refuse(PBRT_HIP_ERR_UNSUPPORTED, s.kind == MaterialKind::Glass ? "set_material_float_texture: this glass has neither reflection nor transmission"
                                              : "set_material_float_texture: this material has no microfacet lobe whose roughness could be textured (plastic, uber, substrate, translucent and metal have; glass switches lobes on roughness == 0 and is not wired)");
    }
    if (textured) m.textured = 1u;
    if (s.bump_tex1) {   // Material::bump's displacement texture (core/src/material.rs:62-101; the `bumpmap` parameter every material takes)
        if (m.none) return refuse(PBRT_HIP_ERR_INVALID_ARG, "set_material_bump: Material \"none\" has no BSDF to bump");
        m.bump_tex1 = s.bump_tex1;
    }
    m.n_lobes = (uint32_t)lobes.size();
    rec = m; out_lobes = std::move(lobes);
    return PBRT_HIP_OK;
}

static MaterialFlags flags_of(const MaterialHost::Item& it) {
    MaterialFlags f;
    f.general = it.spec.kind != MaterialKind::None && it.spec.kind != MaterialKind::Matte;   // not matte: the renderer uses the general BSDF kernel
    f.textured = it.rec.textured || it.rec.bump_tex1;
    f.bump = it.rec.bump_tex1 != 0u;
    f.has_none = it.rec.none || it.rec.rt_mode;   // some hits may have no BSDF: paths can need more rounds than max_depth + 1
    return f;
}
MaterialFlags MaterialHost::flags() const {
    MaterialFlags f;
    for (const Item& it : items) { const MaterialFlags g = flags_of(it); f.general |= g.general; f.textured |= g.textured; f.bump |= g.bump; f.has_none |= g.has_none; }
    return f;
}

int add_material(MaterialHost& h, const MaterialSpec& spec, uint32_t* out_id, std::string& why) {
    MaterialHost::Item it;
    const int rc = derive(spec, it.rec, it.lobes, why);
    if (rc) return rc;
    it.spec = spec;
    h.items.push_back(std::move(it));
    if (out_id) *out_id = (uint32_t)h.items.size() - 1;
    return PBRT_HIP_OK;
}
MaterialSpec mix_spec(const MaterialHost& h, uint32_t material1, uint32_t material2, const float amount[3]) {
    MaterialSpec s(MaterialKind::Mix); s.set(AMOUNT, amount);
    const uint32_t id[2] = {material1, material2};
    for (int k = 0; k < 2; k++) { s.child_lobes[k] = h.items[id[k]].lobes; s.child_rec[k] = h.items[id[k]].rec; }
    return s;
}
static int store_changed(MaterialHost::Item& it, MaterialSpec&& spec, std::string& why) {
    MaterialRec rec; std::vector<LobeRec> lobes;
    const int rc = derive(spec, rec, lobes, why);
    if (rc) return rc;
    rec.sort_class = it.rec.sort_class;   // build_accel's, not derived
    it.spec = std::move(spec); it.rec = rec; it.lobes = std::move(lobes);
    return PBRT_HIP_OK;
}
int set_colour_texture(MaterialHost& h, uint32_t material, int param, uint32_t texture, std::string& why) {
    if (param < 0 || param > 9) { why = "set_material_texture: param must be PBRT_HIP_PARAM_KD / KS / KR / KT / OPACITY / AMOUNT / ETA / K / REFLECT / TRANSMIT"; return PBRT_HIP_ERR_INVALID_ARG; }
    MaterialSpec spec = h.items[material].spec;
    spec.col_tex1[param] = texture + 1u;
    return store_changed(h.items[material], std::move(spec), why);
}
int set_float_texture(MaterialHost& h, uint32_t material, int fparam, uint32_t texture, std::string& why) {
    if (fparam < 0 || fparam > 3) { why = "set_material_float_texture: fparam must be 0 sigma, 1 uroughness, 2 vroughness or 3 index"; return PBRT_HIP_ERR_INVALID_ARG; }
    MaterialSpec spec = h.items[material].spec;
    spec.flt_tex1[fparam] = texture + 1u;
    return store_changed(h.items[material], std::move(spec), why);
}
int set_bump_texture(MaterialHost& h, uint32_t material, uint32_t texture, std::string& why) {
    MaterialSpec spec = h.items[material].spec;
    spec.bump_tex1 = texture + 1u;
    return store_changed(h.items[material], std::move(spec), why);
}
bool uber_index_needs_opacity(const MaterialHost& h, uint32_t material, float opacity[3]) {
    const MaterialSpec& s = h.items[material].spec;
    if (s.kind != MaterialKind::Uber || s.col_tex1[OPACITY]) return false;
    clamp3(s.col[OPACITY], opacity);
    return true;
}

void layout_lobe_pool(const MaterialHost& h, std::vector<MaterialRec>& recs, std::vector<LobeRec>& pool) {
    recs.clear(); pool.clear();
    for (const MaterialHost::Item& it : h.items) {   // per material: what the texture pass has to hand to the shade pass
        MaterialRec m = it.rec;
        m.lobe_base = (uint32_t)pool.size();
        uint32_t cols = m.amount_tex1 ? 1u : 0u; bool hdr = m.bump_tex1 != 0u || m.sigma_tex1 != 0u;
        for (LobeRec l : it.lobes) {
            l.slot0 = cols;   // where this lobe's colours start in TexOut (bsdf_general.h: patch_lobe reads them from there)
            cols += lobe_tex_cols(l);
            if (l.has_pre == PH_PRE_RT || l.sigma_tex1 || l.ax_tex1 || l.ay_tex1 || l.alt || l.has_pre == PH_PRE_RAW_TEST) hdr = true;   // PH_PRE_RT: the lobe's black bit and the material's null-BSDF bit in the header
            pool.push_back(l);
        }
        if (m.sigma_tex1 || hdr) cols = std::max(cols, 2u);   // the per-hit scalars travel in the fourth component of the first two colour slots
        if (m.index_tex1) cols = std::max(cols, 3u);          // ... the per-hit index of refraction in the third one's
        if (m.rt_mode) hdr = true;
        m.tex_cols = std::min<uint32_t>(cols, PH_HIT_COLS); m.tex_hdr = hdr ? 1u : 0u;
        recs.push_back(m);
    }
}

}  // namespace phost
