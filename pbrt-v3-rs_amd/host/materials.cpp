// Materials (api/src/graphics_state.rs:254-340 make_material, each material's From<&TextureParams>): one table row per material type says which parameters it reads, in which
// order, with which defaults, which per-hit slot of the library a texture on each is wired to, and which constructor takes the values.  Everything else here is derived from it.
#include "pbrt_host.hpp"
#include <cstdio>
#include <cstring>

namespace pbrt_host {
namespace {

enum ParamKind {
    kSpectrum, kFloat,
    kRoughnessUV,   // `roughness`, then `uroughness` / `vroughness` which fall back to it: two values (metal.rs:69-76, uber.rs:148-155)
    kIndex          // the index of refraction as quirk B14 has it (eta_of below): one value
};
// pbrt_hip_set_material_float_texture's fparam; kFparamRoughness is the single `roughness`, which fills u and v, each only where nothing is set yet
enum { kNoSlot = -1, kFparamSigma = 0, kFparamURoughness = 1, kFparamVRoughness = 2, kFparamIndex = 3, kFparamRoughness = 4 };
struct MatParam { const char* name; ParamKind kind; float dflt; int slot; };   // slot: PBRT_HIP_PARAM_* (spectrum) or kFparam* (float)
struct MatValues { std::array<float, 3> c[5]; float f[3]; uint32_t sub[2]; int remap; };   // what the parameters came to, spectra and floats each in the row's order
struct MatRow {
    const char* type;
    std::vector<MatParam> params;   // in evaluation order: warnings, the first error and the cache key follow it
    int (*make)(PbrtHipScene*, const MatValues&, uint32_t*);
    bool bump = true;      // MixMaterial and "none" have no bump map
    bool mix = false;      // two named sub-materials follow the parameters
    bool copper = false;   // the two spectra default to copper's measured n and k (metal.rs:136-147)
};
#define MAKE(call) [](PbrtHipScene* s, const MatValues& v, uint32_t* id) -> int { (void)v; return call; }
const std::vector<MatRow> kMaterials = {
    {"none", {}, MAKE(pbrt_hip_add_material_none(s, id)), false},   // no BSDF: graphics_state.rs make_material returns None
    {"matte", {{"Kd", kSpectrum, 0.5f, PBRT_HIP_PARAM_KD}, {"sigma", kFloat, 0.0f, kFparamSigma}}, MAKE(pbrt_hip_add_material_matte(s, v.c[0].data(), v.f[0], id))},
    {"mirror", {{"Kr", kSpectrum, 0.9f, PBRT_HIP_PARAM_KR}}, MAKE(pbrt_hip_add_material_mirror(s, v.c[0].data(), id))},
    {"plastic", {{"Kd", kSpectrum, 0.25f, PBRT_HIP_PARAM_KD}, {"Ks", kSpectrum, 0.25f, PBRT_HIP_PARAM_KS}, {"roughness", kFloat, 0.1f, kFparamRoughness}},
     MAKE(pbrt_hip_add_material_plastic(s, v.c[0].data(), v.c[1].data(), v.f[0], v.remap, id))},
    {"glass", {{"Kr", kSpectrum, 1.0f, PBRT_HIP_PARAM_KR}, {"Kt", kSpectrum, 1.0f, PBRT_HIP_PARAM_KT}, {"uroughness", kFloat, 0.0f, kFparamURoughness}, {"vroughness", kFloat, 0.0f, kFparamVRoughness},
               {"index", kIndex, 1.5f, kFparamIndex}},   // (glass reads no `roughness`)
     MAKE(pbrt_hip_add_material_glass(s, v.c[0].data(), v.c[1].data(), v.f[0], v.f[1], v.f[2], v.remap, id))},
    {"metal", {{"eta", kSpectrum, 0.0f, PBRT_HIP_PARAM_ETA}, {"k", kSpectrum, 0.0f, PBRT_HIP_PARAM_K}, {"roughness", kRoughnessUV, 0.01f, kFparamRoughness}},
     MAKE(pbrt_hip_add_material_metal(s, v.c[0].data(), v.c[1].data(), v.f[0], v.f[1], v.remap, id)), true, false, true},
    {"uber", {{"Kd", kSpectrum, 0.25f, PBRT_HIP_PARAM_KD}, {"Ks", kSpectrum, 0.25f, PBRT_HIP_PARAM_KS}, {"Kr", kSpectrum, 0.0f, PBRT_HIP_PARAM_KR}, {"Kt", kSpectrum, 0.0f, PBRT_HIP_PARAM_KT},
              {"opacity", kSpectrum, 1.0f, PBRT_HIP_PARAM_OPACITY}, {"roughness", kRoughnessUV, 0.1f, kFparamRoughness}, {"index", kIndex, 1.5f, kFparamIndex}},
     MAKE(pbrt_hip_add_material_uber(s, v.c[0].data(), v.c[1].data(), v.c[2].data(), v.c[3].data(), v.c[4].data(), v.f[0], v.f[1], v.f[2], v.remap, id))},
    {"substrate", {{"Kd", kSpectrum, 0.5f, PBRT_HIP_PARAM_KD}, {"Ks", kSpectrum, 0.5f, PBRT_HIP_PARAM_KS}, {"uroughness", kFloat, 0.1f, kFparamURoughness}, {"vroughness", kFloat, 0.1f, kFparamVRoughness}},
     MAKE(pbrt_hip_add_material_substrate(s, v.c[0].data(), v.c[1].data(), v.f[0], v.f[1], v.remap, id))},
    {"translucent", {{"Kd", kSpectrum, 0.25f, PBRT_HIP_PARAM_KD}, {"Ks", kSpectrum, 0.25f, PBRT_HIP_PARAM_KS}, {"reflect", kSpectrum, 0.5f, PBRT_HIP_PARAM_REFLECT},
                     {"transmit", kSpectrum, 0.5f, PBRT_HIP_PARAM_TRANSMIT}, {"roughness", kFloat, 0.1f, kFparamRoughness}},
     MAKE(pbrt_hip_add_material_translucent(s, v.c[0].data(), v.c[1].data(), v.c[2].data(), v.c[3].data(), v.f[0], v.remap, id))},
    // graphics_state.rs:310-330: two named materials, an unknown name falls back to matte made from the same parameters
    {"mix", {{"amount", kSpectrum, 0.5f, PBRT_HIP_PARAM_AMOUNT}}, MAKE(pbrt_hip_add_material_mix(s, v.sub[0], v.sub[1], v.c[0].data(), id)), false, true},
};
#undef MAKE

const MatRow* row_of(const std::string& type) {
    for (const MatRow& r : kMaterials)
        if (type == r.type || (type.empty() && !std::strcmp(r.type, "none"))) return &r;
    return nullptr;
}

// every parameter name some material reads: what a Shape directive may override
std::vector<std::string> parameter_names() {
    std::vector<std::string> names = {"bumpmap"};
    auto add = [&](const char* n) { for (const std::string& s : names) if (s == n) return; names.push_back(n); };
    for (const MatRow& r : kMaterials)
        for (const MatParam& q : r.params) {
            add(q.name);
            if (q.kind == kRoughnessUV) { add("uroughness"); add("vroughness"); }
            if (q.kind == kIndex) add("eta");   // eta_of reports a parameter of that name
        }
    return names;
}

}  // namespace

// MatteMaterial From<&TextureParams> (materials/src/matte.rs:95-110) with TextureParams's lookup order: shape parameters
// first, then the material's own (core/src/paramset/texture_params.rs).
uint32_t Api::material_id_for(const MaterialDesc& m) {
    int64_t ftex_param[4] = {-1, -1, -1, -1};     // by kFparam*: the float parameter names a texture the library evaluates per hit
    int64_t tex_param[10] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};  // by PBRT_HIP_PARAM_*: the same for spectrum parameters
    const MatRow* row = row_of(m.type);
    // one parameter, a float (in all three channels) or a spectrum: a literal or a constant texture as its value; a texture the library evaluates per hit is noted for the
    // parameter's slot and a placeholder returned (white, or the float's default), which the material is created with before the texture is attached
    auto param = [&](const std::string& pname, bool want_float, std::array<float, 3> d, int slot) {
        const TexRef r = resolve(m.params, pname, want_float, d);
        if (r.kind == TexRef::Constant) return r.value;
        const char* what = want_float ? "float" : "spectrum";
        if (r.kind == TexRef::Device) {
            if (slot == kNoSlot || r.is_float != want_float) {
                if (error.empty()) error = "texture '" + r.name + "' on parameter '" + pname + "' of Material \"" + m.type + "\": per-hit " + what + " textures are wired to " +
                                           (want_float ? "matte sigma and to the roughness of plastic / uber / substrate / metal / translucent / glass"
                                                       : "matte Kd, plastic Kd / Ks, mirror Kr, substrate Kd / Ks, glass Kr / Kt, uber Kd / Ks / Kr / Kt / opacity, translucent Kd / Ks / reflect / transmit, mix amount and metal eta / k");
                return r.value;
            }
            if (!want_float) tex_param[slot] = (int64_t)r.id;
            else if (slot == kFparamRoughness) { for (int k : {kFparamURoughness, kFparamVRoughness}) if (ftex_param[k] < 0) ftex_param[k] = (int64_t)r.id; }
            else ftex_param[slot] = (int64_t)r.id;
            return want_float ? d : std::array<float, 3>{1.0f, 1.0f, 1.0f};
        }
        if (r.kind == TexRef::Unsupported && error.empty())
            error = "texture '" + r.name + "' of class '" + r.cls + "' is not evaluated by the library yet (constant, scale, mix and imagemap are)";
        else if (error.empty()) warn(std::string("Couldn't find ") + what + " texture named '" + r.name + "' for parameter '" + pname + "'");
        return r.value;
    };
    auto float_param = [&](const std::string& pname, float d, int slot) { return param(pname, true, {d, d, d}, slot)[0]; };
    // `bumpmap`: get_float_texture_or_none (every material's From<&TextureParams>): a float texture by name, never a literal
    int64_t bump_tex = -1;
    {
        const std::string bn = m.params.find_one_texture("bumpmap");
        if (!bn.empty()) {
            const TexRef r = lookup_texture(bn, true);
            if (r.kind == TexRef::Device && r.is_float) bump_tex = (int64_t)r.id;
            else if (r.kind == TexRef::Constant) {
                uint32_t id = 0;
                if (!check(ABI(pbrt_hip_add_texture_constant(scene_, r.value.data(), &id)), "add_texture_constant")) return 0;
                bump_tex = (int64_t)id;
            } else if (r.kind == TexRef::Unsupported) { if (error.empty()) error = "'bumpmap' texture '" + bn + "' of class '" + r.cls + "' is not evaluated by the library"; }
            else warn("Couldn't find float texture named '" + bn + "' for parameter 'bumpmap'");
            if (bump_tex >= 0 && row && !row->bump) bump_tex = -1;
        }
    }
    // Quirk B14 (glass.rs:158-161, uber.rs:201-204): the reference asks `tp.get_float_texture("eta")`, which is a lookup in the table of NAMED float textures — one
    // declared as `Texture "eta" "float" ...` — and not a parameter look-up: the `"float eta" 2` that pbrt-v3 scenes (and the reference's own depth-of-field.pbrt) write is never
    // read.  Without such a texture the index of refraction is the "index" parameter, default 1.5.  Its render of depth-of-field.pbrt shows eta 1.5 spheres, pixel for pixel.
    auto eta_of = [&](const MatParam& index) {
        const TexRef named = lookup_texture("eta", true);
        if (named.kind == TexRef::Constant) return named.value[0];   // a constant float texture that happens to be called "eta"
        if (named.kind == TexRef::Device && named.is_float) { ftex_param[index.slot] = (int64_t)named.id; return index.dflt; }   // the float texture NAMED "eta": the index of refraction of every hit (glass.rs:158-161)
        if (named.kind == TexRef::Device || named.kind == TexRef::Unsupported) {
            if (error.empty()) error = "Material \"" + m.type + "\": the texture named \"eta\" would set the index of refraction per hit (glass.rs:158), but it is not a float texture the library evaluates";
            return index.dflt;
        }
        if (m.params.floats.count("eta") || !m.params.find_one_texture("eta").empty())
            warn("Material \"" + m.type + "\": the reference does not read the parameter \"eta\" (it looks up a float texture NAMED \"eta\", glass.rs:158 / uber.rs:201); using \"index\"");
        return float_param(index.name, index.dflt, index.slot);
    };
    auto uv_rough = [&](const MatParam& rough, float& u, float& v) {  // `uroughness` / `vroughness` fall back to `roughness` (metal.rs:69-76, uber.rs:148-155)
        const float r = float_param(rough.name, rough.dflt, rough.slot);
        const bool hu = m.params.floats.count("uroughness") || !m.params.find_one_texture("uroughness").empty();
        const bool hv = m.params.floats.count("vroughness") || !m.params.find_one_texture("vroughness").empty();
        u = hu ? float_param("uroughness", r, kFparamURoughness) : r; v = hv ? float_param("vroughness", r, kFparamVRoughness) : r;
    };
    if (!row) {
        if (error.empty()) error = "Material \"" + m.type + "\" is outside the hot-path scope (supported: matte, mirror, plastic, glass, metal, uber, substrate, translucent, mix)";
        return 0;
    }
    MatValues v{};
    v.remap = m.params.find_one_bool("remaproughness", true) ? 1 : 0;
    // every float that defines the material, in order, is the cache key
    std::vector<float> kv;
    std::array<float, 3> copper[2];
    if (row->copper) pbrt_hip_host_copper_rgb(copper[0].data(), copper[1].data());
    int nc = 0, nf = 0;
    for (const MatParam& q : row->params) switch (q.kind) {
        case kSpectrum:
            v.c[nc] = param(q.name, false, row->copper ? copper[nc] : std::array<float, 3>{q.dflt, q.dflt, q.dflt}, q.slot);
            kv.insert(kv.end(), v.c[nc].begin(), v.c[nc].end()); nc++;
            break;
        case kFloat: kv.push_back(v.f[nf++] = float_param(q.name, q.dflt, q.slot)); break;
        case kRoughnessUV: uv_rough(q, v.f[nf], v.f[nf + 1]); kv.push_back(v.f[nf]); kv.push_back(v.f[nf + 1]); nf += 2; break;
        case kIndex: kv.push_back(v.f[nf++] = eta_of(q)); break;
    }
    if (row->mix) {
        const char* pn[2] = {"namedmaterial1", "namedmaterial2"};
        for (int k = 0; k < 2; k++) {
            const std::string nm = m.params.find_one_string(pn[k], "");
            auto it = gs_.named_materials.find(nm);
            MaterialDesc md;
            if (it != gs_.named_materials.end()) md = it->second;
            else { warn("Named material '" + nm + "' undefined. Using 'matte'."); md.type = "matte"; md.params = m.params; }
            v.sub[k] = material_id_for(md);
            if (!error.empty()) return 0;
            kv.push_back((float)v.sub[k]);
        }
    }
    if (!error.empty()) return 0;
    std::string key = m.type + (v.remap ? ":r" : ":n");
    for (float x : kv) { uint32_t u; std::memcpy(&u, &x, 4); char b[12]; std::snprintf(b, sizeof b, ":%08x", u); key += b; }
    if (bump_tex >= 0) key += "|bump=" + std::to_string(bump_tex);
    for (int k = 0; k < 4; k++) if (ftex_param[k] >= 0) key += "|ftex" + std::to_string(k) + "=" + std::to_string(ftex_param[k]);
    for (int k = 0; k < 10; k++) if (tex_param[k] >= 0) key += "|tex" + std::to_string(k) + "=" + std::to_string(tex_param[k]);
    auto it = material_cache_.find(key);
    if (it != material_cache_.end()) return it->second;
    uint32_t id = 0;
    if (!check(ABI(row->make(scene_, v, &id)), "add_material")) return 0;
    // colours first, then the scalars, then the structural parameters (opacity / amount rebuild or annotate the lobe list the others have filled in)
    auto send = [&](int first, int last) {
        for (int k = first; k <= last; k++)
            if (tex_param[k] >= 0 && !check(ABI(pbrt_hip_set_material_texture(scene_, id, k, (uint32_t)tex_param[k])), "set_material_texture")) return false;
        return true;
    };
    auto send_float = [&](int first, int last) {
        for (int k = first; k <= last; k++)
            if (ftex_param[k] >= 0 && !check(ABI(pbrt_hip_set_material_float_texture(scene_, id, k, (uint32_t)ftex_param[k])), "set_material_float_texture")) return false;
        return true;
    };
    if (!send(PBRT_HIP_PARAM_KD, PBRT_HIP_PARAM_KT) || !send_float(kFparamSigma, kFparamVRoughness) || !send(PBRT_HIP_PARAM_OPACITY, PBRT_HIP_PARAM_K)) return 0;
    if (!send_float(kFparamIndex, kFparamIndex)) return 0;   // index: after opacity (an uber's is made per hit with it)
    if (!send(PBRT_HIP_PARAM_REFLECT, PBRT_HIP_PARAM_TRANSMIT)) return 0;   // translucent's reflect / transmit: after Kd / Ks and the roughness (the per-hit lobe list takes their textures over)
    if (bump_tex >= 0 && !check(ABI(pbrt_hip_set_material_bump(scene_, id, (uint32_t)bump_tex)), "set_material_bump")) return 0;
    material_cache_[key] = id;
    return id;
}

// material: shape parameters override the material's (TextureParams looks in the shape's set first, graphics_state.rs:147-165)
MaterialDesc Api::material_for_shape(const ParamSet& p) const {
    MaterialDesc eff = gs_.material;
    static const std::vector<std::string> names = parameter_names();
    for (const std::string& name : names) {
        auto f = p.floats.find(name); auto tx = p.textures.find(name);
        if (tx != p.textures.end()) { eff.params.textures[name] = tx->second; eff.params.floats.erase(name); }
        else if (f != p.floats.end()) { eff.params.floats[name] = f->second; eff.params.textures.erase(name); }
    }
    { auto b = p.bools.find("remaproughness"); if (b != p.bools.end()) eff.params.bools["remaproughness"] = b->second; }
    return eff;
}

}  // namespace pbrt_host
