// Texture directives and the table of texture names (api/src/lib.rs:586-660, api/src/graphics_state.rs:60-130): what a name stands for is asked through Api::lookup_texture /
// Api::resolve and written through Api::declare_texture, nowhere else.
#include "pbrt_host.hpp"
#include <cstdio>
#include <cstring>

namespace pbrt_host {

// What `name` stands for to a reader that wants a float (or a spectrum).  A name is a library texture, or of a class nobody evaluates, or a constant of one type or of both
// (declare_texture says how both can be); Constant's value is left alone for every other answer.
Api::TexRef Api::lookup_texture(const std::string& name, bool want_float) const {
    TexRef r;
    auto dt = gs_.device_textures.find(name);
    auto un = gs_.unsupported_textures.find(name);
    auto f = gs_.float_textures.find(name);
    auto sp = gs_.spectrum_textures.find(name);
    if (dt != gs_.device_textures.end()) { r.kind = TexRef::Device; r.is_float = dt->second.is_float; r.id = dt->second.id; }
    else if (un != gs_.unsupported_textures.end()) { r.kind = TexRef::Unsupported; r.cls = un->second; }
    else if (want_float && f != gs_.float_textures.end()) { r.kind = TexRef::Constant; r.value = {f->second, f->second, f->second}; }
    else if (!want_float && sp != gs_.spectrum_textures.end()) { r.kind = TexRef::Constant; r.value = sp->second; }
    else r.kind = (f != gs_.float_textures.end() || sp != gs_.spectrum_textures.end()) ? TexRef::WrongType : TexRef::Unknown;
    return r;
}

// Parameter `pname` of `p`, wanted as a float (three equal channels) or a spectrum: a "texture pname" reference is looked up, anything else is the literal (or `d`) as a Constant.
// `value` holds the literal whenever the texture gave no constant, for the callers that fall back to it.
Api::TexRef Api::resolve(const ParamSet& p, const std::string& pname, bool want_float, std::array<float, 3> d) const {
    TexRef r;
    if (want_float) { const float f = p.find_one_float(pname, d[0]); r.value = {f, f, f}; }
    else r.value = p.find_one_rgb(pname, d);
    r.name = p.find_one_texture(pname);
    if (r.name.empty()) return r;
    const std::array<float, 3> literal = r.value;
    const std::string name = r.name;
    r = lookup_texture(name, want_float);
    r.name = name;
    if (r.kind != TexRef::Constant) r.value = literal;
    return r;
}

// The one writer of the table: `name` now stands for `what` alone.
void Api::declare_texture(const std::string& name, TexDecl what, bool is_float, std::array<float, 3> value, uint32_t id, const std::string& cls, bool folded) {
    gs_.unsupported_textures.erase(name); gs_.device_textures.erase(name);
    // kept as it was: a "scale" / "mix" folded to a constant leaves a constant of the OTHER type under the same name in place (every other declaration forgets it)
    if (!folded) { gs_.float_textures.erase(name); gs_.spectrum_textures.erase(name); }
    switch (what) {
        case TexDecl::Nothing: break;
        case TexDecl::Constant: if (is_float) gs_.float_textures[name] = value[0]; else gs_.spectrum_textures[name] = value; break;
        case TexDecl::Device: gs_.device_textures[name] = GraphicsState::DeviceTexture{is_float, id}; break;
        case TexDecl::Unsupported: gs_.unsupported_textures[name] = cls; break;
    }
}

// An operand of a texture: a library texture of the wanted type as it is, a constant (a constant texture or the literal) to be sent as one by operand_id.  Anything else fails:
// silently, or — `owner` = the texture being declared — with the sentence the 2D and 3D procedurals give.
Api::Operand Api::operand(const ParamSet& p, const char* pname, bool want_float, float dflt, const std::string& owner) {
    const TexRef r = resolve(p, pname, want_float, {dflt, dflt, dflt});
    Operand o;
    o.value = r.value;
    if (r.kind == TexRef::Constant) o.constant = true;
    else if (r.kind == TexRef::Device && r.is_float == want_float) o.id = r.id;
    else {
        o.ok = false;
        if (!owner.empty() && error.empty()) error = "Texture \"" + owner + "\": operand '" + r.name + "' is not a texture the library evaluates";
    }
    return o;
}
uint32_t Api::operand_id(const Operand& o, bool& ok) {
    if (!o.ok) { ok = false; return 0u; }
    if (!o.constant) return o.id;
    uint32_t id = 0;
    if (!check(ABI(pbrt_hip_add_texture_constant(scene_, o.value.data(), &id)), "add_texture_constant")) ok = false;
    return id;
}

// ImageTexture::from (textures/src/imagemap.rs:117-160): the pyramid comes from the cache (MIPMapCache), the texture over it is new
bool Api::imagemap_texture(const ParamSet& p, bool is_float, const std::string& scene_dir, uint32_t& id) {
    std::string file = p.find_one_string("filename", "");
    if (file.empty()) { if (error.empty()) error = "imagemap path not specified."; return false; }
    if (file[0] != '/' && !scene_dir.empty()) file = scene_dir + "/" + file;
    const bool trilinear = p.find_one_bool("trilinear", false);
    const float max_aniso = p.find_one_float("maxanisotropy", 8.0f), scale = p.find_one_float("scale", 1.0f);
    const std::string wrap_s = p.find_one_string("wrap", "repeat");
    const int wrap = wrap_s == "black" ? 1 : (wrap_s == "clamp" ? 2 : 0);
    auto ends = [&](const char* e) { const size_t n = std::strlen(e); return file.size() >= n && file.compare(file.size() - n, n, e) == 0; };
    const bool gamma = p.find_one_bool("gamma", ends(".tga") || ends(".png"));
    char key[64];
    std::snprintf(key, sizeof key, "|%d|%d|%d|%a|%d|%a", is_float ? 1 : 0, trilinear ? 0 : 1, wrap, (double)scale, gamma ? 1 : 0, (double)max_aniso);
    const std::string ck = file + key;
    uint32_t mip = 0;
    auto it = mipmap_cache_.find(ck);
    if (it != mipmap_cache_.end()) mip = it->second;
    else {
        std::vector<float> rgb; int w = 0, h = 0; std::string err;
        if (!read_image(file, rgb, w, h, err)) { if (error.empty()) error = "Unable to load MIPMap: Error reading texture " + file + ", " + err; return false; }
        if (!check(ABI(pbrt_hip_add_mipmap(scene_, w, h, rgb.data(), is_float ? 1 : 0, scale, gamma ? 1 : 0, trilinear ? 0 : 1, wrap, max_aniso, &mip)), "add_mipmap")) return false;
        mipmap_cache_[ck] = mip;
    }
    return check(ABI(pbrt_hip_add_texture_imagemap(scene_, mip, p.find_one_float("uscale", 1.0f), p.find_one_float("vscale", 1.0f), p.find_one_float("udelta", 0.0f), p.find_one_float("vdelta", 0.0f), &id)), "add_texture_imagemap");
}

// The 2D procedural textures (textures/src/*.rs): checkerboard (dimension 2), uv, bilerp, dots
bool Api::procedural_2d_texture(const std::string& name, const std::string& tex_class, const ParamSet& p, bool is_float, uint32_t& id) {
    const float su = p.find_one_float("uscale", 1.0f), sv = p.find_one_float("vscale", 1.0f), du = p.find_one_float("udelta", 0.0f), dv = p.find_one_float("vdelta", 0.0f);
    bool ok = true;
    if (tex_class == "checkerboard") {
        const uint32_t t1 = operand_id(operand(p, "tex1", is_float, 1.0f, name), ok), t2 = operand_id(operand(p, "tex2", is_float, 0.0f, name), ok);
        std::string aa = p.find_one_string("aamode", "closedform");
        if (aa != "none" && aa != "closedform") { warn("Antialiasing mode '" + aa + "' not understood by Checkerboard2DTexture; using 'closedform'"); aa = "closedform"; }
        return ok && check(ABI(pbrt_hip_add_texture_checkerboard(scene_, t1, t2, su, sv, du, dv, aa == "none" ? 0 : 1, &id)), "add_texture_checkerboard");
    }
    if (tex_class == "dots") {
        // Quirk B13 (textures/src/dots.rs:61-66): the reference's constructor from parameters hands (inside, outside) to DotsTexture::new(outside_dot, inside_dot), so
        // a scene file's "inside" value is what shows OUTSIDE the dots and "outside" fills them — its own render of scenes/shapes/triangles-alpha-mask.pbrt (an opaque
        // cube with holes where `"float inside" 1 "float outside" 0` asks for the opposite) confirms it.  The C ABI keeps DotsTexture's meaning; the swap lives here.
        const uint32_t param_inside = operand_id(operand(p, "inside", is_float, 1.0f, name), ok), param_outside = operand_id(operand(p, "outside", is_float, 0.0f, name), ok);
        return ok && check(ABI(pbrt_hip_add_texture_dots(scene_, /*inside_dot=*/param_outside, /*outside_dot=*/param_inside, su, sv, du, dv, &id)), "add_texture_dots");
    }
    if (tex_class == "uv") return check(ABI(pbrt_hip_add_texture_uv(scene_, su, sv, du, dv, &id)), "add_texture_uv");
    auto corner = [&](const char* pn, float d) { std::array<float, 3> v = {d, d, d}; if (is_float) { const float f = p.find_one_float(pn, d); v = {f, f, f}; } else v = p.find_one_rgb(pn, v); return v; };
    const std::array<float, 3> v00 = corner("v00", 0.0f), v01 = corner("v01", 1.0f), v10 = corner("v10", 0.0f), v11 = corner("v11", 1.0f);
    return check(ABI(pbrt_hip_add_texture_bilerp(scene_, v00.data(), v01.data(), v10.data(), v11.data(), su, sv, du, dv, &id)), "add_texture_bilerp");
}

void Api::pbrt_texture(const std::string& name, const std::string& type, const std::string& tex_class, const ParamSet& p, const std::string& scene_dir) {
    if (!verify_world("Texture")) return;
    const bool is_float = type == "float", is_spec = type == "color" || type == "spectrum";
    if (!is_float && !is_spec) { warn("Texture type '" + type + "' unknown."); return; }
    const std::array<float, 3> none = {0.0f, 0.0f, 0.0f};
    if (tex_class == "scale" || tex_class == "mix") {
        const bool scale = tex_class == "scale";
        const Operand o1 = operand(p, "tex1", is_float, scale ? 1.0f : 0.0f), o2 = operand(p, "tex2", is_float, 1.0f), oa = operand(p, "amount", true, 0.5f);
        // "scale" and "mix" of constant textures are constant: fold them (textures/src/scale.rs:38-40 tex1 * tex2; mix.rs:44-49 (1 - amt) * t1 + amt * t2)
        // kept as it was: a COLOUR "scale" reads "amount" too, and is not folded when that names anything but a constant float texture
        if (o1.constant && o2.constant && (oa.constant || (scale && is_float))) {
            const float amt = oa.value[0];
            std::array<float, 3> v;
            for (int c = 0; c < 3; c++) v[c] = scale ? o1.value[c] * o2.value[c] : ((1.0f - amt) * o1.value[c] + amt * o2.value[c]);
            declare_texture(name, TexDecl::Constant, is_float, v, 0, "", /*folded=*/true);
            return;
        }
        // an operand is evaluated per hit: the whole tree goes to the library
        bool ok = true;
        const uint32_t t1 = operand_id(o1, ok), t2 = operand_id(o2, ok);
        uint32_t id = 0;
        if (ok && scale) ok = check(ABI(pbrt_hip_add_texture_scale(scene_, t1, t2, &id)), "add_texture_scale");
        else if (ok) { const uint32_t amt = operand_id(oa, ok); if (ok) ok = check(ABI(pbrt_hip_add_texture_mix(scene_, t1, t2, amt, &id)), "add_texture_mix"); }
        if (ok) declare_texture(name, TexDecl::Device, is_float, none, id);
        else declare_texture(name, TexDecl::Unsupported, is_float, none, 0, tex_class);   // reported only if something uses it
        return;
    }
    const int dimension = p.find_one_int("dimension", 2);
    const bool imagemap = tex_class == "imagemap";
    if (imagemap || (tex_class == "checkerboard" && dimension != 3) || tex_class == "uv" || tex_class == "bilerp" || tex_class == "dots") {  // textures over a TextureMapping2D
        if (imagemap) declare_texture(name, TexDecl::Nothing, is_float, none);   // kept as it was: an image map that fails has forgotten the name, a procedural that fails has not
        // get_texture_mapping (textures/src/lib.rs:44-67): "uv" travels in the texture's own parameters, the other three are attached afterwards; unknown names fall back to uv
        const std::string mp = p.find_one_string("mapping", "uv");
        if (mp != "uv" && mp != "spherical" && mp != "cylindrical" && mp != "planar") warn("Error 2D texture mapping '" + mp + "' unknown");
        if (tex_class == "checkerboard" && dimension != 2) {
            if (error.empty()) error = "Texture \"" + name + "\": " + std::to_string(dimension) + " dimensional checkerboard texture not supported";
            return;
        }
        if (tex_class == "uv" && is_float) { warn("Unable to create float texture 'uv'."); return; }   // textures/src/lib.rs: only a spectrum variant exists
        uint32_t id = 0;
        bool ok = imagemap ? imagemap_texture(p, is_float, scene_dir, id) : procedural_2d_texture(name, tex_class, p, is_float, id);
        if (ok && mp == "planar") {
            float prm[8] = {1, 0, 0, 0, 1, 0, p.find_one_float("udelta", 0.0f), p.find_one_float("vdelta", 0.0f)};
            if (const std::vector<float>* v = p.find_floats("v1")) if (v->size() >= 3) for (int k = 0; k < 3; k++) prm[k] = (*v)[(size_t)k];
            if (const std::vector<float>* v = p.find_floats("v2")) if (v->size() >= 3) for (int k = 0; k < 3; k++) prm[3 + k] = (*v)[(size_t)k];
            ok = check(ABI(pbrt_hip_set_texture_mapping(scene_, id, 3, prm)), "set_texture_mapping");
        } else if (ok && (mp == "spherical" || mp == "cylindrical"))
            ok = check(ABI(pbrt_hip_set_texture_mapping(scene_, id, mp == "spherical" ? 1 : 2, ctm_.mi)), "set_texture_mapping");  // tex2world.inverse()
        if (ok) declare_texture(name, TexDecl::Device, is_float, none, id);
        return;
    }
    if (tex_class == "fbm" || tex_class == "wrinkled" || tex_class == "windy" || tex_class == "marble" || tex_class == "checkerboard") {  // 3D procedural textures over IdentityMapping3D
        // the reference builds IdentityMapping3D from tex2world = the CTM at the Texture directive (textures/src/fbm.rs:63-65) and applies it as is
        if (tex_class == "marble" && is_float) { warn("Unable to create float texture 'marble'."); return; }
        const float omega = p.find_one_float("roughness", 0.5f); const int octaves = p.find_one_int("octaves", 8);
        uint32_t id = 0; bool ok = true;
        if (tex_class == "fbm") ok = check(ABI(pbrt_hip_add_texture_fbm(scene_, ctm_.m, omega, octaves, &id)), "add_texture_fbm");
        else if (tex_class == "wrinkled") ok = check(ABI(pbrt_hip_add_texture_wrinkled(scene_, ctm_.m, omega, octaves, &id)), "add_texture_wrinkled");
        else if (tex_class == "windy") ok = check(ABI(pbrt_hip_add_texture_windy(scene_, ctm_.m, &id)), "add_texture_windy");
        else if (tex_class == "marble") ok = check(ABI(pbrt_hip_add_texture_marble(scene_, ctm_.m, omega, octaves, p.find_one_float("scale", 1.0f), p.find_one_float("variation", 0.2f), &id)), "add_texture_marble");
        else {
            const uint32_t t1 = operand_id(operand(p, "tex1", is_float, 1.0f, name), ok), t2 = operand_id(operand(p, "tex2", is_float, 0.0f, name), ok);
            if (ok) ok = check(ABI(pbrt_hip_add_texture_checkerboard3d(scene_, t1, t2, ctm_.m, &id)), "add_texture_checkerboard3d");
        }
        if (ok) declare_texture(name, TexDecl::Device, is_float, none, id);
        return;
    }
    if (tex_class != "constant") { declare_texture(name, TexDecl::Unsupported, is_float, none, 0, tex_class); return; }  // ptex: not evaluated by the library
    const float f = p.find_one_float("value", 1.0f);
    declare_texture(name, TexDecl::Constant, is_float, is_float ? std::array<float, 3>{f, f, f} : p.find_one_rgb("value", {1.0f, 1.0f, 1.0f}));
}

}  // namespace pbrt_host
