// Host-side scene API over the C ABI.  See pbrt_host.hpp for scope; reference: api/src/lib.rs, api/src/graphics_state.rs.
#include "pbrt_host.hpp"
#include "../csrc/curve_host.h"
#include "../csrc/loopsubdiv_host.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>

namespace pbrt_host {

// ------------------------------------------------------------------------------------------------ ParamSet
float ParamSet::find_one_float(const std::string& n, float d) const {
    auto it = floats.find(n);
    return (it != floats.end() && it->second.size() == 1) ? it->second[0] : d;  // paramset: one-value lookups need exactly one
}
int ParamSet::find_one_int(const std::string& n, int d) const {
    auto it = ints.find(n);
    return (it != ints.end() && it->second.size() == 1) ? it->second[0] : d;
}
bool ParamSet::find_one_bool(const std::string& n, bool d) const {
    auto it = bools.find(n);
    return (it != bools.end() && it->second.size() == 1) ? it->second[0] : d;
}
std::string ParamSet::find_one_string(const std::string& n, const std::string& d) const {
    auto it = strings.find(n);
    return (it != strings.end() && it->second.size() == 1) ? it->second[0] : d;
}
std::string ParamSet::find_one_texture(const std::string& n) const {
    auto it = textures.find(n);
    return (it != textures.end() && it->second.size() == 1) ? it->second[0] : std::string();
}
const std::vector<float>* ParamSet::find_floats(const std::string& n) const {
    auto it = floats.find(n);
    return it == floats.end() ? nullptr : &it->second;
}
const std::vector<int>* ParamSet::find_ints(const std::string& n) const {
    auto it = ints.find(n);
    return it == ints.end() ? nullptr : &it->second;
}
std::array<float, 3> ParamSet::find_one_rgb(const std::string& n, std::array<float, 3> d) const {
    auto it = floats.find(n);
    if (it == floats.end() || it->second.size() != 3) return d;
    return {it->second[0], it->second[1], it->second[2]};
}

// ------------------------------------------------------------------------------------------------ Api
static Xform identity_xform() {
    Xform x{};
    for (int i = 0; i < 4; i++) x.m[i * 5] = x.mi[i * 5] = 1.0f;
    return x;
}

Api::Api(int device) : check_only_(device < 0), ctm_(identity_xform()), camera_to_world_(identity_xform()) {
    if (check_only_) return;
    scene_ = pbrt_hip_scene_create(device);
    if (!scene_) {
        const char* e = pbrt_hip_last_error(nullptr);
        error = std::string("no usable gfx950 device: ") + (e ? e : "");
    }
}
Api::Api(const std::vector<int>& devices) : check_only_(false), ctm_(identity_xform()), camera_to_world_(identity_xform()) {
    scene_ = pbrt_hip_scene_create_multi(devices.empty() ? nullptr : devices.data(), (int)devices.size());
    if (scene_) n_devices_ = pbrt_hip_scene_devices(scene_, nullptr, 0);
    if (!scene_) {
        const char* e = pbrt_hip_last_error(nullptr);
        error = std::string("no usable gfx950 device: ") + (e ? e : "");
    }
}
Api::~Api() {
    if (scene_) pbrt_hip_scene_destroy(scene_);
}

void Api::warn(const std::string& w) {
    warnings.push_back(w);
    if (!quiet) std::fprintf(stderr, "Warning: %s\n", w.c_str());
}
bool Api::check(int rc, const char* what) {
    if (rc == PBRT_HIP_OK) return true;
    if (error.empty()) {
        const char* e = scene_ ? pbrt_hip_last_error(scene_) : nullptr;
        error = std::string(what) + " failed (" + std::to_string(rc) + "): " + (e ? e : "");
    }
    return false;
}
// `ctm = ctm * t` for every active transform (api/src/lib.rs:140-152); the time-1 copy is dead on this path.
void Api::concat(const Xform& t) {
    Xform r;
    pbrt_hip_host_compose(ctm_.m, ctm_.mi, t.m, t.mi, r.m, r.mi);
    ctm_ = r;
}

void Api::pbrt_identity() { ctm_ = identity_xform(); }
void Api::pbrt_translate(float dx, float dy, float dz) {
    Xform t; const float d[3] = {dx, dy, dz};
    pbrt_hip_host_translate(d, t.m, t.mi);
    concat(t);
}
void Api::pbrt_rotate(float angle, float dx, float dy, float dz) {
    Xform t; const float a[3] = {dx, dy, dz};
    pbrt_hip_host_rotate(angle, a, t.m, t.mi);
    concat(t);
}
void Api::pbrt_scale(float sx, float sy, float sz) {
    Xform t; const float s[3] = {sx, sy, sz};
    pbrt_hip_host_scale(s, t.m, t.mi);
    concat(t);
}
void Api::pbrt_look_at(float ex, float ey, float ez, float lx, float ly, float lz, float ux, float uy, float uz) {
    Xform t; const float e[3] = {ex, ey, ez}, l[3] = {lx, ly, lz}, u[3] = {ux, uy, uz};
    if (pbrt_hip_host_look_at(e, l, u, t.m, t.mi) != 0) {
        // transform.rs:173-181: "up" and the viewing direction are collinear -> identity with an error message
        warn("LookAt: up vector and viewing direction are pointing in the same direction; using the identity transformation");
        t = identity_xform();
    }
    concat(t);
}
// The file format hands matrices over column-major; Matrix4x4::new takes rows (api/src/lib.rs:208-262).
static Xform from_column_major(const float tr[16]) {
    Xform t;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) t.m[r * 4 + c] = tr[c * 4 + r];
    pbrt_hip_host_invert(t.m, t.mi);
    return t;
}
void Api::pbrt_concat_transform(const float tr[16]) { concat(from_column_major(tr)); }
void Api::pbrt_transform(const float tr[16]) { ctm_ = from_column_major(tr); }
void Api::pbrt_coordinate_system(const std::string& name) { named_cs_[name] = ctm_; }
void Api::pbrt_coord_sys_transform(const std::string& name) {
    auto it = named_cs_.find(name);
    if (it != named_cs_.end()) ctm_ = it->second;
    else warn("Couldn't find named coordinate system '" + name + "'");
}

// verify_options / verify_world (api/src/lib.rs:1003-1050): a directive in the wrong block is reported and ignored.
bool Api::verify_options(const char* func) {
    if (!world_block_) return true;
    warn(std::string("Options cannot be set inside world block; '") + func + "' not allowed. Ignoring.");
    return false;
}
bool Api::verify_world(const char* func) {
    if (world_block_) return true;
    warn(std::string("Scene description must be inside world block; '") + func + "' not allowed. Ignoring.");
    return false;
}

void Api::pbrt_pixel_filter(const std::string& name, const ParamSet& p) { if (verify_options("PixelFilter")) { filter_name_ = name; filter_p_ = p; } }
void Api::pbrt_film(const std::string& type, const ParamSet& p) { if (verify_options("Film")) { film_name_ = type; film_p_ = p; } }
void Api::pbrt_sampler(const std::string& name, const ParamSet& p) { if (verify_options("Sampler")) { sampler_name_ = name; sampler_p_ = p; } }
void Api::pbrt_accelerator(const std::string& name, const ParamSet& p) { if (verify_options("Accelerator")) { accel_name_ = name; accel_p_ = p; } }
void Api::pbrt_integrator(const std::string& name, const ParamSet& p) { if (verify_options("Integrator")) { integrator_name_ = name; integrator_p_ = p; } }
void Api::pbrt_camera(const std::string& name, const ParamSet& p) {
    if (!verify_options("Camera")) return;
    camera_name_ = name; camera_p_ = p;
    // camera_to_world = inverse(ctm): swap m and m_inv (api/src/lib.rs:376-392)
    std::memcpy(camera_to_world_.m, ctm_.mi, sizeof ctm_.mi);
    std::memcpy(camera_to_world_.mi, ctm_.m, sizeof ctm_.m);
    named_cs_["camera"] = camera_to_world_;
}

void Api::pbrt_world_begin() {
    if (!verify_options("WorldBegin")) return;
    world_block_ = true;
    ctm_ = identity_xform();
    named_cs_["world"] = ctm_;
}
void Api::pbrt_attribute_begin() { if (!verify_world("AttributeBegin")) return; gs_stack_.push_back(gs_); ctm_stack_.push_back(ctm_); }
void Api::pbrt_attribute_end() {
    if (!verify_world("AttributeEnd")) return;
    if (gs_stack_.empty()) { warn("Unmatched AttributeEnd encountered. Ignoring it."); return; }
    gs_ = gs_stack_.back(); gs_stack_.pop_back();
    ctm_ = ctm_stack_.back(); ctm_stack_.pop_back();
}
void Api::pbrt_transform_begin() { if (!verify_world("TransformBegin")) return; ctm_stack_.push_back(ctm_); }
void Api::pbrt_transform_end() {
    if (!verify_world("TransformEnd")) return;
    if (ctm_stack_.size() <= gs_stack_.size()) { warn("Unmatched TransformEnd encountered. Ignoring it."); return; }
    ctm_ = ctm_stack_.back(); ctm_stack_.pop_back();
}

// pbrt_texture and the table of texture names: textures.cpp
void Api::pbrt_material(const std::string& name, const ParamSet& p) { if (!verify_world("Material")) return; gs_.material.type = name; gs_.material.params = p; }
void Api::pbrt_make_named_material(const std::string& name, const ParamSet& p) {
    if (!verify_world("MakeNamedMaterial")) return;
    MaterialDesc m; m.type = p.find_one_string("type", ""); m.params = p;
    if (m.type.empty()) { warn("No parameter string \"type\" found in MakeNamedMaterial"); return; }
    gs_.named_materials[name] = m;
}
void Api::pbrt_named_material(const std::string& name) {
    if (!verify_world("NamedMaterial")) return;
    auto it = gs_.named_materials.find(name);
    if (it == gs_.named_materials.end()) { warn("NamedMaterial \"" + name + "\" unknown."); return; }
    gs_.material = it->second;
}
// ObjectBegin / ObjectEnd / ObjectInstance (api/src/lib.rs:911-1000)
void Api::pbrt_object_begin(const std::string& name) {
    if (!verify_world("ObjectBegin")) return;
    pbrt_attribute_begin();
    if (!current_object_.empty()) { warn("ObjectBegin called inside of an instance definition."); return; }
    uint32_t id = (uint32_t)objects_.size();
    if (!check(ABI(pbrt_hip_object_begin(scene_, &id)), "object_begin")) return;
    objects_[name] = id; object_tris_[name] = 0;
    current_object_ = name;
}
void Api::pbrt_object_end() {
    if (!verify_world("ObjectEnd")) return;
    if (current_object_.empty()) warn("ObjectEnd called outside of instance definition.");
    else { check(ABI(pbrt_hip_object_end(scene_)), "object_end"); current_object_.clear(); }
    pbrt_attribute_end();
}
void Api::pbrt_object_instance(const std::string& name) {
    if (!verify_world("ObjectInstance") || !error.empty()) return;
    if (!current_object_.empty()) { warn("ObjectInstance can't be called inside of instance definition."); return; }
    auto it = objects_.find(name);
    if (it == objects_.end()) { warn("Unable to find object instance named '" + name + "'"); return; }
    if (object_tris_[name] == 0) return;  // empty object: nothing is added (lib.rs:949-951)
    if (!check(ABI(pbrt_hip_add_instance(scene_, it->second, ctm_.m, ctm_.mi)), "add_instance")) return;
    n_instances_++; n_tris_ += object_tris_[name];
}
void Api::pbrt_reverse_orientation() { if (!verify_world("ReverseOrientation")) return; gs_.reverse_orientation = !gs_.reverse_orientation; }

static std::array<float, 3> mul3(std::array<float, 3> a, std::array<float, 3> b) { return {a[0] * b[0], a[1] * b[1], a[2] * b[2]}; }

void Api::pbrt_light_source(const std::string& name, const ParamSet& p, const std::string& scene_dir) {
    if (!verify_world("LightSource") || !error.empty() || (!scene_ && !check_only_)) return;
    for (auto& u : p.unsupported) { error = "LightSource \"" + name + "\": parameter '" + u + "' has a spectral type this host cannot evaluate"; return; }
    const std::array<float, 3> one = {1.0f, 1.0f, 1.0f};
    const std::array<float, 3> sc = p.find_one_rgb("scale", one);
    if (name == "infinite" || name == "exinfinite") {
        auto L = mul3(p.find_one_rgb("L", one), sc);
        std::string map = p.find_one_string("mapname", "");
        std::vector<float> rgb; int w = 0, h = 0;
        if (!map.empty()) {  // InfiniteAreaLight::new: a map that cannot be read leaves a constant light, with a warning (infinite.rs:63-77)
            if (map[0] != '/' && !scene_dir.empty()) map = scene_dir + "/" + map;
            std::string err;
            if (!read_image(map, rgb, w, h, err)) {
                rgb.clear();
                // a file the reference could read but this host cannot decode must not silently become a constant sky
                if (err.find("not decoded by this host") != std::string::npos) { if (error.empty()) error = "LightSource \"infinite\" 'mapname' " + map + ": " + err; return; }
                warn("Problem reading file '" + map + "'. " + err);
            }
        }
        if (!rgb.empty()) { if (check(ABI(pbrt_hip_add_light_infinite_map(scene_, L.data(), w, h, rgb.data(), ctm_.m, ctm_.mi)), "add_light_infinite_map")) n_lights_++; }
        else if (check(ABI(pbrt_hip_add_light_infinite(scene_, L.data(), ctm_.m, ctm_.mi)), "add_light_infinite")) n_lights_++;
    } else if (name == "distant") {
        auto L = mul3(p.find_one_rgb("L", one), sc);
        auto from = p.find_one_rgb("from", {0.0f, 0.0f, 0.0f}), to = p.find_one_rgb("to", {0.0f, 0.0f, 1.0f});
        float w[3];
        pbrt_hip_host_distant_direction(ctm_.m, from.data(), to.data(), w);
        if (check(ABI(pbrt_hip_add_light_distant(scene_, L.data(), w)), "add_light_distant")) n_lights_++;
    } else if (name == "point") {
        auto I = mul3(p.find_one_rgb("I", one), sc);
        auto from = p.find_one_rgb("from", {0.0f, 0.0f, 0.0f});
        float pw[3];
        pbrt_hip_host_point_position(ctm_.m, ctm_.mi, from.data(), pw);
        if (check(ABI(pbrt_hip_add_light_point(scene_, I.data(), pw)), "add_light_point")) n_lights_++;
    } else if (name == "spot") {
        auto I = mul3(p.find_one_rgb("I", one), sc);
        auto from = p.find_one_rgb("from", {0.0f, 0.0f, 0.0f}), to = p.find_one_rgb("to", {0.0f, 0.0f, 1.0f});
        float l2w[16], w2l[16], cs[2];
        pbrt_hip_host_spot(ctm_.m, ctm_.mi, from.data(), to.data(), p.find_one_float("coneangle", 30.0f), p.find_one_float("conedeltaangle", 5.0f), l2w, w2l, cs);
        if (check(ABI(pbrt_hip_add_light_spot(scene_, I.data(), l2w, w2l, cs[0], cs[1])), "add_light_spot")) n_lights_++;
    } else if (name == "projection" || name == "goniometric") {   // projection.rs:275-296, goniometric.rs:220-237: light_to_world = the CTM
        auto I = mul3(p.find_one_rgb("I", one), sc);
        std::string map = p.find_one_string("mapname", "");
        std::vector<float> rgb; int w = 0, h = 0;
        if (map.empty()) warn(name == "projection" ? "No projection image texture provided." : "No goniophotometric image texture provided.");
        else {   // an image that cannot be read leaves the light without one, with a warning (projection.rs:83-86, goniometric.rs:60-63)
            if (map[0] != '/' && !scene_dir.empty()) map = scene_dir + "/" + map;
            std::string err;
            if (!read_image(map, rgb, w, h, err)) {
                rgb.clear();
                if (err.find("not decoded by this host") != std::string::npos) { if (error.empty()) error = "LightSource \"" + name + "\" 'mapname' " + map + ": " + err; return; }
                warn("Problem reading file '" + map + "'. " + err);
            }
        }
        const float* img = rgb.empty() ? nullptr : rgb.data();
        if (name == "projection") { if (check(ABI(pbrt_hip_add_light_projection(scene_, I.data(), ctm_.m, ctm_.mi, p.find_one_float("fov", 45.0f), w, h, img)), "add_light_projection")) n_lights_++; }
        else if (check(ABI(pbrt_hip_add_light_goniometric(scene_, I.data(), ctm_.m, ctm_.mi, w, h, img)), "add_light_goniometric")) n_lights_++;
    } else {
        error = "LightSource \"" + name + "\" is outside the hot-path scope (supported: infinite, distant, point, spot, projection, goniometric and diffuse area lights)";
    }
}
void Api::pbrt_area_light_source(const std::string& name, const ParamSet& p) { if (!verify_world("AreaLightSource")) return; gs_.area_light = name; gs_.area_light_params = p; }

// material_id_for, material_for_shape: materials.cpp

static bool is_quadric_shape(const std::string& name) {
    return name == "sphere" || name == "cylinder" || name == "cone" || name == "paraboloid" || name == "disk" || name == "hyperboloid";
}

// The six quadric shapes (Api::quadrics): parameters and defaults as each shape's From<(&ParamSet, ..)> reads them; object_to_world is the CTM with the inverse it accumulated
// (api/src/lib.rs:760-773), flags bit 0 the graphics state's reverse orientation (the library takes swaps_handedness from the matrix).
void Api::quadric_shape(const std::string& name, const ParamSet& p) {
    // what the library refuses is refused here as well: check mode calls nothing in it
    if (!current_object_.empty()) { error = "Shape \"" + name + "\" between ObjectBegin and ObjectEnd: quadric shapes inside object definitions are not supported"; return; }
    const bool light = !gs_.area_light.empty();
    if (light) {
        if (gs_.area_light != "diffuse" && gs_.area_light != "area") { error = "AreaLightSource \"" + gs_.area_light + "\" unknown"; return; }
        const bool sampled = name == "disk" || name == "cylinder";   // the reference's other three quadrics have no Shape::sample
        if (quadric_lights && name != "sphere" && !sampled) {
            error = "AreaLightSource \"" + gs_.area_light + "\" on Shape \"" + name + "\": the reference's Shape::sample for this shape is missing (todo!()); only the sphere, the disk and the cylinder can be area lights";
            return;
        }
        if (name != "sphere" && !(quadric_lights && sampled)) { error = "AreaLightSource \"" + gs_.area_light + "\" on Shape \"" + name + "\": of the quadric shapes only the sphere can be an area light"; return; }
        for (auto& u : gs_.area_light_params.unsupported) { error = "AreaLightSource: parameter '" + u + "' has a spectral type this host cannot evaluate"; return; }
    }
    for (const char* an : {"alpha", "shadowalpha"})   // only the triangle mesh reads them (triangle.rs:278-312)
        if (p.floats.count(an) || p.textures.count(an)) warn("Shape \"" + name + "\": the reference's quadric shapes read no '" + an + "'; ignoring it");
    const uint32_t mat = material_id_for(material_for_shape(p));
    if (!error.empty()) return;
    const uint32_t flags = gs_.reverse_orientation ? 1u : 0u;
    const float phi_max = p.find_one_float("phimax", 360.0f);
    if (name == "sphere") {  // shapes/src/sphere.rs:494-520
        const float radius = p.find_one_float("radius", 1.0f);
        const float z_min = p.find_one_float("zmin", -radius), z_max = p.find_one_float("zmax", radius);
        if (light) {  // one DiffuseAreaLight around the shape, numbered where the Shape directive stands (lib.rs:783-812; lights/src/diffuse.rs:230-250)
            const ParamSet& ap = gs_.area_light_params;
            auto L = mul3(ap.find_one_rgb("L", {1.0f, 1.0f, 1.0f}), ap.find_one_rgb("scale", {1.0f, 1.0f, 1.0f}));
            if (!check(ABI(pbrt_hip_add_sphere_light(scene_, ctm_.m, ctm_.mi, radius, z_min, z_max, phi_max, mat, flags, L.data(), ap.find_one_bool("twosided", false) ? 1 : 0)), "add_sphere_light")) return;
            n_lights_++; sphere_light_ = true;
        } else if (!check(ABI(pbrt_hip_add_sphere(scene_, ctm_.m, ctm_.mi, radius, z_min, z_max, phi_max, mat, flags)), "add_sphere")) return;
    } else if (name == "hyperboloid") {  // hyperboloid.rs:425-447: the defaults are the file's own, not pbrt's (0 0 0) and (1 1 1)
        const std::array<float, 3> p1 = p.find_one_rgb("p1", {3.0f, 1.2f, 1.0f}), p2 = p.find_one_rgb("p2", {1.0f, -0.5f, -1.0f});
        if (!check(ABI(pbrt_hip_add_hyperboloid(scene_, ctm_.m, ctm_.mi, p1.data(), p2.data(), phi_max, mat, flags)), "add_hyperboloid")) return;
    } else {
        const float radius = p.find_one_float("radius", 1.0f);
        int kind; float a, b;
        if (name == "cylinder") { kind = 0; a = p.find_one_float("zmin", -1.0f); b = p.find_one_float("zmax", 1.0f); }        // cylinder.rs:351-375
        else if (name == "cone") { kind = 1; a = p.find_one_float("height", 1.0f); b = 0.0f; }                                // cone.rs:321-343
        else if (name == "paraboloid") { kind = 2; a = p.find_one_float("zmin", 0.0f); b = p.find_one_float("zmax", 1.0f); }  // paraboloid.rs:337-361
        else { kind = 3; a = p.find_one_float("height", 0.0f); b = p.find_one_float("innerradius", 0.0f); }                   // disk.rs:237-261
        if (light) {  // as for the sphere above: one DiffuseAreaLight around the shape, numbered where the Shape directive stands
            const ParamSet& ap = gs_.area_light_params;
            auto L = mul3(ap.find_one_rgb("L", {1.0f, 1.0f, 1.0f}), ap.find_one_rgb("scale", {1.0f, 1.0f, 1.0f}));
            if (!check(ABI(pbrt_hip_add_quadric_light(scene_, kind, ctm_.m, ctm_.mi, radius, a, b, phi_max, mat, flags, L.data(), ap.find_one_bool("twosided", false) ? 1 : 0)), "add_quadric_light")) return;
            n_lights_++;
        } else if (!check(ABI(pbrt_hip_add_quadric(scene_, kind, ctm_.m, ctm_.mi, radius, a, b, phi_max, mat, flags)), "add_quadric")) return;
    }
    n_quadrics_++;
}

// Shape "curve" (Api::curves): Curve::from_props (shapes/src/curve.rs:149-316).  The parameters, defaults and warnings are the reference's; where it panics — a bad degree or
// basis, a wrong number of control points or normals, a ribbon without N — the parse stops with one sentence.  The conversion to cubic Bezier segments (degree elevation,
// b-spline blossoming, per-segment widths) is csrc/curve_host.h; each Bezier segment becomes one pbrt_hip_add_curve, i.e. 2^splitdepth Curve segments.
void Api::curve_shape(const ParamSet& p) {
    // what the library refuses is refused here as well: check mode calls nothing in it
    if (!current_object_.empty()) { error = "Shape \"curve\" between ObjectBegin and ObjectEnd: curves inside object definitions are not supported"; return; }
    if (!gs_.area_light.empty()) { error = "AreaLightSource \"" + gs_.area_light + "\" on Shape \"curve\": a curve cannot be an area light (the reference's Curve::sample is todo!())"; return; }
    for (const char* an : {"alpha", "shadowalpha"})   // only the triangle mesh reads them (triangle.rs:278-312)
        if (p.floats.count(an) || p.textures.count(an)) warn(std::string("Shape \"curve\": the reference's curves read no '") + an + "'; ignoring it");
    const float width = p.find_one_float("width", 1.0f);
    const float width0 = p.find_one_float("width0", width), width1 = p.find_one_float("width1", width);
    const int degree = p.find_one_int("degree", 3);
    const std::string basis = p.find_one_string("basis", "bezier");
    if (degree != 2 && degree != 3) { error = "Shape \"curve\": Invalid degree " + std::to_string(degree) + ": only degree 2 and 3 curves are supported."; return; }
    if (basis != "bezier" && basis != "bspline") { error = "Shape \"curve\": Invalid basis '" + basis + "': only 'bezier' and 'bspline' are supported."; return; }
    static const std::vector<float> none;
    const std::vector<float>* pp = p.find_floats("P");
    const std::vector<float>& P = pp ? *pp : none;
    std::vector<pcurve::PropSegment> segs;
    const std::string bad = pcurve::from_props_segments(degree, basis == "bspline", P.data(), P.size() / 3, width0, width1, segs);
    if (!bad.empty()) { error = "Shape \"curve\": " + bad; return; }
    const std::string type_name = p.find_one_string("type", "flat");
    int type = PH_CURVE_CYLINDER;
    if (type_name == "flat") type = PH_CURVE_FLAT;
    else if (type_name == "ribbon") type = PH_CURVE_RIBBON;
    else if (type_name != "cylinder") warn("Unknown curve type '" + type_name + "'.  Using 'cylinder'.");
    const std::vector<float>* np_ = p.find_floats("N");
    std::vector<float> N = np_ ? *np_ : none;
    if (!N.empty()) {
        if (type != PH_CURVE_RIBBON) { warn("Curve normals are only used with 'ribbon' type curves."); N.clear(); }
        else if (N.size() / 3 != segs.size() + 1) {
            error = "Shape \"curve\": Invalid number of normals " + std::to_string(N.size() / 3) + ": must provide " + std::to_string(segs.size() + 1) + " normals for ribbon curves with " +
                    std::to_string(segs.size()) + " segments.";
            return;
        }
    } else if (type == PH_CURVE_RIBBON) { error = "Shape \"curve\": Must provide normals 'N' at curve endpoints with ribbon curves."; return; }
    // `splitdepth` read as a float (truncated), then as an int with that as its default (:228-229)
    const int sd = p.find_one_int("splitdepth", (int)p.find_one_float("splitdepth", 3.0f));
    if (sd < 0 || sd > 16) { error = "Shape \"curve\": splitdepth " + std::to_string(sd) + " is outside [0, 16]"; return; }
    const uint32_t mat = material_id_for(material_for_shape(p));
    if (!error.empty()) return;
    const uint32_t flags = gs_.reverse_orientation ? 1u : 0u;
    for (size_t k = 0; k < segs.size(); k++) {
        if (!check(ABI(pbrt_hip_add_curve(scene_, ctm_.m, ctm_.mi, type, segs[k].cp, segs[k].width, N.empty() ? nullptr : N.data() + 3 * k, sd, mat, flags)), "add_curve")) return;
        n_curves_ += 1ull << sd;
    }
}

// Shape "loopsubdiv" (Api::loopsubdiv): LoopSubDiv::from_props (shapes/src/loopsubdiv.rs:668-689) — "nlevels" (default 3), "indices", "P".  Its two panics, and every mesh the
// library refuses (csrc/loopsubdiv_host.h: check mode calls nothing in the library, so the same header runs here), stop the parse with one sentence.  The surface becomes
// F 4^nlevels triangles through pbrt_hip_add_loopsubdiv: to everything after this function it is a trianglemesh — area lights one per output triangle, object definitions,
// reverse orientation, material parameters on the shape.  TriangleMesh::create is called without alpha textures (:645-658): "alpha" / "shadowalpha" are not read.
void Api::loopsubdiv_shape(const ParamSet& p) {
    const std::string me = "Shape \"loopsubdiv\": ";
    for (const char* an : {"alpha", "shadowalpha"})
        if (p.floats.count(an) || p.textures.count(an)) warn(me + "the reference's loopsubdiv reads no '" + an + "'; ignoring it");
    const int n_levels = p.find_one_int("nlevels", 3);
    const std::vector<int>* vi = p.find_ints("indices");
    const std::vector<float>* pp = p.find_floats("P");
    if (!vi || vi->empty()) { error = me + "Vertex indices 'indices' not provided for LoopSubDiv shape."; return; }
    if (!pp || pp->size() < 3) { error = me + "Vertex positions 'P' not provided for LoopSubDiv shape."; return; }
    const size_t nv = pp->size() / 3;
    for (int v : *vi)
        if (v < 0) { error = me + "Vertex index " + std::to_string(v) + " is out of bounds (" + std::to_string(nv) + " vertices)."; return; }
    if (vi->size() % 3) warn(me + std::to_string(vi->size()) + " indices are no multiple of 3; the last " + std::to_string(vi->size() % 3) + " are dropped");
    const std::vector<uint32_t> idx(vi->begin(), vi->end());
    ploop::Control c;
    const std::string bad = ploop::build_control(pp->data(), nv, idx.data(), idx.size(), n_levels, c);
    if (!bad.empty()) { error = me + bad; return; }
    const uint32_t mat = material_id_for(material_for_shape(p));
    if (!error.empty()) return;
    const uint32_t n_tris = (uint32_t)c.out_faces;
    const uint32_t flags = (gs_.reverse_orientation ? 1u : 0u) | (pbrt_hip_host_swaps_handedness(ctm_.m) ? 2u : 0u);
    int32_t first_light = -1;
    const bool in_object = !current_object_.empty();
    if (!gs_.area_light.empty()) {  // one DiffuseAreaLight per OUTPUT triangle, numbered where the Shape directive stands (lib.rs:783-812)
        if (gs_.area_light != "diffuse" && gs_.area_light != "area") { error = "AreaLightSource \"" + gs_.area_light + "\" unknown"; return; }
        const ParamSet& ap = gs_.area_light_params;
        for (auto& u : ap.unsupported) { error = "AreaLightSource: parameter '" + u + "' has a spectral type this host cannot evaluate"; return; }
        auto L = mul3(ap.find_one_rgb("L", {1.0f, 1.0f, 1.0f}), ap.find_one_rgb("scale", {1.0f, 1.0f, 1.0f}));
        uint32_t id = 0;
        if (!check(ABI(pbrt_hip_add_light_diffuse_area(scene_, L.data(), ap.find_one_bool("twosided", false) ? 1 : 0, n_tris, &id)), "add_light_diffuse_area")) return;
        first_light = (int32_t)id;
        if (in_object) warn("Area lights not supported with object instancing.");
        else n_lights_ += n_tris;
    }
    if (!check(ABI(pbrt_hip_add_loopsubdiv(scene_, ctm_.m, ctm_.mi, pp->data(), (uint32_t)nv, idx.data(), (uint32_t)idx.size(), n_levels, mat, first_light, flags, 1.0f, 1.0f)), "add_loopsubdiv")) return;
    if (!in_object) n_tris_ += n_tris; else object_tris_[current_object_] += n_tris;
}

void Api::pbrt_shape(const std::string& name, const ParamSet& p, const std::string& scene_dir) {
    if (!verify_world("Shape") || !error.empty() || (!scene_ && !check_only_)) return;
    if (quadrics && is_quadric_shape(name)) { quadric_shape(name, p); return; }
    if (curves && name == "curve") { curve_shape(p); return; }
    if (loopsubdiv && name == "loopsubdiv") { loopsubdiv_shape(p); return; }
    std::vector<float> P, N, S, UV;
    std::vector<uint32_t> idx;
    if (name == "trianglemesh") {  // shapes/src/triangle.rs:184-330
        const std::vector<int>* vi = p.find_ints("indices");
        const std::vector<float>* pp = p.find_floats("P");
        if (!vi || vi->empty()) { warn("Vertex indices 'indices' not provided with triangle mesh shape"); return; }
        if (!pp || pp->empty()) { warn("Vertex positions 'P' not provided with triangle mesh shape"); return; }
        const size_t npi = pp->size() / 3;
        P.assign(pp->begin(), pp->begin() + npi * 3);
        const std::vector<float>* uv = p.find_floats("uv");
        if (!uv || uv->empty()) uv = p.find_floats("st");
        if (uv && !uv->empty()) {
            const size_t nuv = uv->size() / 2;
            if (nuv < npi) warn("Not enough of 'uv' for triangle mesh. Discarding.");
            else { if (nuv > npi) warn("More 'uv' provided than will be used for triangle mesh."); UV.assign(uv->begin(), uv->begin() + npi * 2); }
        }
        if (const std::vector<float>* s = p.find_floats("S")) {
            if (s->size() / 3 != npi) warn("Number of 'S' for triangle mesh must match 'P'."); else S = *s;
        }
        if (const std::vector<float>* n = p.find_floats("N")) {
            if (n->size() / 3 != npi) warn("Number of 'N' for triangle mesh must match 'P'."); else N = *n;
        }
        for (int v : *vi)
            if (v < 0 || (size_t)v >= npi) { warn("trianglemesh has out-of-bounds vertex index " + std::to_string(v)); return; }
        idx.assign(vi->begin(), vi->end());
        idx.resize(idx.size() / 3 * 3);
    } else if (name == "plymesh") {  // shapes/src/plymesh.rs:21-141
        std::string fn = p.find_one_string("filename", "");
        if (fn.empty()) { error = "plymesh: no 'filename' parameter"; return; }
        if (fn[0] != '/' && !scene_dir.empty()) fn = scene_dir + "/" + fn;
        PlyMesh mesh; std::string err;
        if (!read_ply(fn, mesh, err)) { error = "Unable to parse PLY file '" + fn + "'. " + err; return; }
        if (mesh.P.empty() || mesh.indices.empty()) { warn("PLY file '" + fn + "' is invalid! No face/vertex elements found!"); return; }
        P.swap(mesh.P); N.swap(mesh.N); UV.swap(mesh.UV); idx.swap(mesh.indices);
    } else {
        error = "Shape \"" + name + "\" is outside the hot-path scope (supported: trianglemesh, plymesh" + (is_quadric_shape(name) ? "; the six quadric shapes are read with --quadrics)" : name == "curve" ? "; curves are read with --curves)" : name == "loopsubdiv" ? "; subdivision surfaces are read with --loopsubdiv)" : ")");
        return;
    }
    // alpha / shadowalpha (triangle.rs:278-312): a float texture by name (constant ones fold to the constant, the others are evaluated per candidate hit) or a float
    uint32_t alpha_tex[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    auto alpha_of = [&](const char* pname) {
        std::string tn = p.find_one_texture(pname);
        if (!tn.empty()) {
            const TexRef r = lookup_texture(tn, true);
            if (r.kind == TexRef::Device && r.is_float) { alpha_tex[std::strcmp(pname, "alpha") ? 1 : 0] = r.id; return 1.0f; }
            if (r.kind == TexRef::Constant) return r.value[0];
            if (r.kind == TexRef::Unsupported) { if (error.empty()) error = std::string("'") + pname + "' texture '" + tn + "' of class '" + r.cls + "' is outside the hot-path scope"; }
            else warn("Couldn't find float texture '" + tn + "' for '" + pname + "' parameter. Using float parameter instead.");
        }
        return p.find_one_float(pname, 1.0f);
    };
    const float alpha = alpha_of("alpha"), shadow_alpha = alpha_of("shadowalpha");
    if (!error.empty()) return;

    const uint32_t mat = material_id_for(material_for_shape(p));
    if (!error.empty()) return;

    // TriangleMesh::new moves the vertices to world space once (triangle.rs:93-99)
    const size_t nv = P.size() / 3;
    std::vector<float> Pw(P.size());
    pbrt_hip_host_transform_points(ctm_.m, P.data(), Pw.data(), nv);
    if (!N.empty()) { std::vector<float> t(N.size()); pbrt_hip_host_transform_normals(ctm_.mi, N.data(), t.data(), nv); N.swap(t); }
    if (!S.empty()) { std::vector<float> t(S.size()); pbrt_hip_host_transform_vectors(ctm_.m, S.data(), t.data(), nv); S.swap(t); }
    const uint32_t n_tris = (uint32_t)(idx.size() / 3);
    const uint32_t flags = (gs_.reverse_orientation ? 1u : 0u) | (pbrt_hip_host_swaps_handedness(ctm_.m) ? 2u : 0u);

    int32_t first_light = -1;
    const bool in_object = !current_object_.empty();
    if (!gs_.area_light.empty()) {  // one DiffuseAreaLight per triangle, numbered where the Shape directive stands (lib.rs:783-812)
        if (gs_.area_light != "diffuse" && gs_.area_light != "area") { error = "AreaLightSource \"" + gs_.area_light + "\" unknown"; return; }
        const ParamSet& ap = gs_.area_light_params;
        for (auto& u : ap.unsupported) { error = "AreaLightSource: parameter '" + u + "' has a spectral type this host cannot evaluate"; return; }
        auto L = mul3(ap.find_one_rgb("L", {1.0f, 1.0f, 1.0f}), ap.find_one_rgb("scale", {1.0f, 1.0f, 1.0f}));
        uint32_t id = 0;
        if (!check(ABI(pbrt_hip_add_light_diffuse_area(scene_, L.data(), ap.find_one_bool("twosided", false) ? 1 : 0, n_tris, &id)), "add_light_diffuse_area")) return;
        first_light = (int32_t)id;
        if (in_object) warn("Area lights not supported with object instancing.");   // lib.rs:877-881: the shape keeps its emission, the scene's lights do not get the light (pbrt_hip_add_mesh does the same)
        else n_lights_ += n_tris;
    }
    if (!check(ABI(pbrt_hip_add_mesh(scene_, Pw.data(), (uint32_t)nv, idx.data(), n_tris, N.empty() ? nullptr : N.data(), S.empty() ? nullptr : S.data(),
                                 UV.empty() ? nullptr : UV.data(), mat, first_light, flags, alpha, shadow_alpha)), "add_mesh")) return;
    if ((alpha_tex[0] != 0xFFFFFFFFu || alpha_tex[1] != 0xFFFFFFFFu) && !check(ABI(pbrt_hip_set_last_mesh_alpha_textures(scene_, alpha_tex[0], alpha_tex[1])), "set_last_mesh_alpha_textures")) return;
    if (current_object_.empty()) n_tris_ += n_tris; else object_tris_[current_object_] += n_tris;
}


int Api::pbrt_world_end(RenderReport& rep) {
    using clk = std::chrono::steady_clock;
    if (!scene_ && !check_only_) return PBRT_HIP_ERR_NO_DEVICE;
    if (!error.empty()) return PBRT_HIP_ERR_UNSUPPORTED;
    if (!verify_world("WorldEnd")) { error = "WorldEnd outside a world block"; return PBRT_HIP_ERR_STATE; }
    while (!gs_stack_.empty()) { warn("Missing end to AttributeBegin"); pbrt_attribute_end(); }
    while (!ctm_stack_.empty()) { warn("Missing end to TransformBegin"); ctm_stack_.pop_back(); }
    // PathIntegrator::li weights a hit on an emitter by the light's pdf, Sphere::pdf_solid_angle, which the library evaluates only on a handle whose switch is on
    // (pbrt_hip_set_path_sphere_lights: its inside branch departs from a reference that crashes there): the library refuses at render time, check mode has to here
    if (sphere_light_ && integrator_name_ == "path" && !path_sphere_lights) {
        error = "Shape \"sphere\" under AreaLightSource \"diffuse\" (a sphere light) is rendered by Integrator \"whitted\" only, not by \"path\" (unless run with --path-sphere-lights)";
        return PBRT_HIP_ERR_UNSUPPORTED;
    }
    // estimate_direct's MIS weight is the same pdf: the direct-lighting integrator follows the path integrator's rule (pbrt_hip_render_direct)
    if (sphere_light_ && integrator_name_ == "directlighting" && !path_sphere_lights) {
        error = "Shape \"sphere\" under AreaLightSource \"diffuse\" (a sphere light) is rendered by Integrator \"directlighting\" only when run with --path-sphere-lights";
        return PBRT_HIP_ERR_UNSUPPORTED;
    }

    // ---- filter + film (make_filter / make_film, graphics_state.rs:600-690; film/mod.rs:420-487)
    int fkind = -1; float rad[2] = {0.5f, 0.5f}, fparams[2] = {0.0f, 0.0f};
    if (filter_name_ == "box") { fkind = 0; rad[0] = filter_p_.find_one_float("xwidth", 0.5f); rad[1] = filter_p_.find_one_float("ywidth", 0.5f); }
    else if (filter_name_ == "gaussian") { fkind = 1; rad[0] = filter_p_.find_one_float("xwidth", 2.0f); rad[1] = filter_p_.find_one_float("ywidth", 2.0f); fparams[0] = filter_p_.find_one_float("alpha", 2.0f); }
    else if (filter_name_ == "mitchell") { fkind = 2; rad[0] = filter_p_.find_one_float("xwidth", 2.0f); rad[1] = filter_p_.find_one_float("ywidth", 2.0f); fparams[0] = filter_p_.find_one_float("B", 1.0f / 3.0f); fparams[1] = filter_p_.find_one_float("C", 1.0f / 3.0f); }
    else if (filter_name_ == "sinc") { fkind = 3; rad[0] = filter_p_.find_one_float("xwidth", 4.0f); rad[1] = filter_p_.find_one_float("ywidth", 4.0f); fparams[0] = filter_p_.find_one_float("tau", 3.0f); }
    else if (filter_name_ == "triangle") { fkind = 4; rad[0] = filter_p_.find_one_float("xwidth", 2.0f); rad[1] = filter_p_.find_one_float("ywidth", 2.0f); }
    else { error = "Filter \"" + filter_name_ + "\" unknown."; return PBRT_HIP_ERR_UNSUPPORTED; }
    if (film_name_ != "image") { error = "Film \"" + film_name_ + "\" unknown."; return PBRT_HIP_ERR_UNSUPPORTED; }
    const int xres = film_p_.find_one_int("xresolution", 1280), yres = film_p_.find_one_int("yresolution", 720);
    float crop[4] = {0.0f, 1.0f, 0.0f, 1.0f};
    auto clamp01 = [](float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); };
    if (const std::vector<float>* cr = film_p_.find_floats("cropwindow")) {
        if (cr->size() != 4) { error = std::to_string(cr->size()) + " values supplied for 'cropwindow'. Expected 4."; return PBRT_HIP_ERR_INVALID_ARG; }
        const float* c = cr->data();
        crop[0] = clamp01(c[0] < c[1] ? c[0] : c[1]); crop[1] = clamp01(c[0] > c[1] ? c[0] : c[1]);
        crop[2] = clamp01(c[2] < c[3] ? c[2] : c[3]); crop[3] = clamp01(c[2] > c[3] ? c[2] : c[3]);
    } else if (has_crop_override) {
        for (int i = 0; i < 4; i++) crop[i] = clamp01(crop_override[i]);
    }
    std::string filename = film_p_.find_one_string("filename", "pbrt.exr");
    if (!override_outfile.empty()) {
        if (film_p_.strings.count("filename")) warn("Output filename supplied on command line, '" + override_outfile + "' is overriding filename provided in scene description file, '" + filename + "'.");
        filename = override_outfile;
    }
    {   // write_image (image_io.rs:225-237) knows .exr, .tga, .png and .pfm; anything else is an error before rendering, not after
        size_t dot = filename.find_last_of('.'), slash = filename.find_last_of('/');
        std::string ext = (dot != std::string::npos && (slash == std::string::npos || dot > slash)) ? filename.substr(dot) : "";
        for (char& c : ext) c = (char)std::tolower((unsigned char)c);
        if (!(ext == ".exr" || ext == ".tga" || ext == ".png" || ext == ".pfm")) {
            error = ext.empty() ? "Can't determine file type from suffix of filename " + filename : "Extension " + ext + " is not supported";
            return PBRT_HIP_ERR_INVALID_ARG;
        }
    }
    const float film_scale = film_p_.find_one_float("scale", 1.0f);
    const float max_lum = film_p_.find_one_float("maxsampleluminance", std::numeric_limits<float>::infinity());
    int cb[4], sb[4]; float table[256];
    if (pbrt_hip_host_film_filter(fkind, fparams, xres, yres, crop, rad, cb, table, sb) != 0) { error = "film filter set-up failed"; return PBRT_HIP_ERR_INVALID_ARG; }
    if (!check(ABI(pbrt_hip_set_film(scene_, xres, yres, cb, rad, table, film_scale, max_lum)), "set_film")) return PBRT_HIP_ERR_INVALID_ARG;

    // ---- camera (perspective_camera.rs:358-419, orthographic_camera.rs:188-244: the same parameters minus the field of view)
    if (camera_name_ != "perspective" && camera_name_ != "orthographic" && camera_name_ != "environment") { error = "Camera \"" + camera_name_ + "\" is outside the hot-path scope (supported: perspective, orthographic, environment)"; return PBRT_HIP_ERR_UNSUPPORTED; }
    float shutter_open = camera_p_.find_one_float("shutteropen", 0.0f), shutter_close = camera_p_.find_one_float("shutterclose", 1.0f);
    if (shutter_close < shutter_open) { warn("Shutter close time < shutter open. Swapping them."); std::swap(shutter_open, shutter_close); }
    const float lens_radius = camera_p_.find_one_float("lensradius", 0.0f), focal_distance = camera_p_.find_one_float("focaldistance", 1e6f);
    const float frame = camera_p_.find_one_float("frameaspectratio", (float)xres / (float)yres);
    float screen[4];
    if (frame > 1.0f) { screen[0] = -frame; screen[1] = frame; screen[2] = -1.0f; screen[3] = 1.0f; }
    else { screen[0] = -1.0f; screen[1] = 1.0f; screen[2] = -1.0f / frame; screen[3] = 1.0f / frame; }
    if (const std::vector<float>* sw = camera_p_.find_floats("screenwindow")) {
        if (sw->size() == 4) for (int i = 0; i < 4; i++) screen[i] = (*sw)[i];
        else warn("'screenwindow' should have four values");
    }
    float fov = camera_p_.find_one_float("fov", 90.0f);
    const float half_fov = camera_p_.find_one_float("halffov", -1.0f);
    if (half_fov > 0.0f) fov = 2.0f * half_fov;
    float r2c[16];
    if (camera_name_ == "environment") {   // environment_camera.rs:86-104: shutter times only
        if (!check(ABI(pbrt_hip_set_camera_environment(scene_, camera_to_world_.m, xres, yres, shutter_open, shutter_close)), "set_camera_environment")) return PBRT_HIP_ERR_INVALID_ARG;
    } else if (camera_name_ == "orthographic") {
        pbrt_hip_host_orthographic_raster_to_camera(xres, yres, screen, r2c);
        if (!check(ABI(pbrt_hip_set_camera_orthographic(scene_, r2c, camera_to_world_.m, lens_radius, focal_distance, shutter_open, shutter_close)), "set_camera_orthographic")) return PBRT_HIP_ERR_INVALID_ARG;
    } else {
        pbrt_hip_host_perspective_raster_to_camera(fov, xres, yres, screen, r2c);
        if (!check(ABI(pbrt_hip_set_camera_perspective(scene_, r2c, camera_to_world_.m, lens_radius, focal_distance, shutter_open, shutter_close)), "set_camera_perspective")) return PBRT_HIP_ERR_INVALID_ARG;
    }

    // ---- sampler (halton.rs:272-290, sobol.rs:201-214)
    int skind;
    if (sampler_name_ == "halton") skind = 0;
    else if (sampler_name_ == "sobol") skind = 1;
    else { error = "Sampler \"" + sampler_name_ + "\" is outside the hot-path scope (supported: halton, sobol)"; return PBRT_HIP_ERR_UNSUPPORTED; }
    const int spp = sampler_p_.find_one_int("pixelsamples", 16);
    if (spp <= 0) { error = "pixelsamples must be positive"; return PBRT_HIP_ERR_INVALID_ARG; }
    if (!check(ABI(pbrt_hip_set_sampler(scene_, skind, (uint32_t)spp, sb, sampler_p_.find_one_bool("samplepixelcenter", false) ? 1 : 0)), "set_sampler")) return PBRT_HIP_ERR_INVALID_ARG;
    if (skind == 1) {
        if (sobol_tables_file.empty()) { error = "Sampler \"sobol\" needs --sobol-tables FILE (the generator matrices are data the library does not embed)"; return PBRT_HIP_ERR_STATE; }
        std::ifstream f(sobol_tables_file, std::ios::binary);
        const size_t n32 = 1024 * 52, nv = 25 * 52, nvi = 26 * 52;
        std::vector<uint32_t> m32(n32); std::vector<uint64_t> vdc(nvi), vdci(nvi);
        if (!f || !f.read((char*)m32.data(), n32 * 4) || !f.read((char*)vdc.data(), nv * 8) || !f.read((char*)vdci.data(), nvi * 8)) {
            error = "cannot read Sobol tables from '" + sobol_tables_file + "'"; return PBRT_HIP_ERR_INVALID_ARG;
        }
        if (!check(ABI(pbrt_hip_set_sobol_tables(scene_, m32.data(), n32, vdc.data(), vdci.data(), nvi)), "set_sobol_tables")) return PBRT_HIP_ERR_INVALID_ARG;
    }

    // ---- accelerator (bvh/mod.rs:339-360)
    int split = 0;
    if (accel_name_ == "bvh") {
        const std::string sm = accel_p_.find_one_string("splitmethod", "sah");
        if (sm == "sah") split = 0;
        else if (sm == "equal") split = 3;
        else if (sm == "hlbvh") split = 1;
        else if (sm == "middle") { error = "BVH splitmethod \"middle\" panics in the reference (sah.rs:67-76) and is not offered (supported: sah, hlbvh, equal)"; return PBRT_HIP_ERR_UNSUPPORTED; }
        else { warn("BVH split method \"" + sm + "\" unknown.  Using \"sah\"."); split = 0; }
    } else { error = "Accelerator \"" + accel_name_ + "\" is outside the hot-path scope (supported: bvh)"; return PBRT_HIP_ERR_UNSUPPORTED; }
    const int max_prims = accel_p_.find_one_int("maxnodeprims", 4);
    if (n_lights_ == 0) warn("No light sources defined in scene; rendering a black image.");
    auto t0 = clk::now();
    // "sah" and "hlbvh" trees are made on the GPU, scenes with object instances included (same trees: csrc/bvh_sah_device.hip, bvh_device.hip); everything else by the library's host builder
    int brc = PBRT_HIP_ERR_UNSUPPORTED;
    if ((split == 0 || split == 1) && !check_only_)   // pbrt_hip_build_accel_device refuses the SAH tree of a scene with quadric shapes; the _shapes entry builds either
        brc = (n_quadrics_ || n_curves_) ? pbrt_hip_build_accel_device_shapes(scene_, split, max_prims) : pbrt_hip_build_accel_device(scene_, split, max_prims);
    if (brc == PBRT_HIP_ERR_UNSUPPORTED) brc = ABI(pbrt_hip_build_accel(scene_, split, max_prims));
    if (!check(brc, "build_accel")) return PBRT_HIP_ERR_DEVICE;
    rep.build_seconds = std::chrono::duration<double>(clk::now() - t0).count();

    // ---- integrator (path.rs:287-327, whitted.rs:121-150, direct_lighting.rs:169-213: "maxdepth" 5 and "pixelbounds", read the same way)
    const bool whitted = integrator_name_ == "whitted", direct = integrator_name_ == "directlighting";
    if (integrator_name_ != "path" && !whitted && !direct) { error = "Integrator \"" + integrator_name_ + "\" is outside the hot-path scope (supported: path, whitted), directlighting"; return PBRT_HIP_ERR_UNSUPPORTED; }
    int direct_strategy = 0;   // direct_lighting.rs:178-186
    if (direct) {
        const std::string st = integrator_p_.find_one_string("strategy", "all");
        if (st == "one") direct_strategy = 1;
        else if (st != "all") warn("Strategy '" + st + "' for direct lighting unknown. Using 'all'.");
        rep.direct_strategy = direct_strategy ? "one" : "all";
    }
    const int max_depth = integrator_p_.find_one_int("maxdepth", 5);
    int pb[4] = {sb[0], sb[1], sb[2], sb[3]};
    if (const std::vector<int>* v = integrator_p_.find_ints("pixelbounds")) {
        if (v->size() != 4) warn("Expected 4 values for 'pixelbounds' parameter.");
        else {
            pb[0] = std::max(pb[0], (*v)[0]); pb[1] = std::max(pb[1], (*v)[1]);
            pb[2] = std::min(pb[2], (*v)[2]); pb[3] = std::min(pb[3], (*v)[3]);
            if (pb[2] <= pb[0] || pb[3] <= pb[1]) { warn("Degenerate 'pixelbounds' specified."); pb[2] = pb[0]; pb[3] = pb[1]; }
        }
    }
    const float rr = integrator_p_.find_one_float("rrthreshold", 1.0f);
    const std::string lss = integrator_p_.find_one_string("lightsamplestrategy", "spatial");
    int strategy = 2;
    if (lss == "uniform") strategy = 0; else if (lss == "power") strategy = 1; else if (lss == "spatial") strategy = 2;
    else { warn("Light sample distribution type \"" + lss + "\" unknown. Using \"spatial\"."); strategy = 2; }

    rep.xres = xres; rep.yres = yres; std::memcpy(rep.crop, cb, sizeof cb);
    rep.n_triangles = n_tris_; rep.n_lights = n_lights_; rep.n_instances = n_instances_; rep.n_quadrics = n_quadrics_; rep.n_curves = n_curves_; rep.warnings = warnings;
    rep.integrator = integrator_name_;
    rep.spp = spp; rep.max_depth = max_depth; rep.light_strategy = strategy; std::memcpy(rep.pixel_bounds, pb, sizeof pb);
    if (check_only_) { rep.out_file = filename; return PBRT_HIP_OK; }
    const size_t npix = (size_t)std::max(0, cb[2] - cb[0]) * (size_t)std::max(0, cb[3] - cb[1]);
    std::vector<float> xyz(npix * 3), wt(npix), rgb(npix * 3);
    if (!check(pbrt_hip_set_sample_record_budget(scene_, sample_record_budget), "set_sample_record_budget")) return PBRT_HIP_ERR_INVALID_ARG;
    if (!check(pbrt_hip_set_path_sphere_lights(scene_, path_sphere_lights ? 1 : 0), "set_path_sphere_lights")) return PBRT_HIP_ERR_INVALID_ARG;
    int rc = whitted ? pbrt_hip_render_whitted_devices(scene_, max_depth, pb, tile_size, 0, 1, xyz.data(), wt.data(), &rep.stats)
             : direct ? pbrt_hip_render_direct_devices(scene_, direct_strategy, max_depth, pb, tile_size, 0, 1, xyz.data(), wt.data(), &rep.stats)
                      : pbrt_hip_render_path(scene_, max_depth, rr, strategy, pb, tile_size, 0, 1, xyz.data(), wt.data(), &rep.stats);
    if (!check(rc, whitted ? "render_whitted_devices" : direct ? "render_direct_devices" : "render_path")) return rc;
    if (!check(pbrt_hip_film_to_rgb(scene_, xyz.data(), wt.data(), rgb.data()), "film_to_rgb")) return PBRT_HIP_ERR_DEVICE;
    std::string err;
    if (!write_image(filename, rgb.data(), cb[2] - cb[0], cb[3] - cb[1], err)) { error = err; return PBRT_HIP_ERR_INVALID_ARG; }
    rep.out_file = filename; rep.warnings = warnings;
    return PBRT_HIP_OK;
}

// core/src/image_io.rs:336-374: "PF", width height, scale -1 (little endian), scanlines bottom-to-top, f32 RGB.
bool write_pfm(const std::string& path, const float* rgb, int w, int h, std::string& err) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { err = "Unable to open output PFM file '" + path + "'"; return false; }
    std::fprintf(f, "PF\n%d %d\n-1\n", w, h);
    for (int y = h - 1; y >= 0; y--)
        if (std::fwrite(rgb + (size_t)y * w * 3, sizeof(float), (size_t)w * 3, f) != (size_t)w * 3) { err = "Error writing PFM file '" + path + "'"; std::fclose(f); return false; }
    std::fclose(f);
    return true;
}

}  // namespace pbrt_host
