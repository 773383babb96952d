// Host-only pin of what the scene-file front end (pbrt-v3-rs_amd/host) sends to the library: this program links the front end, the parser, the image and PLY readers and the
// library's host-side math (csrc/host_setup.cpp, csrc/bvh_build.cpp), and defines every other pbrt_hip_* entry point the front end calls as a RECORDER — one line per call with
// every argument (floats as their 32-bit pattern, small arrays element by element, bulk arrays as a count and a 64-bit FNV-1a hash; ids from one counter per kind, so they show
// the order of creation).  It then feeds scene texts through parse_string / parse_file — the 19 files under tests/golden/ref_scenes, sweeps over every material type x parameter
// x way of giving it, every texture class x type x operand form, the edges the material and texture code has, and the scene texts of tests/test_host_driver_gpu.py — once against
// the recorder and once in check mode (Api(-1)), and writes per scene: label, calls, warnings, error, return value.  tests/golden/front_end_calls.txt is that output;
// tests/test_front_end_calls_cpu.py compares.  The output names every distinct line once and every distinct record once (see below); matrices are written as `I` or a hash.
// Built by scripts/front_end_calls_check.sh with the address and undefined-behaviour sanitizers; CPU only.  Run from the repository's root (the paths in the output are relative).
#ifdef FRONT_END_HOST_HEADER   // the script names the front end under test (another commit's copy, to show where the recorded output comes from)
#include FRONT_END_HOST_HEADER
#else
#include "../pbrt-v3-rs_amd/host/pbrt_host.hpp"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unistd.h>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------- the recorder
static std::string g_calls;
static struct Ids { uint32_t tex = 0, mip = 0, mat = 0, obj = 0, light = 0; int cb[4] = {0, 0, 0, 0}; } g;
static size_t n_pixels() { return (size_t)(g.cb[2] > g.cb[0] ? g.cb[2] - g.cb[0] : 0) * (size_t)(g.cb[3] > g.cb[1] ? g.cb[3] - g.cb[1] : 0); }

struct Rec {   // one call: `name arg arg ...`, written when the object goes
    std::string s;
    explicit Rec(const char* name) : s(name) {}
    ~Rec() { g_calls += s + "\n"; }
    Rec& i(long long v) { s += " " + std::to_string(v); return *this; }
    Rec& f(float v) { uint32_t u; std::memcpy(&u, &v, 4); char b[16]; std::snprintf(b, sizeof b, " %08x", u); s += b; return *this; }
    Rec& fa(const float* p, int n) {
        if (!p) { s += " null"; return *this; }
        if (n == 16) {   // a matrix: I, or its hash
            bool identity = true;
            for (int k = 0; k < 16; k++) identity = identity && p[k] == (k % 5 == 0 ? 1.0f : 0.0f);
            if (identity) { s += " I"; return *this; }
            return bulk(p, 16, 4);
        }
        s += " ["; for (int k = 0; k < n; k++) f(p[k]); s += " ]"; return *this; }
    Rec& ia(const int* p, int n) { s += " ["; for (int k = 0; k < n; k++) i(p[k]); s += " ]"; return *this; }
    Rec& bulk(const void* p, size_t count, size_t elt) {   // count:hash
        if (!p) { s += " null"; return *this; }
        uint64_t h = 1469598103934665603ull;
        for (size_t k = 0; k < count * elt; k++) { h ^= ((const unsigned char*)p)[k]; h *= 1099511628211ull; }
        char b[48]; std::snprintf(b, sizeof b, " %zu:%016llx", count, (unsigned long long)h); s += b; return *this;
    }
    Rec& id(uint32_t v) { s += " -> " + std::to_string(v); return *this; }
};

namespace phost { int set_err(PbrtHipScene*, int code, const std::string&) { return code; } }
namespace hm {   // csrc/host_math.h declares it, the library's api unit defines it: the same Gauss-Jordan with full pivoting
struct M4 { float m[4][4]; };
M4 m4_inverse(const M4& a) {
    int indxc[4] = {0, 0, 0, 0}, indxr[4] = {0, 0, 0, 0}, ipiv[4] = {0, 0, 0, 0};
    float minv[4][4];
    std::memcpy(minv, a.m, sizeof(minv));
    for (int i = 0; i < 4; i++) {
        int irow = 0, icol = 0;
        float big = 0.0f;
        for (int j = 0; j < 4; j++)
            if (ipiv[j] != 1)
                for (int k = 0; k < 4; k++)
                    if (ipiv[k] == 0) { const float av = minv[j][k] < 0.0f ? -minv[j][k] : minv[j][k]; if (av >= big) { big = av; irow = j; icol = k; } }
        ipiv[icol] += 1;
        if (irow != icol) for (int k = 0; k < 4; k++) std::swap(minv[irow][k], minv[icol][k]);
        indxr[i] = irow; indxc[i] = icol;
        const float pivinv = 1.0f / minv[icol][icol];
        minv[icol][icol] = 1.0f;
        for (int j = 0; j < 4; j++) minv[icol][j] *= pivinv;
        for (int j = 0; j < 4; j++)
            if (j != icol) {
                const float save = minv[j][icol];
                minv[j][icol] = 0.0f;
                for (int k = 0; k < 4; k++) minv[j][k] -= minv[icol][k] * save;
            }
    }
    for (int j = 3; j >= 0; j--)
        if (indxr[j] != indxc[j]) for (int k = 0; k < 4; k++) std::swap(minv[k][indxr[j]], minv[k][indxc[j]]);
    M4 r; std::memcpy(r.m, minv, sizeof(minv)); return r;
}
}  // namespace hm

extern "C" {
static char g_scene_storage;
PbrtHipScene* pbrt_hip_scene_create(int) { return (PbrtHipScene*)&g_scene_storage; }
PbrtHipScene* pbrt_hip_scene_create_multi(const int*, int) { return nullptr; }
int pbrt_hip_scene_devices(const PbrtHipScene*, int*, int) { return 1; }
void pbrt_hip_scene_destroy(PbrtHipScene*) {}
const char* pbrt_hip_last_error(const PbrtHipScene*) { return ""; }

int pbrt_hip_add_material_none(PbrtHipScene*, uint32_t* o) { *o = g.mat++; Rec("add_material_none").id(*o); return 0; }
int pbrt_hip_add_material_matte(PbrtHipScene*, const float kd[3], float sigma, uint32_t* o) { *o = g.mat++; Rec("add_material_matte").fa(kd, 3).f(sigma).id(*o); return 0; }
int pbrt_hip_add_material_mirror(PbrtHipScene*, const float kr[3], uint32_t* o) { *o = g.mat++; Rec("add_material_mirror").fa(kr, 3).id(*o); return 0; }
int pbrt_hip_add_material_plastic(PbrtHipScene*, const float kd[3], const float ks[3], float r, int remap, uint32_t* o) { *o = g.mat++; Rec("add_material_plastic").fa(kd, 3).fa(ks, 3).f(r).i(remap).id(*o); return 0; }
int pbrt_hip_add_material_glass(PbrtHipScene*, const float kr[3], const float kt[3], float u, float v, float eta, int remap, uint32_t* o) {
    *o = g.mat++; Rec("add_material_glass").fa(kr, 3).fa(kt, 3).f(u).f(v).f(eta).i(remap).id(*o); return 0;
}
int pbrt_hip_add_material_metal(PbrtHipScene*, const float eta[3], const float k[3], float u, float v, int remap, uint32_t* o) { *o = g.mat++; Rec("add_material_metal").fa(eta, 3).fa(k, 3).f(u).f(v).i(remap).id(*o); return 0; }
int pbrt_hip_add_material_uber(PbrtHipScene*, const float kd[3], const float ks[3], const float kr[3], const float kt[3], const float op[3], float u, float v, float eta, int remap, uint32_t* o) {
    *o = g.mat++; Rec("add_material_uber").fa(kd, 3).fa(ks, 3).fa(kr, 3).fa(kt, 3).fa(op, 3).f(u).f(v).f(eta).i(remap).id(*o); return 0;
}
int pbrt_hip_add_material_substrate(PbrtHipScene*, const float kd[3], const float ks[3], float u, float v, int remap, uint32_t* o) { *o = g.mat++; Rec("add_material_substrate").fa(kd, 3).fa(ks, 3).f(u).f(v).i(remap).id(*o); return 0; }
int pbrt_hip_add_material_translucent(PbrtHipScene*, const float kd[3], const float ks[3], const float re[3], const float tr[3], float r, int remap, uint32_t* o) {
    *o = g.mat++; Rec("add_material_translucent").fa(kd, 3).fa(ks, 3).fa(re, 3).fa(tr, 3).f(r).i(remap).id(*o); return 0;
}
int pbrt_hip_add_material_mix(PbrtHipScene*, uint32_t m1, uint32_t m2, const float amount[3], uint32_t* o) { *o = g.mat++; Rec("add_material_mix").i(m1).i(m2).fa(amount, 3).id(*o); return 0; }

int pbrt_hip_add_mesh(PbrtHipScene*, const float* P, uint32_t nv, const uint32_t* idx, uint32_t nt, const float* N, const float* S, const float* UV, uint32_t mat, int32_t light, uint32_t flags, float alpha, float shadow_alpha) {
    Rec("add_mesh").bulk(P, 3 * (size_t)nv, 4).bulk(idx, 3 * (size_t)nt, 4).bulk(N, 3 * (size_t)nv, 4).bulk(S, 3 * (size_t)nv, 4).bulk(UV, 2 * (size_t)nv, 4).i(mat).i(light).i(flags).f(alpha).f(shadow_alpha); return 0;
}
int pbrt_hip_object_begin(PbrtHipScene*, uint32_t* o) { *o = g.obj++; Rec("object_begin").id(*o); return 0; }
int pbrt_hip_object_end(PbrtHipScene*) { Rec("object_end"); return 0; }
int pbrt_hip_add_instance(PbrtHipScene*, uint32_t obj, const float m[16], const float mi[16]) { Rec("add_instance").i(obj).fa(m, 16).fa(mi, 16); return 0; }
int pbrt_hip_add_sphere(PbrtHipScene*, const float m[16], const float mi[16], float r, float z0, float z1, float phi, uint32_t mat, uint32_t flags) { Rec("add_sphere").fa(m, 16).fa(mi, 16).f(r).f(z0).f(z1).f(phi).i(mat).i(flags); return 0; }
int pbrt_hip_add_hyperboloid(PbrtHipScene*, const float m[16], const float mi[16], const float p1[3], const float p2[3], float phi, uint32_t mat, uint32_t flags) { Rec("add_hyperboloid").fa(m, 16).fa(mi, 16).fa(p1, 3).fa(p2, 3).f(phi).i(mat).i(flags); return 0; }
int pbrt_hip_add_quadric(PbrtHipScene*, int kind, const float m[16], const float mi[16], float r, float a, float b, float phi, uint32_t mat, uint32_t flags) { Rec("add_quadric").i(kind).fa(m, 16).fa(mi, 16).f(r).f(a).f(b).f(phi).i(mat).i(flags); return 0; }
int pbrt_hip_add_curve(PbrtHipScene*, const float m[16], const float mi[16], int type, const float cp[12], const float width[2], const float* n, int sd, uint32_t mat, uint32_t flags) {
    Rec("add_curve").fa(m, 16).fa(mi, 16).i(type).fa(cp, 12).fa(width, 2).fa(n, 6).i(sd).i(mat).i(flags); return 0;
}
int pbrt_hip_add_loopsubdiv(PbrtHipScene*, const float* m, const float* mi, const float* P, uint32_t nv, const uint32_t* idx, uint32_t ni, int levels, uint32_t mat, int32_t light, uint32_t flags, float alpha, float shadow_alpha) {
    Rec("add_loopsubdiv").fa(m, 16).fa(mi, 16).bulk(P, 3 * (size_t)nv, 4).bulk(idx, ni, 4).i(levels).i(mat).i(light).i(flags).f(alpha).f(shadow_alpha); return 0;
}
int pbrt_hip_add_sphere_light(PbrtHipScene*, const float m[16], const float mi[16], float r, float z0, float z1, float phi, uint32_t mat, uint32_t flags, const float L[3], int two) {
    Rec("add_sphere_light").fa(m, 16).fa(mi, 16).f(r).f(z0).f(z1).f(phi).i(mat).i(flags).fa(L, 3).i(two).id(g.light++); return 0;
}
int pbrt_hip_add_quadric_light(PbrtHipScene*, int kind, const float m[16], const float mi[16], float r, float a, float b, float phi, uint32_t mat, uint32_t flags, const float L[3], int two) {
    Rec("add_quadric_light").i(kind).fa(m, 16).fa(mi, 16).f(r).f(a).f(b).f(phi).i(mat).i(flags).fa(L, 3).i(two).id(g.light++); return 0;
}
int pbrt_hip_set_path_sphere_lights(PbrtHipScene*, int on) { Rec("set_path_sphere_lights").i(on); return 0; }
int pbrt_hip_set_last_mesh_alpha_textures(PbrtHipScene*, uint32_t a, uint32_t sa) { Rec("set_last_mesh_alpha_textures").i(a).i(sa); return 0; }

int pbrt_hip_add_mipmap(PbrtHipScene*, int w, int h, const float* rgb, int as_float, float scale, int gamma, int filtering, int wrap, float aniso, uint32_t* o) {
    *o = g.mip++; Rec("add_mipmap").i(w).i(h).bulk(rgb, 3 * (size_t)w * (size_t)h, 4).i(as_float).f(scale).i(gamma).i(filtering).i(wrap).f(aniso).id(*o); return 0;
}
int pbrt_hip_add_texture_constant(PbrtHipScene*, const float v[3], uint32_t* o) { *o = g.tex++; Rec("add_texture_constant").fa(v, 3).id(*o); return 0; }
int pbrt_hip_add_texture_scale(PbrtHipScene*, uint32_t t1, uint32_t t2, uint32_t* o) { *o = g.tex++; Rec("add_texture_scale").i(t1).i(t2).id(*o); return 0; }
int pbrt_hip_add_texture_mix(PbrtHipScene*, uint32_t t1, uint32_t t2, uint32_t amt, uint32_t* o) { *o = g.tex++; Rec("add_texture_mix").i(t1).i(t2).i(amt).id(*o); return 0; }
int pbrt_hip_add_texture_imagemap(PbrtHipScene*, uint32_t mip, float su, float sv, float du, float dv, uint32_t* o) { *o = g.tex++; Rec("add_texture_imagemap").i(mip).f(su).f(sv).f(du).f(dv).id(*o); return 0; }
int pbrt_hip_add_texture_checkerboard(PbrtHipScene*, uint32_t t1, uint32_t t2, float su, float sv, float du, float dv, int aa, uint32_t* o) { *o = g.tex++; Rec("add_texture_checkerboard").i(t1).i(t2).f(su).f(sv).f(du).f(dv).i(aa).id(*o); return 0; }
int pbrt_hip_add_texture_uv(PbrtHipScene*, float su, float sv, float du, float dv, uint32_t* o) { *o = g.tex++; Rec("add_texture_uv").f(su).f(sv).f(du).f(dv).id(*o); return 0; }
int pbrt_hip_add_texture_bilerp(PbrtHipScene*, const float v00[3], const float v01[3], const float v10[3], const float v11[3], float su, float sv, float du, float dv, uint32_t* o) {
    *o = g.tex++; Rec("add_texture_bilerp").fa(v00, 3).fa(v01, 3).fa(v10, 3).fa(v11, 3).f(su).f(sv).f(du).f(dv).id(*o); return 0;
}
int pbrt_hip_add_texture_dots(PbrtHipScene*, uint32_t in, uint32_t out, float su, float sv, float du, float dv, uint32_t* o) { *o = g.tex++; Rec("add_texture_dots").i(in).i(out).f(su).f(sv).f(du).f(dv).id(*o); return 0; }
int pbrt_hip_set_texture_mapping(PbrtHipScene*, uint32_t t, int kind, const float* prm) { Rec("set_texture_mapping").i(t).i(kind).fa(prm, kind == 3 ? 8 : 16); return 0; }
int pbrt_hip_add_texture_fbm(PbrtHipScene*, const float m[16], float omega, int oct, uint32_t* o) { *o = g.tex++; Rec("add_texture_fbm").fa(m, 16).f(omega).i(oct).id(*o); return 0; }
int pbrt_hip_add_texture_wrinkled(PbrtHipScene*, const float m[16], float omega, int oct, uint32_t* o) { *o = g.tex++; Rec("add_texture_wrinkled").fa(m, 16).f(omega).i(oct).id(*o); return 0; }
int pbrt_hip_add_texture_windy(PbrtHipScene*, const float m[16], uint32_t* o) { *o = g.tex++; Rec("add_texture_windy").fa(m, 16).id(*o); return 0; }
int pbrt_hip_add_texture_marble(PbrtHipScene*, const float m[16], float omega, int oct, float scale, float var, uint32_t* o) { *o = g.tex++; Rec("add_texture_marble").fa(m, 16).f(omega).i(oct).f(scale).f(var).id(*o); return 0; }
int pbrt_hip_add_texture_checkerboard3d(PbrtHipScene*, uint32_t t1, uint32_t t2, const float m[16], uint32_t* o) { *o = g.tex++; Rec("add_texture_checkerboard3d").i(t1).i(t2).fa(m, 16).id(*o); return 0; }
int pbrt_hip_set_material_texture(PbrtHipScene*, uint32_t mat, int param, uint32_t tex) { Rec("set_material_texture").i(mat).i(param).i(tex); return 0; }
int pbrt_hip_set_material_float_texture(PbrtHipScene*, uint32_t mat, int fparam, uint32_t tex) { Rec("set_material_float_texture").i(mat).i(fparam).i(tex); return 0; }
int pbrt_hip_set_material_bump(PbrtHipScene*, uint32_t mat, uint32_t tex) { Rec("set_material_bump").i(mat).i(tex); return 0; }

int pbrt_hip_add_light_infinite(PbrtHipScene*, const float L[3], const float m[16], const float mi[16]) { Rec("add_light_infinite").fa(L, 3).fa(m, 16).fa(mi, 16).id(g.light++); return 0; }
int pbrt_hip_add_light_infinite_map(PbrtHipScene*, const float L[3], int w, int h, const float* rgb, const float m[16], const float mi[16]) {
    Rec("add_light_infinite_map").fa(L, 3).i(w).i(h).bulk(rgb, 3 * (size_t)w * (size_t)h, 4).fa(m, 16).fa(mi, 16).id(g.light++); return 0;
}
int pbrt_hip_add_light_projection(PbrtHipScene*, const float I[3], const float m[16], const float mi[16], float fov, int w, int h, const float* rgb) {
    Rec("add_light_projection").fa(I, 3).fa(m, 16).fa(mi, 16).f(fov).i(w).i(h).bulk(rgb, 3 * (size_t)w * (size_t)h, 4).id(g.light++); return 0;
}
int pbrt_hip_add_light_goniometric(PbrtHipScene*, const float I[3], const float m[16], const float mi[16], int w, int h, const float* rgb) {
    Rec("add_light_goniometric").fa(I, 3).fa(m, 16).fa(mi, 16).i(w).i(h).bulk(rgb, 3 * (size_t)w * (size_t)h, 4).id(g.light++); return 0;
}
int pbrt_hip_add_light_distant(PbrtHipScene*, const float L[3], const float w[3]) { Rec("add_light_distant").fa(L, 3).fa(w, 3).id(g.light++); return 0; }
int pbrt_hip_add_light_point(PbrtHipScene*, const float I[3], const float p[3]) { Rec("add_light_point").fa(I, 3).fa(p, 3).id(g.light++); return 0; }
int pbrt_hip_add_light_spot(PbrtHipScene*, const float I[3], const float m[16], const float mi[16], float ct, float cf) { Rec("add_light_spot").fa(I, 3).fa(m, 16).fa(mi, 16).f(ct).f(cf).id(g.light++); return 0; }
int pbrt_hip_add_light_diffuse_area(PbrtHipScene*, const float L[3], int two, uint32_t n, uint32_t* o) { *o = g.light; g.light += n; Rec("add_light_diffuse_area").fa(L, 3).i(two).i(n).id(*o); return 0; }

int pbrt_hip_set_camera_perspective(PbrtHipScene*, const float r2c[16], const float c2w[16], float lens, float focal, float so, float sc) { Rec("set_camera_perspective").fa(r2c, 16).fa(c2w, 16).f(lens).f(focal).f(so).f(sc); return 0; }
int pbrt_hip_set_camera_orthographic(PbrtHipScene*, const float r2c[16], const float c2w[16], float lens, float focal, float so, float sc) { Rec("set_camera_orthographic").fa(r2c, 16).fa(c2w, 16).f(lens).f(focal).f(so).f(sc); return 0; }
int pbrt_hip_set_camera_environment(PbrtHipScene*, const float c2w[16], int xres, int yres, float so, float sc) { Rec("set_camera_environment").fa(c2w, 16).i(xres).i(yres).f(so).f(sc); return 0; }
int pbrt_hip_set_film(PbrtHipScene*, int xres, int yres, const int cb[4], const float rad[2], const float table[256], float scale, float max_lum) {
    std::memcpy(g.cb, cb, sizeof g.cb);
    Rec("set_film").i(xres).i(yres).ia(cb, 4).fa(rad, 2).bulk(table, 256, 4).f(scale).f(max_lum); return 0;
}
int pbrt_hip_set_sampler(PbrtHipScene*, int kind, uint32_t spp, const int sb[4], int centre) { Rec("set_sampler").i(kind).i(spp).ia(sb, 4).i(centre); return 0; }
int pbrt_hip_set_sobol_tables(PbrtHipScene*, const uint32_t* m32, size_t n32, const uint64_t* vdc, const uint64_t* vdci, size_t nv) { Rec("set_sobol_tables").bulk(m32, n32, 4).bulk(vdc, nv, 8).bulk(vdci, nv, 8); return 0; }
int pbrt_hip_build_accel(PbrtHipScene*, int split, int max_prims) { Rec("build_accel").i(split).i(max_prims); return 0; }
int pbrt_hip_build_accel_device(PbrtHipScene*, int split, int max_prims) { Rec("build_accel_device").i(split).i(max_prims); return 0; }
int pbrt_hip_build_accel_device_shapes(PbrtHipScene*, int split, int max_prims) { Rec("build_accel_device_shapes").i(split).i(max_prims); return 0; }
int pbrt_hip_set_sample_record_budget(PbrtHipScene*, uint64_t bytes) { Rec("set_sample_record_budget").i((long long)bytes); return 0; }
static void zero_film(float* xyz, float* wt, PbrtHipStats* st) {
    std::memset(xyz, 0, n_pixels() * 3 * sizeof(float)); std::memset(wt, 0, n_pixels() * sizeof(float));
    if (st) std::memset(st, 0, sizeof *st);
}
int pbrt_hip_render_path(PbrtHipScene*, int depth, float rr, int strategy, const int pb[4], int tile, int part, int parts, float* xyz, float* wt, PbrtHipStats* st) {
    Rec("render_path").i(depth).f(rr).i(strategy).ia(pb, 4).i(tile).i(part).i(parts); zero_film(xyz, wt, st); return 0;
}
int pbrt_hip_render_whitted_devices(PbrtHipScene*, int depth, const int pb[4], int tile, int part, int parts, float* xyz, float* wt, PbrtHipStats* st) {
    Rec("render_whitted_devices").i(depth).ia(pb, 4).i(tile).i(part).i(parts); zero_film(xyz, wt, st); return 0;
}
int pbrt_hip_render_direct_devices(PbrtHipScene*, int strategy, int depth, const int pb[4], int tile, int part, int parts, float* xyz, float* wt, PbrtHipStats* st) {
    Rec("render_direct_devices").i(strategy).i(depth).ia(pb, 4).i(tile).i(part).i(parts); zero_film(xyz, wt, st); return 0;
}
int pbrt_hip_film_to_rgb(const PbrtHipScene*, const float*, const float*, float* rgb) { Rec("film_to_rgb"); std::memset(rgb, 0, n_pixels() * 3 * sizeof(float)); return 0; }
}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- running scenes
using pbrt_host::Api;
static std::string g_tmp;   // image output, and the image files of the texts from tests/test_host_driver_gpu.py
// The output is three parts.  Lines: every distinct line of any record (a call, `W:` a warning, `E:` the error, ...), numbered.  Records: every distinct record — what one
// scene came to — as the numbers of its lines.  Scenes: per section, tables of record numbers; a scene's label is "row @ column", and rows that share their columns share one `cols:` line.
static std::map<std::string, size_t> g_line_no, g_record_no;
static std::vector<std::string> g_lines, g_records;
struct Row { std::string label; std::vector<std::string> cols; std::vector<size_t> recs; };
static std::vector<Row> g_rows;   // of the section being run

static std::string scrub(std::string s) {   // the temporary directory's name is not part of the record
    for (size_t p; (p = s.find(g_tmp)) != std::string::npos;) s.replace(p, g_tmp.size(), "$TMP");
    return s;
}
static std::string outcome(const Api& api, bool ok) {
    std::string s;
    for (const std::string& w : api.warnings) s += "W: " + scrub(w) + "\n";
    if (!api.error.empty()) s += "E: " + scrub(api.error) + "\n";
    if (!ok) s += "parse: false\n";   // (parse_string / parse_file returned false)
    return s;
}
static void configure(Api& api, bool shape_options) {
    api.quiet = true;
    api.override_outfile = g_tmp + "/out.pfm";
    api.quadrics = api.curves = api.loopsubdiv = api.quadric_lights = api.path_sphere_lights = shape_options;
}
// text: the scene's text (file == false, relative names resolved against `dir`) or a file's path
static void scene(const std::string& label, const std::string& text, bool file = false, const std::string& dir = ".", bool shape_options = false) {
    std::string record, rec_outcome;
    {
        g_calls.clear(); g = Ids();
        Api api(0); configure(api, shape_options);
        pbrt_host::RenderReport rep;
        const bool ok = file ? pbrt_host::parse_file(text, api, &rep) : pbrt_host::parse_string(text, dir, api, &rep);
        rec_outcome = outcome(api, ok);
        record = g_calls + rec_outcome;
    }
    {
        g_calls.clear();
        Api api(-1); configure(api, shape_options);
        pbrt_host::RenderReport rep;
        const bool ok = file ? pbrt_host::parse_file(text, api, &rep) : pbrt_host::parse_string(text, dir, api, &rep);
        const std::string o = outcome(api, ok);
        if (o != rec_outcome) record += "check mode differs:\n" + o;   // (nothing is written where check mode gives the same warnings, error and return value)
        if (!g_calls.empty()) record += "check mode made calls:\n" + g_calls;
        char b[256];
        std::snprintf(b, sizeof b, "check report: %llu triangles %llu lights %llu instances %llu quadrics %llu curves %dx%d spp %d depth %d strategy %d integrator '%s'\n", (unsigned long long)rep.n_triangles,
                      (unsigned long long)rep.n_lights, (unsigned long long)rep.n_instances, (unsigned long long)rep.n_quadrics, (unsigned long long)rep.n_curves, rep.xres, rep.yres, rep.spp, rep.max_depth, rep.light_strategy, rep.integrator.c_str());
        if (rep.xres) record += b;   // (a text without WorldEnd fills no report)
    }
    std::string numbers;
    for (size_t p = 0, q; (q = record.find('\n', p)) != std::string::npos; p = q + 1) {
        const std::string line = record.substr(p, q - p);
        auto ln = g_line_no.find(line);
        if (ln == g_line_no.end()) { g_lines.push_back(line); ln = g_line_no.emplace(line, g_lines.size()).first; }
        numbers += (numbers.empty() ? "" : " ") + std::to_string(ln->second);
    }
    auto rn = g_record_no.find(numbers);
    if (rn == g_record_no.end()) { g_records.push_back(numbers); rn = g_record_no.emplace(numbers, g_records.size()).first; }
    const size_t at = label.find(" @ ");
    const std::string row = label.substr(0, at), col = at == std::string::npos ? "" : label.substr(at + 3);
    if (g_rows.empty() || g_rows.back().label != row) g_rows.push_back(Row{row, {}, {}});
    g_rows.back().cols.push_back(col); g_rows.back().recs.push_back(rn->second);
}
static void flush_section() {
    const std::vector<std::string>* cols = nullptr;
    for (const Row& r : g_rows) {
        if (r.cols.size() > 1 && (!cols || *cols != r.cols)) {
            std::string c;
            for (const std::string& x : r.cols) c += " | " + x;
            std::printf("cols:%s\n", c.c_str() + 2);
            cols = &r.cols;
        }
        std::string n;
        for (size_t x : r.recs) n += " " + std::to_string(x);
        std::printf("%s:%s\n", r.label.c_str(), n.c_str());
    }
    g_rows.clear();
}
static void section(const char* title) { flush_section(); std::printf("# ---- %s\n", title); }
static void write_records_and_lines() {
    flush_section();
    std::printf("# ---- records: the lines each consists of\n");
    std::string out;
    for (size_t k = 0; k < g_records.size(); k++) {   // several to a line
        const std::string one = "r" + std::to_string(k + 1) + ": " + g_records[k];
        if (!out.empty() && out.size() + one.size() > 150) { std::printf("%s\n", out.c_str()); out.clear(); }
        out += (out.empty() ? "" : " ; ") + one;
    }
    if (!out.empty()) std::printf("%s\n", out.c_str());
    std::printf("# ---- lines\n");
    for (size_t k = 0; k < g_lines.size(); k++) std::printf("%zu: %s\n", k + 1, g_lines[k].c_str());
}

// ---------------------------------------------------------------------------------------------------------------- the scene texts
static const char* kTri = "Shape \"trianglemesh\" \"integer indices\" [0 1 2] \"point P\" [0 0 0 1 0 0 0 1 0]\n";
static const char* kPng = "tests/golden/ref_scenes/images/checkerboard.png";
// the textures a swept parameter can name: cf / cs constant, df / ds evaluated by the library, un of a class it does not evaluate; "nope" is declared nowhere
// (only those the text names are declared: decoding the image file is most of this program's run time)
static std::string named_textures(const std::string& body) {
    const std::string decl[5][2] = {{"\"cf\"", "Texture \"cf\" \"float\" \"constant\" \"float value\" 0.3\n"}, {"\"cs\"", "Texture \"cs\" \"color\" \"constant\" \"rgb value\" [0.2 0.4 0.6]\n"},
                                    {"\"df\"", std::string("Texture \"df\" \"float\" \"imagemap\" \"string filename\" \"") + kPng + "\"\n"}, {"\"ds\"", std::string("Texture \"ds\" \"color\" \"imagemap\" \"string filename\" \"") + kPng + "\"\n"},
                                    {"\"un\"", "Texture \"un\" \"float\" \"ptex\"\n"}};
    std::string s;
    for (auto& d : decl) if (body.find(d[0]) != std::string::npos) s += d[1];
    return s;
}
struct Way { const char* tag; const char* fmt; };   // %s = the parameter's name
static const Way kWays[] = {{"absent", ""}, {"float", "\"float %s\" 0.7"}, {"rgb", "\"rgb %s\" [0.7 0.5 0.3]"}, {"cf", "\"texture %s\" \"cf\""}, {"cs", "\"texture %s\" \"cs\""},
                            {"df", "\"texture %s\" \"df\""}, {"ds", "\"texture %s\" \"ds\""}, {"un", "\"texture %s\" \"un\""}, {"nope", "\"texture %s\" \"nope\""}};
static std::string give(const Way& w, const std::string& pname) { char b[128]; std::snprintf(b, sizeof b, w.fmt, pname.c_str()); return b; }
static const char* kParams[] = {"Kd", "Ks", "Kr", "Kt", "sigma", "roughness", "uroughness", "vroughness", "eta", "index", "k", "opacity", "bumpmap", "reflect", "transmit", "amount"};
static const char* kTypes[] = {"none", "matte", "mirror", "plastic", "glass", "metal", "uber", "substrate", "translucent", "mix", "hair"};
static const char* kMixChildren = "MakeNamedMaterial \"m1\" \"string type\" \"matte\" \"rgb Kd\" [0.1 0.2 0.3]\nMakeNamedMaterial \"m2\" \"string type\" \"mirror\"\n";
static const char* kMixNames = " \"string namedmaterial1\" \"m1\" \"string namedmaterial2\" \"m2\"";
static std::string material_line(const std::string& type, const std::string& params) {
    return "Material \"" + type + "\" " + params + (type == "mix" ? kMixNames : "") + "\n";
}
static std::string world(const std::string& body) { return "WorldBegin\n" + named_textures(body) + body; }   // no WorldEnd: the record is the captured scene alone

static void fixtures() {
    section("scene files under tests/golden/ref_scenes (read with every shape option)");
    static const char* files[] = {"cameras/depth-of-field", "geometry/cube", "lights/diffuse", "materials/bump", "samplers/halton", "shapes/all-shapes-loopsubdiv", "shapes/all-shapes", "textures/2d-checkerboard",
                                  "textures/2d-mappings", "textures/bilerp", "textures/constant", "textures/dots", "textures/fbm", "textures/marble", "textures/mix", "textures/scale", "textures/uv", "textures/windy", "textures/wrinkled"};
    for (const char* f : files) scene(f, std::string("tests/golden/ref_scenes/") + f + ".pbrt", true, ".", true);
}

static void material_sweep() {
    section("material sweep: type x parameter x way of giving it x remaproughness");
    for (const char* type : kTypes)
        for (const char* pn : kParams)
            for (const Way& w : kWays)
                for (int remap = 1; remap >= 0; remap--) {
                    if (!remap && &w != &kWays[0] && &w != &kWays[1] && &w != &kWays[5]) continue;   // without remapping: absent, a float literal and a float texture of the library's
                    const std::string params = give(w, pn) + (remap ? "" : " \"bool remaproughness\" \"false\"");
                    scene(std::string(type) + " " + pn + " @ " + w.tag + (remap ? "" : " noremap"), world(kMixChildren + material_line(type, params) + kTri));
                }
}

static void material_edges() {
    section("material edges");
    // roughness with uroughness and / or vroughness, as literals and textures (uv_rough's fall-back order; a roughness texture fills only unset slots)
    static const char* rough[] = {"\"float roughness\" 0.3", "\"texture roughness\" \"df\"", "\"texture roughness\" \"cf\""};
    static const char* ur[] = {"", "\"float uroughness\" 0.2", "\"texture uroughness\" \"df\"", "\"texture uroughness\" \"cf\""};
    static const char* vr[] = {"", "\"float vroughness\" 0.4", "\"texture vroughness\" \"df\"", "\"texture vroughness\" \"cf\""};
    for (const char* type : {"metal", "uber", "plastic", "glass", "substrate", "translucent"})
        for (const char* r : rough) for (const char* u : ur) for (const char* v : vr)
            scene(std::string(type) + " " + r + " @ " + u + " " + v, world(material_line(type, std::string(r) + " " + u + " " + v) + kTri));
    // quirk B14: what the name "eta" stands for decides glass's and uber's index of refraction
    static const char* eta_named[] = {"Texture \"eta\" \"float\" \"constant\" \"float value\" 1.7\n", "Texture \"eta\" \"float\" \"imagemap\" \"string filename\" \"%s\"\n", "Texture \"eta\" \"color\" \"imagemap\" \"string filename\" \"%s\"\n",
                                      "Texture \"eta\" \"color\" \"constant\" \"rgb value\" [1.7 1.7 1.7]\n", "Texture \"eta\" \"float\" \"ptex\"\n", ""};
    for (const char* type : {"glass", "uber"})
        for (const char* decl : eta_named)
            for (const char* prm : {"", "\"float eta\" 1.4", "\"float eta\" 1.4 \"float index\" 1.3", "\"texture eta\" \"cf\"", "\"texture index\" \"df\"", "\"texture index\" \"cf\""}) {
                char d[256]; std::snprintf(d, sizeof d, decl, kPng);
                scene(std::string(type) + " eta-named{" + std::string(d).substr(0, std::string(d).find('\n')) + "} @ " + prm, world(d + material_line(type, prm) + kTri));
            }
    // bumpmap on an ordinary material, on mix and on none
    for (const char* type : {"matte", "plastic", "mix", "none", ""})
        for (const char* b : {"df", "cf", "ds", "cs", "un", "nope"})
            scene(std::string("bumpmap '") + type + "' @ " + b, world(kMixChildren + material_line(type, std::string("\"texture bumpmap\" \"") + b + "\"") + kTri));
    // what the material cache shares
    scene("two shapes, one bump-mapped material (device texture)", world(material_line("matte", "\"texture bumpmap\" \"df\"") + kTri + kTri));
    scene("two shapes, one bump-mapped material (constant texture)", world(material_line("matte", "\"texture bumpmap\" \"cf\"") + kTri + kTri));
    scene("two shapes, one plain material", world(material_line("matte", "\"rgb Kd\" [0.3 0.3 0.3]") + kTri + kTri));
    scene("two shapes, one textured material", world(material_line("plastic", "\"texture Kd\" \"ds\" \"texture roughness\" \"df\"") + kTri + kTri));
    scene("the same material under two Material directives", world(material_line("matte", "") + kTri + material_line("mirror", "") + kTri + material_line("matte", "") + kTri));
    // mix: named children defined, undefined, nested; an error in the first child
    const std::string kids = std::string(kMixChildren) + "MakeNamedMaterial \"tex\" \"string type\" \"plastic\" \"texture Kd\" \"ds\" \"texture bumpmap\" \"df\"\nMakeNamedMaterial \"bad\" \"string type\" \"matte\" \"texture Kd\" \"un\"\n"
                             "MakeNamedMaterial \"inner\" \"string type\" \"mix\" \"string namedmaterial1\" \"m1\" \"string namedmaterial2\" \"tex\" \"texture amount\" \"ds\"\n"
                             "MakeNamedMaterial \"deep\" \"string type\" \"mix\" \"string namedmaterial1\" \"inner\" \"string namedmaterial2\" \"inner\"\nMakeNamedMaterial \"notype\" \"rgb Kd\" [1 1 1]\n";
    for (const char* a : {"m1", "tex", "inner", "deep", "bad", "gone", "notype"})
        for (const char* b : {"m2", "tex", "inner", "bad", "gone"})
            scene(std::string("mix ") + a + " @ " + b, world(kids + "Material \"mix\" \"string namedmaterial1\" \"" + a + "\" \"string namedmaterial2\" \"" + b + "\" \"rgb amount\" [0.3 0.3 0.3] \"rgb Kd\" [0.9 0.1 0.1]\n" + kTri));
    scene("mix without names", world(std::string("Material \"mix\"\n") + kTri));
    scene("NamedMaterial known and unknown", world(kids + "NamedMaterial \"tex\"\n" + kTri + "NamedMaterial \"gone\"\n" + kTri + "NamedMaterial \"inner\"\n" + kTri));
    // shape-level overrides of every parameter: literal over texture, texture over literal, and remaproughness
    for (const char* type : {"uber", "glass", "metal", "translucent", "matte", "mix"})
        for (const char* pn : kParams) {
            const bool spec = std::string("Kd Ks Kr Kt opacity reflect transmit amount eta k").find(pn) != std::string::npos && std::string(pn) != "sigma";
            const std::string lit = give(kWays[spec ? 2 : 1], pn), texd = give(kWays[spec ? 6 : 5], pn), texc = give(kWays[spec ? 4 : 3], pn);
            const std::string tri(kTri, std::strlen(kTri) - 1);
            scene(std::string(type) + " shape override @ literal over material texture " + pn, world(kMixChildren + material_line(type, texd) + tri + " " + lit + "\n" + kTri));
            scene(std::string(type) + " shape override @ texture over material literal " + pn, world(kMixChildren + material_line(type, lit) + tri + " " + texd + "\n" + tri + " " + texc + "\n"));
        }
    for (const char* type : {"plastic", "glass"}) {
        const std::string tri(kTri, std::strlen(kTri) - 1);
        scene(std::string(type) + " shape-level remaproughness", world(material_line(type, "\"float roughness\" 0.2 \"float uroughness\" 0.2") + tri + " \"bool remaproughness\" \"false\"\n" + kTri +
                                                                       material_line(type, "\"bool remaproughness\" \"false\"") + tri + " \"bool remaproughness\" \"true\"\n"));
    }
    scene("named material with a shape override", world("MakeNamedMaterial \"n\" \"string type\" \"uber\" \"texture Kd\" \"ds\" \"float index\" 1.2\nNamedMaterial \"n\"\n" + std::string(kTri, std::strlen(kTri) - 1) + " \"rgb Kd\" [0 1 0] \"texture index\" \"df\" \"texture opacity\" \"ds\"\n"));
    scene("alpha and shadowalpha", world(std::string(kTri, std::strlen(kTri) - 1) + " \"texture alpha\" \"df\" \"texture shadowalpha\" \"cf\"\n" + std::string(kTri, std::strlen(kTri) - 1) + " \"texture alpha\" \"ds\" \"float alpha\" 0.5\n" +
                                         std::string(kTri, std::strlen(kTri) - 1) + " \"texture alpha\" \"nope\"\n" + std::string(kTri, std::strlen(kTri) - 1) + " \"texture shadowalpha\" \"un\"\n"));
    scene("materials and textures across AttributeBegin / AttributeEnd", world(std::string("AttributeBegin\nTexture \"cf\" \"float\" \"imagemap\" \"string filename\" \"") + kPng + "\"\nTexture \"local\" \"color\" \"constant\"\n" + material_line("matte", "\"texture sigma\" \"cf\" \"texture Kd\" \"local\"") + kTri +
                                                                               "AttributeEnd\n" + material_line("matte", "\"texture sigma\" \"cf\" \"texture Kd\" \"local\"") + kTri));
}

// after Texture "t": one material that uses the name as a spectrum, or one that uses it as a float
static const char* kUsers[2] = {"Material \"matte\" \"texture Kd\" \"t\"\n", "Material \"matte\" \"texture sigma\" \"t\"\n"};
static const char* kUserTag[2] = {" used as spectrum", " used as float"};

static void texture_sweep() {
    section("texture sweep: class x type x operand form");
    struct Class { const char* name; const char* extra; const char* operands[3]; };
    static const Class classes[] = {{"constant", "", {"value", nullptr, nullptr}}, {"scale", "", {"tex1", "tex2", "amount"}}, {"mix", "", {"tex1", "tex2", "amount"}}, {"imagemap", "\"string filename\" \"%PNG%\"", {nullptr, nullptr, nullptr}},
                                    {"checkerboard", "", {"tex1", "tex2", nullptr}}, {"checkerboard", "\"integer dimension\" 3", {"tex1", "tex2", nullptr}}, {"checkerboard", "\"integer dimension\" 4", {"tex1", nullptr, nullptr}},
                                    {"uv", "", {nullptr, nullptr, nullptr}}, {"bilerp", "", {"v00", "v11", nullptr}}, {"dots", "", {"inside", "outside", nullptr}}, {"fbm", "\"float roughness\" 0.6 \"integer octaves\" 3", {nullptr, nullptr, nullptr}},
                                    {"wrinkled", "\"float roughness\" 0.6", {nullptr, nullptr, nullptr}}, {"windy", "", {nullptr, nullptr, nullptr}}, {"marble", "\"float scale\" 2 \"float variation\" 0.3", {nullptr, nullptr, nullptr}},
                                    {"ptex", "", {nullptr, nullptr, nullptr}}};
    for (const Class& c : classes)
        for (const char* type : {"float", "color", "spectrum", "bogus"})
            for (int op = -1; op < 3; op++) {
                if (op >= 0 && !c.operands[op]) continue;
                for (const Way& w : kWays) {
                    if (op < 0 && &w != &kWays[0]) continue;   // no operand given: once
                    if (op >= 0 && &w == &kWays[0]) continue;
                    std::string extra = c.extra;
                    if (size_t p = extra.find("%PNG%"); p != std::string::npos) extra.replace(p, 5, kPng);
                    const std::string decl = std::string("Texture \"t\" \"") + type + "\" \"" + c.name + "\" " + extra + " " + (op >= 0 ? give(w, c.operands[op]) : std::string()) + "\n";
                    for (int u = 0; u < 2; u++)
                        scene(std::string(c.name) + (c.extra[0] == '"' && c.extra[1] == 'i' ? " dimension " + std::string(1, extra[extra.size() - 1]) : std::string()) + " " + type + " @ " + (op >= 0 ? std::string(c.operands[op]) + "=" + w.tag : std::string("plain")) + kUserTag[u],
                              world(decl + kUsers[u] + kTri));
                }
            }
}

static void texture_edges() {
    section("texture edges");
    const std::string png = std::string("\"string filename\" \"") + kPng + "\"";
    // the four mapping names and an unknown one; planar with and without v1 / v2
    for (const char* cls : {"imagemap", "checkerboard", "uv", "bilerp", "dots"})
        for (const char* mp : {"\"string mapping\" \"uv\" \"float uscale\" 2 \"float vdelta\" 0.5", "\"string mapping\" \"spherical\"", "\"string mapping\" \"cylindrical\"", "\"string mapping\" \"planar\"",
                               "\"string mapping\" \"planar\" \"vector v1\" [0 1 0] \"vector v2\" [0 0 1] \"float udelta\" 0.25 \"float vdelta\" 0.5", "\"string mapping\" \"planar\" \"vector v1\" [0 1]", "\"string mapping\" \"conformal\""})
            scene(std::string(cls) + " @ " + mp, world("Translate 1 2 3\nScale 2 2 2\nTexture \"t\" \"color\" \"" + std::string(cls) + "\" " + (std::string(cls) == "imagemap" ? png : std::string()) + " " + mp + "\n" + kUsers[0] + kTri));
    scene("3D textures take the CTM", world(std::string("Translate 1 2 3\nRotate 30 0 0 1\nTexture \"a\" \"float\" \"fbm\"\nTexture \"b\" \"float\" \"wrinkled\"\nTexture \"c\" \"float\" \"windy\"\nTexture \"d\" \"color\" \"marble\"\nTexture \"e\" \"color\" \"checkerboard\" \"integer dimension\" 3 \"texture tex1\" \"d\"\n"
                                            "Texture \"f\" \"float\" \"marble\"\nMaterial \"matte\" \"texture Kd\" \"e\" \"texture sigma\" \"a\" \"texture bumpmap\" \"b\"\n") + kTri));
    scene("checkerboard aamode", world(std::string("Texture \"a\" \"float\" \"checkerboard\" \"string aamode\" \"none\"\nTexture \"b\" \"float\" \"checkerboard\" \"string aamode\" \"supersample\"\nMaterial \"matte\" \"texture sigma\" \"b\" \"texture bumpmap\" \"a\"\n") + kTri));
    scene("Texture outside the world block", "Texture \"t\" \"float\" \"constant\"\nWorldBegin\n" + std::string(kUsers[1]) + kTri);
    // image files: missing, no name, and the mipmap cache (two key-changing and two key-preserving parameter sets)
    scene("imagemap of a missing file", world(std::string("Texture \"t\" \"color\" \"imagemap\" \"string filename\" \"tests/golden/ref_scenes/images/none.png\"\n") + kUsers[0] + kTri));
    scene("imagemap without a file name", world(std::string("Texture \"t\" \"color\" \"imagemap\"\n") + kUsers[0] + kTri));
    scene("imagemap of a file that is no image", world(std::string("Texture \"t\" \"color\" \"imagemap\" \"string filename\" \"tests/golden/ref_scenes/geometry/cube.pbrt\"\n") + kUsers[0] + kTri));
    for (const char* second : {"", "\"bool trilinear\" \"true\"", "\"string wrap\" \"clamp\"", "\"float scale\" 2", "\"bool gamma\" \"false\"", "\"float maxanisotropy\" 4", "\"float uscale\" 2 \"float vscale\" 3", "\"string mapping\" \"spherical\"", "\"string wrap\" \"repeat\" \"bool gamma\" \"true\""})
        for (const char* type : {"color", "float"})
            scene(std::string("mipmap cache: color imagemap, then ") + second + " @ " + type, world("Texture \"a\" \"color\" \"imagemap\" " + png + "\nTexture \"b\" \"" + type + "\" \"imagemap\" " + png + " " + second + "\nTexture \"c\" \"color\" \"imagemap\" " + png + "\n" +
                                                                                                   "Material \"plastic\" \"texture Kd\" \"a\" \"texture Ks\" \"c\" \"texture " + (std::string(type) == "float" ? "roughness" : "Kd") + "\" \"b\"\n" + kTri));
    // scale / mix: folded to constants, sent to the device, and with one operand that cannot be resolved after one that can
    for (const char* cls : {"scale", "mix"})
        for (const char* type : {"float", "color"}) {
            const bool fl = std::string(type) == "float";
            const std::string c = fl ? "cf" : "cs", d = fl ? "df" : "ds", other = fl ? "cs" : "cf";
            const char* lit = fl ? "\"float tex2\" 0.5" : "\"rgb tex2\" [0.5 0.25 0.125]";
            const std::string head = std::string("Texture \"t\" \"") + type + "\" \"" + cls + "\" ";
            const std::string tail = std::string("\n") + kUsers[fl ? 1 : 0] + kTri;
            scene(head + "@ constant x literal", world(head + "\"texture tex1\" \"" + c + "\" " + lit + tail));
            scene(head + "@ constant x constant, amount constant", world(head + "\"texture tex1\" \"" + c + "\" \"texture tex2\" \"" + c + "\" \"texture amount\" \"cf\"" + tail));
            scene(head + "@ literal amount", world(head + "\"texture tex1\" \"" + c + "\" " + lit + " \"float amount\" 0.25" + tail));
            scene(head + "@ device x literal", world(head + "\"texture tex1\" \"" + d + "\" " + lit + tail));
            scene(head + "@ constant x device, amount device", world(head + "\"texture tex1\" \"" + c + "\" \"texture tex2\" \"" + d + "\" \"texture amount\" \"df\"" + tail));
            scene(head + "@ constant x device, amount spectrum device", world(head + "\"texture tex1\" \"" + c + "\" \"texture tex2\" \"" + d + "\" \"texture amount\" \"ds\"" + tail));
            scene(head + "@ constant x device, amount unsupported", world(head + "\"texture tex1\" \"" + c + "\" \"texture tex2\" \"" + d + "\" \"texture amount\" \"un\"" + tail));
            scene(head + "@ constant x unsupported", world(head + "\"texture tex1\" \"" + c + "\" \"texture tex2\" \"un\"" + tail));
            scene(head + "@ constant x undeclared", world(head + "\"texture tex1\" \"" + c + "\" \"texture tex2\" \"nope\"" + tail));
            scene(head + "@ literal x other type's constant", world(head + lit + " \"texture tex1\" \"" + other + "\"" + tail));
            scene(head + "@ device x other type's device", world(head + "\"texture tex1\" \"" + d + "\" \"texture tex2\" \"" + (fl ? "ds" : "df") + "\"" + tail));
            scene(head + "@ a tree", world(std::string("Texture \"u\" \"") + type + "\" \"" + cls + "\" \"texture tex1\" \"" + d + "\" " + lit + "\n" + head + "\"texture tex1\" \"u\" \"texture tex2\" \"" + c + "\"" + tail));
        }
    // a name declared twice, over every ordered pair of kinds, then used as a spectrum and as a float
    struct Kind { const char* tag; std::string decl; };
    const Kind kinds[] = {{"float constant", "Texture \"t\" \"float\" \"constant\" \"float value\" 0.3\n"}, {"color constant", "Texture \"t\" \"color\" \"constant\" \"rgb value\" [0.2 0.4 0.6]\n"},
                          {"float device", "Texture \"t\" \"float\" \"imagemap\" " + png + "\n"}, {"color device", "Texture \"t\" \"color\" \"imagemap\" " + png + "\n"},
                          {"folded float scale", "Texture \"t\" \"float\" \"scale\" \"float tex1\" 0.5 \"float tex2\" 0.5\n"}, {"folded color mix", "Texture \"t\" \"color\" \"mix\" \"rgb tex1\" [1 0 0] \"rgb tex2\" [0 0 1]\n"},
                          {"unsupported", "Texture \"t\" \"float\" \"ptex\"\n"}, {"device float scale", "Texture \"t\" \"float\" \"scale\" \"texture tex1\" \"df\" \"float tex2\" 0.5\n"}};
    for (const Kind& a : kinds)
        for (const Kind& b : kinds)
            for (int u = 0; u < 2; u++) scene(std::string("redeclared: ") + a.tag + " @ then " + b.tag + kUserTag[u], world(a.decl + b.decl + kUsers[u] + kTri));
    // the same, with the name read as an operand of another texture and as a bump map
    for (const Kind& a : kinds)
        for (const Kind& b : kinds) {
            scene(std::string("redeclared, other uses: ") + a.tag + " @ then " + b.tag + " used as operands", world(a.decl + b.decl + "Texture \"f\" \"float\" \"scale\" \"texture tex1\" \"t\" \"texture tex2\" \"df\"\nTexture \"s\" \"color\" \"checkerboard\" \"texture tex1\" \"t\"\n"));
            scene(std::string("redeclared, other uses: ") + a.tag + " @ then " + b.tag + " used as bump map", world(a.decl + b.decl + "Material \"matte\" \"texture bumpmap\" \"t\"\n" + kTri));
        }
}

static void write_image_or_die(const std::string& path, int w, int h, unsigned seed) {   // small deterministic images for the textured scene text
    std::vector<float> rgb((size_t)w * h * 3);
    for (float& v : rgb) { seed = seed * 1664525u + 1013904223u; v = (float)(seed >> 24) / 255.0f; }
    std::string err;
    if (!pbrt_host::write_image(path, rgb.data(), w, h, err)) { std::fprintf(stderr, "cannot write %s: %s\n", path.c_str(), err.c_str()); std::exit(2); }
}

static void driver_texts() {
    section("the scene texts of tests/test_host_driver_gpu.py (image files written by this program)");
    const std::string quad = "[-1 -1 0 1 -1 0 1 1 0 -1 1 0]";
    const std::string mesh = "  Shape \"trianglemesh\" \"integer indices\" [0 1 2 0 2 3] \"point P\" " + quad;
    scene("materials in a scene file",
          "LookAt 0 -5 2  0 0 0.4  0 0 1\nCamera \"perspective\" \"float fov\" 50\nFilm \"image\" \"integer xresolution\" 36 \"integer yresolution\" 28 \"string filename\" \"m.pfm\"\nSampler \"halton\" \"integer pixelsamples\" 8\n"
          "Integrator \"path\" \"integer maxdepth\" 6\nWorldBegin\nLightSource \"infinite\" \"rgb L\" [0.8 0.9 1.0]\nLightSource \"distant\" \"point from\" [1 -1 2] \"point to\" [0 0 0] \"rgb L\" [2 2 2]\n"
          "MakeNamedMaterial \"gold\" \"string type\" \"metal\" \"rgb eta\" [0.14 0.37 1.44] \"rgb k\" [3.98 2.38 1.6] \"float roughness\" 0.1\n"
          "MakeNamedMaterial \"wet\" \"string type\" \"uber\" \"rgb Kd\" [0.2 0.3 0.2] \"rgb Ks\" [0.3 0.3 0.3] \"rgb Kr\" [0.1 0.1 0.1] \"float index\" 1.33 \"rgb opacity\" [0.8 0.8 0.8]\n"
          "AttributeBegin\n  Material \"plastic\" \"rgb Kd\" [0.4 0.4 0.5] \"float roughness\" 0.2\n  Scale 2.5 2.5 1\n" + mesh + "\nAttributeEnd\n"
          "AttributeBegin\n  NamedMaterial \"gold\"\n  Translate -1.2 0.3 0.6\n  Rotate 60 1 0 0\n  Scale 0.6 0.6 0.6\n" + mesh + "\nAttributeEnd\n"
          "AttributeBegin\n  Material \"glass\" \"float eta\" 1.4\n  Translate 0 -0.4 0.7\n  Rotate 75 1 0 0\n  Scale 0.5 0.5 0.5\n" + mesh + "\n  Translate 0 0 -0.6\n" + mesh + " \"float uroughness\" 0.2 \"float vroughness\" 0.2\nAttributeEnd\n"
          "AttributeBegin\n  NamedMaterial \"wet\"\n  Translate 1.3 0.2 0.5\n  Rotate 80 1 0.2 0\n  Scale 0.6 0.6 0.6\n" + mesh + "\n  Material \"mirror\"\n  Translate 0 0 -0.8\n" + mesh + " \"rgb Kr\" [0.5 0.6 0.7]\nAttributeEnd\nWorldEnd\n");
    scene("mix, substrate, translucent and folded textures in a scene file",
          "LookAt 0 -5 2  0 0 0.4  0 0 1\nCamera \"perspective\" \"float fov\" 50\nFilm \"image\" \"integer xresolution\" 32 \"integer yresolution\" 24 \"string filename\" \"x.pfm\"\nSampler \"halton\" \"integer pixelsamples\" 8\n"
          "Integrator \"path\" \"integer maxdepth\" 5\nWorldBegin\nLightSource \"infinite\" \"rgb L\" [0.8 0.9 1.0]\nLightSource \"spot\" \"point from\" [0 -2 3] \"point to\" [0 0 0] \"rgb I\" [30 30 30] \"float coneangle\" 40 \"float conedeltaangle\" 15\n"
          "Texture \"a\" \"color\" \"constant\" \"rgb value\" [0.8 0.6 0.4]\nTexture \"b\" \"color\" \"constant\" \"rgb value\" [0.5 0.5 1.0]\nTexture \"ab\" \"color\" \"scale\" \"texture tex1\" \"a\" \"texture tex2\" \"b\"\n"
          "Texture \"half\" \"float\" \"constant\" \"float value\" 0.25\nTexture \"blend\" \"color\" \"mix\" \"texture tex1\" \"a\" \"rgb tex2\" [0.1 0.9 0.1] \"texture amount\" \"half\"\n"
          "MakeNamedMaterial \"base\" \"string type\" \"matte\" \"texture Kd\" \"ab\"\nMakeNamedMaterial \"coat\" \"string type\" \"mirror\" \"rgb Kr\" [0.8 0.8 0.8]\n"
          "MakeNamedMaterial \"both\" \"string type\" \"mix\" \"string namedmaterial1\" \"base\" \"string namedmaterial2\" \"coat\" \"rgb amount\" [0.6 0.6 0.6]\n"
          "AttributeBegin\n  Material \"substrate\" \"texture Kd\" \"blend\" \"rgb Ks\" [0.2 0.2 0.2] \"float uroughness\" 0.05\n  Scale 2.5 2.5 1\n" + mesh + "\nAttributeEnd\n"
          "AttributeBegin\n  NamedMaterial \"both\"\n  Translate -1.0 0.3 0.7\n  Rotate 70 1 0 0\n  Scale 0.7 0.7 0.7\n" + mesh + "\nAttributeEnd\n"
          "AttributeBegin\n  Material \"translucent\" \"rgb Kd\" [0.5 0.5 0.3] \"rgb transmit\" [0.7 0.7 0.7]\n  Translate 1.0 0 0.8\n  Rotate 85 1 0 0.3\n  Scale 0.7 0.7 0.7\n" + mesh + "\nAttributeEnd\nWorldEnd\n");
    write_image_or_die(g_tmp + "/a.png", 40, 24, 12u); write_image_or_die(g_tmp + "/m.tga", 16, 16, 13u); write_image_or_die(g_tmp + "/h.pfm", 8, 8, 14u); write_image_or_die(g_tmp + "/sky.pfm", 16, 8, 15u);
    scene("the textured scene file",
          "LookAt 0 -6 1.5  0 0 0.5  0 0 1\nCamera \"perspective\" \"float fov\" [40]\nFilm \"image\" \"integer xresolution\" [48] \"integer yresolution\" [48] \"string filename\" \"tex.pfm\"\nSampler \"halton\" \"integer pixelsamples\" 4\nPixelFilter \"box\"\n"
          "Integrator \"path\" \"integer maxdepth\" 3 \"string lightsamplestrategy\" \"uniform\"\nWorldBegin\nAttributeBegin\n  Rotate 40 0 0 1\n  LightSource \"infinite\" \"rgb L\" [1 0.9 0.8] \"rgb scale\" [0.5 0.5 0.5] \"string mapname\" \"sky.pfm\"\nAttributeEnd\n"
          "Texture \"wood\" \"color\" \"imagemap\" \"string filename\" \"a.png\"\nTexture \"tint\" \"color\" \"scale\" \"texture tex1\" \"wood\" \"rgb tex2\" [0.9 0.6 0.4]\n"
          "Texture \"amt\" \"float\" \"imagemap\" \"string filename\" \"m.tga\" \"bool trilinear\" \"true\" \"string wrap\" \"clamp\" \"bool gamma\" \"false\"\n"
          "Texture \"blend\" \"color\" \"mix\" \"texture tex1\" \"tint\" \"rgb tex2\" [0.1 0.2 0.8] \"texture amount\" \"amt\"\nTexture \"cut\" \"float\" \"checkerboard\" \"float uscale\" 4 \"float vscale\" 4 \"string aamode\" \"none\"\n"
          "Texture \"hdr\" \"color\" \"imagemap\" \"string filename\" \"h.pfm\" \"float scale\" 0.5 \"float uscale\" 2 \"float vscale\" 2 \"string wrap\" \"black\"\nMaterial \"matte\" \"texture Kd\" \"blend\"\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2 0 2 3] \"point P\" [-4 -4 0 4 -4 0 4 4 0 -4 4 0] \"float uv\" [0 0 2 0 2 2 0 2]\nMaterial \"matte\" \"texture Kd\" \"hdr\" \"float sigma\" 20\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2 0 2 3] \"point P\" [-2 3 0 2 3 0 2 3 2.5 -2 3 2.5] \"float st\" [0 0 1 0 1 1 0 1] \"texture alpha\" \"amt\" \"texture shadowalpha\" \"cut\"\n"
          "Texture \"bumps\" \"float\" \"scale\" \"texture tex1\" \"amt\" \"float tex2\" 0.05\nMaterial \"plastic\" \"texture Kd\" \"wood\" \"texture Ks\" \"tint\" \"float roughness\" 0.05 \"texture bumpmap\" \"bumps\"\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2] \"point P\" [-3 1 0.01  -1 1 0.01  -2 2.5 1.5] \"float uv\" [0 0 1 0 0.5 1]\n"
          "MakeNamedMaterial \"glossy\" \"string type\" \"substrate\" \"texture Kd\" \"blend\" \"rgb Ks\" [0.05 0.05 0.05] \"float uroughness\" 0.1 \"float vroughness\" 0.2\nNamedMaterial \"glossy\"\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2] \"point P\" [1 1 0.01  3 1 0.01  2 2.5 1.5] \"float uv\" [0 0 1 0 0.5 1]\nMaterial \"mirror\" \"texture Kr\" \"wood\"\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2] \"point P\" [-1 -1 0.01  1 -1 0.01  0 0 1.2]\nTexture \"checks\" \"color\" \"checkerboard\" \"float uscale\" 6 \"float vscale\" 6 \"texture tex1\" \"wood\" \"rgb tex2\" [0.1 0.1 0.1]\n"
          "Texture \"spots\" \"color\" \"dots\" \"float uscale\" 3 \"float vscale\" 3 \"texture inside\" \"checks\" \"rgb outside\" [0.7 0.2 0.2]\nMaterial \"matte\" \"texture Kd\" \"spots\"\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2 0 2 3] \"point P\" [-4 -4 0.005  -2 -4 0.005  -2 -2 0.005  -4 -2 0.005] \"float uv\" [0 0 1 0 1 1 0 1]\nTransformBegin\n  Scale 2 2 2\n  Rotate 20 0 0 1\n"
          "  Texture \"stone\" \"color\" \"marble\" \"float scale\" 2 \"float variation\" 0.3 \"integer octaves\" 6\n  Texture \"cells\" \"color\" \"checkerboard\" \"integer dimension\" 3 \"texture tex1\" \"stone\" \"rgb tex2\" [0.05 0.3 0.05]\nTransformEnd\n"
          "Material \"matte\" \"texture Kd\" \"cells\"\nShape \"trianglemesh\" \"integer indices\" [0 1 2 0 2 3] \"point P\" [2 -4 0.005  4 -4 0.005  4 -2 0.005  2 -2 0.005]\n"
          "Material \"translucent\" \"texture Kd\" \"wood\" \"rgb Ks\" [0.1 0.1 0.1] \"rgb reflect\" [0.4 0.4 0.4] \"rgb transmit\" [0.6 0.6 0.6] \"texture roughness\" \"amt\"\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2] \"point P\" [-1.8 -2.5 0.3  -0.8 -2.5 0.3  -1.3 -2.5 1.3] \"float uv\" [0 0 1 0 0.5 1]\nMakeNamedMaterial \"m1\" \"string type\" \"plastic\" \"texture Kd\" \"wood\" \"rgb Ks\" [0.2 0.2 0.2]\n"
          "MakeNamedMaterial \"m2\" \"string type\" \"matte\" \"texture Kd\" \"spots\"\nMaterial \"mix\" \"string namedmaterial1\" \"m1\" \"string namedmaterial2\" \"m2\" \"rgb amount\" [0.3 0.3 0.3]\n"
          "Shape \"trianglemesh\" \"integer indices\" [0 1 2] \"point P\" [0.8 -2.5 0.3  1.8 -2.5 0.3  1.3 -2.5 1.3] \"float uv\" [0 0 1 0 0.5 1]\nWorldEnd\n",
          false, g_tmp);
}

int main() {
    char tmpl[] = "/tmp/front_end_calls_XXXXXX";
    if (!mkdtemp(tmpl)) { std::perror("mkdtemp"); return 2; }
    g_tmp = tmpl;
    fixtures();
    material_sweep();
    material_edges();
    texture_sweep();
    texture_edges();
    driver_texts();
    write_records_and_lines();
    for (const char* f : {"/out.pfm", "/a.png", "/m.tga", "/h.pfm", "/sky.pfm"}) std::remove((g_tmp + f).c_str());
    rmdir(g_tmp.c_str());
    std::fprintf(stderr, "front_end_calls_check: done\n");
    return 0;
}
