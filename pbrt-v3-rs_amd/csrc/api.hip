// C ABI of include/pbrt_hip.h: scene capture, BVH build, device upload, batch traversal entry points.
// (The render entry points live in wavefront.hip.)  No CPU fallback exists anywhere in this library: without a
// gfx950 device pbrt_hip_scene_create returns NULL and every compute entry point fails with PBRT_HIP_ERR_NO_DEVICE.
#include "host_math.h"
#include "scene_host.h"
#include "curve_host.h"
#include "loopsubdiv_device.h"
#include "traverse.h"
#include "texture.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>

static std::string g_last_error;
static std::mutex g_err_mu;

namespace phost {

int set_err(PbrtHipScene* s, int code, const std::string& msg) {
    if (s) s->err = msg;
    else { std::lock_guard<std::mutex> g(g_err_mu); g_last_error = msg; }
    return code;
}
int hip_fail(PbrtHipScene* s, hipError_t e, const char* what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return set_err(s, e == hipErrorOutOfMemory ? PBRT_HIP_ERR_OOM : PBRT_HIP_ERR_DEVICE, m);
}
int ensure_buf(PbrtHipScene* s, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return PBRT_HIP_OK;
    if (b.p) { PH_CHECK(s, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    if (bytes == 0) bytes = 16;
    PH_CHECK(s, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    if (bytes <= 4096) PH_CHECK(s, hipMemset(b.p, 0, bytes));  // flags / counters start cleared
    return PBRT_HIP_OK;
}

template <class T> static int upload_array(PbrtHipScene* s, const T* v, size_t n, const T** out) {
    *out = nullptr;
    if (n == 0) return PBRT_HIP_OK;
    void* d = nullptr;
    PH_CHECK(s, hipMalloc(&d, n * sizeof(T)));
    s->owned.push_back(d);
    PH_CHECK(s, hipMemcpyAsync(d, v, n * sizeof(T), hipMemcpyHostToDevice, s->stream));
    *out = reinterpret_cast<const T*>(d);
    return PBRT_HIP_OK;
}
template <class T> static int upload_vec(PbrtHipScene* s, const std::vector<T>& v, const T** out) { return upload_array(s, v.data(), v.size(), out); }

void free_tree_dev(DeviceTree& t) { (void)hipFree(t.nodes); (void)hipFree(t.tris); t = DeviceTree(); }   // (freeing null is no error)

static void free_owned(PbrtHipScene* s) {
    for (void* p : s->owned) (void)hipFree(p);
    s->owned.clear();
    s->uploaded = false;
    s->light_strategy_uploaded = -1;
}

static hm::HaltonTables& halton_tables() {
    static hm::HaltonTables t;
    static std::once_flag once;
    std::call_once(once, []() { t.build(); });
    return t;
}

// Scenes with object instances, once per upload: every instance's leaf record receives what a ray entering it reads (scene_types.h, InstRec) and the hints that let the traversal kernel
// fetch the transform together with the record.  In place on the device arrays (device-built trees never visit the host); idempotent.
__global__ void patch_inst_records_kernel(TriRec* tris, uint32_t n_top, const InstRec* inst, float* extra) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_top) return;
    uint32_t f = tris[i].flags & ~PH_TRI_NEXT_INST;
    if (!(f & PH_TRI_LAST) && i + 1u < n_top && (tris[i + 1u].flags & PH_TRI_INSTANCE)) f |= PH_TRI_NEXT_INST;   // (this kernel never changes a PH_TRI_INSTANCE bit: no race with the neighbour's thread)
    if (f & PH_TRI_INSTANCE) {
        const InstRec& I = inst[tris[i].prim];
        const bool general = !(I.w2i[12] == 0.0f && I.w2i[13] == 0.0f && I.w2i[14] == 0.0f && I.w2i[15] == 1.0f);
        for (int k = 0; k < 3; k++) { tris[i].p0[k] = I.lo[k]; tris[i].p1[k] = I.hi[k]; }
        tris[i].p2[0] = __uint_as_float(I.root_ref); tris[i].p2[1] = __uint_as_float(I.flags | (general ? PH_INST_GENERAL : 0u)); tris[i].p2[2] = 0.0f;
        for (int k = 0; k < 12; k++) extra[12 * (size_t)i + k] = I.w2i[k];
    }
    tris[i].flags = f;
}
__global__ void patch_leaf_refs_kernel(Node64* nodes, uint32_t n_nodes, const TriRec* tris, uint32_t n_top) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    uint32_t c[2] = {nodes[i].c0, nodes[i].c1};
    for (int k = 0; k < 2; k++)
        if ((c[k] & PH_LEAF_BIT) && c[k] < PH_NEED_POP) {
            const uint32_t t = c[k] & ~(PH_LEAF_BIT | PH_LEAF_INST_HINT);
            c[k] = PH_LEAF_BIT | t | ((t < n_top && (tris[t].flags & PH_TRI_INSTANCE)) ? PH_LEAF_INST_HINT : 0u);
        }
    nodes[i].c0 = c[0]; nodes[i].c1 = c[1];
}

int upload_scene(PbrtHipScene* s) {
    if (s->uploaded) return PBRT_HIP_OK;
    free_owned(s);
    DeviceScene& d = s->ds;
    std::memset(&d, 0, sizeof(d));
    int rc;
    if (s->accel_on_device()) { d.nodes = s->accel_nodes(); d.tris = s->accel_records(); }   // built here, never left
    else {
        if ((rc = upload_array(s, s->accel_nodes(), s->accel_n_nodes(), &d.nodes))) return rc;
        if ((rc = upload_array(s, s->accel_records(), s->accel_n_records(), &d.tris))) return rc;
    }
    d.root_ref = s->bvh.root_ref;
    d.n_tris = (uint32_t)(s->idx.size() / 3);
    for (int k = 0; k < 3; k++) { d.root_lo[k] = s->bvh.root_lo[k]; d.root_hi[k] = s->bvh.root_hi[k]; d.world_center[k] = s->world_center[k]; }
    d.world_radius = s->world_radius;
    if ((rc = upload_vec(s, s->P, &d.P))) return rc;
    if (s->any_n && (rc = upload_vec(s, s->N, &d.N))) return rc;
    if (s->any_s && (rc = upload_vec(s, s->S, &d.S))) return rc;
    if (s->any_uv && (rc = upload_vec(s, s->UV, &d.UV))) return rc;
    if ((rc = upload_vec(s, s->idx, &d.idx))) return rc;
    if ((rc = upload_vec(s, s->tri_mesh, &d.tri_mesh))) return rc;
    if ((rc = upload_vec(s, s->tri_flags, &d.tri_flags))) return rc;
    if (s->emission_only.empty()) { if ((rc = upload_vec(s, s->meshes, &d.meshes))) return rc; }
    else {   // emission-only area lights sit behind the scene's lights on the device: their meshes point there
        std::vector<MeshRec> meshes(s->meshes);
        for (MeshRec& m : meshes) if (m.first_light <= -2) m.first_light = (int32_t)(s->lights.size() + (size_t)(-2 - m.first_light));
        if ((rc = upload_vec(s, meshes, &d.meshes))) return rc;
    }
    std::vector<MaterialRec> materials; std::vector<LobeRec> lobes;   // the materials' lists one after the other, with what the texture pass has to hand to the shade pass
    layout_lobe_pool(s->mats, materials, lobes);
    {
        s->alpha_lean = s->alpha_textures;
        for (const MeshRec& m : s->meshes)
            for (uint32_t t1 : {m.alpha_tex1, m.shadow_alpha_tex1})
                if (t1 && !tex_prog_is_simple(s->textures[t1 - 1u].prog)) s->alpha_lean = false;
        s->simple_textures = true;
        for (const PbrtHipScene::TextureHost& t : s->textures)
            if (!tex_prog_is_simple(t.prog)) s->simple_textures = false;
    }
    if ((rc = upload_vec(s, materials, &d.materials))) return rc;
    if ((rc = upload_vec(s, lobes, &d.lobes))) return rc;
    {   // keys of the shade-side work queues (matsort.h): materials the texture pass has work for first, then the others, then "emission only" and "no new vertex"
        const uint32_t kMaxTex = 500u, kMaxPlain = 500u;
        std::vector<uint16_t> key(std::max<size_t>(materials.size(), 1), 0);
        uint32_t n_tex = 0, n_plain = 0;
        for (const MaterialRec& m : materials) if (!m.none && (m.textured || m.bump_tex1)) n_tex++;
        const uint32_t T = std::min(n_tex, kMaxTex);
        uint32_t jt = 0, jp = 0;
        for (size_t i = 0; i < materials.size(); i++) {
            const MaterialRec& m = materials[i];
            if (!m.none && (m.textured || m.bump_tex1)) key[i] = (uint16_t)std::min(jt++, kMaxTex - 1u);
            else { key[i] = (uint16_t)(T + std::min(jp++, kMaxPlain - 1u)); n_plain++; }
        }
        const uint32_t U = std::min(n_plain, kMaxPlain);
        if ((rc = upload_vec(s, key, &d.mat_key))) return rc;
        d.ms_tex_keys = T; d.ms_key_emit = T + U; d.ms_key_idle = T + U + 1u;
    }
    if (!s->textures.empty() || !s->mipmaps.empty()) {   // MIPMaps also belong to lights (radiance map, projection image, goniometric diagram)
        std::vector<TexRec> recs; std::vector<TexOp> ops;
        for (const PbrtHipScene::TextureHost& t : s->textures) {
            recs.push_back(TexRec{(uint32_t)ops.size(), (uint32_t)t.prog.size()});
            ops.insert(ops.end(), t.prog.begin(), t.prog.end());
        }
        std::vector<float> lut(PH_EWA_LUT_SIZE);
        for (int i = 0; i < PH_EWA_LUT_SIZE; i++) {  // mipmap/mod.rs:168-174 (host expf, as in the reference)
            const float r2 = (float)i / (float)(PH_EWA_LUT_SIZE - 1);
            lut[(size_t)i] = std::exp(-2.0f * r2) - std::exp(-2.0f);
        }
        if ((rc = upload_vec(s, recs, &d.textures))) return rc;
        if ((rc = upload_vec(s, ops, &d.tex_ops))) return rc;
        if ((rc = upload_vec(s, s->mipmaps, &d.mipmaps))) return rc;
        if ((rc = upload_vec(s, s->texels, &d.texels))) return rc;
        if ((rc = upload_vec(s, lut, &d.ewa_lut))) return rc;
    }
    s->lights_infinite = s->lights_delta = false; s->lights_area = !s->emission_only.empty();
    for (LightRec& l : s->lights) {   // which kinds of light the shade pass will meet (shade_shapes.h), and whether light_pdf_li needs phi for this light
        if (l.type == PH_L_INFINITE) s->lights_infinite = true; else if (l.type == PH_L_AREA) s->lights_area = true; else s->lights_delta = true;
        if (l.type == PH_L_INFINITE) l.cond_flat = (!l.map_mip1 && std::memcmp(&l.cond_func[0], &l.cond_func[1], 4) == 0 && std::memcmp(&l.cond_func[2], &l.cond_func[3], 4) == 0) ? 1 : 0;
    }
    if (s->emission_only.empty()) { if ((rc = upload_vec(s, s->lights, &d.lights))) return rc; }
    else {
        std::vector<LightRec> all(s->lights);
        all.insert(all.end(), s->emission_only.begin(), s->emission_only.end());
        if ((rc = upload_vec(s, all, &d.lights))) return rc;
    }
    if ((rc = upload_vec(s, s->light_dist, &d.light_dist))) return rc;
    d.n_lights = (uint32_t)s->lights.size();
    if ((rc = upload_vec(s, s->infinite_lights, &d.infinite_lights))) return rc;
    d.n_infinite = (uint32_t)s->infinite_lights.size();
    if ((rc = upload_vec(s, s->inst_recs, &d.instances))) return rc;
    if (s->curves.empty()) { if ((rc = upload_vec(s, s->quadrics, &d.quadrics))) return rc; }
    else {   // the CurveRecs travel behind the last QuadricRec (scene_types.h: ph_curve_rec), in whole QuadricRec slots
        std::vector<QuadricRec> all(s->quadrics);
        for (QuadricRec& q : all) q.curves_at = (uint32_t)s->quadrics.size();
        all.resize(s->quadrics.size() + (s->curves.size() * sizeof(CurveRec) + sizeof(QuadricRec) - 1) / sizeof(QuadricRec));
        std::memcpy(static_cast<void*>(all.data() + s->quadrics.size()), s->curves.data(), s->curves.size() * sizeof(CurveRec));
        if ((rc = upload_vec(s, all, &d.quadrics))) return rc;
    }
    d.n_instances = (uint32_t)s->inst_recs.size();
    // a forest whose trees are all single leaves has no interior node at all (d.nodes == nullptr): the records still need their bounds / root / transform
    if (!s->inst_recs.empty() && !s->top_items.empty() && d.tris) {   // instance leaf records + hints (patch_inst_records_kernel)
        const uint32_t n_top = (uint32_t)s->top_items.size();
        const uint32_t n_nodes = (uint32_t)s->accel_n_nodes();
        void* extra = nullptr;
        PH_CHECK(s, hipMalloc(&extra, (size_t)n_top * 48)); s->owned.push_back(extra);
        hipLaunchKernelGGL(patch_inst_records_kernel, dim3((n_top + 255u) / 256u), dim3(256), 0, s->stream, const_cast<TriRec*>(d.tris), n_top, d.instances, static_cast<float*>(extra));
        if (n_nodes) hipLaunchKernelGGL(patch_leaf_refs_kernel, dim3((n_nodes + 255u) / 256u), dim3(256), 0, s->stream, const_cast<Node64*>(d.nodes), n_nodes, d.tris, n_top);
        PH_CHECK(s, hipGetLastError());
        d.inst_extra = static_cast<const float*>(extra);
    }
    hm::HaltonTables& ht = halton_tables();
    if ((rc = upload_vec(s, ht.perms, &d.halton_perms))) return rc;
    if ((rc = upload_vec(s, ht.primes, &d.primes))) return rc;
    if ((rc = upload_vec(s, ht.prime_sums, &d.prime_sums))) return rc;
    if ((rc = upload_vec(s, ht.magic, &d.prime_magic))) return rc;
    if ((rc = upload_vec(s, s->sobol32, &d.sobol32))) return rc;
    if ((rc = upload_vec(s, s->vdc, &d.vdc))) return rc;
    if ((rc = upload_vec(s, s->vdc_inv, &d.vdc_inv))) return rc;
    {   // device-resident copy of the struct itself (DeviceScene::self), for out-of-line device functions
        void* dself = nullptr;
        PH_CHECK(s, hipMalloc(&dself, sizeof(DeviceScene)));
        s->owned.push_back(dself);
        d.self = reinterpret_cast<const DeviceScene*>(dself);
        PH_CHECK(s, hipMemcpyAsync(dself, &d, sizeof(DeviceScene), hipMemcpyHostToDevice, s->stream));
    }
    PH_CHECK(s, hipStreamSynchronize(s->stream));
    s->uploaded = true;
    return PBRT_HIP_OK;
}

// Light::power().y() per light -> Distribution1D (core/src/integrator/common.rs:304-311); uniform = all ones
// (core/src/light_distrib/uniform.rs:24-31).  create_light_sample_distribution forces Uniform for a single light.
int upload_light_distribution(PbrtHipScene* s, int light_strategy) {
    const size_t n = s->lights.size();
    int strat = (n == 1) ? 0 : light_strategy;
    if (s->light_strategy_uploaded == strat) return PBRT_HIP_OK;
    std::vector<float> f(n, 1.0f), cdf;
    float func_int = 0.0f;
    if (strat == 1) {
        const float wr = s->world_radius;
        for (size_t i = 0; i < n; i++) {
            const LightRec& l = s->lights[i];
            float p[3];
            for (int c = 0; c < 3; c++) {
                switch (l.type) {
                case PH_L_INFINITE: {  // infinite.rs:176-183: PI * r * r * lookup_triangle((.5,.5), .5)
                    if (l.map_mip1) { float t[3]; hmip_lookup_triangle(s, s->mipmaps[l.map_mip1 - 1u], 0.5f, 0.5f, 0.5f, t); p[c] = hm::kPi * wr * wr * t[c]; break; }
                    // 1x1 MIPMap::triangle at st=(0.5,0.5): s = 0, ds = 0 -> tx*1*1 + tx*1*0 + tx*0*1 + tx*0*0
                    float tx = l.L[c];
                    float v = tx * (1.0f - 0.0f) * (1.0f - 0.0f) + tx * (1.0f - 0.0f) * 0.0f + tx * 0.0f * (1.0f - 0.0f) + tx * 0.0f * 0.0f;
                    p[c] = hm::kPi * wr * wr * v;
                    break;
                }
                case PH_L_DISTANT: p[c] = l.L[c] * hm::kPi * wr * wr; break;                       // distant.rs:98-101
                case PH_L_POINT: p[c] = (hm::kPi * 4.0f) * l.L[c]; break;                          // point.rs:95-97
                case PH_L_PROJECTION: case PH_L_GONIO: {   // projection.rs:193-203: spectrum * I * TWO_PI * (1 - cos_total_width); goniometric.rs:115-126: FOUR_PI * I * spectrum
                    float t[3] = {1.0f, 1.0f, 1.0f};
                    if (l.map_mip1) hmip_lookup_triangle(s, s->mipmaps[l.map_mip1 - 1u], 0.5f, 0.5f, 0.5f, t);
                    p[c] = l.type == PH_L_PROJECTION ? t[c] * l.L[c] * (2.0f * hm::kPi) * (1.0f - l.cos_total_width) : (hm::kPi * 4.0f) * l.L[c] * t[c];
                    break;
                }
                case PH_L_SPOT: p[c] = l.L[c] * (2.0f * hm::kPi) * (1.0f - 0.5f * (l.cos_falloff_start + l.cos_total_width)); break;  // spot.rs:86-88
                default: p[c] = (l.two_sided ? 2.0f : 1.0f) * l.L[c] * l.area * hm::kPi; break;    // diffuse.rs:131-134
                }
            }
            f[i] = 0.212671f * p[0] + 0.715160f * p[1] + 0.072169f * p[2];
        }
    }
    if (n) hm::distribution1d(f, cdf, func_int);
    int rc;
    if ((rc = ensure_buf(s, s->d_ld_func, std::max<size_t>(n, 1) * 4))) return rc;
    if ((rc = ensure_buf(s, s->d_ld_cdf, (n + 1) * 4))) return rc;
    if (n) {
        PH_CHECK(s, hipMemcpy(s->d_ld_func.p, f.data(), n * 4, hipMemcpyHostToDevice));
        PH_CHECK(s, hipMemcpy(s->d_ld_cdf.p, cdf.data(), (n + 1) * 4, hipMemcpyHostToDevice));
    }
    s->ds.ld_func = (const float*)s->d_ld_func.p; s->ds.ld_cdf = (const float*)s->d_ld_cdf.p; s->ds.ld_func_int = func_int;
    s->light_strategy_uploaded = strat;
    return PBRT_HIP_OK;
}

int ensure_traversal_workspace(PbrtHipScene* s) {
    if (!s->trav_blocks) {
        hipDeviceProp_t prop;
        PH_CHECK(s, hipGetDeviceProperties(&prop, s->device));
        // EVERY shape launches the grid the flat scenes' mixed kernel keeps resident, at most its 6 waves per SIMD — also the shapes that fit fewer blocks per CU
        int per_cu = 0;
        PH_CHECK(s, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ph::traverse_kernel<ph::ShapeFlat, ph::TRAV_MIXED>, PH_TRAV_BLOCK, 0));
        per_cu = std::max(std::min(per_cu, ph::ShapeFlat::wpe), 1);
        s->trav_blocks = (uint32_t)(prop.multiProcessorCount * per_cu);
    }
    const uint32_t total_threads = s->trav_blocks * PH_TRAV_BLOCK;
    int rc;
    if ((rc = ensure_buf(s, s->d_counter, 64))) return rc;
    if ((rc = ensure_buf(s, s->d_error, 64))) return rc;
    if ((rc = ensure_buf(s, s->d_counts, 64 + 36 * 8))) return rc;
    const bool inst = !s->inst_recs.empty();
    if ((rc = ensure_buf(s, s->d_spill, (size_t)(ph::trav_stack_cap(inst) - ph::TravShapes::spill_lds_depth(inst)) * total_threads * sizeof(uint2)))) return rc;
    return PBRT_HIP_OK;
}

// The traversal kernels' error flag, read once the stream has drained and cleared for the next call: shared by the ray batches below and the two render drivers.
int traversal_overflow_check(PbrtHipScene* s) {
    uint32_t flag = 0;
    PH_CHECK(s, hipMemcpy(&flag, s->d_error.p, 4, hipMemcpyDeviceToHost));
    if (flag) {
        (void)hipMemset(s->d_error.p, 0, 4);
        return set_err(s, PBRT_HIP_ERR_DEVICE, "traversal stack exceeded 64 entries (the reference panics here, bvh/mod.rs:185)");
    }
    return PBRT_HIP_OK;
}

// One traversal kernel shape, launched for mode 0 closest hit, 1 any hit or 2 both queues in one launch (ph::TravMode)
template <class Shape>
static void launch_traverse_shape(PbrtHipScene* s, int mode, uint32_t blocks, const ph::TravParams& p) {
    const dim3 g(blocks), b(PH_TRAV_BLOCK);
    if (mode == ph::TRAV_MIXED) hipLaunchKernelGGL((ph::traverse_kernel<Shape, ph::TRAV_MIXED>), g, b, 0, s->stream, s->ds, p);
    else if (mode == ph::TRAV_ANY) hipLaunchKernelGGL((ph::traverse_kernel<Shape, ph::TRAV_ANY>), g, b, 0, s->stream, s->ds, p);
    else hipLaunchKernelGGL((ph::traverse_kernel<Shape, ph::TRAV_CLOSEST>), g, b, 0, s->stream, s->ds, p);
}
// Row `shape` of the table (ph::pick_shape)
template <class... S>
static void dispatch_traverse_shape(ph::ShapeTable<S...>, int shape, PbrtHipScene* s, int mode, uint32_t blocks, const ph::TravParams& p) {
    static constexpr void (*launchers[])(PbrtHipScene*, int, uint32_t, const ph::TravParams&) = {&launch_traverse_shape<S>...};
    launchers[shape](s, mode, blocks, p);
}

// p.spill / total_threads / error_flag / counts are filled here.  mode: as launch_traverse_shape's.  The shape follows the scene (traverse.h, pick_shape).
void launch_traverse_kernel(PbrtHipScene* s, int mode, uint32_t blocks, const ph::TravParams& p_in) {
    ph::TravParams p = p_in;
    p.spill = (uint2*)s->d_spill.p; p.total_threads = s->trav_blocks * PH_TRAV_BLOCK; p.error_flag = (uint32_t*)s->d_error.p;
    p.counts = (unsigned long long*)s->d_counts.p;
#if PH_PHASE_CLOCK
    p.phase = (unsigned long long*)s->d_counts.p + 8;   // (the measurement build's phase tallies sit behind the eight counters)
#endif
    p.batch = PH_BATCH;
    const int alpha = !s->alpha_textures ? 0 : s->alpha_lean ? 1 : 2;
    dispatch_traverse_shape(ph::TravShapes{}, ph::pick_shape(!s->inst_recs.empty(), alpha, !s->quadrics.empty(), s->count_traversal), s, mode, blocks, p);
}

int launch_traverse(PbrtHipScene* s, bool anyhit, const void* d_rays, void* d_out, uint32_t n, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n == 0) return PBRT_HIP_OK;
    int rc;
    if ((rc = ensure_traversal_workspace(s))) return rc;
    // fewer rays than resident lanes: shrink the grid so idle waves exit immediately
    const uint32_t blocks = std::min<uint32_t>(s->trav_blocks, (n + PH_TRAV_BLOCK - 1) / PH_TRAV_BLOCK);
    PH_CHECK(s, hipMemsetAsync(s->d_counter.p, 0, 4, s->stream));
    ph::TravParams p{};
    p.rays = (const ph::RayIn*)d_rays; p.out = d_out; p.n = n; p.n_ptr = nullptr; p.counter = (uint32_t*)s->d_counter.p;
    if (kernel_ms) PH_CHECK(s, hipEventRecord(s->ev0, s->stream));
    launch_traverse_kernel(s, anyhit ? 1 : 0, blocks, p);
    PH_CHECK(s, hipGetLastError());
    if (kernel_ms) {
        PH_CHECK(s, hipEventRecord(s->ev1, s->stream));
        PH_CHECK(s, hipEventSynchronize(s->ev1));
        PH_CHECK(s, hipEventElapsedTime(kernel_ms, s->ev0, s->ev1));
    }
    return PBRT_HIP_OK;
}

}  // namespace phost

using namespace phost;

int PbrtHipScene::fetch_leaf_records(std::vector<TriRec>& out) {
    if (!accel_on_device()) { out = bvh.tris; return PBRT_HIP_OK; }
    out.resize(accel_n_records());
    PH_CHECK(this, hipMemcpy(out.data(), accel_records(), out.size() * sizeof(TriRec), hipMemcpyDeviceToHost));
    return PBRT_HIP_OK;
}

namespace hm {
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
                    if (ipiv[k] == 0) { float av = fabs_p(minv[j][k]); if (av >= big) { big = av; irow = j; icol = k; } }
        ipiv[icol] += 1;
        if (irow != icol) for (int k = 0; k < 4; k++) std::swap(minv[irow][k], minv[icol][k]);
        indxr[i] = irow; indxc[i] = icol;
        float pivinv = 1.0f / minv[icol][icol];
        minv[icol][icol] = 1.0f;
        for (int j = 0; j < 4; j++) minv[icol][j] *= pivinv;
        for (int j = 0; j < 4; j++)
            if (j != icol) {
                float save = minv[j][icol];
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

int pbrt_hip_device_count(void) {
    return ph_guard(nullptr, "pbrt_hip_device_count", [&]() -> int {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorNoDevice ? 0 : PBRT_HIP_ERR_DEVICE; }
    return n;
    });
}

PbrtHipScene* pbrt_hip_scene_create(int device_ordinal) {
    return ph_guard_ptr<PbrtHipScene>("pbrt_hip_scene_create", [&]() -> PbrtHipScene* {
    int n = pbrt_hip_device_count();
    if (n <= 0 || device_ordinal < 0 || device_ordinal >= n) {
        set_err(nullptr, PBRT_HIP_ERR_NO_DEVICE, "pbrt_hip_scene_create: no usable HIP device (this library has no CPU path)");
        return nullptr;
    }
    if (hipSetDevice(device_ordinal) != hipSuccess) { set_err(nullptr, PBRT_HIP_ERR_DEVICE, "hipSetDevice failed"); return nullptr; }
    PbrtHipScene* s = new PbrtHipScene();
    s->device = device_ordinal;
    if (hipStreamCreate(&s->stream) != hipSuccess || hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) {
        set_err(nullptr, PBRT_HIP_ERR_DEVICE, "stream/event creation failed");
        delete s;
        return nullptr;
    }
    return s;
    });
}

void pbrt_hip_scene_destroy(PbrtHipScene* s) {
    ph_guard_void([&]() {
    if (!s) return;
    free_multi(s);  // the other devices' contexts of a multi-device handle
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    free_wavefront(s);
    free_whitted(s);
    free_owned(s);
    free_tree_dev(s->dev_tree);
    for (DevBuf* b : {&s->d_ld_func, &s->d_ld_cdf, &s->d_counter, &s->d_spill, &s->d_error, &s->d_counts, &s->d_rays_tmp, &s->d_out_tmp})
        if (b->p) (void)hipFree(b->p);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    });
}

const char* pbrt_hip_last_error(const PbrtHipScene* s) {
    if (s) return s->err.c_str();
    std::lock_guard<std::mutex> g(g_err_mu);
    return g_last_error.c_str();
}

// ---- materials: each call describes one (material_host.h: MaterialSpec); which lobes it has is derive's business -------------------------------
using phost::MaterialKind;
static int add_material(PbrtHipScene* s, const phost::MaterialSpec& spec, uint32_t* out_id) {
    std::string why;
    return material_changed(s, phost::add_material(s->mats, spec, out_id, why), why);
}

int pbrt_hip_add_material_matte(PbrtHipScene* s, const float kd[3], float sigma_deg, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_matte", [&]() -> int {
    if (!s || !kd) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_matte: null argument");
    phost::MaterialSpec m(MaterialKind::Matte); m.set(PBRT_HIP_PARAM_KD, kd); m.sigma = sigma_deg;
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_none(PbrtHipScene* s, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_none", [&]() -> int {
    if (!s) return PBRT_HIP_ERR_INVALID_ARG;
    return add_material(s, phost::MaterialSpec(MaterialKind::None), out_id);
    });
}
int pbrt_hip_add_material_mirror(PbrtHipScene* s, const float kr[3], uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_mirror", [&]() -> int {
    if (!s || !kr) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_mirror: null argument");
    phost::MaterialSpec m(MaterialKind::Mirror); m.set(PBRT_HIP_PARAM_KR, kr);
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_plastic(PbrtHipScene* s, const float kd[3], const float ks[3], float roughness, int remap_roughness, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_plastic", [&]() -> int {
    if (!s || !kd || !ks) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_plastic: null argument");
    phost::MaterialSpec m(MaterialKind::Plastic, roughness, roughness, remap_roughness != 0); m.set(PBRT_HIP_PARAM_KD, kd); m.set(PBRT_HIP_PARAM_KS, ks);
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_glass(PbrtHipScene* s, const float kr[3], const float kt[3], float urough, float vrough, float eta, int remap_roughness, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_glass", [&]() -> int {
    if (!s || !kr || !kt) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_glass: null argument");
    phost::MaterialSpec m(MaterialKind::Glass, urough, vrough, remap_roughness != 0); m.set(PBRT_HIP_PARAM_KR, kr); m.set(PBRT_HIP_PARAM_KT, kt); m.index = eta;
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_metal(PbrtHipScene* s, const float eta[3], const float k[3], float urough, float vrough, int remap_roughness, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_metal", [&]() -> int {
    if (!s || !eta || !k) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_metal: null argument");
    phost::MaterialSpec m(MaterialKind::Metal, urough, vrough, remap_roughness != 0); m.set(PBRT_HIP_PARAM_ETA, eta); m.set(PBRT_HIP_PARAM_K, k);
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_uber(PbrtHipScene* s, const float kd[3], const float ks[3], const float kr[3], const float kt[3], const float opacity[3], float urough,
                               float vrough, float eta, int remap_roughness, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_uber", [&]() -> int {
    if (!s || !kd || !ks || !kr || !kt || !opacity) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_uber: null argument");
    phost::MaterialSpec m(MaterialKind::Uber, urough, vrough, remap_roughness != 0); m.index = eta;
    m.set(PBRT_HIP_PARAM_KD, kd); m.set(PBRT_HIP_PARAM_KS, ks); m.set(PBRT_HIP_PARAM_KR, kr); m.set(PBRT_HIP_PARAM_KT, kt); m.set(PBRT_HIP_PARAM_OPACITY, opacity);
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_substrate(PbrtHipScene* s, const float kd[3], const float ks[3], float urough, float vrough, int remap_roughness, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_substrate", [&]() -> int {
    if (!s || !kd || !ks) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_substrate: null argument");
    phost::MaterialSpec m(MaterialKind::Substrate, urough, vrough, remap_roughness != 0); m.set(PBRT_HIP_PARAM_KD, kd); m.set(PBRT_HIP_PARAM_KS, ks);
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_translucent(PbrtHipScene* s, const float kd[3], const float ks[3], const float reflect[3], const float transmit[3], float roughness,
                                      int remap_roughness, uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_translucent", [&]() -> int {
    if (!s || !kd || !ks || !reflect || !transmit) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_translucent: null argument");
    phost::MaterialSpec m(MaterialKind::Translucent, roughness, roughness, remap_roughness != 0);
    m.set(PBRT_HIP_PARAM_KD, kd); m.set(PBRT_HIP_PARAM_KS, ks); m.set(PBRT_HIP_PARAM_REFLECT, reflect); m.set(PBRT_HIP_PARAM_TRANSMIT, transmit);
    return add_material(s, m, out_id);
    });
}
int pbrt_hip_add_material_mix(PbrtHipScene* s, uint32_t material1, uint32_t material2, const float amount[3], uint32_t* out_id) {
    return ph_guard(s, "pbrt_hip_add_material_mix", [&]() -> int {
    if (!s || !amount) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_mix: null argument");
    if (material1 >= s->mats.size() || material2 >= s->mats.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_material_mix: unknown material id");
    return add_material(s, phost::mix_spec(s->mats, material1, material2, amount), out_id);
    });
}

// "the intersection is bogus" (triangle.rs:548-574): depends only on the triangle, so it is decided once here.
static bool triangle_is_bogus(hm::V3 p0, hm::V3 p1, hm::V3 p2, const float* uv0, const float* uv1, const float* uv2) {
    float u0[2] = {0, 0}, u1[2] = {1, 0}, u2[2] = {1, 1};  // default uvs (triangle.rs:384-394)
    if (uv0) { u0[0] = uv0[0]; u0[1] = uv0[1]; u1[0] = uv1[0]; u1[1] = uv1[1]; u2[0] = uv2[0]; u2[1] = uv2[1]; }
    float duv02[2] = {u0[0] - u2[0], u0[1] - u2[1]}, duv12[2] = {u1[0] - u2[0], u1[1] - u2[1]};
    hm::V3 dp02 = hm::sub(p0, p2), dp12 = hm::sub(p1, p2);
    float determinant = duv02[0] * duv12[1] - duv02[1] * duv12[0];
    bool degenerate_uv = std::fabs(determinant) < 1e-8f;
    hm::V3 dpdu{0, 0, 0}, dpdv{0, 0, 0};
    if (!degenerate_uv) {
        float invdet = 1.0f / determinant;
        dpdu = hm::mulf(hm::sub(hm::mulf(dp02, duv12[1]), hm::mulf(dp12, duv02[1])), invdet);
        dpdv = hm::mulf(hm::add(hm::mulf(dp02, -duv12[0]), hm::mulf(dp12, duv02[0])), invdet);
    }
    if (degenerate_uv || hm::len2(hm::cross(dpdu, dpdv)) == 0.0f) {
        hm::V3 ng = hm::cross(hm::sub(p2, p0), hm::sub(p1, p0));
        if (hm::len2(ng) == 0.0f) return true;
    }
    return false;
}

int pbrt_hip_add_mesh(PbrtHipScene* s, const float* P, uint32_t n_verts, const uint32_t* indices, uint32_t n_tris, const float* N,
                      const float* S, const float* UV, uint32_t material_id, int32_t first_area_light_id, uint32_t flags, float alpha,
                      float shadow_alpha) {
    return ph_guard(s, "pbrt_hip_add_mesh", [&]() -> int {
    if (!s || !P || !indices) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_mesh: null argument");
    if (material_id >= s->mats.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_mesh: unknown material id");
    for (uint32_t i = 0; i < 3 * n_tris; i++)
        if (indices[i] >= n_verts) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_mesh: vertex index out of bounds (triangle.rs:252-261)");
    if (first_area_light_id >= 0) {
        if ((size_t)first_area_light_id + n_tris > s->lights.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_mesh: area light ids out of range");
        for (uint32_t k = 0; k < n_tris; k++)
            if (s->lights[first_area_light_id + k].type != PH_L_AREA || s->lights[first_area_light_id + k].prim != 0xFFFFFFFFu)
                return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_mesh: light is not an unbound diffuse area light");
    }
    bool dropped_lights = false;
    if (s->open_object >= 0 && first_area_light_id >= 0) {
        // "Area lights not supported with object instancing" (api/src/lib.rs:877-881): a warning, the primitives keep their area light — a path that looks at such a surface
        // sees its emission (SurfaceInteraction::le) — and the light is not added to the scene's lights: nothing samples it.
        if ((size_t)first_area_light_id + n_tris != s->lights.size())
            return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_mesh: the area lights of a shape inside an object definition must be the lights created last (they leave the scene's light list)");
        const int32_t first = -2 - (int32_t)s->emission_only.size();
        s->emission_only.insert(s->emission_only.end(), s->lights.begin() + first_area_light_id, s->lights.end());
        s->lights.resize((size_t)first_area_light_id);
        first_area_light_id = first;
        dropped_lights = true;
    }
    MeshRec m{};
    m.vert_base = (uint32_t)(s->P.size() / 3); m.tri_base = (uint32_t)(s->idx.size() / 3); m.n_tris = n_tris;
    m.flags = (N ? PH_MESH_N : 0) | (S ? PH_MESH_S : 0) | (UV ? PH_MESH_UV : 0) | ((flags & 1) ? PH_MESH_REV : 0) | ((flags & 2) ? PH_MESH_SWAP : 0);
    m.material = material_id; m.first_light = first_area_light_id;
    const size_t v0 = s->P.size() / 3;
    s->P.insert(s->P.end(), P, P + 3 * (size_t)n_verts);
    // optional attributes stay vertex-aligned with P; arrays are materialised only once some mesh supplies them
    auto grow_attr = [&](std::vector<float>& dst, bool& any, const float* src, int w) {
        if (src && !any) { dst.assign(v0 * w, 0.0f); any = true; }
        if (any) { if (src) dst.insert(dst.end(), src, src + (size_t)w * n_verts); else dst.insert(dst.end(), (size_t)w * n_verts, 0.0f); }
    };
    grow_attr(s->N, s->any_n, N, 3); grow_attr(s->S, s->any_s, S, 3); grow_attr(s->UV, s->any_uv, UV, 2);
    const uint32_t mesh_id = (uint32_t)s->meshes.size();
    for (uint32_t t = 0; t < n_tris; t++) {
        uint32_t i0 = indices[3 * t], i1 = indices[3 * t + 1], i2 = indices[3 * t + 2];
        s->idx.push_back(i0 + m.vert_base); s->idx.push_back(i1 + m.vert_base); s->idx.push_back(i2 + m.vert_base);
        s->tri_mesh.push_back(mesh_id);
        hm::V3 p0 = hm::ld(P + 3 * i0), p1 = hm::ld(P + 3 * i1), p2 = hm::ld(P + 3 * i2);
        uint32_t tf = 0;
        if (triangle_is_bogus(p0, p1, p2, UV ? UV + 2 * i0 : nullptr, UV ? UV + 2 * i1 : nullptr, UV ? UV + 2 * i2 : nullptr)) tf |= PH_TRI_BOGUS;
        if (alpha == 0.0f) tf |= PH_TRI_ALPHA0;
        if (shadow_alpha == 0.0f) tf |= PH_TRI_SALPHA0;
        s->tri_flags.push_back(tf);
        if (first_area_light_id >= 0 || dropped_lights) {
            LightRec& l = dropped_lights ? s->emission_only[(size_t)(-2 - first_area_light_id) + t] : s->lights[first_area_light_id + t];
            l.prim = m.tri_base + t;
            l.area = 0.5f * hm::len(hm::cross(hm::sub(p1, p0), hm::sub(p2, p0)));  // Triangle::area (triangle.rs:906-911)
        }
    }
    s->meshes.push_back(m);
    if (s->open_object >= 0) s->objects[s->open_object].tri1 = m.tri_base + n_tris;
    else for (uint32_t t = 0; t < n_tris; t++) s->top_items.push_back(m.tri_base + t);
    s->built = false; s->uploaded = false;
    if (dropped_lights) s->err = "warning: Area lights not supported with object instancing.";   // the reference's warn! (lib.rs:878); the call succeeds
    return PBRT_HIP_OK;
    });
}

}  // extern "C"

// ---- quadric shapes ------------------------------------------------------------------------------------------------------------------------------------------------
// What the three capture calls share: the refusals, the shape's MeshRec and primitive slot, Shape::world_bound (core/src/geometry/shape.rs: object_to_world(object_bound))
static void quadric_world_bound(const float o2w_m[16], const float obj_lo[3], const float obj_hi[3], float wb[6]) {
    float lo[3], hi[3];   // Bounds3::new of the two corners, then Transform::transform_bounds
    for (int k = 0; k < 3; k++) { lo[k] = obj_lo[k] < obj_hi[k] ? obj_lo[k] : obj_hi[k]; hi[k] = obj_lo[k] > obj_hi[k] ? obj_lo[k] : obj_hi[k]; }
    phost::transform_bounds(o2w_m, lo, hi, wb);
}
static int add_quadric_common(PbrtHipScene* s, const char* what, QuadricRec& q, const float o2w_m[16], const float o2w_minv[16], const float obj_lo[3], const float obj_hi[3],
                              uint32_t material_id, uint32_t flags) {
    if (material_id >= s->mats.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, std::string(what) + ": unknown material id");
    if (s->open_object >= 0) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, std::string(what) + ": quadric shapes inside an object definition are not supported");
    if (!s->lights.empty() && s->lights.back().type == PH_L_AREA && s->lights.back().prim == 0xFFFFFFFFu)
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, std::string(what) + ": a quadric cannot be the shape of a diffuse area light (the unclaimed area lights created last would be its); attach them to a mesh");
    std::memcpy(q.o2w, o2w_m, 64); std::memcpy(q.w2o, o2w_minv, 64);
    const float* m = o2w_m;   // Transform::swaps_handedness (transform.rs:593-599)
    const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
    const bool swaps = det < 0.0f, rev = (flags & 1u) != 0u;
    q.flip = (rev != swaps) ? 1u : 0u;
    float wb[6];
    quadric_world_bound(o2w_m, obj_lo, obj_hi, wb);
    const uint32_t prim = (uint32_t)(s->idx.size() / 3);
    MeshRec mr{};
    mr.vert_base = (uint32_t)s->quadrics.size(); mr.tri_base = prim; mr.n_tris = 1;
    mr.flags = PH_MESH_QUADRIC | (rev ? PH_MESH_REV : 0u) | (swaps ? PH_MESH_SWAP : 0u);
    mr.material = material_id; mr.first_light = -1;
    s->prim_quadric.resize(prim, 0u);
    s->prim_quadric.push_back((uint32_t)s->quadrics.size() + 1u);
    s->quadrics.push_back(q);
    s->quadric_bounds.insert(s->quadric_bounds.end(), wb, wb + 6);
    for (int k = 0; k < 3; k++) s->idx.push_back(0u);   // the slot's index triple; never read
    s->tri_mesh.push_back((uint32_t)s->meshes.size());
    s->tri_flags.push_back(0u);
    s->meshes.push_back(mr);
    s->top_items.push_back(prim);
    // the quadric code lives in the general-BSDF / texture-pass instantiations of the shade kernels (wavefront.hip), like the radiance maps'
    s->general_materials = true; s->textured_materials = true;
    s->built = false; s->uploaded = false;
    return PBRT_HIP_OK;
}
static float to_phi_max(float phi_max_deg) { return hm::clampf(phi_max_deg, 0.0f, 360.0f) * (hm::kPi / 180.0f); }   // f32::to_radians
static float acos_f64(float x) { return (float)std::acos((double)x); }   // transcendentals: f64, rounded once

// The constructors proper: parameters clamped and derived as the reference does, and the corners of object_bound()
static void sphere_rec(float radius, float z_min, float z_max, float phi_max_deg, QuadricRec& q, float lo[3], float hi[3]) {   // Sphere::new (shapes/src/sphere.rs:21-44), object_bound (:53-58)
    q.kind = PH_Q_SPHERE; q.radius = radius;
    const float zlo = z_min < z_max ? z_min : z_max, zhi = z_min > z_max ? z_min : z_max;
    q.z_min = hm::clampf(zlo, -radius, radius); q.z_max = hm::clampf(zhi, -radius, radius);
    q.theta_min = acos_f64(hm::clampf(zlo / radius, -1.0f, 1.0f)); q.theta_max = acos_f64(hm::clampf(zhi / radius, -1.0f, 1.0f));
    q.phi_max = to_phi_max(phi_max_deg);
    lo[0] = lo[1] = -radius; lo[2] = q.z_min; hi[0] = hi[1] = radius; hi[2] = q.z_max;
}
static void hyperboloid_rec(const float p1_in[3], const float p2_in[3], float phi_max_deg, QuadricRec& q, float lo[3], float hi[3]) {   // Hyperboloid::new (hyperboloid.rs:37-110), object_bound (:112-122)
    q.kind = PH_Q_HYPERBOLOID;
    hm::V3 p1 = hm::ld(p1_in), p2 = hm::ld(p2_in);
    const float radius1 = std::sqrt(p1.x * p1.x + p1.y * p1.y), radius2 = std::sqrt(p2.x * p2.x + p2.y * p2.y);
    const float r_max = radius1 > radius2 ? radius1 : radius2;
    q.z_min = p1.z < p2.z ? p1.z : p2.z; q.z_max = p1.z > p2.z ? p1.z : p2.z;
    if (p2.z == 0.0f) { const hm::V3 t = p1; p1 = p2; p2 = t; }
    hm::V3 pp = p1;
    float ah = 0.0f, ch = 0.0f;
    for (int count = 0;; count++) {   // the search for finite implicit coefficients (:70-88)
        pp = hm::add(pp, hm::mulf(hm::sub(p2, p1), 2.0f));
        const float xy1 = pp.x * pp.x + pp.y * pp.y, xy2 = p2.x * p2.x + p2.y * p2.y;
        ah = (1.0f / xy1 - (pp.z * pp.z) / (xy1 * p2.z * p2.z)) / (1.0f - (xy2 * pp.z * pp.z) / (xy1 * p2.z * p2.z));
        ch = (ah * xy2 - 1.0f) / (p2.z * p2.z);
        if (std::isfinite(ah) || count > 100000) break;
    }
    q.ah = ah; q.ch = ch; q.radius = r_max;
    q.p1[0] = p1.x; q.p1[1] = p1.y; q.p1[2] = p1.z; q.p2[0] = p2.x; q.p2[1] = p2.y; q.p2[2] = p2.z;
    q.phi_max = to_phi_max(phi_max_deg);
    lo[0] = lo[1] = -r_max; lo[2] = q.z_min; hi[0] = hi[1] = r_max; hi[2] = q.z_max;
}
// Cylinder::new (cylinder.rs:21-42), Cone::new (cone.rs:21-40), Paraboloid::new (paraboloid.rs:21-42), Disk::new (disk.rs:21-40) and their object_bound
static void quadric_rec(int kind, float radius, float a, float b, float phi_max_deg, QuadricRec& q, float lo[3], float hi[3]) {
    q.kind = (uint32_t)kind; q.radius = radius; q.z_min = 0.0f; q.z_max = 1.0f; q.height = 1.0f;
    lo[0] = lo[1] = -radius; hi[0] = hi[1] = radius; lo[2] = hi[2] = 0.0f;
    if (kind == PH_Q_CYLINDER || kind == PH_Q_PARABOLOID) { q.z_min = a < b ? a : b; q.z_max = a > b ? a : b; lo[2] = q.z_min; hi[2] = q.z_max; }
    else if (kind == PH_Q_CONE) { q.height = a; lo[2] = 0.0f; hi[2] = a; }
    else { q.height = a; q.inner_radius = b; lo[2] = a; hi[2] = a; }
    q.phi_max = to_phi_max(phi_max_deg);
}

extern "C" {

int pbrt_hip_add_sphere(PbrtHipScene* s, const float o2w_m[16], const float o2w_minv[16], float radius, float z_min, float z_max, float phi_max_deg, uint32_t material_id, uint32_t flags) {
    return ph_guard(s, "pbrt_hip_add_sphere", [&]() -> int {
    if (!s || !o2w_m || !o2w_minv) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_sphere: null argument");
    QuadricRec q{}; float lo[3], hi[3];
    sphere_rec(radius, z_min, z_max, phi_max_deg, q, lo, hi);
    return add_quadric_common(s, "add_sphere", q, o2w_m, o2w_minv, lo, hi, material_id, flags);
    });
}
// pbrt_hip_add_sphere plus the DiffuseAreaLight whose shape is that sphere (lights/src/diffuse.rs:46-82): one LightRec in call order, bound to the sphere's primitive slot
int pbrt_hip_add_sphere_light(PbrtHipScene* s, const float o2w_m[16], const float o2w_minv[16], float radius, float z_min, float z_max, float phi_max_deg, uint32_t material_id, uint32_t flags,
                              const float L_rgb[3], int two_sided) {
    return ph_guard(s, "pbrt_hip_add_sphere_light", [&]() -> int {
    if (!s || !o2w_m || !o2w_minv || !L_rgb) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_sphere_light: null argument");
    if (!s->lights.empty() && s->lights.back().type == PH_L_AREA && s->lights.back().prim == 0xFFFFFFFFu)
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "add_sphere_light: the diffuse area lights created last have no mesh yet; attach them first (the sphere brings its own light)");
    QuadricRec q{}; float lo[3], hi[3];
    sphere_rec(radius, z_min, z_max, phi_max_deg, q, lo, hi);
    const int rc = add_quadric_common(s, "add_sphere_light", q, o2w_m, o2w_minv, lo, hi, material_id, flags);
    if (rc) return rc;
    LightRec l{}; l.type = PH_L_AREA; l.two_sided = two_sided ? 1 : 0; l.prim = s->meshes.back().tri_base;
    l.area = q.phi_max * q.radius * (q.z_max - q.z_min);   // Sphere::area (sphere.rs), of the constructor's clamped values
    for (int c = 0; c < 3; c++) l.L[c] = L_rgb[c];
    s->meshes.back().first_light = (int32_t)s->lights.size();
    s->lights.push_back(l);
    s->sphere_lights++;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_add_hyperboloid(PbrtHipScene* s, const float o2w_m[16], const float o2w_minv[16], const float p1[3], const float p2[3], float phi_max_deg, uint32_t material_id, uint32_t flags) {
    return ph_guard(s, "pbrt_hip_add_hyperboloid", [&]() -> int {
    if (!s || !o2w_m || !o2w_minv || !p1 || !p2) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_hyperboloid: null argument");
    QuadricRec q{}; float lo[3], hi[3];
    hyperboloid_rec(p1, p2, phi_max_deg, q, lo, hi);
    return add_quadric_common(s, "add_hyperboloid", q, o2w_m, o2w_minv, lo, hi, material_id, flags);
    });
}
int pbrt_hip_add_quadric(PbrtHipScene* s, int kind, const float o2w_m[16], const float o2w_minv[16], float radius, float a, float b, float phi_max_deg, uint32_t material_id, uint32_t flags) {
    return ph_guard(s, "pbrt_hip_add_quadric", [&]() -> int {
    if (!s || !o2w_m || !o2w_minv) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_quadric: null argument");
    if (kind < 0 || kind > 3) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_quadric: kind must be 0 cylinder, 1 cone, 2 paraboloid or 3 disk");
    QuadricRec q{}; float lo[3], hi[3];
    quadric_rec(kind, radius, a, b, phi_max_deg, q, lo, hi);
    return add_quadric_common(s, "add_quadric", q, o2w_m, o2w_minv, lo, hi, material_id, flags);
    });
}
// pbrt_hip_add_quadric plus the DiffuseAreaLight whose shape is that cylinder or disk: one LightRec in call order, bound to the shape's primitive slot.  The reference's
// Cone, Paraboloid and Hyperboloid ::sample are todo!(): such a light would panic at its first sample
int pbrt_hip_add_quadric_light(PbrtHipScene* s, int kind, const float o2w_m[16], const float o2w_minv[16], float radius, float a, float b, float phi_max_deg, uint32_t material_id,
                               uint32_t flags, const float L_rgb[3], int two_sided) {
    return ph_guard(s, "pbrt_hip_add_quadric_light", [&]() -> int {
    if (!s || !o2w_m || !o2w_minv || !L_rgb) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_quadric_light: null argument");
    if (kind == PH_Q_CONE || kind == PH_Q_PARABOLOID)
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "add_quadric_light: a cone or a paraboloid cannot be an area light: the reference's Shape::sample for it is todo!()");
    if (kind != PH_Q_CYLINDER && kind != PH_Q_DISK) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_quadric_light: kind must be 0 cylinder or 3 disk");
    if (!s->lights.empty() && s->lights.back().type == PH_L_AREA && s->lights.back().prim == 0xFFFFFFFFu)
        return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "add_quadric_light: the diffuse area lights created last have no mesh yet; attach them first (the shape brings its own light)");
    QuadricRec q{}; float lo[3], hi[3];
    quadric_rec(kind, radius, a, b, phi_max_deg, q, lo, hi);
    const int rc = add_quadric_common(s, "add_quadric_light", q, o2w_m, o2w_minv, lo, hi, material_id, flags);
    if (rc) return rc;
    LightRec l{}; l.type = PH_L_AREA; l.two_sided = two_sided ? 1 : 0; l.prim = s->meshes.back().tri_base;
    if (kind == PH_Q_CYLINDER) l.area = (q.z_max - q.z_min) * q.radius * q.phi_max;                        // Cylinder::area (cylinder.rs:313-315)
    else l.area = q.phi_max * 0.5f * (q.radius * q.radius - q.inner_radius * q.inner_radius);              // Disk::area (disk.rs:205-207)
    for (int c = 0; c < 3; c++) l.L[c] = L_rgb[c];
    s->meshes.back().first_light = (int32_t)s->lights.size();
    s->lights.push_back(l);
    s->quadric_lights++;
    return PBRT_HIP_OK;
    });
}

// Curve::create_segments (shapes/src/curve.rs:105-140): one CurveData, 2^split_depth Curve segments over equal u ranges, each a primitive of its own with its own
// Shape::world_bound (object_bound, :660-674, through transform_bounds).  A segment is a QuadricRec of kind PH_Q_CURVE: it shares the quadrics' leaf record, builders and kernel rows
int pbrt_hip_add_curve(PbrtHipScene* s, const float o2w_m[16], const float o2w_minv[16], int type, const float cp[12], const float width[2], const float* n, int split_depth,
                       uint32_t material_id, uint32_t flags) {
    return ph_guard(s, "pbrt_hip_add_curve", [&]() -> int {
    if (!s || !o2w_m || !o2w_minv || !cp || !width) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_curve: null argument");
    if (type != PH_CURVE_FLAT && type != PH_CURVE_CYLINDER && type != PH_CURVE_RIBBON) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_curve: type must be 0 flat, 1 cylinder or 2 ribbon");
    if (type == PH_CURVE_RIBBON && !n) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_curve: a ribbon curve needs its two end normals");
    if (split_depth < 0 || split_depth > 16) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_curve: split_depth must lie in [0, 16]");
    CurveRec c;
    pcurve::curve_data(type, cp, width, type == PH_CURVE_RIBBON ? n : nullptr, c);   // (from_props drops the normals of any other type, curve.rs:211-214)
    const uint32_t curve = (uint32_t)s->curves.size();
    const int n_segments = 1 << split_depth;
    for (int i = 0; i < n_segments; i++) {
        QuadricRec q{}; float lo[3], hi[3];
        q.kind = PH_Q_CURVE; q.curve = curve;
        pcurve::segment_range(i, split_depth, q.z_min, q.z_max);
        pcurve::segment_object_bound(c, q.z_min, q.z_max, lo, hi);
        const int rc = add_quadric_common(s, "add_curve", q, o2w_m, o2w_minv, lo, hi, material_id, flags);   // its refusals depend on the scene alone: the first segment meets them, before anything changed
        if (rc) return rc;
    }
    s->curves.push_back(c);
    return PBRT_HIP_OK;
    });
}

// LoopSubDiv::subdivide (shapes/src/loopsubdiv.rs:321-659): the control mesh on the host (loopsubdiv_host.h), the refinement on the device (loopsubdiv.hip).
// The first half: argument checks and the control mesh, built once per call; needs no device and no handle
static int loopsubdiv_control(PbrtHipScene* s, const char* what, const float* o2w_m, const float* o2w_minv, const float* P, uint32_t n_verts, const uint32_t* indices,
                              uint32_t n_indices, int n_levels, ploop::Control& c) {
    if (o2w_m && !o2w_minv) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, std::string(what) + ": a matrix without its inverse");
    const std::string bad = ploop::build_control(P, n_verts, indices, n_indices, n_levels, c);
    if (!bad.empty()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, std::string(what) + ": " + bad);
    return PBRT_HIP_OK;
}
// The second half: the mesh of `c` into arrays of 3 * c.out_verts, 3 * c.out_verts and 3 * c.out_faces, on the handle's first device and its stream
static int loopsubdiv_refine(PbrtHipScene* s, const char* what, const ploop::Control& c, const float* o2w_m, const float* o2w_minv, const float* P, int n_levels, float* out_P,
                             float* out_N, uint32_t* out_indices) {
    PH_CHECK(s, hipSetDevice(s->device));
    std::string e;
    if (phost::loopsubdiv_device(c, P, n_levels, o2w_m, o2w_minv, s->stream, out_P, out_N, out_indices, e) != 0) return set_err(s, PBRT_HIP_ERR_DEVICE, std::string(what) + ": " + e);
    return PBRT_HIP_OK;
}

int pbrt_hip_loopsubdiv_mesh(PbrtHipScene* s, const float* o2w_m, const float* o2w_minv, const float* P, uint32_t n_verts, const uint32_t* indices, uint32_t n_indices, int n_levels,
                             uint32_t* out_n_verts, uint32_t* out_n_tris, float* out_P, float* out_N, uint32_t* out_indices) {
    return ph_guard(s, "pbrt_hip_loopsubdiv_mesh", [&]() -> int {
    const char* what = "loopsubdiv_mesh";
    if (!out_n_verts || !out_n_tris) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, std::string(what) + ": null count pointer");
    const bool counts_only = !out_P && !out_N && !out_indices;
    if (!counts_only && (!out_P || !out_N || !out_indices)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, std::string(what) + ": out_P, out_N and out_indices go together");
    if (!counts_only && !s) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, std::string(what) + ": null handle (only the counts need none)");
    ploop::Control c;
    const int rc = loopsubdiv_control(s, what, o2w_m, o2w_minv, P, n_verts, indices, n_indices, n_levels, c);
    if (rc) return rc;
    *out_n_verts = (uint32_t)c.out_verts; *out_n_tris = (uint32_t)c.out_faces;
    if (counts_only) return PBRT_HIP_OK;
    return loopsubdiv_refine(s, what, c, o2w_m, o2w_minv, P, n_levels, out_P, out_N, out_indices);
    });
}
// The mesh of the call above, then pbrt_hip_add_mesh with its P, N and indices: TriangleMesh::create without S, UV or alpha textures (loopsubdiv.rs:645-658)
int pbrt_hip_add_loopsubdiv(PbrtHipScene* s, const float* o2w_m, const float* o2w_minv, const float* P, uint32_t n_verts, const uint32_t* indices, uint32_t n_indices, int n_levels,
                            uint32_t material_id, int32_t first_area_light_id, uint32_t flags, float alpha, float shadow_alpha) {
    return ph_guard(s, "pbrt_hip_add_loopsubdiv", [&]() -> int {
    const char* what = "add_loopsubdiv";
    if (!s) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_loopsubdiv: null handle");
    if (material_id >= s->mats.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_loopsubdiv: unknown material id");   // (before any device work; add_mesh checks the rest)
    ploop::Control c;
    int rc = loopsubdiv_control(s, what, o2w_m, o2w_minv, P, n_verts, indices, n_indices, n_levels, c);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)c.out_verts, nt = (uint32_t)c.out_faces;
    if (first_area_light_id >= 0 && (size_t)first_area_light_id + nt > s->lights.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_loopsubdiv: area light ids out of range (one light per output triangle)");
    std::vector<float> mp(3 * (size_t)nv), mn(3 * (size_t)nv);
    std::vector<uint32_t> mi(3 * (size_t)nt);
    rc = loopsubdiv_refine(s, what, c, o2w_m, o2w_minv, P, n_levels, mp.data(), mn.data(), mi.data());
    if (rc) return rc;
    return pbrt_hip_add_mesh(s, mp.data(), nv, mi.data(), nt, mn.data(), nullptr, nullptr, material_id, first_area_light_id, flags, alpha, shadow_alpha);
    });
}

// Host-only run of the BVH builder over triangles AND quadric shapes (include/pbrt_hip_host.h), for inspection and tests; needs no GPU.  The shapes go through the same constructors
// and the same world_bound as the capture calls above.
int pbrt_hip_host_build_bvh_shapes(const float* P, const uint32_t* idx, uint64_t n_prims, const uint32_t* prim_shape, const float* shapes, uint64_t n_shapes, int split_method,
                                   int max_prims_in_node, int n_threads, uint32_t* out_ordered_prims, uint32_t* out_leaf_last, void* out_nodes, uint64_t* out_info, float* out_root_bounds) {
    return ph_guard(nullptr, "pbrt_hip_host_build_bvh_shapes", [&]() -> int {
    if (!idx || !prim_shape || (n_shapes && !shapes)) return PBRT_HIP_ERR_INVALID_ARG;
    std::vector<float> bounds(6 * (size_t)n_shapes);
    for (uint64_t k = 0; k < n_shapes; k++) {
        const float* sp = shapes + 40 * k; const float* par = sp + 33;
        const int kind = (int)sp[0];
        QuadricRec q{}; float lo[3], hi[3];
        if (kind == PH_Q_SPHERE) sphere_rec(par[0], par[1], par[2], par[3], q, lo, hi);
        else if (kind == PH_Q_HYPERBOLOID) hyperboloid_rec(par, par + 3, par[6], q, lo, hi);
        else if (kind >= 0 && kind <= 3) quadric_rec(kind, par[0], par[1], par[2], par[3], q, lo, hi);
        else return PBRT_HIP_ERR_INVALID_ARG;
        quadric_world_bound(sp + 1, lo, hi, &bounds[6 * k]);
    }
    for (uint64_t t = 0; t < n_prims; t++) if (prim_shape[t] > n_shapes) return PBRT_HIP_ERR_INVALID_ARG;
    phost::BuildInput in{P, idx, (size_t)n_prims, nullptr, nullptr};
    in.prim_quadric = prim_shape; in.quad_bounds = bounds.data(); in.n_quadrics = (size_t)n_shapes;
    phost::BuildOutput out;
    const int rc = phost::build_bvh(in, split_method, max_prims_in_node, n_threads, out);
    if (rc) return rc;
    for (size_t i = 0; i < out.tris.size(); i++) {
        if (out_ordered_prims) out_ordered_prims[i] = out.tris[i].prim;
        if (out_leaf_last) out_leaf_last[i] = (out.tris[i].flags & PH_TRI_LAST) ? 1u : 0u;
    }
    if (out_nodes && !out.nodes.empty()) std::memcpy(out_nodes, out.nodes.data(), out.nodes.size() * sizeof(Node64));
    if (out_info) { out_info[0] = out.interior_nodes; out_info[1] = out.leaf_nodes; out_info[2] = out.max_leaf_prims; out_info[3] = (uint64_t)out.max_depth; out_info[4] = out.root_ref; }
    if (out_root_bounds) { for (int k = 0; k < 3; k++) { out_root_bounds[k] = out.root_lo[k]; out_root_bounds[3 + k] = out.root_hi[k]; } }
    return 0;
    });
}

// ObjectBegin / ObjectEnd / ObjectInstance (api/src/lib.rs:911-1000)
int pbrt_hip_object_begin(PbrtHipScene* s, uint32_t* out_object_id) {
    return ph_guard(s, "pbrt_hip_object_begin", [&]() -> int {
    if (!s || !out_object_id) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "object_begin: null argument");
    if (s->open_object >= 0) return set_err(s, PBRT_HIP_ERR_STATE, "object_begin: ObjectBegin called inside of an instance definition");
    PbrtHipScene::ObjectHost ob; ob.tri0 = ob.tri1 = (uint32_t)(s->idx.size() / 3);
    s->objects.push_back(ob);
    s->open_object = (int)s->objects.size() - 1;
    *out_object_id = (uint32_t)s->open_object;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_object_end(PbrtHipScene* s) {
    return ph_guard(s, "pbrt_hip_object_end", [&]() -> int {
    if (!s) return PBRT_HIP_ERR_INVALID_ARG;
    if (s->open_object < 0) return set_err(s, PBRT_HIP_ERR_STATE, "object_end: ObjectEnd called outside of instance definition");
    s->open_object = -1;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_add_instance(PbrtHipScene* s, uint32_t object_id, const float i2w[16], const float w2i[16]) {
    return ph_guard(s, "pbrt_hip_add_instance", [&]() -> int {
    if (!s || !i2w || !w2i) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_instance: null argument");
    if (s->open_object >= 0) return set_err(s, PBRT_HIP_ERR_STATE, "add_instance: ObjectInstance can't be called inside of instance definition");
    if (object_id >= s->objects.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_instance: unknown object");
    if (s->objects[object_id].tri1 == s->objects[object_id].tri0) return PBRT_HIP_OK;  // empty object: nothing is added (lib.rs:949-951)
    PbrtHipScene::InstanceHost in; in.object = object_id;
    std::memcpy(in.i2w, i2w, 64); std::memcpy(in.w2i, w2i, 64);
    s->instances.push_back(in);
    s->top_items.push_back(PH_ITEM_INST | (uint32_t)(s->instances.size() - 1));
    s->built = false; s->uploaded = false;
    return PBRT_HIP_OK;
    });
}

// 1x1 MIPMap::triangle (core/src/mipmap/mod.rs:293-311) for a constant environment
static float env_lookup(float tx, float s_, float t_) {
    float s = s_ * 1.0f - 0.5f, t = t_ * 1.0f - 0.5f;
    float s0 = std::floor(s), t0 = std::floor(t);
    float ds = s - s0, dt = t - t0;
    return tx * (1.0f - ds) * (1.0f - dt) + tx * (1.0f - ds) * dt + tx * ds * (1.0f - dt) + tx * ds * dt;
}

int pbrt_hip_add_light_infinite(PbrtHipScene* s, const float L[3], const float l2w[16], const float w2l[16]) {
    return ph_guard(s, "pbrt_hip_add_light_infinite", [&]() -> int {
    if (!s || !L || !l2w || !w2l) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_light_infinite: null argument");
    LightRec l{};
    l.type = PH_L_INFINITE; l.prim = 0xFFFFFFFFu;
    for (int c = 0; c < 3; c++) l.L[c] = L[c];
    std::memcpy(l.l2w, l2w, 48); std::memcpy(l.w2l, w2l, 48);
    // compute_scalar_image (infinite.rs:326-369): 2x2 image, fwidth 0.25 -> level < 0 -> triangle(0, st)
    float img[2][2];
    for (int v = 0; v < 2; v++) {
        float vp = ((float)v + 0.5f) / 2.0f;
        float sin_theta = std::sin(hm::kPi * ((float)v + 0.5f) / 2.0f);
        for (int u = 0; u < 2; u++) {
            float up = ((float)u + 0.5f) / 2.0f;
            float y = 0.212671f * env_lookup(L[0], up, vp) + 0.715160f * env_lookup(L[1], up, vp) + 0.072169f * env_lookup(L[2], up, vp);
            img[v][u] = y * sin_theta;
        }
    }
    std::vector<float> marg, cdf;
    for (int v = 0; v < 2; v++) {  // Distribution2D::new (distribution_2d.rs:21-29)
        float fi;
        hm::distribution1d({img[v][0], img[v][1]}, cdf, fi);
        l.cond_func[2 * v] = img[v][0]; l.cond_func[2 * v + 1] = img[v][1];
        for (int i = 0; i < 3; i++) l.cond_cdf[3 * v + i] = cdf[i];
        l.cond_int[v] = fi; marg.push_back(fi);
    }
    float mi;
    hm::distribution1d(marg, cdf, mi);
    l.marg_func[0] = marg[0]; l.marg_func[1] = marg[1];
    for (int i = 0; i < 3; i++) l.marg_cdf[i] = cdf[i];
    l.marg_int = mi;
    s->infinite_lights.push_back((uint32_t)s->lights.size());
    s->lights.push_back(l);
    s->uploaded = false;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_add_light_distant(PbrtHipScene* s, const float L[3], const float w[3]) {
    return ph_guard(s, "pbrt_hip_add_light_distant", [&]() -> int {
    if (!s || !L || !w) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_light_distant: null argument");
    LightRec l{}; l.type = PH_L_DISTANT; l.prim = 0xFFFFFFFFu;
    for (int c = 0; c < 3; c++) { l.L[c] = L[c]; l.v[c] = w[c]; }
    s->lights.push_back(l); s->uploaded = false;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_add_light_point(PbrtHipScene* s, const float I[3], const float p[3]) {
    return ph_guard(s, "pbrt_hip_add_light_point", [&]() -> int {
    if (!s || !I || !p) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_light_point: null argument");
    LightRec l{}; l.type = PH_L_POINT; l.prim = 0xFFFFFFFFu;
    for (int c = 0; c < 3; c++) { l.L[c] = I[c]; l.v[c] = p[c]; }
    s->lights.push_back(l); s->uploaded = false;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_add_light_spot(PbrtHipScene* s, const float I[3], const float l2w[16], const float w2l[16], float cos_total_width, float cos_falloff_start) {  // spot.rs:27-50
    return ph_guard(s, "pbrt_hip_add_light_spot", [&]() -> int {
    if (!s || !I || !l2w || !w2l) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_light_spot: null argument");
    LightRec l{}; l.type = PH_L_SPOT; l.prim = 0xFFFFFFFFu;
    for (int c = 0; c < 3; c++) l.L[c] = I[c];
    std::memcpy(l.l2w, l2w, 48); std::memcpy(l.w2l, w2l, 48);
    // p_light = light_to_world.transform_point(Point3f::ZERO) (transform.rs:288-302)
    const float xp = l2w[0] * 0.0f + l2w[1] * 0.0f + l2w[2] * 0.0f + l2w[3], yp = l2w[4] * 0.0f + l2w[5] * 0.0f + l2w[6] * 0.0f + l2w[7];
    const float zp = l2w[8] * 0.0f + l2w[9] * 0.0f + l2w[10] * 0.0f + l2w[11], wp = l2w[12] * 0.0f + l2w[13] * 0.0f + l2w[14] * 0.0f + l2w[15];
    if (wp == 1.0f) { l.v[0] = xp; l.v[1] = yp; l.v[2] = zp; } else { const float inv = 1.0f / wp; l.v[0] = inv * xp; l.v[1] = inv * yp; l.v[2] = inv * zp; }
    l.cos_total_width = cos_total_width; l.cos_falloff_start = cos_falloff_start;
    s->lights.push_back(l); s->uploaded = false;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_add_light_diffuse_area(PbrtHipScene* s, const float L[3], int two_sided, uint32_t n_tris, uint32_t* out_first_id) {
    return ph_guard(s, "pbrt_hip_add_light_diffuse_area", [&]() -> int {
    if (!s || !L) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "add_light_diffuse_area: null argument");
    if (out_first_id) *out_first_id = (uint32_t)s->lights.size();
    for (uint32_t i = 0; i < n_tris; i++) {
        LightRec l{}; l.type = PH_L_AREA; l.two_sided = two_sided ? 1 : 0; l.prim = 0xFFFFFFFFu;
        for (int c = 0; c < 3; c++) l.L[c] = L[c];
        s->lights.push_back(l);
    }
    s->uploaded = false;
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_set_camera_perspective(PbrtHipScene* s, const float r2c[16], const float c2w[16], float lens_radius, float focal_distance,
                                    float shutter_open, float shutter_close) {
    return ph_guard(s, "pbrt_hip_set_camera_perspective", [&]() -> int {
    if (!s || !r2c || !c2w) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_camera_perspective: null argument");
    std::memcpy(s->cam.r2c, r2c, 64); std::memcpy(s->cam.c2w, c2w, 64);
    s->cam.lens_radius = lens_radius; s->cam.focal_distance = focal_distance;
    s->cam.shutter_open = shutter_open; s->cam.shutter_close = shutter_close;
    {   // dx_camera / dy_camera (perspective_camera.rs:70-74): raster_to_camera(1,0,0) - raster_to_camera(0,0,0), same for y
        auto pt = [&](float x, float y, float out[3]) {  // Transform::transform_point (transform.rs:288-302)
            const float* m = r2c;
            const float xp = m[0] * x + m[1] * y + m[2] * 0.0f + m[3], yp = m[4] * x + m[5] * y + m[6] * 0.0f + m[7];
            const float zp = m[8] * x + m[9] * y + m[10] * 0.0f + m[11], wp = m[12] * x + m[13] * y + m[14] * 0.0f + m[15];
            if (wp == 1.0f) { out[0] = xp; out[1] = yp; out[2] = zp; }
            else { const float inv = 1.0f / wp; out[0] = inv * xp; out[1] = inv * yp; out[2] = inv * zp; }  // Point3 / f (point3.rs: times the reciprocal)
        };
        float p0[3], px[3], py[3];
        pt(0.0f, 0.0f, p0); pt(1.0f, 0.0f, px); pt(0.0f, 1.0f, py);
        for (int k = 0; k < 3; k++) { s->cam.dx_camera[k] = px[k] - p0[k]; s->cam.dy_camera[k] = py[k] - p0[k]; }
    }
    s->cam.kind = PH_CAM_PERSPECTIVE;
    s->have_camera = true;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_set_camera_orthographic(PbrtHipScene* s, const float r2c[16], const float c2w[16], float lens_radius, float focal_distance,
                                     float shutter_open, float shutter_close) {  // OrthographicCamera::new (orthographic_camera.rs:39-72)
    return ph_guard(s, "pbrt_hip_set_camera_orthographic", [&]() -> int {
    const int rc = pbrt_hip_set_camera_perspective(s, r2c, c2w, lens_radius, focal_distance, shutter_open, shutter_close);
    if (rc != PBRT_HIP_OK) return rc;
    // dx_camera / dy_camera (:58-64): raster_to_camera.transform_vector((1,0,0)) / ((0,1,0)) (transform.rs:373-380)
    const float* m = r2c;
    const float vx[3] = {1.0f, 0.0f, 0.0f}, vy[3] = {0.0f, 1.0f, 0.0f};
    for (int k = 0; k < 3; k++) {
        s->cam.dx_camera[k] = m[4 * k] * vx[0] + m[4 * k + 1] * vx[1] + m[4 * k + 2] * vx[2];
        s->cam.dy_camera[k] = m[4 * k] * vy[0] + m[4 * k + 1] * vy[1] + m[4 * k + 2] * vy[2];
    }
    s->cam.kind = PH_CAM_ORTHOGRAPHIC;
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_set_camera_environment(PbrtHipScene* s, const float c2w[16], int xres, int yres, float shutter_open, float shutter_close) {  // environment_camera.rs:27-41
    return ph_guard(s, "pbrt_hip_set_camera_environment", [&]() -> int {
    if (!s || !c2w) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_camera_environment: null argument");
    if (xres <= 0 || yres <= 0) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_camera_environment: the film's full resolution must be positive");
    s->cam = CameraRec{};
    for (int k = 0; k < 4; k++) s->cam.r2c[5 * k] = 1.0f;   // unused by this camera; identity keeps the shared prologue of the ray generator finite
    std::memcpy(s->cam.c2w, c2w, 64);
    s->cam.focal_distance = 1e6f; s->cam.shutter_open = shutter_open; s->cam.shutter_close = shutter_close;
    s->cam.full_res[0] = (float)xres; s->cam.full_res[1] = (float)yres;
    s->cam.kind = PH_CAM_ENVIRONMENT;
    s->have_camera = true;
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_set_film(PbrtHipScene* s, int xres, int yres, const int crop[4], const float radius[2], const float table[256], float scale,
                      float max_lum) {
    return ph_guard(s, "pbrt_hip_set_film", [&]() -> int {
    if (!s || !crop || !radius || !table) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_film: null argument");
    if (!(radius[0] > 0.0f) || !(radius[1] > 0.0f)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_film: filter radius must be positive");
    FilmRec& f = s->film;
    f.xres = xres; f.yres = yres;
    for (int i = 0; i < 4; i++) f.crop[i] = crop[i];
    f.radius[0] = radius[0]; f.radius[1] = radius[1];
    f.inv_radius[0] = 1.0f / radius[0]; f.inv_radius[1] = 1.0f / radius[1];  // film_tile.rs:50
    f.scale = scale; f.max_lum = max_lum;
    std::memcpy(f.table, table, sizeof(f.table));
    s->have_film = true;
    return PBRT_HIP_OK;
    });
}

static void ext_gcd(uint64_t a, uint64_t b, int64_t& x, int64_t& y) {  // halton.rs:294-302
    if (b == 0) { x = 1; y = 0; return; }
    int64_t d = (int64_t)(a / b), xp, yp;
    ext_gcd(b, a % b, xp, yp);
    x = yp; y = xp - (d * yp);
}
static uint64_t mult_inverse(int64_t a, int64_t n) {  // halton.rs:304-311
    int64_t x, y;
    ext_gcd((uint64_t)a, (uint64_t)n, x, y);
    int64_t r = x - (x / n) * n;
    return (uint64_t)(r < 0 ? r + n : r);
}

int pbrt_hip_set_sampler(PbrtHipScene* s, int kind, uint32_t spp, const int sb[4], int at_center) {
    return ph_guard(s, "pbrt_hip_set_sampler", [&]() -> int {
    if (!s || !sb) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_sampler: null argument");
    if (kind != 0 && kind != 1) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "set_sampler: only halton (0) and sobol (1) are GPU-friendly (SURVEY §8a-S)");
    if (spp == 0) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_sampler: spp must be > 0");
    SamplerRec& r = s->sampler;
    std::memset(&r, 0, sizeof(r));
    r.kind = kind; r.spp = spp; r.at_center = at_center ? 1 : 0;
    for (int i = 0; i < 4; i++) r.bounds[i] = sb[i];
    if (kind == 0) {  // HaltonSampler::new (halton.rs:61-100)
        int res[2] = {sb[2] - sb[0], sb[3] - sb[1]};
        for (int i = 0; i < 2; i++) {
            uint64_t base = i == 0 ? 2 : 3, scale = 1, e = 0;
            while ((int)scale < std::min(res[i], 128)) { scale *= base; e++; }
            r.base_scales[i] = (uint32_t)scale; r.base_exponents[i] = (uint32_t)e;
        }
        r.sample_stride = r.base_scales[0] * r.base_scales[1];
        r.mult_inverse[0] = (uint32_t)mult_inverse(r.base_scales[1], r.base_scales[0]);
        r.mult_inverse[1] = (uint32_t)mult_inverse(r.base_scales[0], r.base_scales[1]);
        if (((uint64_t)spp + 1) * r.sample_stride >= (1ull << 32))
            return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "set_sampler: halton index exceeds 32 bits at this spp/resolution");
    } else {  // SobolSampler::new (sobol.rs:35-63)
        auto pow2_up = [](uint32_t v) { v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v + 1; };
        if (spp & (spp - 1)) r.spp = pow2_up(spp);
        int ext = std::max(sb[2] - sb[0], sb[3] - sb[1]);
        r.resolution = (int)pow2_up((uint32_t)std::max(ext, 1));
        int lg = 0; for (uint32_t v = (uint32_t)r.resolution; v >>= 1;) lg++;
        r.log2_resolution = lg;
    }
    s->have_sampler = true;
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_set_sobol_tables(PbrtHipScene* s, const uint32_t* m32, size_t n32, const uint64_t* vdc, const uint64_t* vdc_inv, size_t n_each) {
    return ph_guard(s, "pbrt_hip_set_sobol_tables", [&]() -> int {
    if (!s || !m32 || !vdc || !vdc_inv) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_sobol_tables: null argument");
    // 52 entries per dimension / per VdC matrix: check_render_args bounds every Sobol render by what was given here
    if (n32 == 0 || n32 % 52 || n_each % 52) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "set_sobol_tables: table lengths must be non-zero multiples of 52");
    s->sobol32.assign(m32, m32 + n32); s->vdc.assign(vdc, vdc + n_each); s->vdc_inv.assign(vdc_inv, vdc_inv + n_each);
    s->uploaded = false;
    return PBRT_HIP_OK;
    });
}

}  // extern "C"

// ---- build_accel: one entry behind the three public ones (AccelBuilder, scene_host.h), cut into its steps ----------------------------------------------------------------
// what no builder takes, before any work; changes nothing but the error text
static int refuse_accel_build(PbrtHipScene* s, AccelBuilder builder, int split_method) {
    if (split_method == 2) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "build_accel: splitmethod 'middle' panics in the reference (quirk B6, sah.rs:67-76)");
    if (!s->quadrics.empty()) {
        // Both device builders take quadrics (bvh_device.hip, bvh_sah_device.hip).  pbrt_hip_build_accel_device keeps refusing the SAH tree, an answer older tests pin for split
        // method 0: pbrt_hip_build_accel_device_shapes builds it.
        if (builder == AccelBuilder::Device && split_method != 1)
            return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "build_accel_device: the SAH tree of a scene with quadric shapes is built on the device by pbrt_hip_build_accel_device_shapes, or on the host (pbrt_hip_build_accel); the HLBVH tree (1) is built on the device");
        // A leftover with no technical reason: a scene whose object definitions are all unused would build (its definitions are ignored, as in any instanced scene), but two older tests
        // pin this answer.  To be dropped together with their assertions.
        if (!s->objects.empty() && s->instances.empty())
            return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "build_accel: quadric shapes together with object definitions that no instance uses are not supported (a leftover refusal without a technical reason; instance an object, or drop the definitions)");
        // (object instances and alpha-mask textures on the triangle meshes are traversal's business: the QUADRIC rows of TravShapes)
    }
    // every DiffuseAreaLight belongs to a shape (api/src/lib.rs:783-812 creates them per triangle): one that no add_mesh claimed would be sampled
    // through a primitive that does not exist
    for (size_t i = 0; i < s->lights.size(); i++)
        if (s->lights[i].type == PH_L_AREA && s->lights[i].prim == 0xFFFFFFFFu)
            return set_err(s, PBRT_HIP_ERR_STATE, "build_accel: area light " + std::to_string(i) + " was never attached to a mesh (pbrt_hip_add_mesh first_area_light_id)");
    return PBRT_HIP_OK;
}

// material classes (shade-side sorting key): materials with the same sequence of lobe kinds share a class; at most 7 classes
static void assign_material_sort_classes(PbrtHipScene* s) {
    std::vector<uint64_t> sigs;
    for (phost::MaterialHost::Item& it : s->mats.items) {
        MaterialRec& m = it.rec;
        uint64_t sig = 1;
        for (const LobeRec& l : it.lobes) sig = sig * 8 + (l.kind + 1);
        size_t c = 0;
        while (c < sigs.size() && sigs[c] != sig) c++;
        if (c == sigs.size()) sigs.push_back(sig);
        m.sort_class = (uint32_t)std::min<size_t>(c, 6);
        if (m.none) m.sort_class = 7u;
    }
}

// shade-side sorting keys travel in the TriRec: the material's class and its id (scene_types.h)
static std::vector<uint32_t> triangle_build_flags(const PbrtHipScene* s) {
    std::vector<uint32_t> build_flags(s->tri_flags);
    for (size_t t = 0; t < build_flags.size(); t++) {
        const uint32_t mat = s->meshes[s->tri_mesh[t]].material;
        build_flags[t] |= (s->mats.items[mat].rec.sort_class << PH_TRI_CLASS_SHIFT) | (std::min<uint32_t>(mat, 0xFFFu) << PH_TRI_MAT_SHIFT);
    }
    return build_flags;
}

// a builder's answer as the entry's: 0, -1 from a device builder (`e` says what), -2 (the reference's HLBVH assertions), anything else
static int build_answer(PbrtHipScene* s, int brc, bool on_device, const std::string& e) {
    if (brc == 0) return PBRT_HIP_OK;
    if (brc == -1 && on_device) return set_err(s, PBRT_HIP_ERR_DEVICE, "build_accel_device: " + e);
    if (brc == -2) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "build_accel: the reference's HLBVH build asserts on this input (hlbvh.rs:338/356/418)");
    return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "build_accel: bad arguments");
}

// the device builders, on one tree (spec, trees null) or a forest: SAH leaves its arrays where it built them (s->dev_tree), HLBVH hands them back in s->bvh (its numbering is the host's)
static int build_on_device(PbrtHipScene* s, const phost::BuildInput& in, int split_method, int max_prims_in_node, const phost::ForestSpec* spec, std::vector<phost::ForestTreeOut>* trees) {
    PH_CHECK(s, hipSetDevice(s->device));
    std::string e;
    const int brc = split_method == 1 ? phost::build_hlbvh_device(in, max_prims_in_node, s->stream, s->bvh, e, spec, trees)
                                      : phost::build_sah_device(in, max_prims_in_node, s->stream, s->bvh, e, &s->dev_tree, spec, trees);
    return build_answer(s, brc, true, e);
}

// One aggregate per instanced object (make_accelerator at ObjectInstance time, lib.rs:953-971) and the scene's own over its triangles and TransformedPrimitives,
// in one node array and one TriRec array: [scene | objects] (bvh_build.h).  layout, trees: where each instance's tree went and every tree's root.
static int build_forest(PbrtHipScene* s, const phost::BuildInput& in, bool on_device, int split_method, int max_prims_in_node, phost::ForestLayout& layout, std::vector<phost::ForestTreeOut>& trees) {
    if (s->open_object >= 0) return set_err(s, PBRT_HIP_ERR_STATE, "build_accel: an object definition is still open (missing ObjectEnd)");
    std::vector<uint32_t> tri0(s->objects.size()), tri1(s->objects.size()), inst_object(s->instances.size());
    std::vector<float> inst_i2w(16 * s->instances.size());
    for (size_t k = 0; k < s->objects.size(); k++) { tri0[k] = s->objects[k].tri0; tri1[k] = s->objects[k].tri1; }
    for (size_t k = 0; k < s->instances.size(); k++) { inst_object[k] = s->instances[k].object; std::memcpy(&inst_i2w[16 * k], s->instances[k].i2w, 64); }
    const phost::InstancedScene isc{tri0.data(), tri1.data(), tri0.size(), inst_object.data(), inst_i2w.data(), inst_object.size(), s->top_items.data(), s->top_items.size()};
    phost::forest_layout(isc, layout);
    // bit 30 of a leaf reference is PH_LEAF_INST_HINT in an instanced scene: the forest's records must stay below it (both builders)
    if (layout.items.size() >= 0x40000000ull) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "build_accel: an instanced scene may hold at most 2^30 leaf records");
    if (!on_device) return build_answer(s, phost::build_forest_host(in, isc, layout, split_method, max_prims_in_node, s->bvh, trees), false, "");
    const phost::ForestSpec spec = layout.spec(isc);
    return build_on_device(s, in, split_method, max_prims_in_node, &spec, &trees);
}

// every instance's record, from the root of its object's tree
static void make_instance_records(PbrtHipScene* s, const phost::ForestLayout& layout, const std::vector<phost::ForestTreeOut>& trees) {
    for (size_t k = 0; k < s->instances.size(); k++) {
        const PbrtHipScene::InstanceHost& ih = s->instances[k];
        const phost::ForestTreeOut& b = trees[layout.inst_tree[k]];
        InstRec r{};
        std::memcpy(r.w2i, ih.w2i, 64); std::memcpy(r.i2w, ih.i2w, 64);
        for (int a = 0; a < 3; a++) { r.lo[a] = b.lo[a]; r.hi[a] = b.hi[a]; }
        r.root_ref = b.root_ref; r.flags = b.n_items == 1 ? PH_INST_SINGLE : 0u;   // an object with one primitive is used directly, without an aggregate (lib.rs:953-956)
        bool ident = true;
        for (int a = 0; a < 16; a++) if (ih.i2w[a] != ((a % 5 == 0) ? 1.0f : 0.0f)) ident = false;
        if (ident) r.flags |= PH_INST_IDENTITY;
        s->inst_recs.push_back(r);
    }
}

// Light::preprocess: bounding sphere of the world bound (bounds3.rs:196-208; infinite.rs:113-117, distant.rs:54-58)
static void set_world_sphere(PbrtHipScene* s) {
    s->world_radius = 1.0f; s->world_center[0] = s->world_center[1] = s->world_center[2] = 0.0f;
    if (s->bvh.root_ref == PH_INVALID_REF) return;
    const float* lo = s->bvh.root_lo; const float* hi = s->bvh.root_hi;
    float c[3];
    for (int k = 0; k < 3; k++) c[k] = (1.0f - 0.5f) * lo[k] + 0.5f * hi[k];  // lerp(0.5, pmin, pmax) (common.rs:166-175)
    bool inside = (c[0] >= lo[0] && c[0] <= hi[0]) && (c[1] >= lo[1] && c[1] <= hi[1]) && (c[2] >= lo[2] && c[2] <= hi[2]);
    float dx = c[0] - hi[0], dy = c[1] - hi[1], dz = c[2] - hi[2];
    s->world_radius = inside ? std::sqrt(dx * dx + dy * dy + dz * dz) : 0.0f;
    for (int k = 0; k < 3; k++) s->world_center[k] = c[k];
}

static int build_accel(PbrtHipScene* s, AccelBuilder builder, int split_method, int max_prims_in_node) {
    if (int rc = refuse_accel_build(s, builder, split_method)) return rc;
    assign_material_sort_classes(s);
    if (s->accel_on_device()) { PH_CHECK(s, hipSetDevice(s->device)); free_tree_dev(s->dev_tree); }   // a rebuild: the tree an earlier device build left there goes first
    const std::vector<uint32_t> build_flags = triangle_build_flags(s);
    phost::BuildInput in;
    in.P = s->P.data(); in.idx = s->idx.data(); in.n_tris = s->idx.size() / 3; in.tri_flags = build_flags.data(); in.tri_mesh = s->tri_mesh.data();
    if (!s->quadrics.empty()) { s->prim_quadric.resize(in.n_tris, 0u); in.prim_quadric = s->prim_quadric.data(); in.quad_bounds = s->quadric_bounds.data(); in.n_quadrics = s->quadrics.size(); }
    const bool on_device = builder != AccelBuilder::Host;
    s->inst_recs.clear();
    if (s->objects.empty()) {
        // a scene without object definitions: one tree
        const int rc = on_device ? build_on_device(s, in, split_method, max_prims_in_node, nullptr, nullptr) : build_answer(s, phost::build_bvh(in, split_method, max_prims_in_node, 0, s->bvh), false, "");
        if (rc) return rc;
    } else {
        phost::ForestLayout layout;
        std::vector<phost::ForestTreeOut> trees;
        if (int rc = build_forest(s, in, on_device, split_method, max_prims_in_node, layout, trees)) return rc;
        make_instance_records(s, layout, trees);
    }
    set_world_sphere(s);
    s->built = true; s->uploaded = false;
    return PBRT_HIP_OK;
}

// the two device entries: their own argument check in front of build_accel
static int build_accel_by_kernels(PbrtHipScene* s, AccelBuilder builder, int split_method, int max_prims_in_node) {
    if (!s) return PBRT_HIP_ERR_INVALID_ARG;
    if (split_method != 0 && split_method != 1) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "build_accel_device: the device builders make the SAH (0) and the HLBVH (1) tree; EqualCounts is built on the host");
    return build_accel(s, builder, split_method, max_prims_in_node);
}

extern "C" {

int pbrt_hip_build_accel(PbrtHipScene* s, int split_method, int max_prims_in_node) {
    return ph_guard(s, "pbrt_hip_build_accel", [&]() -> int { return s ? build_accel(s, AccelBuilder::Host, split_method, max_prims_in_node) : PBRT_HIP_ERR_INVALID_ARG; });
}
// BVHAccel::from with splitmethod "sah" (the default) or "hlbvh", constructed on the GPU (bvh_sah_device.hip, bvh_device.hip): same tree, same leaf order as pbrt_hip_build_accel
int pbrt_hip_build_accel_device(PbrtHipScene* s, int split_method, int max_prims_in_node) {
    return ph_guard(s, "pbrt_hip_build_accel_device", [&]() -> int { return build_accel_by_kernels(s, AccelBuilder::Device, split_method, max_prims_in_node); });
}
// pbrt_hip_build_accel_device, except that the SAH tree (0) of a scene with quadric shapes is built as well
int pbrt_hip_build_accel_device_shapes(PbrtHipScene* s, int split_method, int max_prims_in_node) {
    return ph_guard(s, "pbrt_hip_build_accel_device_shapes", [&]() -> int { return build_accel_by_kernels(s, AccelBuilder::DeviceShapes, split_method, max_prims_in_node); });
}

int pbrt_hip_world_bound(const PbrtHipScene* s, float out[6]) {
    return ph_guard(const_cast<PbrtHipScene*>(s), "pbrt_hip_world_bound", [&]() -> int {
    if (!s || !out) return PBRT_HIP_ERR_INVALID_ARG;
    if (!s->built) return PBRT_HIP_ERR_STATE;
    for (int k = 0; k < 3; k++) { out[k] = s->bvh.root_lo[k]; out[3 + k] = s->bvh.root_hi[k]; }
    return PBRT_HIP_OK;
    });
}

// measurement aid: sizes of the built acceleration structure in the device layout (bvh/common.rs:8-23 keeps the same tallies as statistics)
int pbrt_hip_accel_stats(const PbrtHipScene* s, uint64_t out[8]) {
    return ph_guard(const_cast<PbrtHipScene*>(s), "pbrt_hip_accel_stats", [&]() -> int {
    if (!s || !out) return PBRT_HIP_ERR_INVALID_ARG;
    if (!s->built) return PBRT_HIP_ERR_STATE;
    out[0] = s->accel_n_nodes(); out[1] = s->accel_n_records();
    out[2] = out[0] * sizeof(Node64); out[3] = out[1] * sizeof(TriRec);
    out[4] = s->bvh.leaf_nodes; out[5] = (uint64_t)s->bvh.max_depth; out[6] = s->bvh.max_leaf_prims;
    out[7] = (uint64_t)(s->bvh.build_seconds * 1e6);
    return PBRT_HIP_OK;
    });
}

// test aid: the built structure itself (device layout), wherever it lives
int pbrt_hip_accel_copy(PbrtHipScene* s, void* out_nodes, uint64_t node_capacity, void* out_leaf_records, uint64_t record_capacity) {
    return ph_guard(s, "pbrt_hip_accel_copy", [&]() -> int {
    if (!s) return PBRT_HIP_ERR_INVALID_ARG;
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, "accel_copy: build_accel first");
    const size_t nn = s->accel_n_nodes(), nt = s->accel_n_records();
    if (node_capacity < nn || record_capacity < nt) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "accel_copy: buffers too small (pbrt_hip_accel_stats gives the sizes)");
    if (s->accel_on_device()) {
        PH_CHECK(s, hipSetDevice(s->device));
        if (nn && out_nodes) PH_CHECK(s, hipMemcpy(out_nodes, s->accel_nodes(), nn * sizeof(Node64), hipMemcpyDeviceToHost));
        if (nt && out_leaf_records) PH_CHECK(s, hipMemcpy(out_leaf_records, s->accel_records(), nt * sizeof(TriRec), hipMemcpyDeviceToHost));
        if (!s->inst_recs.empty()) {   // an upload may have filled the instance records and set the hints in place (patch_inst_records_kernel): hand out the builder's form
            if (out_nodes) { Node64* nd = static_cast<Node64*>(out_nodes); for (size_t i = 0; i < nn; i++) { if ((nd[i].c0 & PH_LEAF_BIT) && nd[i].c0 < PH_NEED_POP) nd[i].c0 &= ~PH_LEAF_INST_HINT; if ((nd[i].c1 & PH_LEAF_BIT) && nd[i].c1 < PH_NEED_POP) nd[i].c1 &= ~PH_LEAF_INST_HINT; } }
            if (out_leaf_records) { TriRec* tr = static_cast<TriRec*>(out_leaf_records); for (size_t i = 0; i < nt; i++) { tr[i].flags &= ~PH_TRI_NEXT_INST; if (tr[i].flags & PH_TRI_INSTANCE) { const uint32_t prim = tr[i].prim, fl = tr[i].flags; std::memset(&tr[i], 0, sizeof(TriRec)); tr[i].prim = prim; tr[i].flags = fl; } } }
        }
    } else {
        if (nn && out_nodes) std::memcpy(out_nodes, s->accel_nodes(), nn * sizeof(Node64));
        if (nt && out_leaf_records) std::memcpy(out_leaf_records, s->accel_records(), nt * sizeof(TriRec));
    }
    return PBRT_HIP_OK;
    });
}

static int batch_common(PbrtHipScene* s, bool anyhit, const void* rays, void* out, uint64_t n, bool device_ptrs, float* kernel_ms) {
    if (!s) return PBRT_HIP_ERR_INVALID_ARG;
    if (n && (!rays || !out)) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "batch: null buffer");
    if (!s->built) return set_err(s, PBRT_HIP_ERR_STATE, "batch: call pbrt_hip_build_accel first");
    if (n > 0xFFFF0000ull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "batch: at most 2^32-65536 rays per call");
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;
    if (n == 0) return PBRT_HIP_OK;
    const size_t out_bytes = anyhit ? (size_t)n : (size_t)n * sizeof(PbrtHipHit);
    const void* d_rays = rays; void* d_out = out;
    if (!device_ptrs) {
        if ((rc = ensure_buf(s, s->d_rays_tmp, (size_t)n * sizeof(PbrtHipRay)))) return rc;
        if ((rc = ensure_buf(s, s->d_out_tmp, out_bytes))) return rc;
        PH_CHECK(s, hipMemcpyAsync(s->d_rays_tmp.p, rays, (size_t)n * sizeof(PbrtHipRay), hipMemcpyHostToDevice, s->stream));
        d_rays = s->d_rays_tmp.p; d_out = s->d_out_tmp.p;
    }
    if ((rc = launch_traverse(s, anyhit, d_rays, d_out, (uint32_t)n, kernel_ms))) return rc;
    if (!device_ptrs) PH_CHECK(s, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s->stream));
    PH_CHECK(s, hipStreamSynchronize(s->stream));
    return traversal_overflow_check(s);
}

int pbrt_hip_intersect_batch(PbrtHipScene* s, const PbrtHipRay* rays, PbrtHipHit* hits, uint64_t n) { return ph_guard(s, "pbrt_hip_intersect_batch", [&]() -> int { return batch_common(s, false, rays, hits, n, false, nullptr); }); }
int pbrt_hip_occluded_batch(PbrtHipScene* s, const PbrtHipRay* rays, uint8_t* out, uint64_t n) { return ph_guard(s, "pbrt_hip_occluded_batch", [&]() -> int { return batch_common(s, true, rays, out, n, false, nullptr); }); }
int pbrt_hip_intersect_batch_device(PbrtHipScene* s, const void* d_rays, void* d_hits, uint64_t n, float* ms) { return ph_guard(s, "pbrt_hip_intersect_batch_device", [&]() -> int { return batch_common(s, false, d_rays, d_hits, n, true, ms); }); }
int pbrt_hip_occluded_batch_device(PbrtHipScene* s, const void* d_rays, void* d_occ, uint64_t n, float* ms) { return ph_guard(s, "pbrt_hip_occluded_batch_device", [&]() -> int { return batch_common(s, true, d_rays, d_occ, n, true, ms); }); }

// Roofline bookkeeping: with counting on, every traversal launch also accumulates the work it did.
// out[0..2] closest-hit {interior nodes passed, triangle tests, rays}, out[3..5] any-hit.  Reference-format node visits of
// the closest-hit rays = rays + 2*out[0] (see traverse.h).  Reading resets the counters.
int pbrt_hip_set_traversal_counting(PbrtHipScene* s, int on) {
    return ph_guard(s, "pbrt_hip_set_traversal_counting", [&]() -> int {
    if (!s) return PBRT_HIP_ERR_INVALID_ARG;
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_traversal_workspace(s))) return rc;
    PH_CHECK(s, hipMemset(s->d_counts.p, 0, 64 + 36 * 8));
    s->count_traversal = on != 0;
    return PBRT_HIP_OK;
    });
}
int pbrt_hip_get_traversal_counts(PbrtHipScene* s, uint64_t out[8]) {
    return ph_guard(s, "pbrt_hip_get_traversal_counts", [&]() -> int {
    if (!s || !out) return PBRT_HIP_ERR_INVALID_ARG;
    if (!s->d_counts.p) { for (int i = 0; i < 8; i++) out[i] = 0; return PBRT_HIP_OK; }
    PH_CHECK(s, hipSetDevice(s->device));
    PH_CHECK(s, hipStreamSynchronize(s->stream));
    PH_CHECK(s, hipMemcpy(out, s->d_counts.p, 64, hipMemcpyDeviceToHost));
#if PH_PHASE_CLOCK
    {   // measurement build: the waves' phase clocks since the last call, to stderr
        unsigned long long ph[36];
        PH_CHECK(s, hipMemcpy(ph, (const char*)s->d_counts.p + 64, sizeof ph, hipMemcpyDeviceToHost));
        static const char* names[10] = {"refill", "node_steps", "instance_entry", "triangle_test", "alpha_test", "instance_exit", "retire", "whole_loop", "stack_pops", "leaf_step_whole"};
        for (int k = 0; k < 10; k++)
            std::fprintf(stderr, "PHASE_CLOCK %-15s cycles %14llu (%5.1f %% of the loop)  executions %12llu  mean active lanes %5.1f\n", names[k], ph[k], ph[7] ? 100.0 * (double)ph[k] / (double)ph[7] : 0.0,
                         ph[12 + k], ph[12 + k] ? (double)ph[24 + k] / (double)ph[12 + k] : 0.0);
    }
    PH_CHECK(s, hipMemset(s->d_counts.p, 0, 64 + 36 * 8));
#else
    PH_CHECK(s, hipMemset(s->d_counts.p, 0, 64 + 36 * 8));
#endif
    return PBRT_HIP_OK;
    });
}

// Film::get_pixel_rgb (core/src/film/mod.rs:392-417); splat is identically zero for the path integrator (quirk B3 kept)
int pbrt_hip_film_to_rgb(const PbrtHipScene* s, const float* xyz, const float* weight, float* out_rgb) {
    return ph_guard(const_cast<PbrtHipScene*>(s), "pbrt_hip_film_to_rgb", [&]() -> int {
    if (!s || !xyz || !weight || !out_rgb) return PBRT_HIP_ERR_INVALID_ARG;
    if (!s->have_film) return PBRT_HIP_ERR_STATE;
    const FilmRec& f = s->film;
    const int w = f.crop[2] - f.crop[0], h = f.crop[3] - f.crop[1];
    const size_t n = (size_t)std::max(w, 0) * (size_t)std::max(h, 0);
    auto to_rgb = [](const float* x, float* r) {  // xyz_to_rgb (spectrum/common.rs:337-343)
        r[0] = 3.240479f * x[0] - 1.537150f * x[1] - 0.498535f * x[2];
        r[1] = -0.969256f * x[0] + 1.875991f * x[1] + 0.041556f * x[2];
        r[2] = 0.055648f * x[0] - 0.204043f * x[1] + 1.057311f * x[2];
    };
    const float zero[3] = {0, 0, 0};
    float splat_rgb[3];
    to_rgb(zero, splat_rgb);
    for (size_t i = 0; i < n; i++) {
        float rgb[3];
        to_rgb(xyz + 3 * i, rgb);
        for (int c = 0; c < 3; c++) {
            float v = rgb[c];
            if (weight[i] != 0.0f) { float inv = 1.0f / weight[i]; float q = v * inv; v = 0.0f > q ? 0.0f : q; }
            v += 1.0f * splat_rgb[0];
            v *= f.scale;
            out_rgb[3 * i + c] = v;
        }
    }
    return PBRT_HIP_OK;
    });
}

}  // extern "C"
