// Host-side scene object behind the opaque PbrtHipScene handle (include/pbrt_hip.h).
#pragma once
#include "../../include/pbrt_hip.h"
#include "band_plan.h"
#include "bvh_build.h"
#include "guard.h"
#include "material_host.h"
#include "raysort_plan.h"
#include "scene_types.h"
#include "shade_shapes.h"
#include <hip/hip_runtime.h>
namespace ph { struct TravParams; struct SpatialRec; }
#include <string>
#include <vector>

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// Everything the capture calls record and build_accel derives, i.e. the part of a scene that does not belong to a device.  A multi-device handle
// (pbrt_hip_scene_create_multi) copies it as a whole to its per-device contexts (multi.hip).
struct SceneHostState {
    // ---- captured scene (host copies, add_mesh order) ----------------------------------------------------------------
    std::vector<float> P, N, S, UV;  // N/S/UV are vertex-aligned with P when any mesh has them (zero-filled otherwise)
    bool any_n = false, any_s = false, any_uv = false;
    std::vector<uint32_t> idx, tri_mesh, tri_flags;
    std::vector<MeshRec> meshes;
    // quadric shapes (add_sphere / add_quadric / add_hyperboloid): each owns one MeshRec and ONE slot of the primitive list (idx holds three zeros for it, tri_flags 0: the builder sets PH_TRI_QUADRIC in the leaf record from prim_quadric);
    // quadric_bounds = its Shape::world_bound {lo xyz, hi xyz}; prim_quadric[prim] = 0, or 1 + the quadric in that slot (sized with the primitive list once a quadric exists)
    std::vector<QuadricRec> quadrics;
    std::vector<CurveRec> curves;   // one CurveData per add_curve, named by its segments' QuadricRec::curve (a segment is a quadric slot of kind PH_Q_CURVE)
    std::vector<float> quadric_bounds;
    std::vector<uint32_t> prim_quadric;
    phost::MaterialHost mats;        // every material's description, record and lobe list (material_host.h); the device arrays are laid out at upload
    // textures: every texture id owns a flattened postfix program (its children's programs followed by its own op)
    struct TextureHost { std::vector<TexOp> prog; int stack_need = 1; };
    std::vector<TextureHost> textures;
    std::vector<MipRec> mipmaps;
    std::vector<Texel> texels;
    bool alpha_textures = false;      // some mesh has an alpha / shadowalpha texture: traversal uses the ALPHA kernel variants
    bool alpha_lean = false;          // ... and all of them are constants / uv-mapped image maps / scale / mix: the inlined test (set at upload)
    bool bump_materials = false;      // some material has a bump map (these four: material_changed, after every change to a material; other scene content sets some of them too)
    bool textured_materials = false;  // some material evaluates a texture per hit
    bool has_none_material = false;  // some material is "none": paths may need more wavefront iterations than max_depth + 1
    bool general_materials = false;  // some material is not matte: the renderer uses the general BSDF kernel
    bool simple_textures = false;    // every texture program is made of constants, image maps (uv mapping), scale and mix: the texture pass runs its lean instantiation (set at upload)
    std::vector<LightRec> lights;
    uint32_t quadric_lights = 0;     // lights whose shape is a disk or a cylinder (add_quadric_light): both drivers sample them, the path integrator with no switch (the reference answers at every reference point)
    uint32_t sphere_lights = 0;      // lights whose shape is a sphere (add_sphere_light): the Whitted driver samples them; the path integrator does on a handle with path_sphere_lights set and refuses the scene on any other
    // DiffuseAreaLights of shapes inside an object definition ("Area lights not supported with object instancing", api/src/lib.rs:877-881): the primitives keep their emission,
    // Scene::lights never sees them.  MeshRec::first_light = -2 - index on the host; uploaded behind the scene's lights (DeviceScene::n_lights does not count them).
    std::vector<LightRec> emission_only;
    std::vector<uint32_t> infinite_lights;
    std::vector<float> light_dist;   // Distribution2D tables of infinite lights with a radiance map
    // object instancing (api/src/lib.rs:911-1000): an object is a contiguous triangle range; top_items is the scene's primitive
    // list in directive order (triangle id, or PH_ITEM_INST | instance index)
    struct ObjectHost { uint32_t tri0 = 0, tri1 = 0; };
    struct InstanceHost { uint32_t object; float i2w[16], w2i[16]; };
    std::vector<ObjectHost> objects;
    std::vector<InstanceHost> instances;
    std::vector<uint32_t> top_items;
    int open_object = -1;
    std::vector<InstRec> inst_recs;  // built by build_accel
    CameraRec cam{};
    FilmRec film{};
    SamplerRec sampler{};
    bool have_camera = false, have_film = false, have_sampler = false, built = false;
    std::vector<uint32_t> sobol32;
    std::vector<uint64_t> vdc, vdc_inv;

    // ---- acceleration structure ---------------------------------------------------------------------------------------
    phost::BuildOutput bvh;
    float world_center[3] = {0, 0, 0}, world_radius = 1.0f;
};

struct MultiDevice;  // multi.hip

enum class AccelBuilder { Host, Device, DeviceShapes };   // which builder a public entry asks build_accel (api.hip) for: pbrt_hip_build_accel, _device, _device_shapes
// A tree that stays where a device builder made it (the SAH builder's, bvh_sah_device.hip): device allocations the handle owns, and how many entries each holds.
struct DeviceTree { Node64* nodes = nullptr; TriRec* tris = nullptr; size_t n_nodes = 0, n_tris = 0; };

struct PbrtHipScene : SceneHostState {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    MultiDevice* multi = nullptr;    // non-null on a handle made by pbrt_hip_scene_create_multi: the other devices' contexts and the exchange state

    // ---- device residency ---------------------------------------------------------------------------------------------
    DeviceScene ds{};
    std::vector<void*> owned;        // every hipMalloc of the scene, freed on destroy / rebuild
    // a tree pbrt_hip_build_accel_device(0, ..) left where it was built: `bvh.nodes` / `bvh.tris` stay empty on the host.  Only build_accel, free_tree_dev and the multi-device
    // driver's peer copy touch it; every reader goes through the accessors below (the arrays are device memory when accel_on_device(), else the host vectors') and never asks where the tree is.
    DeviceTree dev_tree;
    bool accel_on_device() const { return dev_tree.tris != nullptr; }
    const Node64* accel_nodes() const { return accel_on_device() ? dev_tree.nodes : bvh.nodes.data(); }
    size_t accel_n_nodes() const { return accel_on_device() ? dev_tree.n_nodes : bvh.nodes.size(); }
    const TriRec* accel_records() const { return accel_on_device() ? dev_tree.tris : bvh.tris.data(); }
    size_t accel_n_records() const { return accel_on_device() ? dev_tree.n_tris : bvh.tris.size(); }
    int fetch_leaf_records(std::vector<TriRec>& out);   // the leaf records on the host: a device-to-host copy or a plain copy (api.hip); a PBRT_HIP_* code
    bool uploaded = false;
    // the light side of the scene's shade-pass features (shade_shapes.h), derived by upload_scene from the light list it uploads: every call that changes a light clears `uploaded`,
    // so the next render derives them again.  The sampler and the light strategy are read when the variant is picked (wavefront.hip, plan_path_frame).
    bool lights_infinite = false, lights_area = false, lights_delta = false;
    int light_strategy_uploaded = -1;
    DevBuf d_ld_func, d_ld_cdf;

    // traversal workspace
    DevBuf d_counter, d_spill, d_error, d_rays_tmp, d_out_tmp;
    uint32_t trav_blocks = 0;
    bool count_traversal = false;    // roofline bookkeeping mode (pbrt_hip_set_traversal_counting)
    DevBuf d_counts;                 // 8 u64: closest-hit {nodes, tris, rays}, any-hit {nodes, tris, rays}, any-hit reference node visits, spare
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // wavefront workspace (allocated lazily by the renderer, see wavefront.hip)
    struct Wavefront* wf = nullptr;
    struct WhittedWorkspace* wh = nullptr;   // the Whitted driver's (whitted.hip)

    // sample records (band_plan.h): the caller's byte budget for them, 0 = automatic (pbrt_hip_set_sample_record_budget), and what the last render came to
    // (pbrt_hip_get_render_footprint: bands, tiles in the largest band, peak record bytes, the budget that applied, paths per chunk, chunk-scaled bytes, 0, 0)
    uint64_t record_budget = 0;
    bool path_sphere_lights = false;   // pbrt_hip_set_path_sphere_lights: the path integrator samples sphere lights (SceneHostState::sphere_lights) instead of refusing the scene
    uint64_t footprint[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool last_mis_escape = false;      // what the last path render's plan said (PathPlan::mis_escape; pbrt_hip_get_mis_escape)
};

namespace phost {
int set_err(PbrtHipScene* s, int code, const std::string& msg);
int hip_fail(PbrtHipScene* s, hipError_t e, const char* what);
int ensure_buf(PbrtHipScene* s, DevBuf& b, size_t bytes);
int upload_scene(PbrtHipScene* s);
// after a call that changes s->mats (material_host.h): a refusal's message (nothing has changed then); else the scene flags take the materials' and the device copy is stale
inline int material_changed(PbrtHipScene* s, int rc, const std::string& why) {
    if (rc) return set_err(s, rc, why);
    const MaterialFlags f = s->mats.flags();
    s->general_materials |= f.general; s->textured_materials |= f.textured; s->bump_materials |= f.bump; s->has_none_material |= f.has_none;
    s->uploaded = false;
    return PBRT_HIP_OK;
}
// a texture program of constants, uv-mapped image maps, scale and mix only: what the lean alpha test (alpha_prog_r), the texture pass's SIMPLE evaluator and the texture probes' variants 2 to 4 admit
inline bool tex_prog_is_simple(const std::vector<TexOp>& prog) {
    for (const TexOp& op : prog)
        if (!(op.op == PH_TOP_CONST || op.op == PH_TOP_MUL || op.op == PH_TOP_MIX || (op.op == PH_TOP_IMAGE && op.mapping == 0u))) return false;
    return true;
}
void projection_light_setup(float fov_deg, float aspect, float out_proj[16], float out_screen[4], float* out_cos_total_width);   // host_setup.cpp
// MIPMap::lookup_triangle on the host copy of the texel pool (textures_api.hip), for what InfiniteAreaLight computes at construction time
void hmip_lookup_triangle(const PbrtHipScene* s, const MipRec& m, float u, float v, float width, float out[3]);
int upload_light_distribution(PbrtHipScene* s, int light_strategy);
int launch_traverse(PbrtHipScene* s, bool anyhit, const void* d_rays, void* d_out, uint32_t n, float* kernel_ms);
void launch_traverse_kernel(PbrtHipScene* s, int mode, uint32_t blocks, const ph::TravParams& p);  // 0 closest, 1 any hit, 2 both (MIXED)
int ensure_traversal_workspace(PbrtHipScene* s);
int traversal_overflow_check(PbrtHipScene* s);   // after the stream has drained: reads the traversal kernels' error flag, clears it, and reports a stack that ran over
// wavefront.hip: the ray binning between rounds (raysort.h) on device arrays, for callers that do not see the kernels; workspace = raysort_workspace_bytes(sort_blocks) bytes
inline size_t raysort_workspace_bytes(uint32_t sort_blocks) { return ((size_t)sort_blocks + 1) * PH_SORT_KEYS * 4; }
void launch_raysort(PbrtHipScene* s, const uint32_t* keys_cl, const uint32_t* keys_sh, const uint32_t* n_cl, const uint32_t* n_sh, uint32_t* order, uint32_t* workspace,
                    uint32_t sort_blocks);
void free_wavefront(PbrtHipScene* s);
// bvh_device.hip.  forest non-null: the forest form, as build_sah_device's below (the arrays come back on the host)
int build_hlbvh_device(const BuildInput& in, int max_prims_in_node, hipStream_t stream, BuildOutput& out, std::string& err, const ForestSpec* forest = nullptr,
                       std::vector<ForestTreeOut>* trees_out = nullptr);
// bvh_sah_device.hip.  keep non-null: the Node64 / TriRec arrays are not copied to `out` but handed over as device allocations (the caller frees them: free_tree_dev)
// forest non-null: the scene's aggregate and its instanced objects' aggregates in one build, laid out as build_forest_host lays them out; trees_out: every tree's root
int build_sah_device(const BuildInput& in, int max_prims_in_node, hipStream_t stream, BuildOutput& out, std::string& err, DeviceTree* keep = nullptr,
                     const ForestSpec* forest = nullptr, std::vector<ForestTreeOut>* trees_out = nullptr);
void free_tree_dev(DeviceTree& t);   // on the current device
// wavefront.hip: the renderer's building blocks, shared with the multi-device driver (multi.hip)
#define PH_MAX_TILE_PARTS 64
int check_render_args(PbrtHipScene* s, int max_depth, int light_strategy, const int* pixel_bounds, int tile_size, int part, int parts);
size_t tile_buffer_floats_for(const PbrtHipScene* s, int tile_size, int part, int parts);
int render_tiles(PbrtHipScene* s, int max_depth, float rr_threshold, int light_strategy, const int pixel_bounds[4], int tile_size, int part, int parts, void* d_tile_buffer,
                 PbrtHipStats* out_stats);
int merge_tiles(PbrtHipScene* s, int tile_size, int parts, const void* const* d_bufs, float* out_xyz, float* out_weight);
DevBuf& tile_buffer_of(PbrtHipScene* s);  // the handle's own tile buffer (wavefront workspace)
int merge_own_tiles(PbrtHipScene* s, int tile_size, int tile_part, int tile_parts, float* out_xyz, float* out_weight);   // the handle's tile buffer -> film, the other parts taken as empty
// The sample side of a frame, shared by the integrators: the rank's pixel list (tile by tile, row-major) and the records [sample][pixel] an integrator fills —
// rec_L = {L.rgb, p_film.x} (NaN p_film.x: no sample taken), rec_py = p_film.y, px_rounded[pixel] = 1 where a film position rounded up onto the next pixel's coordinate.
// The records of a frame are resident band by band (band_plan.h): `bands` are the rank's, band_px the pixels of the largest, which the buffers are sized for.  A driver takes
// one band at a time (samples_band): n_px, px_xy and `band` are then that band's, and a record's pixel index counts from the band's first pixel.
struct SampleRecords { uint32_t n_px; const int2* px_xy; float4* rec_L; float* rec_py; uint8_t* px_rounded; SampleBand band; uint32_t band_px; std::vector<SampleBand> bands; };
int samples_begin(PbrtHipScene* s, int tile_size, int part, int parts, SampleRecords* out);   // tile and pixel lists; n_px == 0: nothing to render
// a driver's first step: device, upload_scene, samples_begin, *out_stats zeroed; n_px == 0: the tile buffer is cleared, the driver returns
int frame_begin(PbrtHipScene* s, int tile_size, int part, int parts, void* d_tile_buffer, PbrtHipStats* out_stats, SampleRecords* rec);
int samples_plan_bands(PbrtHipScene* s, SampleRecords* out, size_t chunk_held, size_t chunk_per_path);   // the bands, under the handle's budget or the automatic one
int samples_alloc(PbrtHipScene* s, SampleRecords* out);                                        // the records of the largest band
int samples_band(PbrtHipScene* s, const SampleRecords& r, size_t band, SampleRecords* out);   // one band of them, px_rounded cleared
int samples_to_tiles(PbrtHipScene* s, const SampleRecords& r, void* d_tile_buffer);            // the film pass over a band, into its tiles' slots
// what samples_begin left for the rank: its pixel list on the host, its tiles' FilmTile pixel bounds (4 per tile, list order), the tile-buffer slot (the film probe, probe.hip)
void film_layout(PbrtHipScene* s, const int2** px_xy, size_t* n_px, std::vector<int32_t>* tile_pb, uint32_t* slot_w, uint32_t* slot_h);
size_t path_chunk_bytes_per_path(bool general_materials, bool textured_materials);   // what the path driver's chunk table (chunk_plan.h) sums to, for scripts/chunk_plan_check.cpp
// whitted.hip
void free_whitted(PbrtHipScene* s);
size_t whitted_chunk_bytes_per_sample(uint32_t n_frames);   // ... and the Whitted driver's
// the Whitted driver itself: this context's tiles of the part into d_tile_buffer, as render_tiles does for the path integrator (arguments checked by the caller)
int render_whitted_tiles(PbrtHipScene* s, int max_depth, const int pixel_bounds[4], int tile_size, int part, int parts, void* d_tile_buffer, PbrtHipStats* out_stats);
// ... and its direct-lighting mode (strategy 0 all, 1 one); what the chunk table sums to in that mode
int render_direct_tiles(PbrtHipScene* s, int strategy, int max_depth, const int pixel_bounds[4], int tile_size, int part, int parts, void* d_tile_buffer, PbrtHipStats* out_stats);
size_t direct_chunk_bytes_per_sample(uint32_t n_frames);
// ORs the voxels whose light distribution the context's last spatial render filled into `touched` (one byte per voxel, sized on first use); *count = voxels set so far
int spatial_voxels_touched(PbrtHipScene* s, std::vector<uint8_t>& touched, uint64_t* count);
// the spatial light distribution on explicit points (probe.hip: pbrt_hip_spatial_probe_*).  _begin: setup_spatial, as a strategy-2 render's bind step calls it; the record is kept with the
// workspace until the next render resets the tables.  _tables: that record (ERR_STATE without one).  _compute: the distribution pass a render of this scene launches.
int spatial_probe_begin(PbrtHipScene* s, ph::SpatialRec* out);
int spatial_probe_tables(PbrtHipScene* s, ph::SpatialRec* out);
void spatial_probe_compute(PbrtHipScene* s, const ph::SpatialRec& sr);
// multi.hip
int render_path_multi(PbrtHipScene* s, int max_depth, float rr_threshold, int light_strategy, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                      float* out_xyz, float* out_weight, PbrtHipStats* out_stats);
int render_whitted_multi(PbrtHipScene* s, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts, float* out_xyz, float* out_weight,
                         PbrtHipStats* out_stats);
int render_direct_multi(PbrtHipScene* s, int strategy, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts, float* out_xyz, float* out_weight,
                        PbrtHipStats* out_stats);
void free_multi(PbrtHipScene* s);
}  // namespace phost

#define PH_CHECK(s, call)                                              \
    do {                                                               \
        hipError_t e__ = (call);                                       \
        if (e__ != hipSuccess) return phost::hip_fail((s), e__, #call); \
    } while (0)
