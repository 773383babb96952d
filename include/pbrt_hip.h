/*
 * pbrt_hip.h — C ABI of the MI355X-native (gfx950) wavefront path tracer that replaces the hot path of
 * hackmad/pbrt-v3-rs:  SamplerIntegrator::render -> PathIntegrator::li -> BVHAccel::intersect/intersect_p ->
 * Triangle::intersect/intersect_p.
 *
 * Every entry point below names the reference interface it replaces (path:line relative to the reference repo).
 * Plain C types only: pointers + sizes, caller-allocated outputs, int status codes.  No callbacks, no C++ or
 * torch types, no exceptions across the boundary.  A handle is NOT re-entrant (one in-flight call per handle).
 * pbrt_hip_scene_create gives a handle that drives one GPU (one process per GPU: multi-GPU = one handle per rank, the ranks' film
 * tiles gathered by the host); pbrt_hip_scene_create_multi gives one handle that drives several GPUs of a node
 * from one process, the library gathering the film tiles itself over RCCL.
 *
 * Inputs are borrowed for the duration of the call and copied.  All floats are IEEE binary32 ("Float = f32",
 * core/src/pbrt/common.rs:13).  Matrices are row-major float[16], m[r*4+c] (core/src/geometry/matrix4x4.rs:13).
 */
#ifndef PBRT_HIP_H
#define PBRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PbrtHipScene PbrtHipScene;

/* ---- status codes (reference behaviour on the same conditions is panic!/error!) ------------- */
enum {
    PBRT_HIP_OK = 0,
    PBRT_HIP_ERR_INVALID_ARG = -1,  /* NULL handle, bad sizes, out-of-range ids                                  */
    PBRT_HIP_ERR_STATE = -2,        /* call order violated (render before build_accel, no camera, ...)           */
    PBRT_HIP_ERR_DEVICE = -3,       /* a HIP call failed; pbrt_hip_last_error() holds hipGetErrorString()        */
    PBRT_HIP_ERR_NO_DEVICE = -4,    /* no gfx950 device visible: the product path never falls back to the CPU    */
    PBRT_HIP_ERR_UNSUPPORTED = -5,  /* feature outside the hot-path scope (SURVEY §8 "next"/"out of scope")      */
    PBRT_HIP_ERR_OOM = -6
};

/* 32-byte ray = core/src/geometry/ray.rs:10-28 without differentials/medium (dead on this path). */
typedef struct PbrtHipRay {
    float o[3];
    float t_max;
    float d[3];
    float time;
} PbrtHipRay;

/* 32-byte closest-hit record: what Primitive::intersect (core/src/primitive.rs:22) hands back, reduced to the
 * ray-dependent quantities of Triangle::intersect (shapes/src/triangle.rs:438-545): t, barycentrics and the
 * primitive.  prim = index into the concatenation of all meshes' triangles in pbrt_hip_add_mesh order
 * (= position in the reference's `primitives: &[ArcPrimitive]` before BVH reordering); 0xFFFFFFFF on a miss.
 * For a hit inside an object instance prim is the triangle's number in add_mesh order (object meshes included) and pad[1] =
 * instance number + 1 (add_instance call order); t, b0..b2 are those of the instance-space ray, as TransformedPrimitive::intersect
 * leaves them in `r.t_max` (transformed_primitive.rs:56).  pad[1] = 0 otherwise.
 * A quadric shape (pbrt_hip_add_sphere / _add_quadric / _add_hyperboloid) takes ONE slot of that primitive list, in call order with the meshes' triangles: a hit on it
 * reports t and prim, b0 = b1 = b2 = 0 and pad[1] = 0.
 * A curve segment (pbrt_hip_add_curve makes 2^split_depth of them, one slot each) reports t and prim, b0 = u, b1 = v of Curve::intersect's SurfaceInteraction, b2 = 0 and pad[1] = 0.
 * pad[0] carries the library's leaf-order index of the hit triangle and pad[2] its material class | material id << 3 (internal shortcuts for the shade stage and its work queues); ignore them. */
typedef struct PbrtHipHit {
    float t;
    uint32_t prim;
    float b0, b1, b2;
    uint32_t pad[3];
} PbrtHipHit;

/* Counters with the reference's own names (core/src/scene.rs:13-23, core/src/integrator/sampler_integrator.rs:19-23).
 * Mrays/s := (regular_rays + shadow_rays) / render seconds. */
typedef struct PbrtHipStats {
    uint64_t camera_rays;        /* "Integrator/Camera rays traced"                         */
    uint64_t regular_rays;       /* "Intersections/Regular ray intersection tests"          */
    uint64_t shadow_rays;        /* "Intersections/Shadow ray intersection tests"           */
    uint64_t paths_zero_radiance;/* "Integrator/Zero-radiance paths" numerator (path.rs:168) */
    uint64_t paths_total;        /* its denominator (path.rs:164)                            */
    double render_seconds;       /* device time of the render phase (HIP events)             */
    double extend_seconds;       /* of which: traversal launches that carry closest-hit rays (from the second wavefront round on they also
                                    carry that round's shadow rays: one launch per round) */
    double shadow_seconds;       /* of which: any-hit-only traversal launches (0: the render makes none, shadow rays go with extend) */
    double shade_seconds;        /* of which: raygen + shade + film kernels                  */
    uint64_t extend_launches;    /* number of launches counted in extend_seconds             */
    uint64_t shadow_launches;    /* number of launches counted in shadow_seconds             */
    uint64_t light_distributions_created; /* "SpatialLightDistribution/Distributions created" (light_distrib/spatial.rs:17-21) */
} PbrtHipStats;

/* ---- lifetime ------------------------------------------------------------------------------------------- */
int pbrt_hip_device_count(void);                          /* <0 on HIP failure */
PbrtHipScene* pbrt_hip_scene_create(int device_ordinal);  /* NULL if no usable device */
/* One handle over several devices of this node (scene_create(device_ordinals, n_devices); NULL / 0 = every visible device).  It replaces
 * the reference's tile loop over worker threads (core/src/integrator/sampler_integrator.rs:254-296): capture calls act on the handle, pbrt_hip_render_path
 * replicates the scene into every device's HBM, deals the handle's 16x16 tiles round-robin to the devices (tile enumeration :254-259, :314-336), gathers the
 * per-tile film buffers on the first device — ncclSend / ncclRecv over xGMI, the path's one exchange step; RCCL is loaded when first needed — and merges
 * them there in increasing tile index (Film::merge_film_tile, core/src/film/mod.rs:220-248): the film equals the one-device film bit for bit.
 * An ordinal may repeat (contexts sharing a GPU, device-to-device copies instead of RCCL): a rehearsal aid for boxes with one GPU.
 * pbrt_hip_render_whitted_devices drives the Whitted integrator over the same handle in the same way.
 * The batch and *_tiles_device entry points of such a handle act on its first device only. */
PbrtHipScene* pbrt_hip_scene_create_multi(const int* device_ordinals, int n_devices);
int pbrt_hip_scene_devices(const PbrtHipScene*, int* out_ordinals, int capacity);   /* returns the number of devices behind the handle */
/* Self-test of the RCCL binding on the handle's devices (a one-rank communicator on a single-device handle): every device sends n_floats floats to the
 * first one through the same ncclSend / ncclRecv group the film-tile gather uses; out_wrong = floats that arrived wrong. */
int pbrt_hip_selftest_rccl_gather(PbrtHipScene*, uint32_t n_floats, uint64_t* out_wrong);
void pbrt_hip_scene_destroy(PbrtHipScene*);
const char* pbrt_hip_last_error(const PbrtHipScene*);     /* NUL-terminated, owned by the library; NULL handle -> global */

/* ---- scene capture (replaces the string factories, api/src/graphics_state.rs:254-720) -------------------- */

/* MatteMaterial with constant textures (materials/src/matte.rs:47-92). sigma in degrees, clamped to [0,90]. */
int pbrt_hip_add_material_matte(PbrtHipScene*, const float kd_rgb[3], float sigma_deg, uint32_t* out_id);

/* More materials, all with constant textures: the library builds the BxDF list their compute_scattering_functions would
 * (allow_multiple_lobes = true, TransportMode::Radiance, as PathIntegrator calls it, integrators/src/path.rs:143).  Roughness is
 * remapped by TrowbridgeReitzDistribution::roughness_to_alpha when remap_roughness != 0 (the scene-file default).
 *   mirror   materials/src/mirror.rs:40-62     SpecularReflection(Kr, FresnelNoOp)
 *   plastic  materials/src/plastic.rs:50-82    LambertianReflection(Kd) + MicrofacetReflection(Ks, TR(rough), Dielectric(1.5, 1))
 *   glass    materials/src/glass.rs:62-118     FresnelSpecular(Kr, Kt, 1, eta) if both roughnesses are 0, else MicrofacetReflection +
 *                                              MicrofacetTransmission over TR(urough, vrough)
 *   metal    materials/src/metal.rs:62-98      MicrofacetReflection(1, TR(urough, vrough), Conductor(1, eta, k)); eta/k as RGB (the
 *                                              reference's copper default needs its spectral tables: pass them explicitly)
 *   uber     materials/src/uber.rs:116-186     opacity pass-through + Lambert(Kd) + Microfacet(Ks) + SpecularReflection(Kr) +
 *                                              SpecularTransmission(Kt); pass urough = vrough = roughness when the file gives one value
 *   substrate   materials/src/substrate.rs:55-84   FresnelBlend(Kd, Ks, TR(urough, vrough))
 *   translucent materials/src/translucent.rs:57-112 Lambertian R/T (reflect*Kd, transmit*Kd) + Microfacet R/T (reflect*Ks, transmit*Ks), eta 1.5;
 *                                               reflect = transmit = 0: no BSDF at any hit (the reference returns before making one), i.e. Material "none"
 *   mix         materials/src/mix.rs:51-88        the two materials' lobes as ScaledBxDF(amount) / ScaledBxDF(1 - amount); at most 8 lobes,
 *                                               mixes of mixes up to two levels
 * Bump maps are outside the scope (constant textures have no gradient: Material::bump is the identity for them). */
int pbrt_hip_add_material_none(PbrtHipScene*, uint32_t* out_id);   /* Material "none" / "": no BSDF; PathIntegrator::li passes through the surface without
                                                                       counting a bounce (integrators/src/path.rs:142-150) */
int pbrt_hip_add_material_mirror(PbrtHipScene*, const float kr_rgb[3], uint32_t* out_id);
int pbrt_hip_add_material_plastic(PbrtHipScene*, const float kd_rgb[3], const float ks_rgb[3], float roughness, int remap_roughness, uint32_t* out_id);
int pbrt_hip_add_material_glass(PbrtHipScene*, const float kr_rgb[3], const float kt_rgb[3], float uroughness, float vroughness, float eta,
                                int remap_roughness, uint32_t* out_id);
int pbrt_hip_add_material_metal(PbrtHipScene*, const float eta_rgb[3], const float k_rgb[3], float uroughness, float vroughness, int remap_roughness,
                                uint32_t* out_id);
int pbrt_hip_add_material_uber(PbrtHipScene*, const float kd_rgb[3], const float ks_rgb[3], const float kr_rgb[3], const float kt_rgb[3],
                               const float opacity_rgb[3], float uroughness, float vroughness, float eta, int remap_roughness, uint32_t* out_id);

int pbrt_hip_add_material_substrate(PbrtHipScene*, const float kd_rgb[3], const float ks_rgb[3], float uroughness, float vroughness, int remap_roughness,
                                    uint32_t* out_id);
int pbrt_hip_add_material_translucent(PbrtHipScene*, const float kd_rgb[3], const float ks_rgb[3], const float reflect_rgb[3], const float transmit_rgb[3],
                                      float roughness, int remap_roughness, uint32_t* out_id);
int pbrt_hip_add_material_mix(PbrtHipScene*, uint32_t material1, uint32_t material2, const float amount_rgb[3], uint32_t* out_id);

/* TriangleMesh (shapes/src/triangle.rs:75-113): P/N/S must ALREADY be in world space exactly as TriangleMesh::new
 * leaves them (:93-99).  N, S, UV may be NULL.  One GeometricPrimitive per triangle (api/src/lib.rs:783-812).
 * first_area_light_id: -1, or the id returned by pbrt_hip_add_light_diffuse_area for the SAME n_tris (triangle k
 * is bound to light id+k).  flags: bit0 reverse_orientation, bit1 transform_swaps_handedness
 * (core/src/geometry/shape.rs:163-177).  alpha / shadowalpha: constant float textures only (triangle.rs:291-312);
 * pass 1.0f,1.0f for the defaults. */
int pbrt_hip_add_mesh(PbrtHipScene*, const float* P, uint32_t n_verts, const uint32_t* indices, uint32_t n_tris,
                      const float* N, const float* S, const float* UV, uint32_t material_id,
                      int32_t first_area_light_id, uint32_t flags, float alpha, float shadow_alpha);

/* Object instancing (api/src/lib.rs:911-1000, core/src/primitives/transformed_primitive.rs:33-73).  Meshes added between
 * object_begin and object_end belong to the object, not to the scene (ObjectBegin/ObjectEnd); add_instance places one
 * TransformedPrimitive(object aggregate, instance_to_world) in the scene's primitive list (ObjectInstance) — nothing if the
 * object is empty.  The object's aggregate uses the split method of pbrt_hip_build_accel; an object with exactly one
 * primitive is used directly (lib.rs:953-971).  Area lights of meshes inside an object definition behave as in the reference
 * ("Area lights not supported with object instancing", lib.rs:877-881): the call succeeds, pbrt_hip_last_error holds that warning, the triangles keep their
 * emission where a path looks at them (SurfaceInteraction::le) and the lights leave the scene's light list — nothing samples them; they must be the lights
 * created last, so that no other light's number changes.  Transforms are static (AnimatedTransform with equal end points). */
int pbrt_hip_object_begin(PbrtHipScene*, uint32_t* out_object_id);
int pbrt_hip_object_end(PbrtHipScene*);
int pbrt_hip_add_instance(PbrtHipScene*, uint32_t object_id, const float instance_to_world[16], const float world_to_instance[16]);

/* The reference's six quadric shapes.  object_to_world is handed over as the reference's Transform holds it — the matrix AND the inverse the CTM accumulated (row-major;
 * transform.rs:644-656 multiplies the inverses, nothing is inverted here).  Parameters are clamped and derived as the constructors do; phi_max in degrees; flags bit 0 =
 * reverse orientation (swaps_handedness is taken from the matrix).  Each shape takes one slot of the primitive list (see PbrtHipHit) and its Shape::world_bound
 * (object_to_world(object_bound)) enters the BVH.
 *   pbrt_hip_add_sphere       Sphere::new (shapes/src/sphere.rs:21-44): radius, zmin, zmax, phimax
 *   pbrt_hip_add_hyperboloid  Hyperboloid::new (hyperboloid.rs:37-110): p1, p2, phimax
 *   pbrt_hip_add_quadric      kind 0 Cylinder::new (cylinder.rs:21-42; a, b = zmin, zmax), 1 Cone::new (cone.rs:21-40; a = height), 2 Paraboloid::new (paraboloid.rs:21-42;
 *                             a, b = zmin, zmax), 3 Disk::new (disk.rs:21-40; a = height, b = innerradius)
 * PBRT_HIP_ERR_UNSUPPORTED, with nothing changed: a quadric between object_begin and object_end; a quadric right after pbrt_hip_add_light_diffuse_area lights that no mesh
 * has claimed (it would be the area light's shape; a sphere light is made by pbrt_hip_add_sphere_light, a cylinder or disk light by pbrt_hip_add_quadric_light; the reference's Shape::sample of the other three is todo!()); pbrt_hip_set_last_mesh_alpha_textures when the shape added last is a
 * quadric.  Scene-level quadrics and object instances share a scene freely (instanced triangle objects, single-primitive and empty ones included; definitions that no instance
 * uses are ignored, as in any instanced scene): a quadric stands in the scene-level tree next to the instances and is tested in its place in its leaf's order.  One leftover
 * refusal, with no technical reason and kept only because older tests pin it: pbrt_hip_build_accel returns PBRT_HIP_ERR_UNSUPPORTED for a scene that holds a quadric and object
 * definitions but NOT ONE instance.  Both device builders take a scene with quadrics, forest included: pbrt_hip_build_accel_device builds its HLBVH tree (split_method 1) and, because
 * older tests pin that answer, still refuses its SAH tree (split_method 0) with PBRT_HIP_ERR_UNSUPPORTED; pbrt_hip_build_accel_device_shapes builds either.  Quadrics and triangle
 * meshes with alpha / shadow-alpha textures share a scene freely: the masks belong to the meshes' triangles, a quadric in the same leaf is tested in its place in the leaf's order. */
int pbrt_hip_add_sphere(PbrtHipScene*, const float o2w_m[16], const float o2w_minv[16], float radius, float z_min, float z_max, float phi_max_deg,
                        uint32_t material_id, uint32_t flags);
int pbrt_hip_add_hyperboloid(PbrtHipScene*, const float o2w_m[16], const float o2w_minv[16], const float p1[3], const float p2[3], float phi_max_deg,
                             uint32_t material_id, uint32_t flags);
int pbrt_hip_add_quadric(PbrtHipScene*, int kind, const float o2w_m[16], const float o2w_minv[16], float radius, float a, float b, float phi_max_deg,
                         uint32_t material_id, uint32_t flags);

/* Curve::create_segments (shapes/src/curve.rs:105-140): ONE cubic Bezier curve — the CurveData of CurveData::new (:743-762), stored once — cut into 2^split_depth Curve
 * segments over equal u ranges, which take that many consecutive slots of the primitive list, in order.  cp = the four control points in object space (what Curve::from_props,
 * :149-316, arrives at after degree elevation and b-spline blossoming); width = the widths at u = 0 and u = 1; type 0 flat, 1 cylinder, 2 ribbon; n = a ribbon's two end normals
 * (6 floats; read for type 2 only, may be NULL otherwise).  object_to_world as for the quadrics; flags bit 0 = reverse orientation.  Each segment enters the accelerator with its own
 * Shape::world_bound (Curve::object_bound, :660-674, through Transform::transform_bounds) and is intersected as the reference RUNS Curve::intersect / intersect_p (:339-645), which
 * differ from each other and depend on the t_max the ray carries when the segment is tested: DESIGN §4.4 lists the quirks that are reproduced and the one departure (where the
 * reference would panic — assert!(dpdu != 0), a degenerate LookAt — the segment is missed).  A segment is a quadric in every other respect: scenes with instances and with
 * alpha-masked meshes, all three integrators, every driver, both device builders.
 * PBRT_HIP_ERR_INVALID_ARG: a null handle, matrix, cp or width; a type outside 0 .. 2; a ribbon without n; split_depth outside [0, 16]; an unknown material.
 * PBRT_HIP_ERR_UNSUPPORTED, with nothing changed: between object_begin and object_end; while pbrt_hip_add_light_diffuse_area lights that no mesh has claimed are pending (the
 * curve would be their shape, and Curve::sample is todo!(), :709-711); pbrt_hip_set_last_mesh_alpha_textures when the shape added last is a curve segment. */
int pbrt_hip_add_curve(PbrtHipScene*, const float o2w_m[16], const float o2w_minv[16], int type, const float cp[12], const float width[2], const float* n /* 6 or NULL */,
                       int split_depth, uint32_t material_id, uint32_t flags);

/* LoopSubDiv::subdivide (shapes/src/loopsubdiv.rs:321-659, with from_props :668-689 and beta, loop_gamma, weight_one_ring, weight_boundary :695-768): the control mesh
 * (P, n_verts positions in object space; indices, of which those beyond the last multiple of 3 are ignored) refined n_levels times by the Loop rules, every vertex pushed to the
 * limit surface, a normal s x t per vertex from the ring of limit positions (not normalised), and the move to world space of TriangleMesh::new (shapes/src/triangle.rs:75-113):
 * P through the matrix, N through the transpose of the inverse.  F control faces give F 4^n_levels triangles; V' = V + E, E' = 2E + 3F, F' = 4F per level.  The control
 * mesh's pointers and flags are made on the host (csrc/loopsubdiv_host.h), the levels, limit positions, normals and world pass run as kernels on the handle's first device and
 * stream (csrc/loopsubdiv.hip) in the reference's f32 expression order — the mesh equals the reference's word for word; cos / sin come from a host table (cosf / sinf).
 *   pbrt_hip_loopsubdiv_mesh  writes the counts, then the mesh: out_P and out_N 3 * *out_n_verts floats, out_indices 3 * *out_n_tris (face.v[0..3] in face order, :636-643).
 *                             With the three out arrays NULL it only validates and writes the counts — no device work, and the handle may be NULL (what a caller uses to size
 *                             the arrays and the area lights).  o2w_m NULL: the mesh stays in object space (o2w_minv is not read).
 *   pbrt_hip_add_loopsubdiv   the call above followed by exactly what pbrt_hip_add_mesh does with that P, N and indices (S and UV absent): area lights (one per output triangle,
 *                             pbrt_hip_add_light_diffuse_area with n_tris = F 4^n_levels), object definitions, pbrt_hip_set_last_mesh_alpha_textures afterwards, every builder,
 *                             integrator and driver serve it as they serve a mesh.  flags, first_area_light_id, alpha, shadow_alpha as for pbrt_hip_add_mesh.
 * PBRT_HIP_ERR_INVALID_ARG, with nothing changed and one sentence in pbrt_hip_last_error — where the reference panics, or its ring walks would not end: no indices, or no P
 * (:674-679); an index >= n_verts; a face that names a vertex twice; a vertex no face uses (:377-382); an edge in more than two faces; an edge its two faces run through in the
 * same direction; n_levels < 0; a count of vertices or faces, at any level, above 0x7FFFFFFF / 3 = 715 827 882 (the library forms 3 * index in 32 signed bits); also null count pointers, some but not all of the out arrays, a matrix without its inverse, and whatever
 * pbrt_hip_add_mesh refuses.  Accepted as the reference accepts it: a vertex whose faces form several fans (its ring is the fan of its start_face, the last face naming it). */
int pbrt_hip_loopsubdiv_mesh(PbrtHipScene*, const float* o2w_m /* 16 or NULL */, const float* o2w_minv, const float* P, uint32_t n_verts, const uint32_t* indices, uint32_t n_indices,
                             int n_levels, uint32_t* out_n_verts, uint32_t* out_n_tris, float* out_P, float* out_N, uint32_t* out_indices);
int pbrt_hip_add_loopsubdiv(PbrtHipScene*, const float* o2w_m /* 16 or NULL */, const float* o2w_minv, const float* P, uint32_t n_verts, const uint32_t* indices, uint32_t n_indices,
                            int n_levels, uint32_t material_id, int32_t first_area_light_id, uint32_t flags, float alpha, float shadow_alpha);

/* A sphere that is the shape of a DiffuseAreaLight (Shape "sphere" under AreaLightSource "diffuse": api/src/lib.rs:783-812 makes the shape, then the light of lights/src/diffuse.rs:46-82
 * around it): pbrt_hip_add_sphere with the same arguments, plus one light that joins the scene's lights in call order.  The light's area is Sphere::area — phi_max * radius *
 * (z_max - z_min) of the constructor's clamped values — so a partial sphere emits and is sampled as the reference does it: Sphere::sample_solid_angle (shapes/src/sphere.rs:344-410)
 * draws from the cone the FULL sphere subtends, or from the full sphere's area where the reference point lies inside it, and DiffuseAreaLight::sample_li (diffuse.rs:114-129) takes the point
 * as it comes.  A ray that meets the sphere sees L on the side its normal faces (reverse orientation and the transform's handedness included), on both sides if two_sided (diffuse.rs:220-226).
 * pbrt_hip_render_whitted renders such a scene.  pbrt_hip_render_path and pbrt_hip_render_path_tiles_device render it on a handle that asked for it with
 * pbrt_hip_set_path_sphere_lights (below); on any other they return PBRT_HIP_ERR_UNSUPPORTED before any work (message: "sphere light") and the handle stays usable.
 * PathIntegrator::li needs Sphere::pdf_solid_angle (shapes/src/sphere.rs:462-475) for its MIS weight.  Outside the sphere that is the cone's uniform pdf, as the reference computes it.
 * INSIDE (the reference point, offset towards the centre, lies in or on the sphere) the reference calls `Shape::pdf_solid_angle(self, hit, wi)` from inside `impl Shape for Sphere`,
 * which resolves to the same function: it recurses until its stack ends and has no answer.  A documented departure from a reference that crashes: the library evaluates the trait's
 * default there (core/src/geometry/shape.rs:86-107, the counterpart of sample_solid_angle's inside branch and what upstream pbrt-v3 does) — the ray hit.spawn_ray(wi) against the cut
 * sphere, alpha ignored, distance^2 / (|n . -wi| * area), 0 for a miss or an infinite value.  The batch intersection entry points treat the sphere as ordinary geometry.
 * PBRT_HIP_ERR_UNSUPPORTED, with nothing changed: between object_begin and object_end, as for any quadric; while pbrt_hip_add_light_diffuse_area lights that no mesh has claimed are pending.
 * A cylinder or a disk becomes a light through pbrt_hip_add_quadric_light (below); cone, paraboloid and hyperboloid cannot be lights.  The pbrt_hip_render front end makes this call for Shape "sphere" under AreaLightSource "diffuse" when run with --quadrics (without the
 * option it refuses the six quadric Shape directives), and refuses such a scene under Integrator "path" itself unless it is also run with --path-sphere-lights. */
int pbrt_hip_add_sphere_light(PbrtHipScene*, const float o2w_m[16], const float o2w_minv[16], float radius, float z_min, float z_max, float phi_max_deg,
                              uint32_t material_id, uint32_t flags, const float L_rgb[3], int two_sided);
/* on != 0: pbrt_hip_render_path and pbrt_hip_render_path_tiles_device sample the lights made by pbrt_hip_add_sphere_light (DiffuseAreaLight::sample_li / pdf_li on a Sphere, in
 * uniform_sample_one_light and, under light strategy 2, in the spatial light distribution) instead of refusing the scene.  0, the default: every answer is as before the switch
 * existed.  Legal at any time before a render; holds until it is changed; applies to every device of a handle made by pbrt_hip_scene_create_multi, to tile parts, chunks and
 * sample-record bands.  A scene without a sphere light launches the same kernels whatever the switch says.  A sphere light draws the 5 sampler dimensions per vertex of any
 * non-delta light.  PBRT_HIP_ERR_INVALID_ARG: null handle. */
int pbrt_hip_set_path_sphere_lights(PbrtHipScene*, int on);
/* A cylinder (kind 0) or a disk (kind 3) that is the shape of a DiffuseAreaLight: pbrt_hip_add_quadric with the same arguments plus ONE light, numbered in call order among the
 * add_light_* calls, with radiance L_rgb and `two_sided`.  area = Cylinder::area `(z_max - z_min) * radius * phi_max` (cylinder.rs:313-315) or Disk::area
 * `phi_max * 0.5 * (radius^2 - inner_radius^2)` (disk.rs:205-207) of the constructor's values, whatever the transform scales.  Both shapes leave Shape::sample_solid_angle and
 * Shape::pdf_solid_angle to the trait's defaults (core/src/geometry/shape.rs:64-107): sample_li draws Disk::sample (disk.rs:214-234) / Cylinder::sample (cylinder.rs:322-348) — uniform
 * over the FULL shape's area; the disk's sample ignores inner_radius and phi_max, so a point may land on the part that is cut away, as in the reference — and turns 1/area into a
 * solid-angle pdf, 0 (no sample) for a zero-length direction or an infinite value; pdf_li intersects spawn_ray(ref, wi) with the shape itself, cuts included, 0 for a miss.  The
 * sampled normal is flipped for reverse orientation only; a ray that meets the shape sees L on the side its hit normal faces (reverse orientation XOR the transform's handedness),
 * on both sides if two_sided.  The reference has an answer at every reference point, so pbrt_hip_render_path, _tiles_device, multi-device handles, chunks and bands render such a
 * scene with no switch, and so do pbrt_hip_render_whitted, _devices and _tiles_device.  pbrt_hip_set_path_sphere_lights keeps its meaning for spheres only: a scene that also holds
 * a sphere light is still refused by the path integrator on a handle whose switch is off.
 * PBRT_HIP_ERR_UNSUPPORTED, with nothing changed: kind 1 (cone) or 2 (paraboloid), whose Shape::sample in the reference is todo!() (as is the hyperboloid's); between object_begin
 * and object_end; while pbrt_hip_add_light_diffuse_area lights that no mesh has claimed are pending.  PBRT_HIP_ERR_INVALID_ARG: any other kind, a null argument, an unknown material. */
int pbrt_hip_add_quadric_light(PbrtHipScene*, int kind, const float o2w_m[16], const float o2w_minv[16], float radius, float a, float b, float phi_max_deg,
                               uint32_t material_id, uint32_t flags, const float L_rgb[3], int two_sided);

/* Alpha masks: the float textures behind a mesh's `alpha` / `shadowalpha` parameters (TriangleMesh::alpha_mask, shadow_alpha_mask: shapes/src/triangle.rs:291-312),
 * for the mesh added last; 0xFFFFFFFF keeps the constant given to add_mesh.  A candidate hit is rejected where the texture evaluates to exactly 0 at the hit's
 * uv / point, with no differentials (triangle.rs:587-607; intersect_p also consults shadowalpha, :868-898). */
int pbrt_hip_set_last_mesh_alpha_textures(PbrtHipScene*, uint32_t alpha_texture, uint32_t shadow_alpha_texture);

/* ---- textures (textures/src/{constant,scale,mix,imagemap}.rs, core/src/mipmap/mod.rs) -------------------------------
 * Float- and spectrum-valued textures share one id space; a float texture is a spectrum texture whose channels are equal.
 * add_mipmap is generate_mipmap + MIPMap::new (core/src/mipmap/cache.rs:74-120, mod.rs:115-189): `rgb` is width*height
 * texels as the reference's read_image returns them (row 0 = top of the image); the library flips them, applies
 * `scale * (gamma ? inv_gamma_correct(x) : x)` (as_float: to the texel's luminance, ImageTexture<Float>), resamples to powers of two and
 * builds the pyramid.  filtering: 0 trilinear, 1 EWA.  wrap: 0 repeat, 1 black, 2 clamp.  Image file decoding is the host's job.
 * imagemap uses UVMapping2D (su, sv, du, dv) (core/src/texture/mapping/uv_2d.rs); other mappings are not provided yet.
 * mix: (1 - amount) * tex1 + amount * tex2 with `amount` a float texture.  Trees that need more than 6 live values are refused. */
int pbrt_hip_add_mipmap(PbrtHipScene*, int width, int height, const float* rgb, int as_float, float scale, int gamma, int filtering, int wrap,
                        float max_anisotropy, uint32_t* out_mipmap);
int pbrt_hip_add_texture_constant(PbrtHipScene*, const float value[3], uint32_t* out_texture);
int pbrt_hip_add_texture_scale(PbrtHipScene*, uint32_t tex1, uint32_t tex2, uint32_t* out_texture);
int pbrt_hip_add_texture_mix(PbrtHipScene*, uint32_t tex1, uint32_t tex2, uint32_t amount, uint32_t* out_texture);
int pbrt_hip_add_texture_imagemap(PbrtHipScene*, uint32_t mipmap, float su, float sv, float du, float dv, uint32_t* out_texture);
/* Procedural 2D textures over the same uv mapping: CheckerboardTexture2D (textures/src/checkerboard_2d.rs; aa_mode 0 "none", 1 "closedform"),
 * UVTexture (uv.rs), BilerpTexture (bilerp.rs; four constant corner values), DotsTexture (dots.rs; Perlin noise of core/src/texture/common.rs).
 * add_texture_dots takes DotsTexture's fields: `inside` is evaluated inside a dot.  A caller that translates SCENE-FILE parameters must swap them: the reference builds the
 * texture with DotsTexture::new(outside_dot = "inside" parameter, inside_dot = "outside" parameter) (dots.rs:61-66, quirk B13; pbrt_hip_render does the swap). */
int pbrt_hip_add_texture_checkerboard(PbrtHipScene*, uint32_t tex1, uint32_t tex2, float su, float sv, float du, float dv, int aa_mode, uint32_t* out_texture);
int pbrt_hip_add_texture_uv(PbrtHipScene*, float su, float sv, float du, float dv, uint32_t* out_texture);
int pbrt_hip_add_texture_bilerp(PbrtHipScene*, const float v00[3], const float v01[3], const float v10[3], const float v11[3], float su, float sv, float du, float dv,
                                uint32_t* out_texture);
int pbrt_hip_add_texture_dots(PbrtHipScene*, uint32_t inside, uint32_t outside, float su, float sv, float du, float dv, uint32_t* out_texture);
/* The other TextureMapping2D kinds for a 2D texture (imagemap, checkerboard, uv, bilerp, dots; core/src/texture/mapping/): kind 1 SphericalMapping2D and
 * 2 CylindericalMapping2D take params = the row-major 4x4 world_to_texture matrix (the reference passes tex2world.inverse(), textures/src/lib.rs:54-55),
 * 3 PlanarMapping2D takes params = v1[3], v2[3], udelta, vdelta.  Set it before the texture is used as an operand of another texture. */
int pbrt_hip_set_texture_mapping(PbrtHipScene*, uint32_t texture, int kind, const float* params);
/* 3D procedural textures over IdentityMapping3D (core/src/texture/mapping/identity_3d.rs): `m` is the row-major 4x4 matrix the mapping applies to the
 * hit point and to dp/dx, dp/dy — the reference hands it the Texture directive's CTM (tex2world, textures/src/fbm.rs:65), so pass that.
 * FBmTexture, WrinkledTexture (fbm.rs, wrinkled.rs; omega = "roughness", octaves), WindyTexture (windy.rs), MarbleTexture (marble.rs; scale, variation),
 * CheckerboardTexture3D (checkerboard_3d.rs).  fbm / wrinkled / windy are float-valued (three equal channels). */
int pbrt_hip_add_texture_fbm(PbrtHipScene*, const float m[16], float omega, int octaves, uint32_t* out_texture);
int pbrt_hip_add_texture_wrinkled(PbrtHipScene*, const float m[16], float omega, int octaves, uint32_t* out_texture);
int pbrt_hip_add_texture_windy(PbrtHipScene*, const float m[16], uint32_t* out_texture);
int pbrt_hip_add_texture_marble(PbrtHipScene*, const float m[16], float omega, int octaves, float scale, float variation, uint32_t* out_texture);
int pbrt_hip_add_texture_checkerboard3d(PbrtHipScene*, uint32_t tex1, uint32_t tex2, const float m[16], uint32_t* out_texture);
/* Replaces a colour parameter of an existing material by a texture evaluated at every hit (`self.kd.evaluate(..).clamp_default()` in
 * compute_scattering_functions: materials/src/matte.rs:63, plastic.rs:62-70, mirror.rs:53-55, substrate.rs:60-62), with the ray
 * differentials of camera rays (SurfaceInteraction::compute_differentials) driving the MIPMap filter.  Which lobes a hit gets follows the
 * reference's `is_black` tests on the value at that hit.  Texturable so far: matte Kd, plastic Kd / Ks, mirror Kr, substrate Kd / Ks, glass Kr / Kt (glass.rs:72-78)
 * uber Kd / Ks / Kr / Kt (multiplied by its constant opacity, uber.rs:133-160) and translucent Kd / Ks (each feeds a reflection and a transmission
 * lobe; the texel is tested for black BEFORE its product with the constant reflect / transmit, translucent.rs:77-84, :87);
 * the material must have been created with a non-black constant for that parameter.  Scalar parameters: see set_material_float_texture.
 * Materials with per-hit textures may be children of a mix (each lobe is kept or dropped as its own material would, mix.rs:63-87) as long as the
 * mix has at most 6 textured colours and one textured roughness / sigma. */
/* More per-hit parameters (same call): OPACITY — UberMaterial's opacity (uber.rs:126-160: it decides the pass-through lobe, multiplies Kd / Ks / Kr / Kt and picks BSDF::eta);
 * AMOUNT — MixMaterial's amount (mix.rs:59-60: s1 = amount(hit), s2 = 1 - s1, clamped); ETA / K — MetalMaterial's conductor indices (metal.rs:121-125, not clamped).
 * GlassMaterial's u / v roughness go through set_material_float_texture: a hit where both evaluate to 0 gets FresnelSpecular, any other the microfacet pair (glass.rs:110-141).
 * A bump-mapped material may be a child of a mix: the FIRST child's bump map shapes the mixture's shading frame, the second child's has no effect (mix.rs:63-76 builds the
 * BSDF on the interaction the first child bumped). */
/* REFLECT / TRANSMIT — TranslucentMaterial's `reflect` / `transmit` (translucent.rs:70-98): evaluated and clamped at every hit; a lobe is added where its reflect-or-transmit value and its
 * Kd-or-Ks value are both non-black, with their product as colour; where reflect and transmit are BOTH black the reference makes no BSDF for the hit (:72-74) and PathIntegrator::li passes
 * through the surface without counting a bounce (path.rs:142-150) — so does the library, per hit.  (Constants reflect = transmit = 0 behave like Material "none" everywhere.) */
enum { PBRT_HIP_PARAM_KD = 0, PBRT_HIP_PARAM_KS = 1, PBRT_HIP_PARAM_KR = 2, PBRT_HIP_PARAM_KT = 3, PBRT_HIP_PARAM_OPACITY = 4, PBRT_HIP_PARAM_AMOUNT = 5, PBRT_HIP_PARAM_ETA = 6,
       PBRT_HIP_PARAM_K = 7, PBRT_HIP_PARAM_REFLECT = 8, PBRT_HIP_PARAM_TRANSMIT = 9 };
int pbrt_hip_set_material_texture(PbrtHipScene*, uint32_t material, int param, uint32_t texture);
/* Scalar parameters as float textures, evaluated at every hit: fparam 0 = MatteMaterial's sigma (matte.rs:64-70: Lambert where it evaluates to 0, Oren-Nayar elsewhere),
 * 1 / 2 = u / v roughness of the Trowbridge-Reitz distribution of plastic, uber, substrate, translucent and metal (remapped per hit if the material was created with remap_roughness;
 * plastic's and translucent's single `roughness`: set both), and of glass, whose lobe structure switches per hit on `urough == 0 && vrough == 0` (glass.rs:110-141);
 * 3 = `index` of GlassMaterial and UberMaterial (glass.rs:102, uber.rs:128): the hit's index of refraction, taken as the texture gives it, for FresnelSpecular, the
 * FresnelDielectric(1, index) of the reflection lobes, the transmission lobes and — uber — BSDF::eta; an uber's constant opacity then becomes a per-hit constant as well.
 */
int pbrt_hip_set_material_float_texture(PbrtHipScene*, uint32_t material, int fparam, uint32_t texture);
/* Bump mapping: Material::bump (core/src/material.rs:62-101) with the float texture `texture` as displacement, run before the BSDF of a hit is made
 * (every material's `bumpmap` parameter).  Not for Material "none".  Set it before the material becomes a child of a mix. */
int pbrt_hip_set_material_bump(PbrtHipScene*, uint32_t material, uint32_t texture);
/* = add_material_matte((1,1,1), sigma) + set_material_texture(KD) */
int pbrt_hip_add_material_matte_tex(PbrtHipScene*, uint32_t kd_texture, float sigma_degrees, uint32_t* out_material);
/* Test aids: evaluate a texture on the device at explicit contexts (u, v, du/dx, dv/dx, du/dy, dv/dy, p[3], dp/dx[3], dp/dy[3]); read back the pyramid the host built. */
int pbrt_hip_texture_eval_batch(PbrtHipScene*, uint32_t texture, uint64_t n, const float* contexts /*15 per point*/, float* out_rgb /*3 per point*/);
/* The same through the evaluator the renderer uses for every ray but a camera ray (no differentials: an image map's look-up ends in MIPMap::triangle(0, st), mipmap/mod.rs:222-231,
 * :250-262): the contexts' derivative fields are ignored as if zero.  Must equal pbrt_hip_texture_eval_batch on contexts whose derivatives ARE zero. */
int pbrt_hip_texture_eval_batch_nodiff(PbrtHipScene*, uint32_t texture, uint64_t n, const float* contexts /*15 per point*/, float* out_rgb /*3 per point*/);
int pbrt_hip_mipmap_levels(PbrtHipScene*, uint32_t mipmap, int* out_levels, int* out_width_height /*2 per level, <= 16 levels*/);
int pbrt_hip_mipmap_level_texels(PbrtHipScene*, uint32_t mipmap, int level, float* out_rgb);


/* Lights are numbered in call order = position in Scene::lights (core/src/scene.rs:50-75). */
int pbrt_hip_add_light_infinite(PbrtHipScene*, const float L_rgb[3], const float light_to_world[16],
                                const float world_to_light[16]);       /* lights/src/infinite.rs:63-107, constant L */
/* InfiniteAreaLight with a radiance map (`mapname`; lights/src/infinite.rs:52-100): `rgb` = width*height texels as read_image returns them (row 0 = top);
 * the library multiplies them by L, builds the MIPMap (EWA, repeat; no y flip on this path, as in the reference) and the Distribution2D of the 2w x 2h
 * scalar image (compute_scalar_image, :326-369).  Le / sample_li / pdf_li / power then follow :127-211. */
int pbrt_hip_add_light_infinite_map(PbrtHipScene*, const float L[3], int width, int height, const float* rgb, const float light_to_world[16], const float world_to_light[16]);
/* ProjectionLight (lights/src/projection.rs:55-127, :145-203) and GonioPhotometricLight (goniometric.rs:34-126): point lights whose intensity is scaled by an
 * image looked up by direction (MIPMap::new(.., Ewa, Repeat, 8.0), lookup_triangle(st, 0)).  rgb = width x height x 3 floats, top row first, or NULL for "no image"
 * (white inside the frustum / in every direction); I = intensity * scale; light_to_world / world_to_light as for the spot light. */
int pbrt_hip_add_light_projection(PbrtHipScene*, const float I_rgb[3], const float light_to_world[16], const float world_to_light[16], float fov_deg,
                                  int width, int height, const float* rgb);
int pbrt_hip_add_light_goniometric(PbrtHipScene*, const float I_rgb[3], const float light_to_world[16], const float world_to_light[16],
                                   int width, int height, const float* rgb);
int pbrt_hip_add_light_distant(PbrtHipScene*, const float L_rgb[3], const float w_light_world[3]); /* distant.rs:36-50: already transformed+normalized */
int pbrt_hip_add_light_point(PbrtHipScene*, const float I_rgb[3], const float p_world[3]);         /* point.rs:36-55 */
int pbrt_hip_add_light_spot(PbrtHipScene*, const float I_rgb[3], const float light_to_world[16], const float world_to_light[16],
                            float cos_total_width, float cos_falloff_start);                       /* lights/src/spot.rs:27-90 */
int pbrt_hip_add_light_diffuse_area(PbrtHipScene*, const float L_rgb[3], int two_sided, uint32_t n_tris,
                                    uint32_t* out_first_id);           /* lights/src/diffuse.rs:46-82, one per triangle */

/* PerspectiveCamera (cameras/src/perspective_camera.rs:47-95): the two transforms the ray generator uses. */
int pbrt_hip_set_camera_perspective(PbrtHipScene*, const float raster_to_camera[16], const float camera_to_world[16],
                                    float lens_radius, float focal_distance, float shutter_open, float shutter_close);
/* OrthographicCamera (cameras/src/orthographic_camera.rs:39-72, :121-178): same two transforms (raster_to_camera from Transform::orthographic(0, 1):
 * pbrt_hip_host_orthographic_raster_to_camera); rays leave the film point along camera +z, the lens model and the ray differentials are the reference's. */
int pbrt_hip_set_camera_orthographic(PbrtHipScene*, const float raster_to_camera[16], const float camera_to_world[16],
                                     float lens_radius, float focal_distance, float shutter_open, float shutter_close);
/* EnvironmentCamera (cameras/src/environment_camera.rs:27-78): directions over the whole sphere from the film position relative to the film's FULL
 * resolution (pass the same xres / yres as to pbrt_hip_set_film); ray differentials are the Camera trait's finite differences (core/src/camera.rs:29-78). */
int pbrt_hip_set_camera_environment(PbrtHipScene*, const float camera_to_world[16], int xres, int yres, float shutter_open, float shutter_close);

/* Film (core/src/film/mod.rs:89-146).  cropped_pixel_bounds = {x0,y0,x1,y1}.  filter_table = the 16x16 table of
 * Film::new (:117-129).  max_sample_luminance: INFINITY for none. */
int pbrt_hip_set_film(PbrtHipScene*, int xres, int yres, const int cropped_pixel_bounds[4],
                      const float filter_radius[2], const float filter_table_16x16[256], float scale,
                      float max_sample_luminance);

/* Sampler (samplers/src/halton.rs:61-100, sobol.rs:35-63). kind: 0 halton, 1 sobol. sample_bounds = Film::get_sample_bounds. */
int pbrt_hip_set_sampler(PbrtHipScene*, int kind, uint32_t samples_per_pixel, const int sample_bounds[4],
                         int sample_at_pixel_center);

/* Optional: Sobol generator matrices (core/src/sobol_matrices.rs) as data: 1024*52 u32, then VdC 25x? tables.
 * Required before rendering with kind==1; the library does not embed them.  Both lengths must be multiples of 52 (INVALID_ARG
 * otherwise); a render whose path needs more than n32/52 dimensions (5 + 8 (max_depth + 1)) or whose sample bounds' log2
 * resolution exceeds n_vdc_each/52 is refused with UNSUPPORTED. */
int pbrt_hip_set_sobol_tables(PbrtHipScene*, const uint32_t* sobol_matrices32, size_t n32,
                              const uint64_t* vdc_matrices, const uint64_t* vdc_matrices_inv, size_t n_vdc_each);

/* BVHAccel::from (accelerators/src/bvh/mod.rs:339-360) = Integrator::preprocess time.  split_method: 0 SAH (sah.rs),
 * 1 HLBVH (hlbvh.rs, the reference's tree incl. its Morton-code quirk), 3 EqualCounts; 2 (Middle) panics in the reference
 * and returns UNSUPPORTED. */
int pbrt_hip_build_accel(PbrtHipScene*, int split_method, int max_prims_in_node);

/* The same with the tree constructed on the GPU: identical topology, leaf order and boxes, so hits do not depend on where the tree was built.
 * split_method 0 (SAH, the reference's default; accelerators/src/bvh/sah.rs:26-367): one level of the tree per round of kernels — bucket boxes by atomics,
 * the reference's cost loop per node, itertools::partition's element order from a prefix sum.  split_method 1 (HLBVH; hlbvh.rs:33-449, morton.rs:33-120):
 * Morton codes, radix sort, the treelets emitted side by side one tree LEVEL per launch, SAH over the treelet roots on the host.  EqualCounts (3) is a host build: UNSUPPORTED here.  Scenes with object
 * instances (SAH and HLBVH): the scene's aggregate and every instanced object's are built side by side as one forest.  Scenes with quadric shapes: HLBVH only (above); the next call builds their SAH tree. */
int pbrt_hip_build_accel_device(PbrtHipScene*, int split_method, int max_prims_in_node);

/* pbrt_hip_build_accel_device in every respect, except that split_method 0 (SAH; sah.rs:26-367) also takes a scene with quadric shapes: a quadric enters the build with its
 * Shape::world_bound (core/src/geometry/shape.rs) as a triangle does with Triangle::world_bound (triangle.rs:427-431), in the flat tree and, at scene level, in a forest.  The tree
 * is the one pbrt_hip_build_accel(scene, 0, ..) makes, array for array, and stays on the GPU.  Every refusal of pbrt_hip_build_accel holds here as well. */
int pbrt_hip_build_accel_device_shapes(PbrtHipScene*, int split_method, int max_prims_in_node);

/* World bound of the built aggregate (BVHAccel::world_bound, bvh/mod.rs:161-167): {pmin[3], pmax[3]}. */
int pbrt_hip_world_bound(const PbrtHipScene*, float out_bounds[6]);

/* Measurement aid (not a reference interface): the built structure in the device layout.  out[0] interior nodes (64 B each: both children's boxes),
 * out[1] leaf records (48 B each), out[2] / out[3] their bytes, out[4] leaves, out[5] depth, out[6] largest leaf, out[7] build time in microseconds. */
int pbrt_hip_accel_stats(const PbrtHipScene*, uint64_t out[8]);
/* Test aid: copies the structure out (out[0] x 64-byte nodes, out[1] x 48-byte leaf records), from wherever it was built. */
int pbrt_hip_accel_copy(PbrtHipScene*, void* out_nodes, uint64_t node_capacity, void* out_leaf_records, uint64_t record_capacity);

/* ---- the hot path ---------------------------------------------------------------------------------------- */

/* Primitive::intersect on a batch (accelerators/src/bvh/mod.rs:173-226): host buffers, synchronous. */
int pbrt_hip_intersect_batch(PbrtHipScene*, const PbrtHipRay* rays, PbrtHipHit* hits, uint64_t n);
/* Primitive::intersect_p on a batch (bvh/mod.rs:231-283): out[i] = 1 if occluded. */
int pbrt_hip_occluded_batch(PbrtHipScene*, const PbrtHipRay* rays, uint8_t* out_occluded, uint64_t n);

/* Same, device-resident buffers on the handle's device; enqueued on the handle's stream and synchronised
 * before returning unless sync==0.  kernel_ms (may be NULL) receives the HIP-event duration of the kernel alone. */
int pbrt_hip_intersect_batch_device(PbrtHipScene*, const void* d_rays, void* d_hits, uint64_t n, float* kernel_ms);
int pbrt_hip_occluded_batch_device(PbrtHipScene*, const void* d_rays, void* d_occluded, uint64_t n, float* kernel_ms);

/* Measurement aid (not a reference interface): with counting on, traversal launches also tally their work.
 * out[0..2] closest-hit {interior nodes whose box test passed, triangle tests, rays}, out[3..5] the same for any-hit.
 * Reference-format node visits of the closest-hit rays = out[2] + 2*out[0]; of the any-hit rays (which stop early) = out[6],
 * counted as they happen.  out[7] is spare.  get resets the tallies.  Never timed. */
int pbrt_hip_set_traversal_counting(PbrtHipScene*, int on);
int pbrt_hip_get_traversal_counts(PbrtHipScene*, uint64_t out[8]);

/* Integrator::render for PathIntegrator (core/src/integrator/sampler_integrator.rs:243-415 +
 * integrators/src/path.rs:103-284).  Renders the 16x16 (tile_size) sample tiles whose index t satisfies
 * t % tile_parts == tile_part (tile enumeration = sampler_integrator.rs:254-259,314-336), i.e. the whole frame for
 * (0,1).  light_strategy: 0 uniform, 1 power, 2 spatial (the reference's default, core/src/light_distrib/spatial.rs;
 * with one light the reference itself forces uniform, light_distrib/mod.rs:59-64).
 *
 * Output = the per-pixel state Film keeps (core/src/film/mod.rs:33-47): out_xyz[3*i..] = sum of rgb_to_xyz(tile
 * contrib), out_weight[i] = filter weight sum, i indexing cropped_pixel_bounds row-major.  Film::write_image's
 * normalisation (:356-417) is pbrt_hip_film_to_rgb. */
int pbrt_hip_render_path(PbrtHipScene*, int max_depth, float rr_threshold, int light_strategy,
                         const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                         float* out_xyz, float* out_weight, PbrtHipStats* out_stats);

/* Integrator::render for WhittedIntegrator (core/src/integrator/sampler_integrator.rs:243-415 + integrators/src/whitted.rs:51-118, with
 * SamplerIntegrator::specular_reflect / specular_transmit, sampler_integrator.rs:79-238).  Film, sampler, camera, tile enumeration, pixel_bounds and the
 * output convention are pbrt_hip_render_path's.  li per camera ray: a miss adds every light's le (whitted.rs:57-61); a Material "none" surface is passed at the
 * same depth (:63-66); a hit gets its differentials, bump map and BSDF with allow_multiple_lobes = false — smooth glass is SpecularReflection(Kr, dielectric)
 * followed by SpecularTransmission(Kt), each where its colour is not black, instead of FresnelSpecular (glass.rs:112-129) —, adds its emission (:84) and, for
 * every light in order, one sample `f * Li * |wi.ns| / pdf` behind one occlusion ray, sent only where the sample is valid, f is not black and the pdf is not
 * zero (:88-104): no MIS, no light distribution, no Russian roulette.  A light made by pbrt_hip_add_sphere_light is sampled by Sphere::sample_solid_angle (shapes/src/sphere.rs:344-410)
 * and seen by the rays that meet its sphere; this is the only integrator that renders such a scene.  If depth + 1 < max_depth the reflected and then the refracted ray are followed (:108-113),
 * each with the ray differentials of sampler_integrator.rs:96-119 / :171-230 when its parent carries some, and `L += reflected + refracted`.
 * Evaluated as the recursion it is: every level keeps its partial L and the factors its child's value is multiplied by.
 * max_depth in [0, 16], INVALID_ARG beyond.  UNSUPPORTED, before any work: a render whose recursion COULD draw more sampler dimensions than the tables hold —
 * 5 + V * 2 * n_lights + I * 4 must stay below 1000 (Halton, halton.rs:106-110) / 1024 (Sobol) and within the n32 / 52 dimensions given to pbrt_hip_set_sobol_tables,
 * where, with d = max(max_depth, 1), the recursion tree has V = 2^d - 1 vertices of which I = 2^(d-1) - 1 lie above the last level if the scene's materials hold specular
 * reflection AND specular transmission lobes, V = d and I = d - 1 with one of the two kinds, V = 1 and I = min(d - 1, 1) with neither; and a handle made by pbrt_hip_scene_create_multi (several devices render with pbrt_hip_render_whitted_devices).
 * out_stats: camera_rays, regular_rays, shadow_rays and render_seconds are filled, the rest is zero. */
int pbrt_hip_render_whitted(PbrtHipScene*, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                            float* out_xyz, float* out_weight, PbrtHipStats* out_stats);
/* pbrt_hip_render_whitted for a handle over any number of devices: the reference's tile loop over worker threads (core/src/integrator/sampler_integrator.rs:254-296) with one
 * device per worker.  On a one-device handle it is pbrt_hip_render_whitted, call for call.  On a handle over n devices (pbrt_hip_scene_create_multi) device k renders the tiles t
 * with t % (tile_parts * n) == tile_part + tile_parts * k, with its own workspace, chunk plan and film bands (the handle's sample-record budget applies to each); the tile buffers
 * are gathered on the first device and merged there in increasing tile index (Film::merge_film_tile, core/src/film/mod.rs:220-279), as pbrt_hip_render_path does on such a handle:
 * the film equals the one-device film bit for bit.  out_stats: camera_rays, regular_rays and shadow_rays are summed over the devices, render_seconds is the largest of theirs, the
 * rest is zero; pbrt_hip_get_render_footprint reports per entry the largest value of any device.  Refusals are pbrt_hip_render_whitted's (checked on the handle's state, before any
 * device is touched) and INVALID_ARG where tile_parts * n exceeds 64; all of them before any work, the outputs untouched and the handle usable. */
int pbrt_hip_render_whitted_devices(PbrtHipScene*, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                                    float* out_xyz, float* out_weight, PbrtHipStats* out_stats);

/* Integrator::render for DirectLightingIntegrator (core/src/integrator/sampler_integrator.rs:243-415 + integrators/src/direct_lighting.rs:110-166), on the Whitted driver:
 * film, sampler, camera, tiles, pixel_bounds, the recursion (specular_reflect then specular_transmit, sampler_integrator.rs:79-238, while depth + 1 < max_depth), the BSDF
 * (allow_multiple_lobes = false), the miss and the Material "none" cases are pbrt_hip_render_whitted's.  What differs is the light phase of a vertex, after `L += isect.le(wo)`:
 * strategy 0 ("all"): uniform_sample_all_lights AS IT RUNS in the reference (core/src/integrator/common.rs:22-78).  preprocess (direct_lighting.rs:72-90) requests sample arrays on
 *   the integrator's own sampler, but render_tile works on clone_sampler copies that hold none (samplers/src/halton.rs:177-183, sobol.rs:110-112), get_2d_array returns an empty
 *   vector (core/src/sampler/common.rs:108-122) and the branch `nl == 0 || sl == 0` (common.rs:42-57) is always taken: per light, in Scene::lights order, u_light = get_2d,
 *   u_scattering = get_2d, l += estimate_direct; `l` joins L once.  n_light_samples never matters and no array dimension is skipped.
 * strategy 1 ("one"): uniform_sample_one_light with no distribution (common.rs:89-133): get_1d, light = min(u * n, n - 1), then u_light, u_scattering, estimate_direct / (1 / n).
 * estimate_direct (common.rs:146-299, specular = false, handle_media = false) is the path integrator's: the light half behind an occlusion ray, weighted by the power heuristic
 * for a non-delta light; for such a light also the BSDF half, a closest-hit ray that counts where it meets this very light (or, on a miss, its le).  Those rays count as regular_rays.
 * INVALID_ARG: strategy other than 0 / 1, max_depth outside [0, 16].  UNSUPPORTED, before any work: a recursion that COULD draw more sampler dimensions than the tables hold —
 * 5 + V * D + I * 4 with V and I as for pbrt_hip_render_whitted and D = 4 * n_lights (all) or 5 (one; 0 without lights) must stay below 1000 (Halton) / 1024 (Sobol) and within the
 * n32 / 52 dimensions given to pbrt_hip_set_sobol_tables; a scene with a light made by pbrt_hip_add_sphere_light on a handle without pbrt_hip_set_path_sphere_lights (the MIS weight
 * needs Sphere::pdf_solid_angle, whose inside branch is that switch's documented departure; disk and cylinder lights need no switch); a handle made by pbrt_hip_scene_create_multi
 * (several devices render with pbrt_hip_render_direct_devices).  The outputs are untouched and the handle stays usable.
 * out_stats: camera_rays, regular_rays, shadow_rays and render_seconds are filled, the rest is zero. */
int pbrt_hip_render_direct(PbrtHipScene*, int strategy, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                           float* out_xyz, float* out_weight, PbrtHipStats* out_stats);
/* pbrt_hip_render_direct for a handle over any number of devices, as pbrt_hip_render_whitted_devices is for pbrt_hip_render_whitted (sampler_integrator.rs:254-296; the merge:
 * core/src/film/mod.rs:220-279): the same tile deal, gather, merge order, stats and refusals, and a film that equals the one-device film bit for bit. */
int pbrt_hip_render_direct_devices(PbrtHipScene*, int strategy, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                                   float* out_xyz, float* out_weight, PbrtHipStats* out_stats);

/* Memory for the sample records. A render keeps one 20-byte record {L.rgb, p_film} per camera sample until the film pass has replayed FilmTile::add_sample over it
 * (core/src/film/film_tile.rs:62-108).  The reference holds O(pixels): every worker thread adds its samples to its FilmTile as they are made and Film::merge_film_tile
 * (core/src/film/mod.rs:220-279) folds the tile into the film.  Here the records of a frame are resident in BANDS: consecutive runs of this rank's 16x16 (tile_size) tiles,
 * in increasing tile index, each band with all of its samples.  A FilmTile takes samples of its own tile only (film_tile.rs:62-108; Film::get_film_tile, film/mod.rs:182-198),
 * so a band is rendered and passed to the film on its own and the film, the weights and every counter equal the one-band render bit for bit, for every filter.
 * `bytes` bounds pixels * spp * 20 B of one band; a band is never less than one tile, so a budget below one tile's records renders one tile per band and
 * pbrt_hip_get_render_footprint reports the overshoot (not an error).  0 = automatic: one band whenever all records fit beside the smallest chunk of paths in the
 * memory that is free or already held by the handle, else half of the memory the chunk planner counts as available.  The setting holds until it is changed and
 * applies to every render entry point and to every device of a handle made by pbrt_hip_scene_create_multi. */
int pbrt_hip_set_sample_record_budget(PbrtHipScene*, uint64_t bytes);
/* What the last render of the handle came to (film/mod.rs and film_tile.rs keep no such tally; a measurement aid): out[0] bands, out[1] tiles in the largest band,
 * out[2] peak sample-record bytes (the largest band's pixels * spp * 20), out[3] the budget that applied (the automatic one where none was set), out[4] paths per
 * chunk, out[5] bytes of the chunk-scaled buffers for them, out[6] = out[7] = 0.  All zero before the first render; out[0] = 0 after a render without pixels.
 * A multi-device handle reports, entry by entry, the largest value any of its devices came to. */
int pbrt_hip_get_render_footprint(PbrtHipScene*, uint64_t out[8]);
/* pbrt_hip_get_mis_escape: *out = 1 if the handle's last pbrt_hip_render_path* call traced estimate_direct's BSDF-sampled ray as an escape query, else 0 (also before any render).
 * In a scene without area lights of any shape, whose traversal row has neither alpha-mask textures nor quadrics, and with traversal counting off, the shade pass reads one bit of
 * that ray's result — did it hit anything —, so the traversal kernel stops it at the first primitive the reference's intersect would accept instead of refining a closest hit
 * nobody reads.  The ray remains a closest-hit ray in every respect a caller can see: the film, PbrtHipStats (regular_rays, shadow_rays, paths) and the footprint
 * (pbrt_hip_get_render_footprint: bytes per path, paths per chunk) are bit for bit what they are without the query.  PBRT_HIP_ERR_INVALID_ARG: a null argument. */
int pbrt_hip_get_mis_escape(PbrtHipScene*, int* out);

/* Multi-GPU form: writes this rank's FilmTiles (contrib rgb + weight, 4 floats per tile pixel, tiles in
 * increasing index order, each tile's pixel bounds as Film::get_film_tile computes them) into a DEVICE buffer
 * the caller owns (e.g. a torch tensor) so the host can gather them with RCCL; then any rank calls
 * pbrt_hip_merge_tiles on the gathered buffers.  Query sizes with pbrt_hip_tile_buffer_floats. */
int pbrt_hip_tile_buffer_floats(PbrtHipScene*, int tile_size, int tile_part, int tile_parts, uint64_t* out_floats);
int pbrt_hip_render_path_tiles_device(PbrtHipScene*, int max_depth, float rr_threshold, int light_strategy,
                                      const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                                      void* d_tile_buffer, PbrtHipStats* out_stats);
/* The same for the Whitted integrator: pbrt_hip_render_whitted's arguments and refusals (then INVALID_ARG for a null buffer), this rank's FilmTiles (the tiles t with
 * t % tile_parts == tile_part, sampler_integrator.rs:254-296) into the caller's device buffer of pbrt_hip_tile_buffer_floats floats, ready for pbrt_hip_merge_tiles_device
 * (Film::merge_film_tile, core/src/film/mod.rs:220-279).  One process per GPU renders a Whitted frame with it as with the path form. */
int pbrt_hip_render_whitted_tiles_device(PbrtHipScene*, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                                         void* d_tile_buffer, PbrtHipStats* out_stats);
/* ... and for the direct-lighting integrator (direct_lighting.rs:110-166): pbrt_hip_render_direct's arguments and refusals (then INVALID_ARG for a null buffer), this rank's
 * FilmTiles (sampler_integrator.rs:254-296) into the caller's device buffer, ready for pbrt_hip_merge_tiles_device. */
int pbrt_hip_render_direct_tiles_device(PbrtHipScene*, int strategy, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts,
                                        void* d_tile_buffer, PbrtHipStats* out_stats);
/* Film::merge_film_tile (core/src/film/mod.rs:220-279) in increasing tile order over tile_parts device buffers. */
int pbrt_hip_merge_tiles_device(PbrtHipScene*, int tile_size, int tile_parts, const void* const* d_tile_buffers,
                                float* out_xyz, float* out_weight);

/* Film::get_pixel_rgb (core/src/film/mod.rs:392-417) on the host: rgb[3*i..]. */
int pbrt_hip_film_to_rgb(const PbrtHipScene*, const float* xyz, const float* weight, float* out_rgb);

/* K1 alone, for parity tests of a-S/a-C: camera rays for sample index s of every pixel of pixel_bounds,
 * row-major (get_camera_sample + generate_ray_differential, sampler/mod.rs:45-53, perspective_camera.rs:144-204). */
int pbrt_hip_generate_camera_rays(PbrtHipScene*, const int pixel_bounds[4], uint32_t sample_index,
                                  PbrtHipRay* out_rays, float* out_pfilm_xy);

/* Test aids for a-M and a-S: the device's BSDF and sampler code on explicit inputs.  A binding does not need them.  Both need an uploaded scene only (no accelerator), launch a
 * kernel that calls the functions the render kernels call, and leave the handle usable after a refusal.
 *
 * pbrt_hip_bsdf_probe_batch: `material`'s BSDF (BSDF::new, core/src/reflection/bsdf.rs:100-116) in the frame `frame` = {shading normal ns, geometric normal ng, shading dpdu}
 * (9 floats; NULL: ns = ng = +z, dpdu = +x), n probes, 8 floats out each, world-space directions:
 *   op 0  out[0..2] = BSDF::f(wo, wi, flags) (bsdf.rs:133-158), out[3] = BSDF::pdf(wo, wi, flags) (bsdf.rs:331-356)
 *   op 1  BSDF::sample_f(wo, u, flags) (bsdf.rs:160-292): out[0..2] = f, out[3] = pdf, out[4..6] = wi, out[7] = the sampled BxDFType (0 for a failed sample)
 *   op 2  out[0] = BSDF::num_components(flags), out[1] = number of BxDFs, out[2] = BSDF::eta
 * path 0: the general lobe list, as the shade pass makes it for scenes that hold more than MatteMaterial.  path 1: the one-lobe BSDF of scenes made of MatteMaterial alone, which has
 * neither flags nor a sampled type: every flags[i] must hold REFLECTION | DIFFUSE (PBRT_HIP_ERR_INVALID_ARG otherwise), and out[7] is the lobe's type where pdf != 0.
 * PBRT_HIP_ERR_UNSUPPORTED: the material takes any parameter from a texture (bump map included); path 1 for a material not made by pbrt_hip_add_material_matte.
 * PBRT_HIP_ERR_INVALID_ARG: unknown material, op or path; a null array with n > 0. */
int pbrt_hip_bsdf_probe_batch(PbrtHipScene*, uint32_t material, int op, int path, uint64_t n, const float* wo /*3n*/, const float* wi /*3n*/, const float* u /*2n*/,
                              const uint32_t* flags /*n*/, const float* frame /*9 or NULL*/, float* out /*8n*/);
/* pbrt_hip_sampler_value_batch: out[i] = the configured sampler's value for pixel xy[i], sample number sample[i], dimension dim[i] — GlobalSampler::get_index_for_sample followed by
 * sample_dimension (samplers/src/halton.rs:118-160, samplers/src/sobol.rs:65-93).  use_lds != 0: under Halton the block first stages the tables of the first 54 dimensions in LDS,
 * as the shade pass does, and reads those dimensions from there.  PBRT_HIP_ERR_STATE: no sampler, or Sobol without tables.  PBRT_HIP_ERR_UNSUPPORTED: Sobol beyond the tables given
 * (dimension, sample-bounds resolution, or a sample number whose index needs more than the 52 columns of a matrix).  PBRT_HIP_ERR_INVALID_ARG: a Halton dimension >= 1000
 * (PRIME_TABLE_SIZE); a Sobol pixel outside the sampler's power-of-two square. */
int pbrt_hip_sampler_value_batch(PbrtHipScene*, uint64_t n, const int* xy /*2n*/, const uint32_t* sample /*n*/, const uint32_t* dim /*n*/, int use_lds, float* out /*n*/);
/* pbrt_hip_light_probe_batch (a-Li, a-T2, f6): light number `light` (the order of the add_light_* / add_sphere_light calls) of a scene whose accelerator is built, on n reference points.
 * ref = per probe {p[3], p_error[3], n[3], time}: the fields of the Interaction the light code reads; u = the 2D sample, wi = a world-space direction.
 * Layout 1 of the output: PBRT_HIP_LIGHT_PROBE_STRIDE = 28 floats per probe, zeroed first, then
 *   op 0  Light::sample_li(ref, u): out[0..2] wi, [3] pdf, [4..6] radiance, [7] 1 where a sample was made, [8..10] / [11..13] / [14..16] the point, error and normal of the
 *         VisibilityTester's far end, and the ray Interaction::spawn_ray_to_hit (core/src/interaction/mod.rs:212-223) makes towards it: [17..19] origin, [20..22] direction, [23] t_max.
 *         Where no sample was made ([7] = 0) the record is as sample_li initialised it and the ray slots stay zero.  [24..27] are spare.
 *   op 1  out[0] = Light::pdf_li(ref, wi)
 *   op 2  out[0..2] = Light::le of a ray with direction wi
 * variant 0: the code of scenes with textures (radiance, projection and goniometric maps are read); variant 1: the code of scenes without, PBRT_HIP_ERR_UNSUPPORTED for a light that
 * holds such a map; variant 2: sample_li as pbrt_hip_render_whitted's light loop calls it (op 0 only), the one variant that admits a light made by pbrt_hip_add_sphere_light
 * or pbrt_hip_add_quadric_light (PBRT_HIP_ERR_UNSUPPORTED under 0 and 1: those are the forms whose area lights are triangles).
 * PBRT_HIP_ERR_INVALID_ARG: unknown light, op or variant; op 1 or 2 under variant 2; a null array with n > 0; n > 2^32 - 1.  PBRT_HIP_ERR_STATE: no accelerator built; an area light
 * without its mesh.  Nothing is launched on a refusal. */
#define PBRT_HIP_LIGHT_PROBE_STRIDE 28
int pbrt_hip_light_probe_batch(PbrtHipScene*, uint32_t light, int op, int variant, uint64_t n, const float* ref /*10n*/, const float* u /*2n*/, const float* wi /*3n*/,
                               float* out /*28n*/);
/* pbrt_hip_sphere_light_probe_batch: a light made by pbrt_hip_add_sphere_light or pbrt_hip_add_quadric_light as the path integrator's sphere-light shade pass calls it.  op 0:
 * Light::sample_li — the function variant 2 of pbrt_hip_light_probe_batch runs; op 1: out[0] = Light::pdf_li(ref, wi), Sphere::pdf_solid_angle as described at
 * pbrt_hip_add_sphere_light, the trait's default Shape::pdf_solid_angle for a disk or a cylinder.  Inputs and the 28-float
 * output layout are pbrt_hip_light_probe_batch's; the handle's pbrt_hip_set_path_sphere_lights switch is not consulted.  PBRT_HIP_ERR_UNSUPPORTED: the light's shape is not
 * a quadric.  PBRT_HIP_ERR_INVALID_ARG: unknown light or op; a null handle; a null array with n > 0; n > 2^32 - 1.  PBRT_HIP_ERR_STATE: no accelerator built. */
int pbrt_hip_sphere_light_probe_batch(PbrtHipScene*, uint32_t light, int op, uint64_t n, const float* ref /*10n*/, const float* u /*2n*/, const float* wi /*3n*/, float* out /*28n*/);
/* pbrt_hip_spatial_probe_begin / _batch / _voxel: the spatial light distribution (light strategy 2) on explicit points (a test aid like the probes above).
 * _begin sets the tables up exactly as a strategy-2 render does: the world bound of the built tree, the voxel resolution (out_nv), a pool of *out_capacity slots
 * (PBRT_HIP_SPATIAL_POOL_BYTES is honoured), tables and counters cleared.  PBRT_HIP_ERR_STATE: no accelerator, or fewer than two lights (a render builds no tables then).
 * _batch, strategy 2: one claim pass over the n points p (the first point in an untouched voxel claims a pool slot, as the render's claim pass does), one pass of the kernel that
 * builds the claimed voxels' distributions (the instantiation a render of this scene launches), one pass that picks a light per point with the sample u[i]:
 * out_pi[3i..] = the point's voxel, out_light[i] = the light picked, out_pick_pdf[i] = its discrete probability.  Tables stay from one call to the next, until the next _begin or
 * render.  strategy 0 / 1: the pick alone, on the scene-wide uniform / power table; out_pi is not written and no _begin is needed.  out_counters (may be null) = slots claimed,
 * slots computed, pool-exhausted flag, blocks-finished count, as left on the device.  PBRT_HIP_ERR_OOM: the pool ran out (as a render reports it; the handle stays usable).
 * PBRT_HIP_ERR_STATE: strategy 2 without _begin since the last render; no accelerator; no light.  PBRT_HIP_ERR_INVALID_ARG: a null array with n > 0; n > 2^32 - 1; unknown strategy.
 * _voxel reads back func[n_lights], cdf[n_lights + 1] and func_int of a computed voxel.  PBRT_HIP_ERR_STATE: no tables, or the voxel has no slot.  PBRT_HIP_ERR_INVALID_ARG: pi outside the grid.
 * All three: PBRT_HIP_ERR_UNSUPPORTED for a scene the path integrator refuses, one that holds a light made by pbrt_hip_add_sphere_light on a handle without
 * pbrt_hip_set_path_sphere_lights (_voxel cannot meet it: such a scene gets no tables).  A slot's layout is fixed by the number of lights at _begin: _batch with strategy 2 and
 * _voxel return PBRT_HIP_ERR_STATE when a light was added since. */
int pbrt_hip_spatial_probe_begin(PbrtHipScene*, int out_nv[3], uint32_t* out_capacity);
int pbrt_hip_spatial_probe_batch(PbrtHipScene*, uint64_t n, const float* p /*3n*/, const float* u /*n*/, int strategy, int32_t* out_pi /*3n*/, uint32_t* out_light /*n*/,
                                 float* out_pick_pdf /*n*/, uint32_t out_counters[4]);
int pbrt_hip_spatial_probe_voxel(PbrtHipScene*, const int pi[3], float* func, float* cdf, float* func_int);
/* pbrt_hip_curve_probe_batch: the two device functions behind a curve segment, on explicit rays (a test aid like the probes above).  prim = the segment's slot in the primitive list.
 * Each ray is tested with its OWN t_max by curve_test — Curve::intersect(r, is_shadow_ray) up to the accept decision (curve.rs:543-645 with recursive_intersect, :339-501) —; on a hit
 * in closest-hit mode (shadow == 0) curve_surface rebuilds the SurfaceInteraction from (ray, t, u, v) as the shade pass does (:463-471, :496-534).  out, 20 floats per ray: hit flag
 * (1.0 / 0.0), t, u, v, then in world space p, p_error, dpdu, dpdv, n (3 each), one pad word; everything after the flag is zero on a miss and with shadow != 0 (Curve::intersect_p).
 * PBRT_HIP_ERR_INVALID_ARG: a null handle; a null array with n > 0; n > 2^32 - 1; prim is not a curve segment.  PBRT_HIP_ERR_STATE: no accelerator built. */
#define PBRT_HIP_CURVE_PROBE_STRIDE 20
int pbrt_hip_curve_probe_batch(PbrtHipScene*, uint32_t prim, int shadow, uint64_t n, const PbrtHipRay* rays, float* out /*20n*/);
/* pbrt_hip_surface_probe_batch: the code between "the traversal reported (prim, b0, b1, b2, instance)" and "BSDF, textures, lights and the next ray read a surface interaction", on
 * explicit hits (a test aid like the probes above).  Needs a built accelerator — the leaf records and a hit's pad[0] exist only then.  Per probe: the world-space ray; a PbrtHipHit as
 * pbrt_hip_intersect_batch writes it, whose t, b0, b1, b2 the caller may then set freely (a quadric's interaction is rebuilt from the ray, a curve segment's from the ray and t, b0, b1);
 * and PBRT_HIP_SURFACE_PROBE_AUX = 48 floats:
 *   [0..1] p_film  [2..3] lens sample  [4..6] wi  [7..9] hp  [10..12] hp_error  [13..15] hn (the target of spawn_ray_to_hit)
 *   op 4 only: [16..18] / [19..21] the parent ray's rx_direction / ry_direction (its offset origins are not read by the reference's formulas), [22..25] du/dx dv/dx du/dy dv/dy,
 *   [26..28] dp/dx, [29..31] dp/dy, [32..34] dn/du, [35..37] dn/dv, [38] the BSDF's eta, [39] != 0: the refracted ray, else the reflected one.  [40..47] spare.
 * variant = how the interaction is made: 0 make_surface_hit, indexed by prim (what Light::pdf_li's Triangle::intersect uses; PBRT_HIP_ERR_UNSUPPORTED for a hit with pad[1] != 0 — there
 * is no such path for instances — and for a quadric's or curve segment's slot); 1 make_surface_hit_any, from the leaf record, through an instance if pad[1] != 0 (UNSUPPORTED for a
 * quadric's or curve segment's slot); 2 make_surface_hit_q<true>, the form of scenes that hold quadric shapes (UNSUPPORTED for a scene without one: its kernels have no such instantiation).
 * op = what is computed from that interaction, by the functions the render kernels call.  Output: PBRT_HIP_SURFACE_PROBE_STRIDE = 40 words per probe, zeroed first, then
 *   op 0  the interaction: [0..2] p, [3..5] p_error, [6..8] wo, [9..11] n, [12..14] shading n, [15..17] shading dp/du, [18] time, [19] prim (as an integer's bits)
 *   op 1  the texture side without displacement: [0..1] uv, [2..4] / [5..7] the geometric dp/du, dp/dv in world space, [8..11] du/dx dv/dx du/dy dv/dy and [12..14] / [15..17]
 *         dp/dx, dp/dy of the context the texture pass evaluates (hit_tex_ctx; for a quadric or curve hit tex_ctx_from on the shape's own u, v, dp/du, dp/dv) — zero unless camera_ray —,
 *         [18..29] rx_origin, ry_origin, rx_direction, ry_direction of the camera ray's scaled differentials (camera_ray_differentials on p_film, lens and the ray; zero unless camera_ray),
 *         [30..32] / [33..35] the shading dn/du, dn/dv (tri_shading_dn; the shape's own for a quadric)
 *   op 2  Material::bump with `texture` as the displacement on op 1's context (hit_bump; bump_shading on the shape's frame for a quadric): [0..2] the new shading n, [3..5] shading dp/du
 *   op 3  [0..7] Interaction::spawn_ray(wi) and [8..15] spawn_ray_to_hit(hp, hp_error, hn), each as a PbrtHipRay: origin, t_max, direction, time
 *   op 4  the differentials of the specularly reflected / refracted ray (sampler_integrator.rs:96-119, :171-230) with the interaction's p, wo and shading n, the direction wi and
 *         aux[16..39]: [0..2] rx_origin, [3..5] ry_origin, [6..8] rx_direction, [9..11] ry_direction
 *   [39] is left zero (the test oracle's counterpart reports the branches a probe took there).
 * camera_ray != 0 (ops 1 and 2): the ray is a camera ray of the handle's camera, made at p_film with the lens sample `lens`; the sampler supplies its samples per pixel.
 * Refusals, before anything is launched; the handle stays usable.  PBRT_HIP_ERR_INVALID_ARG: a null handle; a null array with n > 0; n > 2^32 - 1; an unknown op or variant; a hit
 * whose prim is 0xFFFFFFFF or no primitive, whose pad[0] is no leaf record of that primitive or whose pad[1] names no instance that holds it; an unknown texture under op 2.
 * PBRT_HIP_ERR_STATE: no accelerator; camera_ray under op 1 or 2 without a camera, a film and a sampler.  PBRT_HIP_ERR_UNSUPPORTED: as listed with the variants; op 2 on a curve segment. */
#define PBRT_HIP_SURFACE_PROBE_AUX 48
#define PBRT_HIP_SURFACE_PROBE_STRIDE 40
int pbrt_hip_surface_probe_batch(PbrtHipScene*, int op, int variant, uint32_t texture, int camera_ray, uint64_t n, const PbrtHipRay* rays, const PbrtHipHit* hits,
                                 const float* aux /*48n*/, float* out /*40n*/);
/* pbrt_hip_raysort_probe: the ray binning between wavefront rounds (csrc/raysort.h) on explicit keys, through the launch the path integrator's rounds use.  keys_cl / keys_sh = the
 * bin keys (< 4096) of n_cl closest-hit and n_sh any-hit rays; the keys and the two counts are uploaded and read from device memory, as in a render.  order_out[0 .. n_cl + n_sh) =
 * the queue positions (closest-hit rays 0 .. n_cl, any-hit rays behind them) grouped by bin, closest-hit rays first; the order inside a bin is unspecified.  sort_blocks = the grid
 * of the two passes over the keys (a render uses 1024).  Needs a handle only: no geometry, no accelerator.
 * A closest-hit key may carry the escape-query mark, 4096, on top of its bin (pbrt_hip_get_mis_escape): that ray's entry of order_out then has bit 31 set, and the ray is grouped
 * with the unmarked closest-hit rays of its bin; an unmarked key gives the entry it always gave.
 * PBRT_HIP_ERR_INVALID_ARG: a null handle; sort_blocks 0 or above 65536; a null array with a non-zero count; a closest-hit key >= 8192 or an any-hit key >= 4096;
 * n_cl + n_sh >= 0x7FFF0000.  Nothing is launched on a refusal. */
int pbrt_hip_raysort_probe(PbrtHipScene*, uint32_t n_cl, uint32_t n_sh, const uint32_t* keys_cl, const uint32_t* keys_sh, uint32_t sort_blocks, uint32_t* order_out /* n_cl + n_sh */);
/* pbrt_hip_texture_probe_batch (a-SI, f3): texture number `texture` at n explicit contexts (the 15 floats per point of pbrt_hip_texture_eval_batch), through each piece of code the
 * renderer evaluates textures with; 3 floats out per probe.
 *   variant 0  the general evaluator with differentials (camera rays of scenes with procedural textures)      variant 1  the same without: the derivative fields are ignored as if zero
 *   variant 2  the evaluator of scenes whose programs hold only constants, uv-mapped image maps, scale and mix, with differentials      variant 3  the same without
 *   variant 4  the lean alpha test's evaluator on the context's (u, v): red channel in out[0], out[1] = out[2] = 0
 * Variants 2 and 3 must equal 0 and 1; 1 must equal 0 on zero derivatives; 4 must equal the red channel of 1.
 * pbrt_hip_bump_probe_batch: Material::bump (core/src/material.rs:62-101) with `texture` as the displacement, on an explicit shading frame.  in = per probe the 15 context floats (the
 * hit point is the context's p), then n, ns, dpdu_s, dpdv_s, dndu, dndv (33 floats); out = the new shading normal and shading dp/du (6 floats).  variant 0 .. 3 as above.
 * Both need an uploaded scene only (no accelerator) and leave the handle usable after a refusal.
 * PBRT_HIP_ERR_INVALID_ARG: unknown texture or variant; a null array with n > 0; n > 2^32 - 1.  PBRT_HIP_ERR_UNSUPPORTED: variant 2, 3 or 4 on a program that holds any other
 * operation than constant, uv-mapped image map, scale and mix.  Nothing is launched on a refusal. */
int pbrt_hip_texture_probe_batch(PbrtHipScene*, uint32_t texture, int variant, uint64_t n, const float* contexts /*15n*/, float* out /*3n*/);
int pbrt_hip_bump_probe_batch(PbrtHipScene*, uint32_t texture, int variant, uint64_t n, const float* in /*33n*/, float* out /*6n*/);
/* pbrt_hip_traverse_probe: the traversal kernel (csrc/traverse.h) on an explicit work queue, launched as a wavefront round launches it.  mode 0: n_cl closest-hit rays (n_sh = 0),
 * mode 1: n_sh any-hit rays (n_cl = 0), mode 2: both queues in one launch — queue positions 0 .. n_cl are the closest-hit rays, n_cl .. n_cl + n_sh the any-hit rays; either count may
 * be 0.  The rays and the two counts are uploaded and the counts read from device memory, as in a render.  order = NULL, or n_cl + n_sh queue positions: the queue is walked in that
 * order (what the ray binning hands a round).  n_heads (1 .. 8) queue heads, head h serving the head_chunk-ray chunks c with c % n_heads == h; with n_heads = 1 the single counter
 * is used and head_chunk is ignored.  blocks = the grid: 1 .. the resident grid the handle launches its renders with (6 blocks of 256 lanes per CU).  The kernel row is the scene's,
 * the counting rows with pbrt_hip_set_traversal_counting on.  hits_out[n_cl] / occluded_out[n_sh] = what pbrt_hip_intersect_batch / pbrt_hip_occluded_batch give for the same rays:
 * the result of a ray depends on nothing but the ray.  A result the kernel did not write comes back as 0xFF bytes.
 * An entry of `order` with bit 31 set (mode 2, a closest-hit position, a scene whose kernel row has neither alpha-mask textures nor quadrics, counting off) passes through to the
 * kernel as the ray binning would hand it over: that ray is an escape query (pbrt_hip_get_mis_escape).  Its hit record comes back as t = the ray's t_max when it stopped,
 * prim = 0 if it hit anything and 0xFFFFFFFF if not — the same verdict as the unmarked ray's prim != 0xFFFFFFFF —, b0 = b1 = 0, and the other 16 bytes as they were (0xFF).
 * PBRT_HIP_ERR_INVALID_ARG: a null handle; a null array with a non-zero count; an unknown mode; mode 0 with n_sh > 0 or mode 1 with n_cl > 0; n_cl + n_sh >= 0x7FFF0000; n_heads 0 or
 * above 8; n_heads > 1 with head_chunk 0 or no multiple of 64 (the kernel's precondition: a batch of 64 rays lies in one chunk); blocks 0 or above the resident grid; an order that
 * is no permutation of 0 .. n_cl + n_sh, bit 31 aside (checked on the host); bit 31 on an entry where the line above does not allow it.  PBRT_HIP_ERR_STATE: no accelerator built.  PBRT_HIP_ERR_DEVICE: a ray's traversal stack ran over, as in
 * pbrt_hip_intersect_batch.  Nothing is launched on a refusal and the handle stays usable. */
int pbrt_hip_traverse_probe(PbrtHipScene*, int mode, const PbrtHipRay* rays_cl, uint32_t n_cl, const PbrtHipRay* rays_sh, uint32_t n_sh, const uint32_t* order /* NULL or n_cl + n_sh */,
                            uint32_t n_heads, uint32_t head_chunk, uint32_t blocks, PbrtHipHit* hits_out /* n_cl */, uint8_t* occluded_out /* n_sh */);
/* pbrt_hip_film_probe: the film side of a render (FilmTile::add_sample per tile, Film::merge_film_tile) on explicit camera samples instead of an integrator's.  Needs
 * pbrt_hip_set_film and a sampler (for its samples per pixel); no accelerator.  The tiles t with t % tile_parts == tile_part, their pixel list, the bands under
 * pbrt_hip_set_sample_record_budget, the record buffers, the film pass and the merge are the render's own.
 * pbrt_hip_film_probe_layout: out[0] = n_px, the length of this part's pixel list (tile by tile in increasing index, row-major inside a tile), out[1] = its tiles,
 * out[2], out[3] = width and height of a tile's slot in the tile buffer (4 floats per slot pixel: contribution rgb, weight sum; a tile's pixel (x, y) at row y - pb[1], column
 * x - pb[0] of its slot, the rest of the slot zero); out_px_xy (NULL or 2 n_px) = the list's pixels; out_tile_pb (NULL or 4 per tile) = every tile's FilmTile pixel bounds.
 * pbrt_hip_film_probe: L[spp][n_px][3] radiance and p_film[spp][n_px][2] film positions in that order; a NaN p_film x means "no sample taken" (a pixel outside an integrator's
 * pixel bounds).  d_tile_buffer: a DEVICE buffer of pbrt_hip_tile_buffer_floats floats for this part's tiles, or NULL for the handle's own.  out_xyz / out_weight (both or
 * neither; only with d_tile_buffer NULL): the film of this part's tiles alone, as pbrt_hip_render_path gives it.  out_tiles: NULL or a host copy of the tile buffer.
 * PBRT_HIP_ERR_INVALID_ARG, before anything is launched and leaving the handle usable: a null argument; a bad partition; n_px other than the list's length; a position outside
 * [x, x + 1] x [y, y + 1] of its pixel (the upper ends are positions that float32 rounded up onto the next pixel: the film pass rests on this bound); a non-finite radiance
 * (the integrators zero those before they record a sample).  PBRT_HIP_ERR_STATE: no film or no sampler. */
int pbrt_hip_film_probe_layout(PbrtHipScene*, int tile_size, int tile_part, int tile_parts, uint64_t out[4], int32_t* out_px_xy, int32_t* out_tile_pb);
int pbrt_hip_film_probe(PbrtHipScene*, int tile_size, int tile_part, int tile_parts, uint64_t n_px, const float* L, const float* p_film, void* d_tile_buffer, float* out_xyz,
                        float* out_weight, float* out_tiles);

#ifdef __cplusplus
}
#endif
#endif /* PBRT_HIP_H */
