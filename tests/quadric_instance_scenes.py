"""Scenes that hold quadric shapes NEXT TO object instances, for either binding (pbrt_hip.Scene on the device library or tests/oracle_binding.OracleScene): one builder feeds both
sides of the bit-for-bit comparisons of tests/test_quadric_instances_gpu.py and the CPU checks of tests/test_quadric_instances_oracle.py.

The stage (`stage`) takes the instanced scene of tests/test_instancing_gpu.py — 300 random triangles as object `ob`, its first triangle x 2 as the single-primitive object `one`, an
empty object, seven ObjectInstance directives under four transforms (six instances: the empty object's adds none), a 4 x 4 floor grid at z = -1.2 — and puts four quadrics among the directives: a mirror sphere ahead of
everything, a partial cylinder between the first two instances, a disk after the third instance and a cone last.  The floor may carry an alpha and a shadow-alpha mask
(quadric_alpha_scenes.mask_textures): "imagemap" keeps the scene in the traversal kernel's lean alpha row, "checkerboard" needs the general evaluator's.

`one_leaf` puts a triangle, two quadrics and two instances into ONE scene-level leaf (max_prims_in_node = 255), in either directive order."""
import numpy as np

import closed_form as cf
import pbrt_hip
import scenes
from quadric_alpha_scenes import cf_ctm, mask_textures, sobol_fixture_64
from sphere_light_scenes import add_sphere_light

MISS = 0xFFFFFFFF
INST_BIT = 0x80000000      # ORC_INST_BIT of the oracle's ordered primitive list
MASKS = (None, "imagemap", "checkerboard")
RES, SPP = (48, 40), 4
FLOOR = 3.0                # the floor grid spans [-FLOOR, FLOOR]^2; uv = (xy + FLOOR) / (2 FLOOR)
SPHERE_C, SPHERE_R = (0.3, 0.2, 0.6), 0.8
I4 = (np.eye(4, dtype=np.float32).reshape(16),) * 2
T_OFFSETS = ((2.5, 0.3, -0.2), (-2.0, 0.5, 0.4), (0.2, -2.2, 0.1))


def transforms(host):
    """the four instance transforms of tests/test_instancing_gpu.py::_transforms"""
    mul = host.compose
    return [mul(mul(I4, host.translate(T_OFFSETS[0])), host.rotate(40, [0.2, 1, 0.3])),
            mul(mul(I4, host.translate(T_OFFSETS[1])), host.scale([0.7, 1.3, 0.9])),
            mul(mul(I4, host.translate(T_OFFSETS[2])), host.scale([-1.0, 1.0, 1.0])),   # handedness flip
            I4]


def stage(s, host, split=0, mask=None, max_prims=4, sphere_at=SPHERE_C, fancy=False, whitted=False, sphere_light=False, sampler="halton", camera=True,
          build=True):
    """-> {name: (first primitive, count)} of the scene-level shapes.  split 1 (HLBVH) replaces the regular floor grid, on which the reference's HLBVH build asserts, by random
    triangles and takes no mask.  fancy: plastic / glass on two of the quadrics and a bump map on the instanced object's material.  whitted: plus a glass sphere;
    sphere_light: plus a spherical area light above the scene (Whitted only)."""
    prims, n = {}, [0]

    def took(name, count=1):
        prims[name] = (n[0], count); n[0] += count
    P, idx = host.gen_random_tris(300, 5)
    N = np.random.default_rng(1).normal(size=P.shape).astype(np.float32)
    Pg, ig = scenes.grid_mesh(4, z=-1.2, size=FLOOR)
    UVg = ((Pg[:, :2] + FLOOR) / (2 * FLOOR)).astype(np.float32)
    Pf, i_f, UVf = Pg, ig, UVg
    if split == 1:
        assert mask is None
        Pf, i_f = host.gen_random_tris(40, 9)
        Pf = Pf * np.float32(2.5) + np.float32([0, 0, -1.5]); UVf = None
    T = transforms(host)
    C = lambda *steps: cf_ctm(host, *steps)

    s.add_light_infinite((0.5, 0.6, 0.7))
    s.add_light_point((30, 28, 25), (0.5, -1.0, 2.5))
    m = s.add_material_matte((0.6, 0.5, 0.4), 15.0)
    m2 = s.add_material_matte((0.2, 0.6, 0.8), 0.0)
    mirror = s.add_material_mirror((0.9, 0.9, 0.9))
    red = s.add_material_matte((0.8, 0.2, 0.1))
    m_cyl = s.add_material_plastic((0.1, 0.1, 0.8), (0.3, 0.3, 0.3), 0.1) if fancy else s.add_material_matte((0.1, 0.1, 0.8))
    m_disk = s.add_material_glass(kr=(0.9, 0.95, 1.0), kt=(0.95, 0.9, 0.85), eta=1.5) if fancy else s.add_material_matte((0.8, 0.8, 0.1))
    if fancy:
        s.set_material_bump(m2, s.add_texture_windy())

    s.add_sphere(*C(host.translate(sphere_at)), SPHERE_R, None, None, 360.0, mirror, False); took("sphere")          # ahead of everything
    s.add_mesh(Pf, i_f, m, UV=UVf); took("floor", len(i_f) // 3)
    if mask: s.set_last_mesh_alpha_textures(*mask_textures(s, mask, shadow=True))
    ob = s.object_begin(); s.add_mesh(P, idx, m2, N=N); s.object_end(); n[0] += len(idx) // 3
    one = s.object_begin(); s.add_mesh(P[:3] * np.float32(2.0), [0, 1, 2], m); s.object_end(); n[0] += 1               # single primitive: used directly
    empty = s.object_begin(); s.object_end()
    s.add_instance(ob, *T[0])
    s.add_quadric("cylinder", *C(host.translate(T_OFFSETS[0]), host.rotate(70.0, (1, 1, 0))), 0.45, -0.9, 0.9, 270.0, m_cyl, False); took("cylinder")   # between the first two instances
    s.add_instance(ob, *T[1]); s.add_instance(one, *T[0])
    s.add_quadric("disk", *C(host.translate(T_OFFSETS[1]), host.rotate(15.0, (0, 1, 0))), 1.0, 0.0, 0.0, 360.0, m_disk, False); took("disk")            # after the third instance
    s.add_instance(empty, *T[1])
    s.add_instance(ob, *T[2]); s.add_instance(ob, *T[3]); s.add_instance(one, *T[3])
    if whitted:
        glass = s.add_material_glass(kr=(0.9, 0.95, 1.0), kt=(0.95, 0.9, 0.85), eta=1.5)
        s.add_sphere(*C(host.translate((-1.0, -1.6, 0.4))), 0.6, None, None, 360.0, glass, False); took("glass")
    if sphere_light:
        add_sphere_light(s, C(host.translate((0.6, -0.9, 3.5))), 0.4, material=s.add_material_matte((0.0, 0.0, 0.0)), L=(14.0, 13.0, 12.0)); took("sphere light")
    s.add_quadric("cone", *C(host.translate((0.2, -2.2, -0.4))), 0.6, 1.2, 0.0, 360.0, red, False); took("cone")       # last
    if camera:
        w2c, c2w = host.look_at((0.5, -7.5, 2.0), (0, 0, 0.5), (0, 0, 1))
        s.set_camera_perspective(host.perspective_raster_to_camera(50.0, RES[0], RES[1]), c2w)
        cb, table, sb = host.film_box(RES[0], RES[1])
        s.set_film(RES[0], RES[1], cb, (0.5, 0.5), table)
        if sampler == "sobol":
            s.set_sobol_tables(*sobol_fixture_64())
        s.set_sampler(cf.SOBOL if sampler == "sobol" else cf.HALTON, SPP, sb)
    if build:
        s.build_accel(split, max_prims)
    return prims


def stage_rays():
    return np.concatenate([scenes.random_rays(60000, 3, bound=3.0), scenes.axis_rays()])


def in_range(prim, r):
    return (prim >= r[0]) & (prim < r[0] + r[1])


def tally(hits, prims):
    """-> {quadric name: rays that end on it}, rays that end on scene-level triangles, rays per instance (index = instance number), misses"""
    hit = hits["prim"] != MISS
    inst = hits["pad"][:, 1]
    top = hit & (inst == 0)
    quadrics = {k: int((top & in_range(hits["prim"], prims[k])).sum()) for k in ("sphere", "cylinder", "disk", "cone")}
    tris = int(top.sum()) - sum(quadrics.values())
    return quadrics, tris, np.bincount(inst[hit & (inst != 0)] - 1, minlength=6), int((~hit).sum())


def oracle_leaves(orc, n_items):
    """the scene-level tree's leaves, each the tuple of its items in the leaf's order (a primitive, or INST_BIT | instance)"""
    nodes = orc.bvh_nodes()
    oprims = np.zeros(n_items, np.uint32); orc.b.lib.oracle_bvh_ordered_prims(orc.h, oprims.ctypes.data)
    return [tuple(int(v) for v in oprims[l["offset"]:l["offset"] + l["n_primitives"]]) for l in nodes[nodes["n_primitives"] > 0]]


# ---- everything in one leaf -----------------------------------------------------------------------------------------------------------------------------------------
ONE_LEAF_ITEMS = 5


def one_leaf(s, host, instance_first=False, build=True):
    """Five items whose bounds overlap almost entirely, so that no SAH split beats the leaf (sah.rs: a split must cost less than the item count): a triangle, a half-open sphere, an
    instance, a partial cylinder, another instance — or, instance_first, the same in the opposite directive order.  With max_prims_in_node = 255 the scene-level root is ONE leaf in
    directive order: no leaf reference, no hint.  The quadrics are open towards +y / -x, so rays reach the instanced triangles inside them from one side and the quadric first from the other.
    -> {name: (first primitive, count)}"""
    P, idx = host.gen_random_tris(150, 17)
    P = P * np.float32(0.7)
    m = s.add_material_matte((0.5, 0.5, 0.5))
    s.add_light_infinite((1.0, 1.0, 1.0))
    ob = s.object_begin(); s.add_mesh(P, idx, m); s.object_end()
    C = lambda *steps: cf_ctm(host, *steps)
    tri = lambda: s.add_mesh(np.array([[-1.1, -1.0, -0.9], [1.1, -0.9, 1.0], [-0.2, 1.1, -0.1]], np.float32), [0, 1, 2], m)
    sphere = lambda: s.add_sphere(*C(host.translate((0.05, 0.0, 0.0))), 1.05, None, None, 200.0, m, False)
    inst1 = lambda: s.add_instance(ob, *host.compose(host.compose(I4, host.translate((0.05, -0.05, 0.0))), host.rotate(30, [0.3, 1, 0.2])))
    cyl = lambda: s.add_quadric("cylinder", *C(host.translate((0.0, 0.05, 0.0)), host.rotate(90.0, (0, 1, 0))), 0.95, -1.0, 1.0, 250.0, m, True)
    inst2 = lambda: s.add_instance(ob, *host.compose(host.compose(I4, host.translate((-0.05, 0.0, 0.05))), host.scale([-1.0, 1.0, 1.0])))
    order = [("triangle", tri), ("sphere", sphere), ("inst1", inst1), ("cylinder", cyl), ("inst2", inst2)]
    prims, n = {}, len(idx) // 3
    for name, add in (order[::-1] if instance_first else order):
        add()
        if not name.startswith("inst"):
            prims[name] = (n, 1); n += 1
    if build:
        s.build_accel(0, 255)
    return prims


def one_leaf_rays(seed=6, n=4000):
    """Rays through the quadrics towards the instanced object in their middle, from every side, plus axis_rays(); a third end at a finite t_max just beyond the first surface they could
    meet (the target inside the object's cloud: t = 1 is the target)"""
    g = np.random.default_rng(seed)
    tgt = g.uniform(-0.6, 0.6, (n, 3))
    d = g.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    org = tgt + d * g.uniform(1.6, 3.5, (n, 1))
    r = np.zeros(n, pbrt_hip.RAY_DTYPE)
    r["o"] = org.astype(np.float32); r["d"] = (tgt - org).astype(np.float32); r["t_max"] = np.inf
    r["t_max"][::3] = g.uniform(0.55, 1.05, len(r["t_max"][::3])).astype(np.float32)
    return np.concatenate([r, scenes.axis_rays()])
