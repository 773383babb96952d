"""-m gpu: the HLBVH forest of an instanced scene built on the device (csrc/bvh_device.hip, forest form; the host's share in csrc/hlbvh_forest_stitch.h) against the host forest
builder with split_method = 1 — node array and leaf records entry by entry, statistics, world bound — and against the oracle: hits, occlusion, traversal counters, one film.
root_ref has no accessor of its own: a wrong root cannot give the oracle's hits, and scripts/hlbvh_forest_stitch_check.cpp compares it tree by tree on the CPU."""
import numpy as np
import pytest

import pbrt_hip
import scenes
from oracle_binding import OracleScene, set_libm_mode

pytestmark = pytest.mark.gpu
I4 = (np.eye(4, dtype=np.float32).reshape(16),) * 2


def _transforms(host):
    mul = host.compose
    return [mul(mul(I4, host.translate([2.5, 0.3, -0.2])), host.rotate(40, [0.2, 1, 0.3])),
            mul(mul(I4, host.translate([-2.0, 0.5, 0.4])), host.scale([0.7, 1.3, 0.9])),
            mul(mul(I4, host.translate([0.2, -2.2, 0.1])), host.scale([-1.0, 1.0, 1.0])),   # handedness flip
            I4]


# ---- the scenes: capture(s) adds materials, meshes, objects and instances, and builds nothing ----------------------------------------------------------------------------
def scene_grid_object_instances(host, with_normals=False):
    """test_instancing_gpu._instanced_scene with split 1: four instances of one object, three of a one-triangle object, an empty object, scene-level triangles before and between"""
    P, idx = host.gen_random_tris(300, 5)
    N = np.random.default_rng(1).normal(size=P.shape).astype(np.float32) if with_normals else None
    Pg, ig = host.gen_random_tris(40, 9)     # (the regular grid makes hlbvh.rs assert in the reference itself: equal treelet centroids, :338)
    Pg = Pg * np.float32(2.5) + np.float32([0, 0, -1.5])
    T = _transforms(host)

    def capture(s):
        m = s.add_material_matte((0.6, 0.5, 0.4), 15.0)
        m2 = s.add_material_matte((0.2, 0.6, 0.8), 0.0)
        s.add_mesh(Pg, ig, m)
        ob = s.object_begin(); s.add_mesh(P, idx, m2, N=N); s.object_end()
        one = s.object_begin(); s.add_mesh(P[:3] * np.float32(2.0), [0, 1, 2], m); s.object_end()
        empty = s.object_begin(); s.object_end()
        s.add_instance(ob, *T[0]); s.add_instance(ob, *T[1]); s.add_instance(one, *T[0]); s.add_instance(empty, *T[1])
        s.add_mesh(Pg + np.float32([0, 0, 3.5]), ig, m)
        s.add_instance(ob, *T[2]); s.add_instance(ob, *T[3]); s.add_instance(one, *T[3])
    return capture


def scene_one_object(host, n_inst, n_obj_tris=200):
    """test_instancing_gpu.test_instance_records_with_and_without_hints: n_inst instances of one object, lone scene-level triangles between them; n_inst = 1: one instance, nothing else"""
    P, idx = host.gen_random_tris(n_obj_tris, 11)
    Ts = _transforms(host)

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        ob = s.object_begin(); s.add_mesh(P, idx, m); s.object_end()
        for k in range(n_inst):
            if k % 3 == 1:
                s.add_mesh(P[:3] * np.float32(1.5) + np.float32([0.1 * k, 0, 0]), [0, 1, 2], m)
            s.add_instance(ob, *Ts[k % len(Ts)])
    return capture


def _soup(rng, n, centre, spread, size):
    c = centre + rng.uniform(-spread, spread, (n, 1, 3))
    return np.ascontiguousarray((c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3).astype(np.float32)), np.arange(3 * n, dtype=np.uint32)


def scene_many_small_objects(host):
    """300 object definitions of 1 .. 40 triangles, each instanced once or twice, and 50 scene-level triangles: 301 trees (a second radix digit of the tree index), objects of
    one triangle (PH_INST_SINGLE), tree boundaries inside the thread blocks of every pass"""
    rng = np.random.default_rng(2024)
    sizes = rng.integers(1, 41, 300); sizes[:4] = [1, 40, 1, 2]
    objs = [_soup(rng, int(k), np.zeros(3), 0.5, 0.15) for k in sizes]
    top = _soup(rng, 50, np.zeros(3), 3.0, 0.2)
    where = rng.uniform(-3, 3, (300, 2, 3)); twice = rng.random(300) < 0.5; scl = rng.uniform(0.5, 1.5, (300, 2, 3))

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        s.add_mesh(top[0][:75], top[1][:75], m)
        for k, (P, idx) in enumerate(objs):
            ob = s.object_begin(); s.add_mesh(P, idx, m); s.object_end()
            for j in range(2 if twice[k] else 1):
                s.add_instance(ob, *host.compose(host.compose(I4, host.translate(where[k, j])), host.scale(scl[k, j])))
            if k == 150:
                s.add_mesh(top[0][75:], top[1][:75], m)
    return capture


def scene_large_and_small(host):
    """a 5 000-triangle (jittered) grid object — treelets that span blocks and several emit levels — beside two 3-triangle objects, five instances in all"""
    rng = np.random.default_rng(7)
    Pg, ig = scenes.grid_mesh(50, z=0.0, size=1.0)
    Pg = (Pg + rng.uniform(-0.004, 0.004, Pg.shape)).astype(np.float32)      # (a regular grid makes hlbvh.rs assert in the reference itself)
    small = [_soup(rng, 3, np.zeros(3), 0.4, 0.3) for _ in range(2)]
    T = _transforms(host)

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        big = s.object_begin(); s.add_mesh(Pg, ig, m); s.object_end()
        a = s.object_begin(); s.add_mesh(*small[0], m); s.object_end()
        b = s.object_begin(); s.add_mesh(*small[1], m); s.object_end()
        s.add_instance(big, *T[0]); s.add_instance(a, *T[1]); s.add_instance(big, *T[2]); s.add_instance(b, *T[3]); s.add_instance(a, *T[2])
    return capture


def scene_equal_codes(host):
    """an object of 40 triangles that share one centroid (one triangle scaled about the centre of its bound): no code bit splits the range"""
    base = np.array([[-1, -1, -1], [1, 1, 1], [0.25, -0.5, 0.125]], np.float32)      # bound (-1 .. 1)^3, centroid 0
    P = np.concatenate([base * np.float32(0.1 + 0.02 * k) for k in range(40)]); idx = np.arange(120, dtype=np.uint32)
    T = _transforms(host)

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        ob = s.object_begin(); s.add_mesh(P, idx, m); s.object_end()
        s.add_instance(ob, *T[0]); s.add_instance(ob, *T[1])
        s.add_mesh(base * np.float32(0.3) + np.float32([0, 0, 2]), [0, 1, 2], m)
    return capture


def scene_no_interior_node(host, n_obj_tris):
    """test_instancing_gpu.test_forest_without_any_interior_node: ONE instance of a 1- or 3-triangle object and nothing else"""
    P1, _ = host.gen_random_tris(1, 21)
    P = np.concatenate([P1 + np.float32(1e-3 * k) for k in range(n_obj_tris)]); idx = np.arange(3 * n_obj_tris, dtype=np.uint32)
    T = _transforms(host)[0]

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        ob = s.object_begin(); s.add_mesh(P, idx, m); s.object_end()
        s.add_instance(ob, *T)
    return capture


def scene_projective_and_identity(host):
    """one instance with the identity (PH_INST_IDENTITY), one whose matrix has a last row other than (0, 0, 0, 1): its bound goes through transform_bounds' divide"""
    P, idx = host.gen_random_tris(120, 31)
    m = np.eye(4, dtype=np.float64); m[:3, 3] = [1.5, -0.5, 0.25]; m[0, 0] = 1.25; m[3] = [0.03, -0.02, 0.01, 1.2]
    proj = (m.astype(np.float32).reshape(16), np.linalg.inv(m).astype(np.float32).reshape(16))

    def capture(s):
        mat = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        ob = s.object_begin(); s.add_mesh(P, idx, mat); s.object_end()
        s.add_instance(ob, *I4); s.add_instance(ob, *proj)
        s.add_mesh(P[:9] + np.float32([0, 0, 2.5]), np.arange(9, dtype=np.uint32), mat)
    return capture


SCENES = {
    "grid object instances": lambda h: scene_grid_object_instances(h),
    "one object x 9": lambda h: scene_one_object(h, 9),
    "one instance of one object": lambda h: scene_one_object(h, 1),
    "300 small objects": scene_many_small_objects,
    "large beside small": scene_large_and_small,
    "equal codes": scene_equal_codes,
    "no interior node, 1": lambda h: scene_no_interior_node(h, 1),
    "no interior node, 3": lambda h: scene_no_interior_node(h, 3),
    "projective and identity": scene_projective_and_identity,
}


def _stats(s):
    st = s.accel_stats(); st.pop("build_seconds"); return st


def assert_same_arrays(dev, hst):
    (dn, dr), (hn, hr) = dev.accel_copy(), hst.accel_copy()
    assert dn.shape == hn.shape and dr.shape == hr.shape
    assert np.array_equal(dn[:, 12:16], hn[:, 12:16]), f"child references / axes differ at nodes {np.flatnonzero((dn[:, 12:16] != hn[:, 12:16]).any(axis=1))[:5]}"
    # the planes bit for bit, but for the sign of a zero: the one thing the ordered-integer atomic min / max of the tree bounds does not keep as the host's sequential min / max does
    same = (dn[:, :12] == hn[:, :12]) | (((dn[:, :12] | hn[:, :12]) & 0x7FFFFFFF) == 0)
    assert same.all(), f"child boxes differ at nodes {np.flatnonzero(~same.all(axis=1))[:5]}"
    assert np.array_equal(dr, hr), f"leaf records differ at {np.flatnonzero((dr != hr).any(axis=1))[:5]}"
    assert _stats(dev) == _stats(hst)
    assert np.array_equal(dev.world_bound(), hst.world_bound())


def _try_build(s, fn, *args):
    try:
        fn(*args)
        return 0
    except pbrt_hip.PbrtHipError as e:
        return e.code


@pytest.mark.parametrize("max_prims", [1, 4])
@pytest.mark.parametrize("name", list(SCENES))
def test_device_forest_equals_host_forest_and_oracle(host, name, max_prims):
    capture = SCENES[name](host)
    dev, hst, orc = pbrt_hip.Scene(), pbrt_hip.Scene(), OracleScene()
    for s in (dev, hst, orc):
        capture(s)
    hrc = _try_build(hst, hst.build_accel, 1, max_prims)
    drc = _try_build(dev, dev.build_accel_device, 1, max_prims)
    assert drc == hrc, (drc, hrc, dev.b.fn("last_error")(dev.h))
    if hrc != 0:     # the reference's assertions (hlbvh.rs:338 / 356 / 418): both builders refuse the input with the same code
        assert hrc == pbrt_hip.ERR_INVALID_ARG and name == "equal codes"
        return
    orc.build_accel(1, max_prims)
    assert_same_arrays(dev, hst)
    rays = np.concatenate([scenes.random_rays(4000, 3, bound=3.5), scenes.axis_rays()])
    want, wst = orc.intersect_batch_stats(rays); wocc, wost = orc.occluded_batch_stats(rays)

    def traced(s):
        s.set_traversal_counting(True); s.traversal_counts()
        hits = s.intersect_batch(rays); cnt_c = s.traversal_counts()
        occ = s.occluded_batch(rays); cnt_a = s.traversal_counts()
        s.set_traversal_counting(False)
        return hits, occ, cnt_c, cnt_a
    got, gocc, cnt_c, cnt_a = traced(dev)
    _, _, hcnt_c, hcnt_a = traced(hst)
    eq = scenes.hits_equal(got, want)
    assert eq.all(), f"{(~eq).sum()} of {len(rays)} differ; first {np.flatnonzero(~eq)[:5]}"
    assert np.array_equal(gocc, wocc)
    # Counters.  Every tally of the device-built handle is the host-built handle's.  Against the oracle: rays and primitive tests equal; node visits with the relation of
    # test_render_gpu.py::test_traversal_work_counters_equal_the_oracles for instanced scenes — the oracle also counts the roots of the objects' own BVHs, the device's tally leaves
    # instance roots out, under either builder (270 719 against 273 511 on the first scene here, host-built and device-built alike).
    assert (cnt_c, cnt_a) == (hcnt_c, hcnt_a)
    assert (cnt_c["closest"]["rays"], cnt_c["closest"]["tri_tests"]) == (wst.rays, wst.tri_tests)
    assert (cnt_a["any_hit"]["rays"], cnt_a["any_hit"]["tri_tests"]) == (wost.rays, wost.tri_tests)
    low = 1 if dev.accel_stats()["interior_nodes"] else 0      # (a forest without any interior node has no node to pass)
    assert low <= cnt_c["closest"]["ref_node_visits"] <= wst.nodes_visited and low <= cnt_a["any_hit"]["ref_node_visits"] <= wost.nodes_visited
    assert np.array_equal(dev.world_bound(), orc.world_bound())
    dev.close(); hst.close(); orc.close()


@pytest.mark.parametrize("which", ["grid object instances", "one object x 9"])
def test_instanced_film_of_the_device_built_forest_bit_exact(host, which):
    """16 x 16 at 4 spp, path depth 3, the forest built on the device with HLBVH: film, weights and ray counters of the oracle (libm mode 1); both scene builders of case 1"""
    base = scene_grid_object_instances(host, with_normals=True) if which == "grid object instances" else scene_one_object(host, 9)

    def cap(s):
        s.add_light_infinite((0.5, 0.6, 0.7))
        s.add_light_point((30, 28, 25), (0.5, -1.0, 2.5))
        base(s)
        w2c, c2w = host.look_at([0.5, -7.5, 2.0], [0, 0, 0.5], [0, 0, 1])
        s.set_camera_perspective(host.perspective_raster_to_camera(50.0, 16, 16), c2w)
        cb, table, sb = host.film_box(16, 16)
        s.set_film(16, 16, cb, (0.5, 0.5), table)
        s.set_sampler(0, 4, sb)
    prod = pbrt_hip.Scene(); orc = OracleScene()
    cap(prod); cap(orc)
    prod.build_accel_device(1, 4); orc.build_accel(1, 4)
    set_libm_mode(1)
    try:
        oxyz, owt, ost, _ = orc.render_path_ex(max_depth=3)
    finally:
        set_libm_mode(0)
    gxyz, gwt, gst = prod.render_path(max_depth=3)
    assert (gst.regular_rays, gst.shadow_rays) == (ost.regular_rays, ost.shadow_rays)
    assert np.array_equal(gwt.view(np.uint32), owt.view(np.uint32))
    nb = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    assert nb == 0, f"{nb} pixels differ"
    assert float(oxyz.max()) > 0
    prod.close(); orc.close()


def test_build_accel_best_takes_the_device_path_and_rebuilds_leave_nothing_behind(host):
    """build_accel_best(1, 4) on an instanced scene builds on the device — seen here by watching the handle's own build_accel_device and build_accel: the first is called and
    returns, the second is not called — and gives the host forest's arrays.  SAH -> HLBVH -> SAH on one handle gives each time the tree of a fresh handle: an SAH device build leaves
    its forest on the device, the HLBVH build that follows must not find it there, nor the other way round."""
    capture = scene_grid_object_instances(host)
    best, hst = pbrt_hip.Scene(), pbrt_hip.Scene()
    capture(best); capture(hst)
    calls = []
    dev_build, host_build = best.build_accel_device, best.build_accel
    best.build_accel_device = lambda *a: (calls.append(("device",) + a), dev_build(*a))[1]
    best.build_accel = lambda *a: (calls.append(("host",) + a), host_build(*a))[1]
    best.build_accel_best(1, 4); hst.build_accel(1, 4)
    del best.build_accel_device, best.build_accel
    assert calls == [("device", 1, 4)], calls
    assert_same_arrays(best, hst)
    rays = np.concatenate([scenes.random_rays(3000, 9, bound=3.5), scenes.axis_rays()])
    one = pbrt_hip.Scene(); capture(one)
    for split in (0, 1, 0):
        one.build_accel_device(split, 4)
        fresh = pbrt_hip.Scene(); capture(fresh); fresh.build_accel(split, 4)
        assert_same_arrays(one, fresh)
        assert scenes.hits_equal(one.intersect_batch(rays), fresh.intersect_batch(rays)).all()      # (uploads the tree: the next build starts from an uploaded handle)
        fresh.close()
    best.close(); hst.close(); one.close()


def test_refusals_that_stay(host):
    capture = scene_grid_object_instances(host)
    s = pbrt_hip.Scene(); capture(s)
    for split in (3, 2):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.build_accel_device(split, 4)          # EqualCounts stays a host build, Middle is not offered
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
    s.build_accel_device(1, 4)                      # ... and the handle still builds and traces
    orc = OracleScene(); capture(orc); orc.build_accel(1, 4)
    rays = scenes.random_rays(3000, 4, bound=3.5)
    assert scenes.hits_equal(s.intersect_batch(rays), orc.intersect_batch_stats(rays)[0]).all()
    s.close(); orc.close()
