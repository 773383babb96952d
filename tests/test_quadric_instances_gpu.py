"""-m gpu: quadric shapes in one scene with object instances — the traversal kernel's rows (inst, quadric, alpha 0 / 1 / 2) and their counting rows, through every entry point: ray
batches (host and device forms), the path integrator (two light strategies, both samplers, tile parts, device tile buffers, a sample-record budget, a multi-device handle), the
Whitted integrator with a spherical area light, the work counters, build_accel_best, and what stays refused.  Every comparison is against the CPU oracle in libm mode 1 and on bits.
The scenes are those of tests/quadric_instance_scenes.py; tests/test_quadric_instances_oracle.py shows on the CPU that the rays reach every kind of item in them, that a SAH leaf
holds a quadric between two instances and that the quadrics are not inert in the film."""
import numpy as np
import pytest
import torch   # device buffers for the *_device entry points.  At module level: first imported inside a test, after the library had run kernels in the process, torch found no device

import pbrt_hip
import quadric_instance_scenes as QI
import scenes
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1
from sphere_light_scenes import oracle_whitted

pytestmark = pytest.mark.gpu
COUNTERS = ("camera_rays", "regular_rays", "shadow_rays", "paths_total", "paths_zero_radiance", "light_distributions_created")


def pair(host, build, **kw):
    """build(scene, host, **kw) on a device scene and, in libm mode 1, on an oracle scene -> (prod, orc, what build returned)"""
    prod = pbrt_hip.Scene(); orc = OracleScene()
    info = build(prod, host, **kw)
    with libm1():
        build(orc, host, **kw)
    return prod, orc, info


def assert_hits_equal(got, want, what):
    bad = ~scenes.hits_equal(got, want)
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:5], got[bad][:3], want[bad][:3])


def assert_films_equal(got, want, what="", counters=COUNTERS):
    gxyz, gwt, gst = got[:3]; oxyz, owt, ost = want[:3]
    assert np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)), what
    nd = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    assert nd == 0, (what, nd, float(np.abs(gxyz - oxyz).max()))
    for f in counters:
        assert getattr(gst, f) == getattr(ost, f), (what, f, getattr(gst, f), getattr(ost, f))


# ---- 1. hits and occlusion, per split and per alpha row, timed and counting -----------------------------------------------------------------------------------------
BATCH_CASES = [(split, mask) for split in (0, 3) for mask in QI.MASKS] + [(1, None)]   # the HLBVH leg carries no mask: the reference's build asserts on the regular grid that carries it


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
@pytest.mark.parametrize("split,mask", BATCH_CASES, ids=[f"split{c[0]}-{c[1] or 'nomask'}" for c in BATCH_CASES])
def test_stage_batches(host, split, mask, counting):
    prod, orc, prims = pair(host, QI.stage, split=split, mask=mask)
    rays = QI.stage_rays()
    with libm1():
        want, wst = orc.intersect_batch_stats(rays); wocc, wost = orc.occluded_batch_stats(rays)
    quadrics, tris, per_inst, _ = QI.tally(want, prims)
    assert min(quadrics.values()) >= 200 and (per_inst >= 1000).sum() >= 4 and tris >= 1000, (quadrics, tris, per_inst)
    if counting:
        prod.set_traversal_counting(True)
        prod.traversal_counts()
    got = prod.intersect_batch(rays); cnt_c = prod.traversal_counts() if counting else None
    gocc = prod.occluded_batch(rays); cnt_a = prod.traversal_counts() if counting else None
    what = f"split {split} mask {mask} counting {counting}"
    assert_hits_equal(got, want, what)
    assert np.array_equal(gocc, wocc), (what, int((gocc != wocc).sum()))
    assert np.array_equal(prod.world_bound(), orc.world_bound())
    if counting:
        prod.set_traversal_counting(False)
        # rays and primitive tests are the reference's; its node tally also counts the roots of the objects' own aggregates, which the device's leaves out (tests/test_render_gpu.py)
        assert (cnt_c["closest"]["rays"], cnt_c["closest"]["tri_tests"]) == (wst.rays, wst.tri_tests), (what, cnt_c, wst.tri_tests)
        assert (cnt_a["any_hit"]["rays"], cnt_a["any_hit"]["tri_tests"]) == (wost.rays, wost.tri_tests), (what, cnt_a, wost.tri_tests)
        assert 0 < cnt_c["closest"]["ref_node_visits"] <= wst.nodes_visited and 0 < cnt_a["any_hit"]["ref_node_visits"] <= wost.nodes_visited
        assert wst.tri_tests > len(rays) // 2
        assert_hits_equal(prod.intersect_batch(rays), want, what + ", timed row after counting")
    else:
        # the device forms: rays and results stay in device memory
        sub = rays[::7]
        d_rays = torch.from_numpy(np.ascontiguousarray(sub).view(np.uint8).copy()).cuda()
        d_hits = torch.zeros(len(sub) * pbrt_hip.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        prod.intersect_batch_device(d_rays.data_ptr(), d_hits.data_ptr(), len(sub))
        d_occ = torch.full((len(sub),), 7, dtype=torch.uint8, device="cuda")
        prod.occluded_batch_device(d_rays.data_ptr(), d_occ.data_ptr(), len(sub))
        torch.cuda.synchronize()
        assert_hits_equal(d_hits.cpu().numpy().view(pbrt_hip.HIT_DTYPE), want[::7], what + " device form")
        assert np.array_equal(d_occ.cpu().numpy(), wocc[::7]), what + " device form, occlusion"
    prod.close(); orc.close()


# ---- 2. one leaf holds everything -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instance_first", [False, True], ids=["triangle-first", "instance-first"])
def test_one_leaf_holds_a_triangle_two_quadrics_and_two_instances(host, instance_first):
    prod, orc, prims = pair(host, QI.one_leaf, instance_first=instance_first)
    assert len(orc.bvh_nodes()) == 1     # the scene-level root is a leaf: no leaf reference, no hint
    rays = QI.one_leaf_rays()
    with libm1():
        want = orc.intersect_batch(rays); wocc = orc.occluded_batch(rays)
    what = f"one leaf, instance_first {instance_first}"
    assert_hits_equal(prod.intersect_batch(rays), want, what)
    assert np.array_equal(prod.occluded_batch(rays), wocc), what
    hit = want["prim"] != QI.MISS; inst = want["pad"][:, 1]
    on_quadric = hit & (inst == 0) & (QI.in_range(want["prim"], prims["sphere"]) | QI.in_range(want["prim"], prims["cylinder"]))
    assert on_quadric.sum() >= 500 and (hit & (inst == 1)).sum() >= 200 and (hit & (inst == 2)).sum() >= 200, what
    # after the upload has filled the instance records in place, accel_copy still hands out the builder's form
    nodes, recs = prod.accel_copy()     # TriRec words: p0[3], prim, p1[3], flags, p2[3], mesh
    top = recs[:QI.ONE_LEAF_ITEMS]; flags = top[:, 7]
    assert not (recs[:, 7] & 64).any()                                                           # PH_TRI_NEXT_INST
    is_inst = (flags & 16) != 0; is_quad = (flags & 128) != 0                                  # PH_TRI_INSTANCE, PH_TRI_QUADRIC
    expect = ["i", "q", "i", "q", "t"] if instance_first else ["t", "q", "i", "q", "i"]
    assert ["i" if a else "q" if b else "t" for a, b in zip(is_inst, is_quad)] == expect
    assert not top[is_inst][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].any() and list(top[is_inst][:, 3]) == [0, 1]
    # quadric records: the table index in p0[0] (the quadrics' call order), the primitive slot in `prim`
    names = ["cylinder", "sphere"] if instance_first else ["sphere", "cylinder"]
    assert list(top[is_quad][:, 0]) == [0, 1] and list(top[is_quad][:, 3]) == [prims[k][0] for k in names]
    assert (flags[-1] & 1) and not (flags[:-1] & 1).any()                                        # PH_TRI_LAST: one leaf
    assert not (recs[QI.ONE_LEAF_ITEMS:, 7] & (16 | 128)).any()                                  # the object's tree holds triangles only
    prod.close(); orc.close()


# ---- 3. path films --------------------------------------------------------------------------------------------------------------------------------------------------
PATH_CASES = [dict(light_strategy=0), dict(light_strategy=2), dict(light_strategy=2, sampler="sobol"), dict(light_strategy=2, mask="imagemap"), dict(light_strategy=2, fancy=True)]


@pytest.mark.parametrize("case", PATH_CASES, ids=["uniform", "spatial", "sobol", "imagemap-mask", "plastic-glass-bump"])
def test_path_films(host, case):
    kw = dict(case); strategy = kw.pop("light_strategy")
    prod, orc, _ = pair(host, QI.stage, **kw)
    with libm1():
        want = orc.render_path_ex(max_depth=4, light_strategy=strategy)
    got = prod.render_path(max_depth=4, light_strategy=strategy)
    assert_films_equal(got, want, str(case))
    assert float(want[0].max()) > 0 and got[2].shadow_rays > 0 and got[2].regular_rays > got[2].camera_rays
    prod.close(); orc.close()


# ---- 4. Whitted films -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [None, "checkerboard"], ids=["nomask", "checkerboard"])
def test_whitted_films_with_a_sphere_light(host, mask):
    prod, orc, _ = pair(host, QI.stage, mask=mask, whitted=True, sphere_light=True)
    want = oracle_whitted(orc, max_depth=4)
    got = prod.render_whitted(max_depth=4)
    assert_films_equal(got, want, f"whitted {mask}", counters=("camera_rays", "regular_rays", "shadow_rays"))
    assert got[2].shadow_rays > 0 and got[2].regular_rays > got[2].camera_rays and float(want[0].max()) > 0
    prod.close(); orc.close()


# ---- 5. plumbing ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_build_accel_best_ends_on_the_host_builders(host):
    prod, orc, _ = pair(host, QI.stage)
    rays = QI.stage_rays()[::3]
    with libm1():
        want = orc.intersect_batch(rays)
    with pbrt_hip.Scene() as best:
        QI.stage(best, host, build=False)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:      # what build_accel_best tries first
            best.build_accel_device(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
        best.build_accel_best(0, 4)
        assert_hits_equal(best.intersect_batch(rays), want, "build_accel_best")
        for a, b in zip(best.accel_copy(), prod.accel_copy()):   # the host builders' forest, as build_accel makes it
            assert np.array_equal(a, b)
    prod.close(); orc.close()


def test_sample_record_budget_tile_parts_and_device_tiles(host):
    prod, orc, _ = pair(host, QI.stage)
    kw = dict(max_depth=4, light_strategy=2)
    with libm1():
        want = orc.render_path_ex(**kw)
    one = prod.render_path(**kw)
    assert_films_equal(one, want, "one band")
    prod.set_sample_record_budget(2 * 256 * QI.SPP * 20)       # two whole 16 x 16 tiles' sample records (20 bytes each): the 3 x 3 tiles render in several bands
    banded = prod.render_path(**kw)
    assert prod.render_footprint()["bands"] > 1
    prod.set_sample_record_budget(0)
    assert_films_equal(banded, want, "banded")
    bufs = []
    for part in range(2):
        with libm1():
            ox, ow, _, _ = orc.render_path_ex(tile_part=part, tile_parts=2, **kw)
        px, pw, _ = prod.render_path(tile_part=part, tile_parts=2, **kw)
        assert np.array_equal(px.view(np.uint32), ox.view(np.uint32)) and np.array_equal(pw, ow), part
        buf = torch.full((prod.tile_buffer_floats(16, part, 2),), float("nan"), dtype=torch.float32, device="cuda")
        prod.render_path_tiles_device(buf.data_ptr(), tile_part=part, tile_parts=2, **kw)
        bufs.append(buf)
    mx, mw = prod.merge_tiles_device([b.data_ptr() for b in bufs])
    assert np.array_equal(mw.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(mx.view(np.uint32), want[0].view(np.uint32))
    prod.close(); orc.close()


def test_multi_device_film_equals_the_oracles(host):
    with pbrt_hip.Scene(devices=[0, 0]) as multi, OracleScene() as orc:
        QI.stage(multi, host)
        with libm1():
            QI.stage(orc, host)
            want = orc.render_path_ex(max_depth=4)
        assert_films_equal(multi.render_path(max_depth=4), want, "two shares of one device")


# ---- 6. what stays refused ------------------------------------------------------------------------------------------------------------------------------------------
def _usable(s, host):
    """the handle still builds a valid scene and traces it"""
    s.build_accel(0, 4)
    rays = QI.stage_rays()[:2000]
    assert (s.intersect_batch(rays)["prim"] != QI.MISS).sum() > 100


def test_refusals_leave_the_handle_usable(host):
    tri = (np.array([[-1, -1, 3], [1, -1, 3], [0, 1, 3]], np.float32), np.array([0, 2, 1], np.uint32))

    def sphere_and_definition(t):
        m = t.add_material_matte((0.5, 0.5, 0.5))
        ob = t.object_begin(); t.add_mesh(*tri, m); t.object_end()
        t.add_sphere(*QI.cf_ctm(host, host.translate((0.0, 0.0, -1.0))), 0.5, None, None, 360.0, m, False)
        return ob
    # a quadric and an object definition that no instance uses: the leftover refusal ...
    with pbrt_hip.Scene() as t, OracleScene() as orc:
        ob = sphere_and_definition(t)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            t.build_accel(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object" in str(e.value)
        t.add_instance(ob, *QI.I4)          # ... which an instance of the object lifts
        t.build_accel(0, 4)
        rays = scenes.random_rays(2000, 2, bound=1.5)
        with libm1():
            orc.add_instance(sphere_and_definition(orc), *QI.I4)
            orc.build_accel(0, 4)
            want = orc.intersect_batch(rays)
        assert (want["prim"] != QI.MISS).sum() > 100
        assert_hits_equal(t.intersect_batch(rays), want, "after the leftover refusal")
    with pbrt_hip.Scene() as s:
        QI.stage(s, host, build=False)
        # a quadric inside a definition (the definition itself stays, unused: allowed beside instances)
        s.object_begin()
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.add_sphere(*QI.cf_ctm(host, host.translate((0.0, 0.0, 5.0))), 0.5, None, None, 360.0, 0, False)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object definition" in str(e.value)
        s.add_mesh(*tri, 0)
        s.object_end()
        # the device builders on the stage
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.build_accel_device(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
        _usable(s, host)
    # the path integrator on the stage with the sphere light
    with pbrt_hip.Scene() as s:
        QI.stage(s, host, whitted=True, sphere_light=True)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.render_path(max_depth=3)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
        _usable(s, host)
        assert float(s.render_whitted(max_depth=2)[0].max()) > 0
