"""-m gpu: the HLBVH tree of a scene with quadric shapes built on the device (csrc/bvh_device.hip: f_bounds_kernel and f_gather_kernel take a quadric as a third kind of item)
against the host builder with split method 1 — node array and leaf records entry by entry, statistics, world bound, every traversal tally — and against the oracle: world bound,
closest hits, occlusion, two films.  The scenes are those of tests/hlbvh_quadric_scenes.py; tests/test_hlbvh_quadrics_cpu.py pins the host builder to the oracle's tree on the flat
ones and counts the scenes on which the reference's HLBVH assertions fire (none of the edge scenes, two of the twelve fuzz seeds).  Oracle comparisons run in libm mode 1."""
import numpy as np
import pytest

import pbrt_hip
import hlbvh_quadric_scenes as HQ
import quadric_instance_scenes as QI
import scenes
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1
from sphere_light_scenes import oracle_whitted
from test_hlbvh_forest_device_gpu import assert_same_arrays
from test_hlbvh_quadrics_cpu import FUZZ_REFUSED, fuzz_cases
from test_quadric_instances_gpu import assert_films_equal, assert_hits_equal

pytestmark = pytest.mark.gpu
SCENES = HQ.all_scenes()
PH_TRI_QUADRIC = 128


def _try_build(fn, *args):
    try:
        fn(*args)
        return 0
    except pbrt_hip.PbrtHipError as e:
        return e.code


def _traced(s, rays):
    s.set_traversal_counting(True); s.traversal_counts()
    hits = s.intersect_batch(rays); cnt_c = s.traversal_counts()
    occ = s.occluded_batch(rays); cnt_a = s.traversal_counts()
    s.set_traversal_counting(False)
    return hits, occ, cnt_c, cnt_a


def device_against_host_and_oracle(capture, max_prims, rays, what):
    """-> the common return code of the two builders; on 0 every comparison of this file's docstring has been made"""
    dev, hst, orc = pbrt_hip.Scene(), pbrt_hip.Scene(), OracleScene()
    try:
        capture(dev); capture(hst)
        with libm1():
            capture(orc)
        hrc = _try_build(hst.build_accel, 1, max_prims)
        drc = _try_build(dev.build_accel_device, 1, max_prims)
        orc_rc = _try_build(orc.build_accel, 1, max_prims)
        assert drc == hrc == orc_rc, (what, drc, hrc, orc_rc, dev.b.fn("last_error")(dev.h))
        if hrc != 0:      # the reference's assertions (hlbvh.rs:338 / 356 / 418): every side refuses the input with the same code
            assert hrc == pbrt_hip.ERR_INVALID_ARG, what
            return hrc
        assert_same_arrays(dev, hst)
        assert (dev.accel_copy()[1][:, 7] & PH_TRI_QUADRIC).any(), what       # (the scene does hold a quadric)
        assert np.array_equal(dev.world_bound(), orc.world_bound()), what
        with libm1():
            want = orc.intersect_batch(rays); wocc = orc.occluded_batch(rays)
        got, gocc, cnt_c, cnt_a = _traced(dev, rays)
        _, _, hcnt_c, hcnt_a = _traced(hst, rays)
        assert_hits_equal(got, want, what)
        assert np.array_equal(gocc, wocc), (what, int((gocc != wocc).sum()))
        assert (cnt_c, cnt_a) == (hcnt_c, hcnt_a), what
        assert cnt_c["closest"]["rays"] > 0 and cnt_a["any_hit"]["rays"] > 0, what      # (counting was on)
        return 0
    finally:
        dev.close(); hst.close(); orc.close()


# ---- 1. the smallest scenes at which the new code can go wrong --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_prims", [1, 4])
@pytest.mark.parametrize("name", list(SCENES))
def test_device_hlbvh_of_a_quadric_scene_equals_host_hlbvh_and_oracle(host, name, max_prims):
    rays = np.concatenate([scenes.random_rays(4000, 3, bound=HQ.RAY_BOUND.get(name, 1.2)), scenes.axis_rays()])
    rc = device_against_host_and_oracle(SCENES[name](host), max_prims, rays, f"{name}, max_prims {max_prims}")
    assert rc == 0      # tests/test_hlbvh_quadrics_cpu.py: the reference builds every one of these scenes


# ---- 2. films ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _stage_16(host, **kw):
    def cap(s):
        QI.stage(s, host, split=1, build=False, camera=False, **kw)
        w2c, c2w = host.look_at((0.5, -7.5, 2.0), (0, 0, 0.5), (0, 0, 1))
        s.set_camera_perspective(host.perspective_raster_to_camera(50.0, 16, 16), c2w)
        cb, table, sb = host.film_box(16, 16)
        s.set_film(16, 16, cb, (0.5, 0.5), table)
        s.set_sampler(0, 4, sb)
    return cap


def _film_pair(host, **kw):
    cap = _stage_16(host, **kw)
    prod, orc = pbrt_hip.Scene(), OracleScene()
    cap(prod)
    with libm1():
        cap(orc)
    prod.build_accel_device(1, 4); orc.build_accel(1, 4)
    return prod, orc


def test_path_film_of_the_device_built_tree_bit_exact(host):
    """16 x 16 at 4 spp, path depth 3, the staged instanced scene: film, weights and counters of the oracle built with build_accel(1, 4)"""
    prod, orc = _film_pair(host)
    with libm1():
        want = orc.render_path_ex(max_depth=3)
    assert_films_equal(prod.render_path(max_depth=3), want, "path")
    assert float(want[0].max()) > 0 and want[2].shadow_rays > 0
    prod.close(); orc.close()


def test_whitted_film_of_the_device_built_tree_bit_exact(host):
    prod, orc = _film_pair(host, whitted=True, sphere_light=True)
    want = oracle_whitted(orc, max_depth=3)
    assert_films_equal(prod.render_whitted(max_depth=3), want, "whitted", counters=("camera_rays", "regular_rays", "shadow_rays"))
    assert float(want[0].max()) > 0 and want[2].shadow_rays > 0
    prod.close(); orc.close()


def test_multi_device_handle_builds_on_the_device_and_gives_the_single_device_film(host):
    cap = _stage_16(host)
    with pbrt_hip.Scene() as one, pbrt_hip.Scene(devices=[0, 0]) as multi:
        cap(one); cap(multi)
        one.build_accel_device(1, 4); multi.build_accel_device(1, 4)
        assert_same_arrays(multi, one)
        assert_films_equal(multi.render_path(max_depth=3), one.render_path(max_depth=3), "two shares of one device")


# ---- 3. plumbing ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_build_accel_best_takes_the_device_path_on_a_quadric_scene(host):
    """build_accel_best(1, 4) calls the handle's build_accel_device, which returns, and not build_accel; the arrays are the host builder's"""
    for name in ("stage", "meshes around quadrics"):
        capture = SCENES[name](host)
        best, hst = pbrt_hip.Scene(), pbrt_hip.Scene()
        capture(best); capture(hst)
        calls = []
        dev_build, host_build = best.build_accel_device, best.build_accel
        best.build_accel_device = lambda *a: (calls.append(("device",) + a), dev_build(*a))[1]
        best.build_accel = lambda *a: (calls.append(("host",) + a), host_build(*a))[1]
        best.build_accel_best(1, 4); hst.build_accel(1, 4)
        del best.build_accel_device, best.build_accel
        assert calls == [("device", 1, 4)], (name, calls)
        assert_same_arrays(best, hst)
        best.close(); hst.close()


@pytest.mark.parametrize("name", ["stage", "meshes around quadrics"])
def test_rebuilds_on_one_handle_give_the_fresh_handles_arrays(host, name):
    """host SAH, device HLBVH, host SAH on one handle, each traced (uploaded) before the next: every time the arrays and hits of a fresh handle built the same way"""
    capture = SCENES[name](host)
    rays = np.concatenate([scenes.random_rays(3000, 9, bound=HQ.RAY_BOUND.get(name, 1.2)), scenes.axis_rays()])
    one = pbrt_hip.Scene(); capture(one)
    for where, split in (("host", 0), ("device", 1), ("host", 0)):
        (one.build_accel_device if where == "device" else one.build_accel)(split, 4)
        fresh = pbrt_hip.Scene(); capture(fresh); fresh.build_accel(split, 4)
        assert_same_arrays(one, fresh)
        assert_hits_equal(one.intersect_batch(rays), fresh.intersect_batch(rays), f"{where} {split}")
        fresh.close()
    one.close()


def test_refusals_on_one_handle(host):
    rays = np.concatenate([scenes.random_rays(3000, 4, bound=3.5), scenes.axis_rays()])
    with pbrt_hip.Scene() as s, OracleScene() as orc:
        QI.stage(s, host, split=1, build=False)
        with libm1():
            QI.stage(orc, host, split=1, build=False)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.build_accel_device(0, 4)          # the SAH device builder takes no quadric
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
        s.build_accel_device(1, 4)              # ... and the handle still builds on the device and traces
        orc.build_accel(1, 4)
        with libm1():
            want = orc.intersect_batch(rays)
        assert_hits_equal(s.intersect_batch(rays), want, "after the refusal")
    # the leftover refusal: a quadric beside object definitions of which none is instanced, from either builder
    tri = (np.array([[-1, -1, 3], [1, -1, 3], [0, 1, 3]], np.float32), np.array([0, 2, 1], np.uint32))
    with pbrt_hip.Scene() as t:
        m = t.add_material_matte((0.5, 0.5, 0.5))
        ob = t.object_begin(); t.add_mesh(*tri, m); t.object_end()
        t.add_sphere(*QI.cf_ctm(host, host.translate((0.0, 0.0, -1.0))), 0.5, None, None, 360.0, m, False)
        for build in (t.build_accel_device, t.build_accel):
            with pytest.raises(pbrt_hip.PbrtHipError) as e:
                build(1, 4)
            assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object" in str(e.value)
        t.add_instance(ob, *QI.I4)              # ... which an instance of the object lifts
        t.build_accel_device(1, 4)
        assert (t.intersect_batch(scenes.random_rays(2000, 2, bound=1.5))["prim"] != QI.MISS).sum() > 100


# ---- 4. fuzz -------------------------------------------------------------------------------------------------------------------------------------------------------------
# (the reference's HLBVH build asserts on FUZZ_REFUSED, two of the twelve — tests/test_hlbvh_quadrics_cpu.py: both builders must refuse them, and with the same code)
@pytest.mark.parametrize("k", range(12))
def test_fuzz_device_hlbvh_equals_host_hlbvh_and_oracle(host, k):
    name, capture, max_prims = fuzz_cases(host)[k]
    rays = np.concatenate([scenes.random_rays(4000, 100 + k, bound=2.0), scenes.axis_rays()])
    rc = device_against_host_and_oracle(capture, max_prims, rays, name)
    assert (rc != 0) == (name in FUZZ_REFUSED), (name, rc)
