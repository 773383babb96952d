"""-m gpu: the SAH tree of a scene with quadric shapes built on the device (csrc/bvh_sah_device.hip with csrc/bvh_sah_steps.h: init_elem and emit_tri take a quadric as a third kind
of item) through pbrt_hip_build_accel_device_shapes, against the host builder with split method 0 — node array and leaf records entry by entry, statistics, world bound, every
traversal tally — and against the oracle built with build_accel(0, ..): world bound, closest hits, occlusion, two films.  The scenes are those of tests/hlbvh_quadric_scenes.py;
tests/test_sah_quadric_steps_cpu.py pins the host SAH builder to the oracle's tree on the flat ones, rehearses the step functions on the CPU and says which branch of k_init each
scene takes.  Under SAH the reference asserts on no scene: none is refused.  Oracle comparisons run in libm mode 1."""
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
from test_hlbvh_quadrics_cpu import fuzz_cases
from test_hlbvh_quadrics_device_gpu import _stage_16, _traced, _try_build
from test_quadric_instances_gpu import assert_films_equal, assert_hits_equal

pytestmark = pytest.mark.gpu
SCENES = HQ.all_scenes()
PH_TRI_QUADRIC = 128


def device_against_host_and_oracle(capture, max_prims, rays, what):
    """-> the common return code of the three builders; on 0 every comparison of this file's docstring has been made"""
    dev, hst, orc = pbrt_hip.Scene(), pbrt_hip.Scene(), OracleScene()
    try:
        capture(dev); capture(hst)
        with libm1():
            capture(orc)
        hrc = _try_build(hst.build_accel, 0, max_prims)
        drc = _try_build(dev.build_accel_device_shapes, 0, max_prims)
        orc_rc = _try_build(orc.build_accel, 0, max_prims)
        assert drc == hrc == orc_rc, (what, drc, hrc, orc_rc, dev.b.fn("last_error")(dev.h))
        if hrc != 0:
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
def test_device_sah_of_a_quadric_scene_equals_host_sah_and_oracle(host, name, max_prims):
    rays = np.concatenate([scenes.random_rays(4000, 3, bound=HQ.RAY_BOUND.get(name, 1.2)), scenes.axis_rays()])
    assert device_against_host_and_oracle(SCENES[name](host), max_prims, rays, f"{name}, max_prims {max_prims}") == 0


# ---- 2. fuzz -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(12))
def test_fuzz_device_sah_equals_host_sah_and_oracle(host, k):
    name, capture, max_prims = fuzz_cases(host)[k]
    rays = np.concatenate([scenes.random_rays(4000, 100 + k, bound=2.0), scenes.axis_rays()])
    assert device_against_host_and_oracle(capture, max_prims, rays, name) == 0, name


# ---- 3. films ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _film_pair(host, **kw):
    cap = _stage_16(host, **kw)
    prod, orc = pbrt_hip.Scene(), OracleScene()
    cap(prod)
    with libm1():
        cap(orc)
    prod.build_accel_device_shapes(0, 4); orc.build_accel(0, 4)
    return prod, orc


def test_path_film_of_the_device_built_tree_bit_exact(host):
    """16 x 16 at 4 spp, path depth 3, the staged instanced scene: film, weights and counters of the oracle built with build_accel(0, 4)"""
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


# ---- 4. plumbing ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_old_entry_still_refuses_and_the_new_one_then_builds(host):
    rays = np.concatenate([scenes.random_rays(3000, 4, bound=3.5), scenes.axis_rays()])
    with pbrt_hip.Scene() as s, OracleScene() as orc:
        QI.stage(s, host, split=1, build=False)
        with libm1():
            QI.stage(orc, host, split=1, build=False)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.build_accel_device(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
        s.build_accel_device_shapes(0, 4)
        orc.build_accel(0, 4)
        with libm1():
            want = orc.intersect_batch(rays)
        assert_hits_equal(s.intersect_batch(rays), want, "after the refusal")
        with pytest.raises(pbrt_hip.PbrtHipError) as e:      # what pbrt_hip_build_accel_device refuses for every scene, the new entry refuses too
            s.build_accel_device_shapes(3, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
        s.build_accel_device_shapes(1, 4)                    # split method 1 as before
        with pbrt_hip.Scene() as h:
            QI.stage(h, host, split=1, build=False); h.build_accel(1, 4)
            assert_same_arrays(s, h)
    # the leftover refusal: a quadric beside object definitions of which none is instanced
    tri = (np.array([[-1, -1, 3], [1, -1, 3], [0, 1, 3]], np.float32), np.array([0, 2, 1], np.uint32))
    with pbrt_hip.Scene() as t:
        m = t.add_material_matte((0.5, 0.5, 0.5))
        ob = t.object_begin(); t.add_mesh(*tri, m); t.object_end()
        t.add_sphere(*QI.cf_ctm(host, host.translate((0.0, 0.0, -1.0))), 0.5, None, None, 360.0, m, False)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            t.build_accel_device_shapes(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object" in str(e.value)
        t.add_instance(ob, *QI.I4)              # ... which an instance of the object lifts
        t.build_accel_device_shapes(0, 4)
        assert (t.intersect_batch(scenes.random_rays(2000, 2, bound=1.5))["prim"] != QI.MISS).sum() > 100


def _watched(scene):
    calls = []
    for label, name in (("device", "build_accel_device"), ("shapes", "build_accel_device_shapes"), ("host", "build_accel")):
        fn = getattr(scene, name)
        setattr(scene, name, lambda *a, fn=fn, label=label: (calls.append((label,) + a), fn(*a))[1])
    return calls


def test_build_accel_best_takes_the_device_path_on_a_quadric_scene(host):
    """build_accel_best(0, 4) calls the handle's build_accel_device, which refuses, then build_accel_device_shapes, which returns, and never build_accel; the arrays are the host
    builder's.  On a triangle-only scene it calls build_accel_device alone."""
    for name in ("stage", "meshes around quadrics"):
        capture = SCENES[name](host)
        best, hst = pbrt_hip.Scene(), pbrt_hip.Scene()
        capture(best); capture(hst)
        calls = _watched(best)
        best.build_accel_best(0, 4); hst.build_accel(0, 4)
        del best.build_accel_device, best.build_accel_device_shapes, best.build_accel
        assert calls == [("device", 0, 4), ("shapes", 0, 4)], (name, calls)
        assert_same_arrays(best, hst)
        best.close(); hst.close()
    P, idx = host.gen_random_tris(200, 5)
    with pbrt_hip.Scene() as tri:
        tri.add_mesh(P, idx, tri.add_material_matte((0.5, 0.5, 0.5), 0.0))
        calls = _watched(tri)
        tri.build_accel_best(0, 4)
        del tri.build_accel_device, tri.build_accel_device_shapes, tri.build_accel
        assert calls == [("device", 0, 4)], calls


@pytest.mark.parametrize("name", ["stage", "meshes around quadrics"])
def test_rebuilds_on_one_handle_give_the_fresh_handles_arrays(host, name):
    """host HLBVH, device SAH, host SAH, device SAH on one handle, each traced (uploaded) before the next: every time the arrays and hits of a fresh handle built on the host"""
    capture = SCENES[name](host)
    rays = np.concatenate([scenes.random_rays(3000, 9, bound=HQ.RAY_BOUND.get(name, 1.2)), scenes.axis_rays()])
    one = pbrt_hip.Scene(); capture(one)
    for where, split in (("host", 1), ("device", 0), ("host", 0), ("device", 0)):
        (one.build_accel_device_shapes if where == "device" else one.build_accel)(split, 4)
        fresh = pbrt_hip.Scene(); capture(fresh); fresh.build_accel(split, 4)
        assert_same_arrays(one, fresh)
        assert_hits_equal(one.intersect_batch(rays), fresh.intersect_batch(rays), f"{where} {split}")
        assert_same_arrays(one, fresh)      # (after the upload has patched the instance records in place)
        fresh.close()
    one.close()


# ---- 5. a multi-device handle ----------------------------------------------------------------------------------------------------------------------------------------------
def test_multi_device_handle_builds_on_the_device_and_gives_the_single_device_film(host):
    cap = _stage_16(host)
    with pbrt_hip.Scene() as one, pbrt_hip.Scene(devices=[0, 0]) as multi:
        cap(one); cap(multi)
        one.build_accel_device_shapes(0, 4); multi.build_accel_device_shapes(0, 4)
        assert_same_arrays(multi, one)
        assert_films_equal(multi.render_path(max_depth=3), one.render_path(max_depth=3), "two shares of one device")
