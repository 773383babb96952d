"""-m gpu: where the built tree lives.  An SAH device build leaves its arrays on the device, every other build hands them to the host (csrc/scene_host.h: DeviceTree and the
accessors accel_on_device / accel_nodes / accel_records / fetch_leaf_records); a rebuild through another builder must leave nothing of the earlier tree behind, and no reader may
see the wrong one.  One handle per scene goes through

    device SAH by the shapes entry -> host SAH -> device HLBVH -> host EqualCounts -> device SAH

(the last through build_accel_device, or through the shapes entry where the scene holds a quadric, which build_accel_device refuses), and after every step its statistics, arrays,
world bound and closest hits are those of a fresh handle built by the same call, and its hits the oracle's.  After the last step the probe entry that reads the leaf records
(pbrt_hip_surface_probe_batch) answers as on the fresh handle.  A refused build_accel_device(3, 4) leaves no mark: the build_accel that follows is a fresh host build.

The scenes are the smallest that have both homes and every kind of leaf record: 17 random triangles and a sphere; one object of 3 triangles instanced twice and one top-level
triangle.  Rays: 2 000 random ones and the axis rays, origins in [-1, 1]^3 aimed into [-0.5, 0.5]^3, where the sphere (radius 0.8 about the origin) and the object's three large
triangles (one across each coordinate plane) stand: at least a fifth of them must hit, or equal answers would say little."""
import numpy as np
import pytest

import pbrt_hip
import scenes
from oracle_binding import OracleScene

pytestmark = pytest.mark.gpu
I4 = (np.eye(4, dtype=np.float32).reshape(16),) * 2
HOST, DEVICE, SHAPES = "build_accel", "build_accel_device", "build_accel_device_shapes"


def scene_triangles_and_sphere(host):
    P, idx = host.gen_random_tris(17, 3)

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        s.add_mesh(P, idx[:24], m)
        s.add_sphere(*I4, radius=0.8, material=m)
        s.add_mesh(P, idx[24:], m)
    return capture, (SHAPES, 0), 2


def scene_instanced_object(host):
    # one large triangle across each coordinate plane, none through the origin's neighbourhood edge-on
    P = np.array([[-1.5, -1.4, 0.05], [1.6, -1.2, -0.05], [0.1, 1.7, 0.02],
                  [0.04, -1.5, -1.3], [-0.03, 1.4, -1.5], [0.02, 0.2, 1.6],
                  [-1.4, 0.03, -1.5], [1.5, -0.04, -1.2], [0.1, 0.05, 1.7]], np.float32)
    top = np.array([[-0.9, -0.8, 0.6], [0.9, -0.7, 0.5], [0.0, 0.9, 0.7]], np.float32)
    T = host.compose(host.compose(I4, host.translate([0.2, -0.1, 0.15])), host.rotate(35, [0.3, 1, 0.2]))

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        ob = s.object_begin(); s.add_mesh(P, np.arange(9, dtype=np.uint32), m); s.object_end()
        s.add_instance(ob, *I4)
        s.add_mesh(top, [0, 1, 2], m)
        s.add_instance(ob, *T)
    return capture, (DEVICE, 0), 1


SCENES = {"17 triangles and a sphere": scene_triangles_and_sphere, "an object of 3 triangles twice, one triangle": scene_instanced_object}


def _rays():
    return np.concatenate([scenes.random_rays(2000, 17, bound=0.5), scenes.axis_rays()])


def _stats(s):
    st = s.accel_stats(); st.pop("build_seconds"); return st


def assert_same_tree(one, fresh, what):
    (an, ar), (bn, br) = one.accel_copy(), fresh.accel_copy()
    assert _stats(one) == _stats(fresh), what
    assert np.array_equal(an, bn) and np.array_equal(ar, br), what
    assert np.array_equal(one.world_bound().view(np.uint32), fresh.world_bound().view(np.uint32)), what


@pytest.mark.parametrize("name", list(SCENES))
def test_every_build_in_a_sequence_is_a_fresh_handles_build(host, name):
    capture, last_step, probe_variant = SCENES[name](host)
    rays = _rays()
    oracle_hits = {}
    for split in (0, 1, 3):
        orc = OracleScene(); capture(orc); orc.build_accel(split, 4)
        oracle_hits[split] = orc.intersect_batch_stats(rays)[0]
        orc.close()
    one = pbrt_hip.Scene(); capture(one)
    fresh = None
    for step, (entry, split) in enumerate([(SHAPES, 0), (HOST, 0), (DEVICE, 1), (HOST, 3), last_step]):
        what = f"{name}, step {step + 1}: {entry}({split}, 4)"
        if fresh is not None:
            fresh.close()
        fresh = pbrt_hip.Scene(); capture(fresh)
        getattr(one, entry)(split, 4); getattr(fresh, entry)(split, 4)
        assert_same_tree(one, fresh, what)
        want = fresh.intersect_batch(rays)
        n_hit = int((want["prim"] != 0xFFFFFFFF).sum())
        print(f"{what}: {n_hit} of {len(rays)} rays hit on the fresh handle")
        assert 5 * n_hit >= len(rays), what        # the fresh handle alone
        assert scenes.hits_equal(want, oracle_hits[split]).all(), what
        got = one.intersect_batch(rays)            # (uploads the tree: the next build starts from an uploaded handle)
        assert scenes.hits_equal(got, want).all() and np.array_equal(got["pad"], want["pad"]), what
    # the leaf records a probe checks its hits against, read from a tree that lives on the device
    hit = want["prim"] != 0xFFFFFFFF
    aux = np.zeros((int(hit.sum()), pbrt_hip.Scene.SURFACE_PROBE_AUX), np.float32)
    a = one.surface_probe_batch(0, rays[hit], got[hit], aux, variant=probe_variant)
    b = fresh.surface_probe_batch(0, rays[hit], want[hit], aux, variant=probe_variant)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    bad = got[hit].copy(); bad["pad"][0, 0] = one.accel_stats()["leaf_records"]      # one past the last record: the check that reads them refuses it
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        one.surface_probe_batch(0, rays[hit], bad, aux, variant=probe_variant)
    assert e.value.code == pbrt_hip.ERR_INVALID_ARG
    one.close(); fresh.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_a_refused_device_build_leaves_the_next_build_on_the_host(host, name):
    capture = SCENES[name](host)[0]
    one, fresh = pbrt_hip.Scene(), pbrt_hip.Scene()
    capture(one); capture(fresh)
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        one.build_accel_device(3, 4)               # EqualCounts is the host's
    assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
    one.build_accel(3, 4); fresh.build_accel(3, 4)
    assert_same_tree(one, fresh, name + ", EqualCounts")
    one.build_accel(0, 4); fresh.build_accel(0, 4)
    assert_same_tree(one, fresh, name + ", SAH")
    rays = _rays()
    assert scenes.hits_equal(one.intersect_batch(rays), fresh.intersect_batch(rays)).all()
    one.close(); fresh.close()
