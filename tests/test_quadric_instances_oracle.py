"""CPU only: the oracle alone on the stage of tests/quadric_instance_scenes.py (quadric shapes among object instances).  The device comparisons of
tests/test_quadric_instances_gpu.py are against this renderer; shown here are the conditions that make them meaningful: the rays of the batch tests end on every quadric, on most
instances and on scene-level triangles, the SAH tree has a leaf in which a quadric record stands directly between two instance records, the one-leaf scenes are one leaf in
directive order, and the quadrics are not inert in the film.  (Passes with and without the device library's support for such scenes: it shows the yardstick, not the feature.)"""
import numpy as np
import pytest

import quadric_instance_scenes as QI
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1

N_TOP = 32 + 4 + 6     # the stage's scene-level items: the floor's triangles, four quadrics, six instances (the instance of the empty object adds none: lib.rs:946-949)


@pytest.fixture(scope="module")
def staged(host):
    with OracleScene() as orc, libm1():
        prims = QI.stage(orc, host)
        hits = orc.intersect_batch(QI.stage_rays())
        xyz = orc.render_path_ex(max_depth=4, light_strategy=0)[0]
        yield prims, hits, QI.oracle_leaves(orc, N_TOP), xyz


def test_the_batch_rays_end_on_every_kind_of_item(staged):
    prims, hits, _, _ = staged
    quadrics, tris, per_inst, misses = QI.tally(hits, prims)
    print(quadrics, tris, per_inst, misses)
    assert min(quadrics.values()) >= 200, quadrics
    assert (per_inst >= 1000).sum() >= 4, per_inst
    assert tris >= 5000
    assert misses > 0


def test_a_sah_leaf_holds_a_quadric_between_two_instances(staged):
    prims, _, leaves, _ = staged
    quadric = {prims[k][0] for k in ("sphere", "cylinder", "disk", "cone")}
    assert sorted(v for l in leaves for v in l) == sorted(list(range(1, 33)) + sorted(quadric) + [QI.INST_BIT | k for k in range(6)])
    between = [l for l in leaves for i in range(1, len(l) - 1) if l[i] in quadric and (l[i - 1] & QI.INST_BIT) and (l[i + 1] & QI.INST_BIT)]
    assert between, leaves


@pytest.mark.parametrize("instance_first", [False, True])
def test_the_one_leaf_scene_is_one_leaf_in_directive_order(host, instance_first):
    with OracleScene() as orc, libm1():
        prims = QI.one_leaf(orc, host, instance_first)
        leaves = QI.oracle_leaves(orc, QI.ONE_LEAF_ITEMS)
        assert len(orc.bvh_nodes()) == 1 and len(leaves) == 1
        t, sp, cy = prims["triangle"][0], prims["sphere"][0], prims["cylinder"][0]
        assert leaves[0] == ((QI.INST_BIT, cy, QI.INST_BIT | 1, sp, t) if instance_first else (t, sp, QI.INST_BIT, cy, QI.INST_BIT | 1))
        # along many rays a quadric AND an instanced triangle (or the scene-level triangle) lie: with and without the quadrics the same ray ends elsewhere
        rays = QI.one_leaf_rays()
        hits = orc.intersect_batch(rays)
    hit = hits["prim"] != QI.MISS; inst = hits["pad"][:, 1]
    on_quadric = hit & (inst == 0) & (QI.in_range(hits["prim"], prims["sphere"]) | QI.in_range(hits["prim"], prims["cylinder"]))
    assert on_quadric.sum() >= 500 and (hit & (inst == 1)).sum() >= 200 and (hit & (inst == 2)).sum() >= 200 and (hit & (inst == 0) & ~on_quadric).sum() >= 100
    assert np.isfinite(rays["t_max"]).sum() >= len(rays) // 4


def test_the_quadrics_are_not_inert_in_the_film(host, staged):
    with OracleScene() as orc, libm1():
        QI.stage(orc, host, sphere_at=(0.3, 0.2, 60.0))     # the mirror sphere far above the view
        away = orc.render_path_ex(max_depth=4, light_strategy=0)[0]   # (uniform light sampling: the strategy does not depend on the world bound)
    differ = (away != staged[3]).any(-1)
    assert differ.mean() >= 0.05, float(differ.mean())
    assert float(staged[3].max()) > 0
