"""-m gpu: randomized differential test of quadric shapes in scenes with object instances.  Each seed draws 2 - 6 quadrics of random kind, cut and transform
(tests/test_fuzz_quadrics_gpu.py's generator), 1 - 3 objects of 1 - 200 random triangles, 1 - 8 instances of them under random affine transforms (handedness flips included),
scene-level triangles or none, all in shuffled directive order; an alpha / shadow-alpha mask of either texture class (image maps: the traversal kernel's lean alpha row;
checkerboards, dots: its general row) on a mesh inside an object or at scene level, or no mask; the SAH or EqualCounts builder, HLBVH only when no regular grid is drawn (the
reference's build asserts on one); max_prims_in_node 1, 4 or 255; the path or the Whitted integrator.  No "none" materials, so the renderer's cap of 1 024 pass-through surfaces per
path cannot refuse a scene.  Per seed 20 000 rays of closest hits and occlusion and a 32 x 24 film @ 4 spp are compared with the oracle's bit for bit (f64-libm mode), counters
included.  The oracle renders all twelve seeds of the list (checked on the CPU when it was written), so a refusal on either side fails a seed; the sweep reports a seed that BOTH
sides refuse with the same code and message apart.  `python tests/test_fuzz_quadric_instances_gpu.py FIRST LAST` sweeps more seeds."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "pbrt-v3-rs_amd"), os.path.join(_root, "tests")]

import numpy as np
import pytest

import pbrt_hip
import scenes
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1
from sphere_light_scenes import oracle_whitted
from test_fuzz_gpu import random_transform
from test_fuzz_quadric_alpha_gpu import random_mask, random_material
from test_fuzz_quadrics_gpu import random_shape, random_textured_material

pytestmark = pytest.mark.gpu
SEEDS = tuple(range(201, 213))
RES, SPP, DEPTH, N_RAYS = (32, 24), 4, 4, 20000


def build_case(host, seed):
    """-> (cap(scene), whitted)"""
    rng = np.random.default_rng(seed)
    geo_seed = int(rng.integers(0, 2 ** 31))
    whitted = bool(rng.integers(0, 2))

    def cap(s):
        g = np.random.default_rng(geo_seed)
        s.add_light_infinite(tuple(g.uniform(0.2, 0.8, 3)))
        if g.integers(0, 2): s.add_light_point(tuple(g.uniform(2, 12, 3)), g.uniform(-1.5, 1.5, 3).astype(np.float32) + np.float32([0, 0, 2.5]))
        mats = [random_material(s, g) for _ in range(3)] + [random_textured_material(s, g) for _ in range(2)]
        mat = lambda: mats[int(g.integers(0, 5))]
        mask_class = int(g.integers(0, 3))            # 0 none, 1 image maps only, 2 a general texture somewhere
        grid = bool(g.integers(0, 2))                 # a regular grid among the scene-level triangles
        n_objects = int(g.integers(1, 4)); n_instances = int(g.integers(1, 9)); n_quadrics = int(g.integers(2, 7)); n_meshes = int(g.integers(0, 3))
        masked = []                                   # the masks drawn so far: one general mask pins the general row

        def mask_last_mesh():
            if not mask_class: return
            general = mask_class == 2 and (not masked or bool(g.integers(0, 2)))
            which = int(g.integers(0, 3))             # alpha, shadow-alpha or both
            mk = lambda: random_mask(s, g, general)
            s.set_last_mesh_alpha_textures(mk() if which != 1 else None, mk() if which != 0 else None)
            masked.append(general)

        def random_mesh(lo, hi, with_mask):
            P, idx = host.gen_random_tris(int(g.integers(lo, hi + 1)), int(g.integers(1, 1000)))
            s.add_mesh(P, idx, mat(), UV=g.uniform(0, 1, (len(P), 2)).astype(np.float32))
            if with_mask: mask_last_mesh()
        objects = []
        for _ in range(n_objects):                    # definitions first (an ObjectInstance names an earlier ObjectBegin), their instances among the other directives
            ob = s.object_begin()
            random_mesh(1, 200, bool(g.integers(0, 2)))
            s.object_end()
            objects.append(ob)
        order = ["q"] * n_quadrics + ["i"] * n_instances + ["m"] * n_meshes + (["g"] if grid else [])
        g.shuffle(order)
        for what in order:
            if what == "q": random_shape(s, host, g, mat())
            elif what == "i": s.add_instance(objects[int(g.integers(0, n_objects))], *random_transform(host, g))
            elif what == "m": random_mesh(1, 60, bool(g.integers(0, 2)))
            else:
                side = int(g.integers(2, 6))
                P, idx = scenes.grid_mesh(side, z=float(g.uniform(-1.3, -0.8)), size=float(g.uniform(1.5, 2.5)))
                s.add_mesh(P, idx, mat(), UV=((P[:, :2] - P[:, :2].min(0)) / np.ptp(P[:, :2], axis=0)).astype(np.float32))
                mask_last_mesh()
        if mask_class and (not masked or (mask_class == 2 and not any(masked))):   # (the draws above may have masked nothing, or image maps every time)
            P, idx = host.gen_random_tris(12, int(g.integers(1, 1000)))
            s.add_mesh(P, idx, mat(), UV=g.uniform(0, 1, (len(P), 2)).astype(np.float32))
            s.set_last_mesh_alpha_textures(random_mask(s, g, mask_class == 2), None)
        if whitted and g.integers(0, 2):
            s.add_light_distant(tuple(g.uniform(0.3, 2, 3)), np.float32([0.3, -0.2, 1.0]))
        w2c, c2w = host.look_at(g.uniform(-0.5, 0.5, 3) + np.array([0, -4.5, 0.5]), [0, 0, 0], [0, 0, 1])
        s.set_camera_perspective(host.perspective_raster_to_camera(float(g.uniform(30, 60)), RES[0], RES[1]), c2w)
        cb, table, sb = host.film_box(RES[0], RES[1])
        s.set_film(RES[0], RES[1], cb, (0.5, 0.5), table)
        s.set_sampler(0, SPP, sb)
        s.build_accel(int(g.choice([0, 3] if grid else [0, 3, 1])), int(g.choice([1, 4, 255])))
    return cap, whitted


def oracle_side(host, seed):
    """-> (rays, hits, occlusion, (film, weights, counters)) of the oracle; raises what the oracle raises"""
    cap, whitted = build_case(host, seed)
    rays = scenes.random_rays(N_RAYS, seed, bound=2.0)
    with OracleScene() as orc:
        with libm1():
            cap(orc)
            hits = orc.intersect_batch(rays); occ = orc.occluded_batch(rays)
            film = None if whitted else orc.render_path_ex(max_depth=DEPTH)[:3]
        if whitted:
            film = oracle_whitted(orc, max_depth=DEPTH)
    return rays, hits, occ, film


def run_seed(host, seed):
    """-> (equal, detail), or raises pbrt_hip.PbrtHipError when BOTH sides refuse the scene alike"""
    cap, whitted = build_case(host, seed)
    refused = None
    try:
        rays, whits, wocc, (oxyz, owt, ost) = oracle_side(host, seed)
    except pbrt_hip.PbrtHipError as e:
        refused = e
    with pbrt_hip.Scene() as prod:
        try:
            cap(prod)
            if refused is None:
                ghits = prod.intersect_batch(rays); gocc = prod.occluded_batch(rays)
            gxyz, gwt, gst = prod.render_whitted(max_depth=DEPTH) if whitted else prod.render_path(max_depth=DEPTH)
        except pbrt_hip.PbrtHipError as e:
            if refused is not None and (e.code, str(e)) == (refused.code, str(refused)):
                raise
            return False, dict(seed=seed, device_error=str(e), oracle_error=str(refused))
    if refused is not None:
        return False, dict(seed=seed, device_error=None, oracle_error=str(refused))
    # (the Whitted integrator keeps the three ray counters only)
    counters = lambda st: (st.camera_rays, st.regular_rays, st.shadow_rays) + (() if whitted else (st.paths_total, st.paths_zero_radiance, st.light_distributions_created))
    nb = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    nh = int((~scenes.hits_equal(ghits, whits)).sum()); no = int((gocc != wocc).sum())
    ok = counters(gst) == counters(ost) and np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)) and nb == 0 and nh == 0 and no == 0
    return ok, dict(seed=seed, whitted=whitted, pixels=nb, hits=nh, occlusion=no, rays_that_hit=int((whits["prim"] != 0xFFFFFFFF).sum()), device=counters(gst), oracle=counters(ost))


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_quadric_instance_scene_bit_exact(host, seed):
    try:
        ok, detail = run_seed(host, seed)
    except pbrt_hip.PbrtHipError as e:
        pytest.fail(f"seed {seed} is refused by both sides ({e}): the oracle rendered every seed of the list when it was written")
    assert ok, detail
    assert detail["rays_that_hit"] > N_RAYS // 20, detail


if __name__ == "__main__":
    host = pbrt_hip.Host()
    first, last = int(sys.argv[1]), int(sys.argv[2])
    bad, refused = [], []
    for seed in range(first, last):
        try:
            ok, detail = run_seed(host, seed)
        except pbrt_hip.PbrtHipError as e:   # a scene BOTH sides refuse with the same code and message is reported, not compared
            refused.append(seed); print("REFUSED", seed, e, flush=True); continue
        if not ok:
            bad.append(seed); print("MISMATCH", detail, flush=True)
    print("checked seeds", first, "..", last - 1, ":", last - first, "scenes, differing:", bad, "refused:", refused, flush=True)
