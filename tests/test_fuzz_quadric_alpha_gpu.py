"""-m gpu: randomized differential test of quadric shapes next to alpha-masked triangle meshes.  Each of the twelve seeds below draws 2 - 12 quadrics of random kinds, cuts and
transforms (tests/test_fuzz_quadrics_gpu.py's generator), 1 - 3 meshes of 8 - 200 triangles that carry random alpha and shadow-alpha masks of both texture classes (image maps:
the traversal kernel's lean alpha row; checkerboards, dots, 3-D checkerboards: its general row), and random materials of every class but "none" (so the renderer's cap of 1 024
pass-through surfaces per path cannot refuse a scene).  Film 24 x 16 @ 2 spp, depth 4, path integrator; every third seed the Whitted integrator.  Film, weights and counters must
equal the oracle's bit for bit (f64-libm mode); a refusal or an error on either side fails the seed.  The oracle renders all twelve (checked when the list was written)."""
import numpy as np
import pytest

import pbrt_hip
import scenes
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1
from sphere_light_scenes import oracle_whitted
from test_fuzz_quadrics_gpu import random_shape, random_textured_material

pytestmark = pytest.mark.gpu
SEEDS = (101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112)
RES, SPP, DEPTH = (24, 16), 2, 4


def random_material(s, g):
    """One of the material classes tests/test_fuzz_gpu.py draws from, "none" left out: every class is named here, so nothing another file changes can bring it back"""
    c = lambda lo=0.05, hi=0.95: tuple(g.uniform(lo, hi, 3).astype(np.float32))
    k = ("matte", "mirror", "plastic", "glass", "metal", "uber", "substrate", "translucent", "mix", "black")[int(g.integers(0, 10))]
    if k == "matte": return s.add_material_matte(c(), float(g.choice([0.0, g.uniform(1, 60)])))
    if k == "mirror": return s.add_material_mirror(c(0.3, 1.0))
    if k == "plastic": return s.add_material_plastic(c(), c(0.05, 0.5), float(g.uniform(0.01, 0.4)), bool(g.integers(0, 2)))
    if k == "glass":
        rough = g.integers(0, 2)
        return s.add_material_glass(c(0.5, 1), c(0.5, 1), float(rough * g.uniform(0.02, 0.3)), float(rough * g.uniform(0.02, 0.3)), float(g.uniform(1.1, 1.8)), True)
    if k == "metal": return s.add_material_metal(c(0.1, 2.0), c(1.5, 6.0), float(g.uniform(0.01, 0.3)), float(g.uniform(0.01, 0.3)), bool(g.integers(0, 2)))
    if k == "uber":
        op = float(g.choice([1.0, g.uniform(0.3, 0.9)]))
        return s.add_material_uber(c(), c(0.05, 0.4), c(0, 0.3), c(0, 0.3), (op, op, op), float(g.uniform(0.02, 0.3)), float(g.uniform(0.02, 0.3)), float(g.uniform(1.1, 1.7)), True)
    if k == "substrate": return s.add_material_substrate(c(), c(0.05, 0.6), float(g.uniform(0.02, 0.4)), float(g.uniform(0.02, 0.4)), bool(g.integers(0, 2)))
    if k == "translucent": return s.add_material_translucent(c(), c(0, 0.5), c(0.1, 0.9), c(0, 0.9), float(g.uniform(0.02, 0.3)), True)
    if k == "mix":
        a = s.add_material_plastic(c(), c(0.05, 0.5), float(g.uniform(0.01, 0.4)), True)
        b = s.add_material_mirror(c(0.3, 1.0)) if g.integers(0, 2) else s.add_material_glass(c(0.5, 1), c(0.5, 1), 0.0, 0.0, 1.5, True)
        return s.add_material_mix(a, b, c(0.1, 0.9))
    return s.add_material_matte((0, 0, 0), 0.0)   # black: no BxDF at all


def random_mask(s, g, general):
    uvp = dict(su=float(g.uniform(1, 6)), sv=float(g.uniform(1, 6)))
    if not general:
        m = (g.uniform(0, 1, (int(g.integers(2, 6)), int(g.integers(2, 6)))) > 0.5).astype(np.float32)
        m = np.kron(m, np.ones((3, 3), np.float32))   # blocks of 3 x 3 texels: a bilinear look-up is exactly 0 inside a zero block
        return s.add_texture_imagemap(s.add_mipmap(np.repeat(m[..., None], 3, axis=2), as_float=True, trilinear=True, wrap=str(g.choice(["repeat", "black", "clamp"]))), **uvp)
    k = int(g.integers(0, 3)); c = s.add_texture_constant
    if k == 0: return s.add_texture_checkerboard(c(1.0), c(0.0), aa="none", **uvp)
    if k == 1: return s.add_texture_dots(c(0.0), c(1.0), **uvp)
    return s.add_texture_checkerboard3d(c(0.0), c(1.0))


def build_case(host, seed):
    """-> (cap(scene), whitted)"""
    rng = np.random.default_rng(seed)
    geo_seed = int(rng.integers(0, 2 ** 31))
    general = bool(rng.integers(0, 2))           # the scene's alpha row: one general mask anywhere takes the whole scene there
    whitted = seed % 3 == 0

    def cap(s):
        g = np.random.default_rng(geo_seed)
        s.add_light_infinite(tuple(g.uniform(0.2, 0.8, 3)))
        if g.integers(0, 2): s.add_light_point(tuple(g.uniform(2, 12, 3)), g.uniform(-1.5, 1.5, 3).astype(np.float32) + np.float32([0, 0, 2.5]))
        mats = [random_material(s, g) for _ in range(3)] + [random_textured_material(s, g) for _ in range(2)]
        n_quadrics = int(g.integers(2, 13)); n_meshes = int(g.integers(1, 4))
        order = ["q"] * n_quadrics + ["m"] * n_meshes
        g.shuffle(order)
        for what in order:
            if what == "q":
                random_shape(s, host, g, mats[int(g.integers(0, 5))])
                continue
            if g.integers(0, 2):
                side = int(g.integers(2, 11))                                 # 8 - 200 triangles in a grid ...
                P, idx = scenes.grid_mesh(side, z=float(g.uniform(-0.8, 0.8)), size=float(g.uniform(0.8, 1.6)))
                UV = ((P[:, :2] - P[:, :2].min(0)) / np.ptp(P[:, :2], axis=0)).astype(np.float32)
            else:
                P, idx = host.gen_random_tris(int(g.integers(8, 201)), int(g.integers(1, 1000)))   # ... or as many random ones
                UV = g.uniform(0, 1, (len(P), 2)).astype(np.float32) if g.integers(0, 2) else None
            s.add_mesh(P, idx, mats[int(g.integers(0, 5))], UV=UV)
            which = int(g.integers(0, 3))                                     # alpha, shadow-alpha or both
            mk = lambda: random_mask(s, g, general and bool(g.integers(0, 2)))
            s.set_last_mesh_alpha_textures(mk() if which != 1 else None, mk() if which != 0 else None)
        if general:   # (the draw above may have picked image maps every time: one general mask pins the row)
            P, idx = scenes.grid_mesh(2, z=-1.0, size=0.7)
            s.add_mesh(P, idx, mats[0]); s.set_last_mesh_alpha_textures(random_mask(s, g, True), None)
        Pg, ig = scenes.grid_mesh(3, z=-1.3, size=2.5)
        s.add_mesh(Pg, ig, mats[3])
        w2c, c2w = host.look_at(g.uniform(-0.5, 0.5, 3) + np.array([0, -4.5, 0.5]), [0, 0, 0], [0, 0, 1])
        s.set_camera_perspective(host.perspective_raster_to_camera(float(g.uniform(30, 60)), RES[0], RES[1]), c2w)
        cb, table, sb = host.film_box(RES[0], RES[1])
        s.set_film(RES[0], RES[1], cb, (0.5, 0.5), table)
        s.set_sampler(0, SPP, sb)
        s.build_accel(0, int(g.choice([1, 4, 8])))
    return cap, whitted


def oracle_film(host, seed):
    cap, whitted = build_case(host, seed)
    with OracleScene() as orc:
        with libm1():
            cap(orc)
            if not whitted:
                return orc.render_path_ex(max_depth=DEPTH)[:3]
        return oracle_whitted(orc, max_depth=DEPTH)


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_quadric_alpha_scene_bit_exact(host, seed):
    cap, whitted = build_case(host, seed)
    oxyz, owt, ost = oracle_film(host, seed)
    with pbrt_hip.Scene() as prod:
        cap(prod)
        gxyz, gwt, gst = prod.render_whitted(max_depth=DEPTH) if whitted else prod.render_path(max_depth=DEPTH)
    # (the Whitted integrator keeps the three ray counters only)
    counters = lambda st: (st.camera_rays, st.regular_rays, st.shadow_rays) + (() if whitted else (st.paths_total, st.paths_zero_radiance, st.light_distributions_created))
    nb = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    detail = dict(seed=seed, whitted=whitted, pixels=nb, device=counters(gst), oracle=counters(ost))
    assert counters(gst) == counters(ost) and np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)) and nb == 0, detail
