"""-m gpu: randomized differential test of the quadric shapes.  Each seed draws a scene of random quadrics (all six kinds, random parameters and cuts, transforms that
rotate, mirror and scale — down to near-singular scales —, reversed orientation) with random materials of every kind, textured mattes (uv, checkerboard, 3-D marble / fbm, a bump map)
and random triangles among them, under an infinite light, delta lights and a triangle area light; the film, the ray counters and the path counters must equal the oracle's bit for
bit (f64-libm mode).  Failures print the seed.  `python tests/test_fuzz_quadrics_gpu.py FIRST LAST` sweeps more seeds of the same generator."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "pbrt-v3-rs_amd"), os.path.join(_root, "tests")]

import numpy as np
import pytest

import pbrt_hip
import scenes
from oracle_binding import OracleScene, set_libm_mode
from test_fuzz_gpu import random_material, random_transform

pytestmark = pytest.mark.gpu
KINDS = ("sphere", "cylinder", "disk", "cone", "paraboloid", "hyperboloid")


def random_textured_material(s, g):
    k = int(g.integers(0, 5))
    c = s.add_texture_constant
    if k == 0: m = s.add_material_matte_tex(s.add_texture_uv(float(g.uniform(-2, 2)), float(g.uniform(-2, 2))))
    elif k == 1: m = s.add_material_matte_tex(s.add_texture_checkerboard(c(1.0), c(0.1), float(g.uniform(2, 12)), float(g.uniform(2, 12))))
    elif k == 2: m = s.add_material_matte_tex(s.add_texture_marble(scale=float(g.uniform(1, 3)), variation=float(g.uniform(0.1, 4))))
    elif k == 3: m = s.add_material_matte_tex(s.add_texture_fbm())
    else:
        m = s.add_material_matte(tuple(g.uniform(0.2, 0.9, 3)))
        s.set_material_bump(m, s.add_texture_windy())
    return m


def random_shape(s, host, g, material):
    kind = KINDS[int(g.integers(0, 6))]
    t = random_transform(host, g, 1.2)
    sc = float(g.choice([1.0, 0.5, 0.2, 1e-3]))   # 1e-3 on one axis: a near-singular object_to_world
    axis = [1.0, 1.0, 1.0]; axis[int(g.integers(0, 3))] = sc
    t = host.compose(t, host.scale(tuple(np.float32(axis) * np.float32(g.uniform(0.3, 0.8)))))
    phi = float(g.choice([360.0, 360.0, g.uniform(20, 340)]))
    rev = bool(g.integers(0, 2))
    if kind == "sphere":
        r = float(g.uniform(0.5, 1.2)); cut = bool(g.integers(0, 2))
        s.add_sphere(t[0], t[1], r, float(g.uniform(-r, 0)) if cut else None, float(g.uniform(0, 1.3 * r)) if cut else None, phi, material, rev)
    elif kind == "hyperboloid":
        s.add_hyperboloid(t[0], t[1], tuple(g.uniform(-1, 1, 3)), tuple(g.uniform(-1, 1, 3)), phi, material, rev)
    elif kind == "cylinder":
        s.add_quadric("cylinder", t[0], t[1], float(g.uniform(0.3, 1)), float(g.uniform(-1, 1)), float(g.uniform(-1, 1)), phi, material, rev)
    elif kind == "cone":
        s.add_quadric("cone", t[0], t[1], float(g.uniform(0.3, 1)), float(g.uniform(0.3, 1.5)), 0.0, phi, material, rev)
    elif kind == "paraboloid":
        s.add_quadric("paraboloid", t[0], t[1], float(g.uniform(0.3, 1)), float(g.uniform(0, 0.5)), float(g.uniform(0.6, 1.5)), phi, material, rev)
    else:
        s.add_quadric("disk", t[0], t[1], float(g.uniform(0.4, 1.2)), float(g.uniform(-0.5, 0.5)), float(g.choice([0.0, g.uniform(0, 0.3)])), phi, material, rev)


def build_case(host, seed):
    rng = np.random.default_rng(seed)
    res = (int(rng.integers(17, 41)), int(rng.integers(13, 37)))
    spp = int(rng.choice([1, 2, 3, 5, 8]))
    split = int(rng.choice([0, 0, 1]))
    geo_seed = int(rng.integers(0, 2 ** 31))
    lens = float(rng.choice([0.0, 0.05]))

    def cap(s):
        g = np.random.default_rng(geo_seed)
        if g.integers(0, 4):
            t = random_transform(host, g)
            s.add_light_infinite(tuple(g.uniform(0.1, 0.8, 3)), t[0], t[1])
        for _ in range(int(g.integers(0, 3))):
            if g.integers(0, 2): s.add_light_point(tuple(g.uniform(2, 12, 3)), g.uniform(-1.5, 1.5, 3).astype(np.float32) + np.float32([0, 0, 2.5]))
            else:
                w = g.normal(size=3); w /= np.linalg.norm(w)
                s.add_light_distant(tuple(g.uniform(0.3, 2, 3)), np.float32(w))
        mats = [random_material(s, g) for _ in range(3)] + [random_textured_material(s, g) for _ in range(2)]
        P, idx = host.gen_random_tris(int(g.integers(1, 4)), int(g.integers(1, 1000)))
        lid = s.add_light_diffuse_area(tuple(g.uniform(2, 10, 3)), len(idx) // 3, two_sided=bool(g.integers(0, 2)))
        s.add_mesh(P * np.float32(0.4) + np.float32([0, 0, 1.6]), idx, mats[0], first_area_light=lid)
        for k in range(int(g.integers(1, 9))):
            random_shape(s, host, g, mats[int(g.integers(0, 5))])
            if g.integers(0, 2):
                P, idx = host.gen_random_tris(int(g.integers(1, 60)), int(g.integers(1, 1000)))
                s.add_mesh(P, idx, mats[int(g.integers(0, 5))], UV=(g.uniform(0, 1, (len(P), 2)).astype(np.float32) if g.integers(0, 2) else None))
        Pg, ig = scenes.grid_mesh(3, z=-1.3, size=2.5)
        s.add_mesh(Pg, ig, mats[3])
        w2c, c2w = host.look_at(g.uniform(-0.5, 0.5, 3) + np.array([0, -4.5, 0.5]), [0, 0, 0], [0, 0, 1])
        s.set_camera_perspective(host.perspective_raster_to_camera(float(g.uniform(30, 60)), res[0], res[1]), c2w, lens_radius=lens, focal_distance=4.5)
        cb, table, sb = host.film_box(res[0], res[1])
        s.set_film(res[0], res[1], cb, (0.5, 0.5), table)
        s.set_sampler(0, spp, sb)
        s.build_accel(split, int(g.choice([1, 4, 8])))
    return cap, dict(max_depth=int(rng.integers(1, 8)), light_strategy=int(rng.integers(0, 3)), rr_threshold=float(rng.choice([1.0, 0.5, 10.0])))


def run_seed(host, seed):
    """-> (equal, detail)"""
    cap, kw = build_case(host, seed)
    prod = pbrt_hip.Scene(); orc = OracleScene()
    try:
        cap(prod)
        set_libm_mode(1)   # before the oracle's scene is captured: Sphere::new evaluates acos (theta_min / theta_max), and the comparison mode is the f64-rounded one
        try:
            cap(orc)
            oxyz, owt, ost, _ = orc.render_path_ex(**kw)
        finally:
            set_libm_mode(0)
        gxyz, gwt, gst = prod.render_path(**kw)
    finally:
        prod.close(); orc.close()
    counters = lambda st: (st.camera_rays, st.regular_rays, st.shadow_rays, st.paths_total, st.paths_zero_radiance, st.light_distributions_created)
    nb = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    ok = counters(gst) == counters(ost) and np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)) and nb == 0
    return ok, dict(seed=seed, kw=kw, pixels=nb, device=counters(gst), oracle=counters(ost))


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_quadric_scene_bit_exact(host, seed):
    ok, detail = run_seed(host, seed)
    assert ok, detail


if __name__ == "__main__":
    host = pbrt_hip.Host()
    first, last = int(sys.argv[1]), int(sys.argv[2])
    bad, refused = [], []
    for seed in range(first, last):
        try:
            ok, detail = run_seed(host, seed)
        except pbrt_hip.PbrtHipError as e:   # a scene one side refuses (e.g. the null-surface cap of the renderer) is reported, not compared
            refused.append(seed); print("REFUSED", seed, e, flush=True); continue
        if not ok:
            bad.append(seed); print("MISMATCH", detail, flush=True)
    print("checked seeds", first, "..", last - 1, ":", last - first, "scenes, differing:", bad, "refused:", refused)
