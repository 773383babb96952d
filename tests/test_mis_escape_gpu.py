"""-m gpu: frames whose BSDF-sampled MIS ray is traced as an escape query (csrc/mis_escape.h) against the CPU oracle in libm mode 1.  The query changes how one ray in three is
walked and nothing a caller can see: the film matches the oracle bit for bit and regular_rays, shadow_rays, paths_total and paths_zero_radiance are the oracle's — the MIS ray is
still counted where the reference counts it.  Scenes: the flat and the instanced soup (both eligible rows), two meshes with constant alphas (a shadowalpha-0 mesh stops the ray, an
alpha-0 mesh does not: the reference's intersect, not intersect_p), traversal counting on (the frame is traced as the reference traces it, the counts are the oracle's) and
off again (same film), and a scene with one triangle area light (ineligible: the resolve compares the hit primitive with the sampled light)."""
import numpy as np
import pytest

import pbrt_hip
from oracle_binding import OracleScene, set_libm_mode

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
SPEC = pbrt_hip.SceneSpec(n_tris=3000, xres=48, yres=40, spp=4, max_depth=4)


def _bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def oracle_frame(orc, **kw):
    set_libm_mode(1)
    try:
        return orc.render_path_ex(**kw)
    finally:
        set_libm_mode(0)


def assert_frame_is_the_oracles(g, o):
    gxyz, gwt, gst = g
    oxyz, owt, ost = o[:3]
    assert (gst.regular_rays, gst.shadow_rays, gst.camera_rays) == (ost.regular_rays, ost.shadow_rays, ost.camera_rays), (gst.as_dict(), ost.as_dict())
    assert (gst.paths_total, gst.paths_zero_radiance) == (ost.paths_total, ost.paths_zero_radiance), (gst.as_dict(), ost.as_dict())
    assert _bits_equal(gwt, owt), "filter weight sums differ"
    nb = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    assert nb == 0, f"{nb} pixels differ from the oracle"
    assert float(oxyz.max()) > 0.0


@pytest.mark.parametrize("instances", [0, 3], ids=["flat", "instanced"])
def test_soup_under_the_sky(host, instances):
    prod = pbrt_hip.Scene(); orc = OracleScene()
    pbrt_hip.capture_spec(SPEC, prod, host, instances=instances); pbrt_hip.capture_spec(SPEC, orc, host, instances=instances)
    assert prod.mis_escape() is False     # nothing rendered yet
    o = oracle_frame(orc, max_depth=4)
    g = prod.render_path(max_depth=4)
    assert prod.mis_escape() is True
    assert_frame_is_the_oracles(g, o)
    assert o[2].regular_rays > 2 * o[2].camera_rays     # bounce and MIS rays were traced


def _alpha_capture(host, alpha_of_third):
    """three small soups in one cloud: a plain mesh, one with constant shadowalpha 0 and one whose constant alpha is alpha_of_third"""
    P, idx = host.gen_random_tris(900, 23)

    def capture(s):
        m = s.add_material_matte((0.6, 0.6, 0.6), 0.0)
        s.add_light_infinite((1.0, 0.9, 0.8))
        s.add_mesh(P[:900], idx[:900], m)
        s.add_mesh(P[900:1800], idx[900:1800] - 900, m, shadow_alpha=0.0)
        s.add_mesh(P[1800:], idx[1800:] - 1800, m, alpha=alpha_of_third)
        w2c, c2w = host.look_at([0, -4, 0.3], [0, 0, 0], [0, 0, 1])
        s.set_camera_perspective(host.perspective_raster_to_camera(38.0, 40, 32), c2w)
        cb, table, sb = host.film_box(40, 32)
        s.set_film(40, 32, cb, (0.5, 0.5), table)
        s.set_sampler(0, 4, sb)
        s.build_accel(0, 4)
    return capture


def test_constant_alphas_follow_intersect_not_intersect_p(host):
    cap = _alpha_capture(host, 0.0)
    prod = pbrt_hip.Scene(); orc = OracleScene(); twin = OracleScene()
    cap(prod); cap(orc); _alpha_capture(host, 1.0)(twin)    # the twin's third mesh is opaque: what the alpha-0 mesh would have stopped
    orc.record_rays(1 << 20)
    o = oracle_frame(orc, max_depth=4)
    rays = orc.recorded_rays(False)                          # camera, bounce and MIS rays: the latter two leave hit points into the facing hemisphere
    assert len(rays) > 3000
    found = orc.ray_stats_batch(rays)["found"] != 0
    found_p = orc.ray_stats_batch(rays, any_hit=True)["found"] != 0
    found_twin = twin.ray_stats_batch(rays)["found"] != 0
    only_salpha = found & ~found_p          # nothing but shadowalpha-0 triangles in the way: intersect_p's rule would let these rays escape
    only_alpha0 = found_twin & ~found       # nothing but alpha-0 triangles in the way: a rule that forgot PH_TRI_ALPHA0 would stop these rays
    assert only_salpha.sum() > 20 and only_alpha0.sum() > 20, (int(only_salpha.sum()), int(only_alpha0.sum()))
    hits, _ = orc.intersect_batch_stats(rays)
    assert ((hits["prim"] >= 300) & (hits["prim"] < 600)).sum() > 100 and not ((hits["prim"] >= 600) & (hits["prim"] != MISS)).any()
    g = prod.render_path(max_depth=4)
    assert prod.mis_escape() is True
    assert_frame_is_the_oracles(g, o)


def test_counting_on_traces_the_reference_and_off_gives_the_same_film(host):
    prod = pbrt_hip.Scene(); orc = OracleScene()
    pbrt_hip.capture_spec(SPEC, prod, host); pbrt_hip.capture_spec(SPEC, orc, host)
    set_libm_mode(1)
    try:
        oxyz, owt, ost, nvnt = orc.render_path_ex(max_depth=4, count_traversal=True)
    finally:
        set_libm_mode(0)
    prod.set_traversal_counting(True)
    g_on = prod.render_path(max_depth=4)
    assert prod.mis_escape() is False
    cnt = prod.traversal_counts()
    prod.set_traversal_counting(False)
    assert cnt["closest"]["rays"] == ost.regular_rays and cnt["any_hit"]["rays"] == ost.shadow_rays
    assert cnt["closest"]["tri_tests"] == nvnt[1] and cnt["any_hit"]["tri_tests"] == nvnt[3]
    assert cnt["closest"]["ref_node_visits"] == nvnt[0] and cnt["any_hit"]["ref_node_visits"] == nvnt[2]
    g_off = prod.render_path(max_depth=4)
    assert prod.mis_escape() is True
    for g in (g_on, g_off):
        assert_frame_is_the_oracles(g, (oxyz, owt, ost))
    assert _bits_equal(g_on[0], g_off[0]) and _bits_equal(g_on[1], g_off[1])


def test_a_triangle_area_light_switches_the_query_off(host):
    P, idx = host.gen_random_tris(3000, 11)
    tri = np.array([[-0.4, -0.4, 1.6], [0.4, -0.4, 1.6], [0.0, 0.5, 1.6]], np.float32)

    def cap(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        s.add_light_infinite((0.3, 0.3, 0.35))
        s.add_mesh(P, idx, m)
        lid = s.add_light_diffuse_area((9.0, 8.0, 7.0), 1, two_sided=True)
        s.add_mesh(tri, [0, 1, 2], m, first_area_light=lid)
        w2c, c2w = host.look_at([0, -4, 0.5], [0, 0, 0], [0, 0, 1])
        s.set_camera_perspective(host.perspective_raster_to_camera(40.0, 48, 40), c2w)
        cb, table, sb = host.film_box(48, 40)
        s.set_film(48, 40, cb, (0.5, 0.5), table)
        s.set_sampler(0, 4, sb)
        s.build_accel(0, 4)
    prod = pbrt_hip.Scene(); orc = OracleScene()
    cap(prod); cap(orc)
    o = oracle_frame(orc, max_depth=4)
    g = prod.render_path(max_depth=4)
    assert prod.mis_escape() is False
    assert_frame_is_the_oracles(g, o)
