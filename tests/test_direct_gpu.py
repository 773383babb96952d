"""-m gpu: the direct-lighting integrator on the device (pbrt_hip_render_direct, DirectLightingIntegrator::li, integrators/src/direct_lighting.rs:110-166).

The oracle restates the path and the Whitted integrator, not this one, so each check holds the device film against an oracle film that must equal it for a reason written down:
  one == path       strategy "one" against the oracle's PathIntegrator at max_depth 1 with the uniform light strategy, bit for bit (libm mode 1)
  delta lights      "all" and "one" against the oracle's li_whitted on point / spot / distant lights, within a bound derived from the two associations
  all ~ path        "all" with area and infinite lights against the oracle's path at max_depth 1: two unbiased estimators of Le + direct, 5 standard errors
then tile parts, chunks, bands and a two-context handle against the one-device film bit for bit, the refusals, and the front end."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import closed_form as cf
import driver_scene as ds
import pbrt_hip
import reference_scenes as R
from oracle_binding import OracleScene, set_libm_mode
from test_whitted_gpu import _quad, _uv_sphere, assert_same_film, oracle_whitted
from texture_scenes import make_image

pytestmark = pytest.mark.gpu
U = 2.0 ** -24   # float32 unit roundoff


def oracle_path(orc, max_depth=1):
    """The oracle's PathIntegrator with `lightsamplestrategy "uniform"`"""
    orc.b.lib.oracle_set_integrator.argtypes = [C.c_void_p, C.c_int]
    assert orc.b.lib.oracle_set_integrator(orc.h, 0) == 0
    set_libm_mode(1)
    try:
        xyz, wt, st, _ = orc.render_path_ex(max_depth=max_depth, light_strategy=0)
    finally:
        set_libm_mode(0)
    return xyz, wt, st


def finish(s, host, sampler, res, spp, eye=(0.4, -6.0, 2.6), look=(0.0, 0.5, 0.8)):
    _, c2w = host.look_at(list(eye), list(look), [0, 0, 1])
    s.set_camera_perspective(host.perspective_raster_to_camera(42.0, res, res), c2w)
    cb, table, sb = host.film_box(res, res)
    s.set_film(res, res, cb, (0.5, 0.5), table)
    s.set_sampler(cf.SOBOL if sampler == "sobol" else cf.HALTON, spp, sb)
    if sampler == "sobol":
        s.set_sobol_tables(*cf.sobol_fixture())
    s.build_accel(0, 4)


def quad_emitter(s, mat, L, two_sided, z=3.2):
    P, idx, UV = _quad((-0.8, -0.4, z), (1.4, 0, 0), (0, 1.0, 0.15))
    s.add_mesh(P, idx, mat, first_area_light=s.add_light_diffuse_area(L, 2, two_sided=two_sided), reverse_orientation=True)


# ---- 1. "one" against the oracle's path integrator at max_depth 1 --------------------------------------------------------------------------------------------------
ENV = np.random.default_rng(11).uniform(0.0, 0.4, (8, 16, 3)).astype(np.float32)
ENV[1:3, 4:7] = (30.0, 25.0, 20.0)
# name -> number of lights, a power of two: the uniform Distribution1D then picks min(u n, n - 1) with pdf 1 / n exactly
LIGHTS = {"sky": 1, "envmap": 1, "quad_one_sided": 2, "quad_two_sided": 2, "quad_point_spot": 4, "disk": 1}
CASES = [(name, "halton") for name in LIGHTS] + [("quad_point_spot", "sobol"), ("envmap", "sobol")]


def lobeless_scene(s, host, lights, sampler="halton", res=32, spp=4):
    """No material holds a specular lobe: matte with sigma > 0 under a textured Kd, plastic, metal, substrate, translucent, a mix, a bump-mapped matte; one object instance, one
    alpha-masked mesh and a Material "none" sheet in front of the camera; a blocker between the emitters and the floor."""
    checks = s.add_texture_checkerboard(s.add_texture_constant((0.15, 0.2, 0.6)), s.add_texture_constant((0.8, 0.8, 0.7)), su=6.0, sv=6.0)
    floor = s.add_material_matte_tex(checks, sigma=25.0)
    plastic = s.add_material_plastic((0.3, 0.25, 0.2), (0.3, 0.3, 0.3), 0.15)
    metal = s.add_material_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.2, 0.3)
    substrate = s.add_material_substrate((0.4, 0.3, 0.2), (0.3, 0.3, 0.3), 0.2, 0.1)
    translucent = s.add_material_translucent((0.3, 0.3, 0.2), (0.2, 0.2, 0.3), (0.6,) * 3, (0.4,) * 3, 0.2)
    matte = s.add_material_matte((0.6, 0.3, 0.2), 10.0)
    mix = s.add_material_mix(plastic, matte, (0.3, 0.5, 0.7))
    bumpy = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
    s.set_material_bump(bumpy, s.add_texture_imagemap(s.add_mipmap(make_image(32, 32, seed=21), as_float=True, scale=0.05), su=2.0, sv=2.0))
    veil = s.add_material_none()
    P, idx, UV = _quad((-4, -4, 0), (8, 0, 0), (0, 8, 0))
    s.add_mesh(P, idx, floor, UV=UV)
    for k, m in enumerate((plastic, metal, substrate, translucent, mix)):
        P, idx, UV = _quad((-2.6 + k * 1.05, 1.6 - 0.1 * k, 0.0), (0.95, 0.1, 0), (0, 0.25, 1.5))
        s.add_mesh(P, idx, m, UV=UV)
    P, idx, N, UV = _uv_sphere((-0.9, -0.2, 0.7), 0.7)
    s.add_mesh(P, idx, bumpy, N=N, UV=UV)
    P, idx, UV = _quad((0.2, -0.8, 1.6), (1.2, 0, 0), (0, 1.0, 0))   # the blocker
    s.add_mesh(P, idx, matte, UV=UV)
    P, idx, UV = _quad((-2.8, -1.4, 0.0), (1.2, 0.2, 0), (0, 0, 1.4), n=2)
    s.add_mesh(P, idx, plastic, UV=UV)
    s.set_last_mesh_alpha_textures(alpha=s.add_texture_checkerboard(s.add_texture_constant((0.0,) * 3), s.add_texture_constant((1.0,) * 3), su=3.0, sv=3.0, aa="none"))
    P, idx, UV = _quad((-1.0, -4.5, 1.5), (1.5, 0, 0), (0, 0.1, 1.5))   # a "none" sheet over part of the view
    s.add_mesh(P, idx, veil, UV=UV)
    obj = s.object_begin()
    s.add_mesh(R.CUBE_P * 0.3, R.CUBE_IDX, matte)
    s.object_end()
    m = host.compose(host.translate((1.8, -0.4, 0.3)), host.rotate(30.0, (0, 0, 1)))
    s.add_instance(obj, m, host.invert(m))
    black = s.add_material_matte((0.0, 0.0, 0.0))
    if lights == "sky":
        s.add_light_infinite((0.5, 0.6, 0.8))
    elif lights == "envmap":
        t = host.compose(host.rotate(35.0, [0, 0, 1]), host.rotate(-60.0, [1, 0, 0]))
        s.add_light_infinite_map((1.0, 0.9, 0.8), ENV, t[0], t[1])
    elif lights in ("quad_one_sided", "quad_two_sided"):
        quad_emitter(s, black, (14.0, 12.0, 10.0), lights == "quad_two_sided")
    elif lights == "quad_point_spot":
        quad_emitter(s, black, (14.0, 12.0, 10.0), False)
        s.add_light_point((20.0, 18.0, 15.0), (-2.0, -2.0, 3.0))
        l2w, w2l, cos_total, cos_start = host.spot(R._ident(), (2.5, -2.0, 3.5), (0.0, 0.5, 0.0), 35.0, 8.0)
        s.add_light_spot((60.0, 70.0, 80.0), l2w, w2l, cos_total, cos_start)
    elif lights == "disk":
        t = R.ctm(host, host.translate((-0.2, 0.1, 3.0)), host.rotate(15.0, (1, 0, 0)))
        s.add_quadric_light("disk", t[0], t[1], 0.7, 0.0, 0.0, 360.0, black, True, L=(14.0, 12.0, 10.0))
    else:
        raise KeyError(lights)
    finish(s, host, sampler, res, spp)


@pytest.fixture(scope="module")
def lobeless(host):
    """(device scene, oracle path film at max_depth 1) per case, built and rendered once"""
    made = {}

    def get(name, sampler):
        if (name, sampler) not in made:
            prod = pbrt_hip.Scene()
            lobeless_scene(prod, host, name, sampler)
            if name == "disk":   # the oracle has no quadric lights (its tests hold them against closed forms): the device's own path integrator, which the oracle pins on every other case here
                want = prod.render_path(max_depth=1, light_strategy=0)
            else:
                with OracleScene() as orc:
                    lobeless_scene(orc, host, name, sampler)
                    want = oracle_path(orc)
            made[(name, sampler)] = (prod, want)
        return made[(name, sampler)]
    yield get
    for prod, _ in made.values():
        prod.close()


def assert_one_equals_path(got, want, label):
    """film and weights as uint32, camera_rays and shadow_rays; regular_rays differs: the path spawns its continuation ray, estimate_direct's BSDF-sampled rays are in both"""
    gxyz, gwt, gst = got
    oxyz, owt, ost = want
    assert np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)), label
    diff = (gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(-1)
    assert not diff.any(), (label, int(diff.sum()), float(np.abs(gxyz - oxyz).max()))
    assert (gst.camera_rays, gst.shadow_rays) == (ost.camera_rays, ost.shadow_rays), (label, gst.as_dict(), ost.as_dict())


@pytest.mark.parametrize("name,sampler", CASES)
def test_one_equals_the_oracles_path_at_depth_one(lobeless, name, sampler):
    """PathIntegrator::li stopped after its first vertex is Le + uniform_sample_one_light on the same sampler dimensions (path.rs:116-172), where no BSDF holds a specular lobe"""
    prod, want = lobeless(name, sampler)
    assert len({LIGHTS[name]} & {1, 2, 4}) == 1
    got = prod.render_direct("one", max_depth=1)
    assert_one_equals_path(got, want, f"{name} {sampler}")
    assert got[2].shadow_rays > 0 and got[0].max() > 0
    deep = prod.render_direct("one", max_depth=5)   # nothing to recurse into: specular_reflect and specular_transmit return zero
    assert np.array_equal(deep[0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(deep[1], got[1])
    a1, a5 = prod.render_direct("all", max_depth=1), prod.render_direct("all", max_depth=5)
    assert np.array_equal(a1[0].view(np.uint32), a5[0].view(np.uint32))


def test_the_bsdf_half_is_traced(lobeless):
    """a non-delta light costs a closest-hit ray per vertex that samples a direction the light's pdf is not zero for; a scene of delta lights costs none"""
    st = lobeless("sky", "halton")[0].render_direct("one", max_depth=1)[2]
    assert st.regular_rays > st.camera_rays


# ---- 2. delta lights: against li_whitted within a derived bound ----------------------------------------------------------------------------------------------------
def delta_scene(s, host, one_light=False, emitter=False, res=48, spp=4):
    """point + spot + distant lights over a mirror, a glass sphere, rough glass, an uber surface under a checkerboard and matte geometry (test_whitted_gpu.recursion_scene's
    surfaces; the uber surface is opaque, so that no BSDF holds two specular lobes of one kind and sample_f never chooses between lobes by its sample).  emitter: a quad
    emitter on top, for the partition checks."""
    checks = s.add_texture_checkerboard(s.add_texture_constant((0.15, 0.2, 0.6)), s.add_texture_constant((0.8, 0.8, 0.7)), su=6.0, sv=6.0)
    floor = s.add_material_matte_tex(checks)
    glass = s.add_material_glass(kr=(0.9, 0.95, 1.0), kt=(0.95, 0.9, 0.85), eta=1.5)
    rough = s.add_material_glass(kr=(0.8, 0.8, 0.8), kt=(0.9, 0.9, 0.9), uroughness=0.2, vroughness=0.3, eta=1.3)
    mirror = s.add_material_mirror((0.9, 0.8, 0.7))
    uber = s.add_material_uber(kd=(0.3, 0.2, 0.1), ks=(0.2, 0.2, 0.2), kr=(0.3, 0.3, 0.35), kt=(0.25, 0.3, 0.25), opacity=(1.0, 1.0, 1.0), uroughness=0.15, vroughness=0.15, eta=1.4)
    s.set_material_texture(uber, "Kd", checks)
    matte = s.add_material_matte((0.6, 0.3, 0.2))
    P, idx, UV = _quad((-4, -4, 0), (8, 0, 0), (0, 8, 0))
    s.add_mesh(P, idx, floor, UV=UV)
    P, idx, N, UV = _uv_sphere((-0.9, 0.2, 0.8), 0.8)
    s.add_mesh(P, idx, glass, N=N, UV=UV)
    P, idx, UV = _quad((-3, 2.5, 0), (6, 0, 0), (0, 0.3, 3))
    s.add_mesh(P, idx, mirror, UV=UV)
    P, idx, UV = _quad((0.6, -0.6, 0.05), (1.6, 0.3, 0), (0, 0.2, 1.6))
    s.add_mesh(P, idx, uber, UV=UV)
    P, idx, UV = _quad((1.0, -1.6, 0.0), (1.4, 0.0, 0), (0, 0.1, 1.2))
    s.add_mesh(P, idx, rough, UV=UV)
    P, idx, UV = _quad((-2.6, -1.2, 0.0), (1.2, 0.2, 0), (0, 0, 1.4), n=2)
    s.add_mesh(P, idx, matte, UV=UV)
    s.add_light_point((30.0, 28.0, 25.0), (-2.0, -2.0, 4.0))
    if not one_light:
        l2w, w2l, cos_total, cos_start = host.spot(R._ident(), (2.5, -2.0, 3.5), (0.0, 0.5, 0.0), 40.0, 8.0)
        s.add_light_spot((60.0, 70.0, 80.0), l2w, w2l, cos_total, cos_start)
        s.add_light_distant((0.8, 0.8, 0.9), host.distant_direction(R._ident(), (3.0, -2.0, 5.0), (0.0, 0.0, 0.0)))
    if emitter:
        quad_emitter(s, matte, (6.0, 5.0, 4.0), True, z=4.0)
    finish(s, host, "halton", res, spp)


@pytest.fixture(scope="module")
def delta_pairs(host):
    pairs = {}
    for one_light in (False, True):
        prod, orc = pbrt_hip.Scene(), OracleScene()
        delta_scene(prod, host, one_light); delta_scene(orc, host, one_light)
        pairs[one_light] = (prod, orc, {})
    yield pairs
    for prod, orc, _ in pairs.values():
        prod.close(); orc.close()


BOUND = 64 * U


@pytest.mark.parametrize("strategy,depth", [("all", 1), ("all", 2), ("all", 5), ("one", 1), ("one", 2), ("one", 5)])
def test_delta_lights_equal_whitted_up_to_association(delta_pairs, strategy, depth):
    """A delta light's sample_li ignores its sample, estimate_direct has no BSDF half for it and a specular lobe's sample_f ignores its sample, so the two integrators trace the
    same rays and compute the same radiance with two differences of association:
      a light's term    Whitted  f * Li * |wi.ns| / pdf     direct lighting  (f * |wi.ns|) * Li / pdf     3 roundings each: the terms differ by at most 6 u relatively
      a vertex's sum    Whitted  ((Le + c1) + c2) + ..      direct lighting  Le + (((0 + c1) + c2) + ..)  Le = 0 here (no emitter), 0 + c1 is exact: n - 1 roundings each, 2 (n - 1) u
    so a vertex's direct light differs by at most (4 + 2 n) u; every term is non-negative, the box filter's weights are 1 and the RGB -> XYZ matrix is positive, so relative
    differences do not grow in the sums.  The issue's figure is depth * (4 + 2 n) u = 50 u for 3 lights at depth 5, asserted as 64 u.  A recount that also charges the shared
    operations above a vertex (f * Li(child) * |wi.ns| / pdf, refl + trans, L + that: 5 roundings whose inputs now differ, 10 u per level) and the film's sums gives a worst
    case above 64 u; the bound asserted stays the issue's.  The largest ratio observed is in DESIGN §4.6.  "one" runs on the one-light variant, where light_pdf = 1."""
    prod, orc, cache = delta_pairs[strategy == "one"]
    if depth not in cache:
        cache[depth] = oracle_whitted(orc, max_depth=depth)
    want = cache[depth]
    got = prod.render_direct(strategy, max_depth=depth)
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for f in ("camera_rays", "regular_rays", "shadow_rays"):
        assert getattr(got[2], f) == getattr(want[2], f), f
    g, w = got[0].astype(np.float64), want[0].astype(np.float64)
    assert np.array_equal(g == 0.0, w == 0.0)   # a channel that is zero in one film is zero in the other
    nz = w != 0.0
    ratio = np.abs(g[nz] - w[nz]) / w[nz]
    print(f"direct {strategy} depth {depth}: largest relative difference {ratio.max() / U:.2f} u over {int(nz.sum())} channels")
    assert ratio.max() <= BOUND, ratio.max() / U
    assert got[2].shadow_rays > 0 and (depth == 1 or got[2].regular_rays > got[2].camera_rays)


# ---- 3. "all" with non-delta lights: statistically against the oracle's path ---------------------------------------------------------------------------------------
def mis_scene(s, host, scale=1.0, res=32, spp=64):
    white = s.add_material_matte((0.7, 0.7, 0.7))
    grey = s.add_material_matte((0.4, 0.4, 0.4))
    P, idx, UV = _quad((-4, -4, 0), (8, 0, 0), (0, 8, 0))
    s.add_mesh(P, idx, white)
    P, idx, UV = _quad((0.3, -0.5, 0.9), (1.0, 0, 0), (0, 1.0, 0))
    s.add_mesh(P, idx, grey)
    quad_emitter(s, grey, tuple(scale * v for v in (14.0, 12.0, 10.0)), True, z=2.2)
    s.add_light_infinite((0.1, 0.12, 0.15))
    finish(s, host, "halton", res, spp)


def five_se(a, b):
    """the project's 5-standard-error convention (tests/test_quadric_lights_cpu.py) on the per-pixel luminance difference of two films"""
    d = (a[0][..., 1] / a[1]).astype(np.float64) - (b[0][..., 1] / b[1]).astype(np.float64)
    se = d.std(ddof=1) / np.sqrt(d.size)
    return abs(d.mean()), 5.0 * se


def test_all_agrees_with_the_oracles_path_and_the_criterion_rejects_five_percent(host):
    """both are unbiased for Le + direct: uniform_sample_all_lights sums one estimate_direct per light, the path's first vertex takes one light and divides by 1 / n"""
    with pbrt_hip.Scene() as prod, OracleScene() as orc, OracleScene() as off:
        mis_scene(prod, host); mis_scene(orc, host); mis_scene(off, host, scale=1.05)
        got = prod.render_direct("all", max_depth=1)
        mean, bound = five_se(got, oracle_path(orc))
        off_mean, off_bound = five_se(got, oracle_path(off))
    print(f"direct all against path: |mean d| {mean:.3e} against 5 SE {bound:.3e}; emitter x 1.05: {off_mean:.3e} against {off_bound:.3e}")
    assert got[2].regular_rays > got[2].camera_rays and got[2].shadow_rays > 0
    assert mean <= bound, (mean, bound)
    assert off_mean > off_bound, (off_mean, off_bound)


# ---- 4. parts, chunks, bands, two contexts: the one-device, one-band film bit for bit -------------------------------------------------------------------------------
DEPTH = 3


@pytest.fixture(scope="module")
def whole(host):
    with pbrt_hip.Scene() as one:
        delta_scene(one, host, emitter=True)
        want = {st: one.render_direct(st, max_depth=DEPTH) for st in ("all", "one")}
        assert one.render_footprint()["bands"] == 1
        yield one, want


@pytest.mark.parametrize("strategy", ["all", "one"])
def test_tile_parts_merge_to_the_whole_frame(whole, strategy):
    one, want = whole
    bufs, rays = [], [0, 0, 0]
    for part in range(2):
        buf = torch.full((one.tile_buffer_floats(16, part, 2),), float("nan"), dtype=torch.float32, device="cuda")   # every slot has to be written
        st = one.render_direct_tiles_device(buf.data_ptr(), strategy, max_depth=DEPTH, tile_part=part, tile_parts=2)
        rays = [a + b for a, b in zip(rays, (st.camera_rays, st.regular_rays, st.shadow_rays))]
        bufs.append(buf)
    torch.cuda.synchronize()
    xyz, wt = one.merge_tiles_device([b.data_ptr() for b in bufs])
    w = want[strategy]
    assert np.array_equal(xyz.view(np.uint32), w[0].view(np.uint32)) and np.array_equal(wt, w[1])
    assert rays == [w[2].camera_rays, w[2].regular_rays, w[2].shadow_rays]


@pytest.mark.parametrize("strategy", ["all", "one"])
def test_small_chunks_and_one_tile_bands(whole, strategy, monkeypatch):
    one, want = whole
    monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(48 * 48 * 3 // 2))   # four chunks of one sample per pixel
    assert_same_film(one.render_direct(strategy, max_depth=DEPTH), want[strategy], "chunked")
    monkeypatch.delenv("PBRT_HIP_MAX_PATHS")
    one.set_sample_record_budget(256 * 4 * 20)   # one tile's records
    try:
        got = one.render_direct(strategy, max_depth=DEPTH)
        assert one.render_footprint()["bands"] == 9 and one.render_footprint()["band_tiles"] == 1
    finally:
        one.set_sample_record_budget(0)
    assert_same_film(got, want[strategy], "one tile per band")


def test_two_contexts(host, whole):
    one, want = whole
    with pbrt_hip.Scene(devices=[0, 0]) as multi:
        delta_scene(multi, host, emitter=True)
        for strategy in ("all", "one"):
            assert_same_film(multi.render_direct_devices(strategy, max_depth=DEPTH), want[strategy], f"two contexts, {strategy}")
        assert_same_film(one.render_direct_devices("all", max_depth=DEPTH), want["all"], "the _devices entry on a one-device handle")


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(s, entry, strategy, max_depth):
    h, w = s.film_shape
    xyz = np.full((h, w, 3), np.nan, np.float32); wt = np.full((h, w), -7.0, np.float32)
    pb = np.ascontiguousarray(s.sample_bounds, dtype=np.int32)
    fp = C.POINTER(C.c_float)
    rc = s.b.fn(entry)(s.h, strategy, max_depth, pb.ctypes.data_as(C.POINTER(C.c_int)), 16, 0, 1, xyz.ctypes.data_as(fp), wt.ctypes.data_as(fp), None)
    return rc, bool(np.isnan(xyz).all() and (wt == -7.0).all())


def test_refusals_leave_the_outputs_and_the_handle_as_they_were(host, lobeless):
    prod, want = lobeless("quad_point_spot", "sobol")   # 4 lights, 48 Sobol dimensions, no specular lobe: "one" draws 5 + 5 + 4, "all" 5 + 16 + 4

    def still_renders():
        assert_one_equals_path(prod.render_direct("one", max_depth=1), want, "after a refusal")

    for entry in ("render_direct", "render_direct_devices"):
        for strategy, depth in ((2, 1), (-1, 1), (0, 17), (1, -1)):
            rc, untouched = _raw(prod, entry, strategy, depth)
            assert rc == pbrt_hip.ERR_INVALID_ARG and untouched, (entry, strategy, depth, prod.last_error())
        still_renders()
    # the recursion could outrun the tables: a glass surface makes the tree binary, and at max_depth 3 "all" could draw 5 + 7 * 16 + 3 * 4 = 129 of the 48 dimensions given
    with pbrt_hip.Scene() as s:
        glass = s.add_material_glass()   # (lobeless_scene plus one glass triangle out of view)
        s.add_mesh(np.float32([[5, 5, 0], [6, 5, 0], [5, 6, 0]]), np.uint32([0, 1, 2]), glass)
        lobeless_scene(s, host, "quad_point_spot", "sobol")
        for entry in ("render_direct", "render_direct_devices"):
            rc, untouched = _raw(s, entry, 0, 3)
            assert rc == pbrt_hip.ERR_UNSUPPORTED and untouched and "Sobol" in s.last_error(), s.last_error()
        rc, untouched = _raw(s, "render_direct", 1, 1)   # 5 + 5 dimensions: renders
        assert rc == 0 and not untouched
    still_renders()


def test_a_sphere_light_needs_the_handles_switch(host):
    with pbrt_hip.Scene() as s:
        grey = s.add_material_matte((0.5, 0.5, 0.5))
        P, idx, UV = _quad((-4, -4, 0), (8, 0, 0), (0, 8, 0))
        s.add_mesh(P, idx, grey)
        t = R.ctm(host, host.translate((0.0, 0.5, 2.0)))
        s.add_sphere_light(t[0], t[1], 0.4, material=grey, L=(10.0, 9.0, 8.0))
        finish(s, host, "halton", 16, 4)
        rc, untouched = _raw(s, "render_direct", 0, 1)
        assert rc == pbrt_hip.ERR_UNSUPPORTED and untouched and "pbrt_hip_set_path_sphere_lights" in s.last_error()
        s.set_path_sphere_lights(True)
        for strategy in ("all", "one"):
            xyz, wt, st = s.render_direct(strategy, max_depth=1)
            assert np.isfinite(xyz).all() and xyz.max() > 0 and st.regular_rays > st.camera_rays
        s.set_path_sphere_lights(False)
        assert _raw(s, "render_direct_devices", 1, 1)[0] == pbrt_hip.ERR_UNSUPPORTED
        assert np.isfinite(s.render_whitted(max_depth=1)[0]).all()   # the handle still renders what needs no switch


def test_a_multi_device_handle_is_sent_to_the_devices_entry(host):
    with pbrt_hip.Scene(devices=[0, 0]) as s:
        mis_scene(s, host, res=16, spp=4)
        rc, untouched = _raw(s, "render_direct", 0, 1)
        assert rc == pbrt_hip.ERR_UNSUPPORTED and untouched and "pbrt_hip_render_direct_devices" in s.last_error()
        xyz, wt, _ = s.render_direct_devices("all", max_depth=1)
        assert np.isfinite(xyz).all() and (wt > 0).all()


# ---- 6. the front end -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["all", "one"])
def test_front_end_renders_the_film_of_the_c_abi(tmp_path, host, strategy):
    """tests/driver_scene.py's scene file (an infinite, a distant, a point and an area light) under Integrator "directlighting", against the same scene captured call by call"""
    path = ds.write_files(str(tmp_path), filter_line=ds.FILTERS["box"][0], strategy="uniform")
    text = open(path).read()
    line = next(ln for ln in text.splitlines() if ln.startswith('Integrator "path"'))
    text = text.replace(line, f'Integrator "directlighting" "integer maxdepth" 3 "string strategy" "{strategy}"')
    open(path, "w").write(text)
    r = subprocess.run([ds.RENDER_BIN, "--quiet", path], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = ds.read_pfm(str(tmp_path / "scene.pfm"))
    with pbrt_hip.Scene() as s:
        cb, sb = ds.capture(s, host, "box")
        xyz, wt, _ = s.render_direct(strategy, max_depth=3, pixel_bounds=sb)
        rgb = s.film_to_rgb(xyz, wt).reshape(ds.YRES, ds.XRES, 3)
    assert img.max() > 0 and (img.view(np.uint32) == rgb.view(np.uint32)).all(), f"{(img != rgb).sum()} differing values"
