"""-m gpu: the Whitted integrator on the device (pbrt_hip_render_whitted) against the CPU oracle's li_whitted bit for bit (libm mode 1: film and weights as uint32, the three ray
counters), against the renders the reference commits next to its scenes, through the front end, against a closed form that owes nothing to the oracle, and its refusals."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import closed_form as cf
import driver_scene as ds
import pbrt_hip
import reference_scenes as R
from oracle_binding import OracleScene, set_libm_mode
from test_quadrics_gpu import generic_adders   # the scene builders' quadric calls through Scene.add_sphere / add_quadric / add_hyperboloid, which serve either binding
from test_reference_renders import DETERMINISTIC, NOISY, WHITTED

pytestmark = pytest.mark.gpu


def oracle_whitted(orc, **kw):
    orc.b.lib.oracle_set_integrator.argtypes = [C.c_void_p, C.c_int]
    assert orc.b.lib.oracle_set_integrator(orc.h, 1) == 0
    set_libm_mode(1)
    try:
        xyz, wt, st, _ = orc.render_path_ex(**kw)
    finally:
        set_libm_mode(0)
    return xyz, wt, st


def assert_same_film(got, want, label=""):
    gxyz, gwt, gst = got
    oxyz, owt, ost = want
    assert np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)), label
    diff = (gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(-1)
    assert not diff.any(), (label, int(diff.sum()), float(np.abs(gxyz - oxyz).max()))
    for f in ("camera_rays", "regular_rays", "shadow_rays"):
        assert getattr(gst, f) == getattr(ost, f), (label, f, getattr(gst, f), getattr(ost, f))


# ---- 1. the reference's scenes, small ------------------------------------------------------------------------------------------------------------------------------
SIX = ["fbm", "wrinkled", "windy", "marble", "dots", "bilerp", "uv", "mix", "scale", "constant", "2d-checkerboard"]
SMALL = ([(n, lambda s, host, n=n: getattr(R, n)(s, host, spp=8, res=96)) for n, _ in DETERMINISTIC + NOISY] +
         [("materials_bump", lambda s, host: R.materials_bump(s, host, spp=8, res=96)),
          ("samplers_halton", lambda s, host: R.samplers_scene(s, host, "halton", spp=8)),
          ("samplers_sobol", lambda s, host: R.samplers_scene(s, host, "sobol", spp=8)),
          ("cameras_depth_of_field", lambda s, host: R.cameras_depth_of_field(s, host, spp=8, crop=(0.42, 0.62, 0.45, 0.7))),   # the focused sphere
          ("textures_2d_mappings", lambda s, host: R.textures_2d_mappings(s, host, spp=8, crop=(0.0, 1.0, 0.4, 0.6)))] +
         [("textures_" + w, lambda s, host, w=w: R.textures_six_shapes(s, host, w, spp=8)) for w in SIX])


@pytest.mark.parametrize("name,build", SMALL, ids=[n for n, _ in SMALL])
def test_device_whitted_film_equals_the_oracle_film_on_the_reference_scenes(host, name, build):
    with pbrt_hip.Scene() as prod, OracleScene() as orc:
        with generic_adders():
            build(prod, host)
        build(orc, host)
        pb = None
        if name.startswith("textures_") and name != "textures_2d_mappings":   # 400 x 400 scenes without a resolution parameter: a window that holds all six shapes' rows
            pb = [100, 150, 300, 260]
        assert_same_film(prod.render_whitted(max_depth=5, pixel_bounds=pb), oracle_whitted(orc, max_depth=5, pixel_bounds=pb), name)


# ---- 2. a scene made for the recursion ---------------------------------------------------------------------------------------------------------------------------
def _uv_sphere(center, radius, nu=12, nv=8):
    P, N, UV, idx = [], [], [], []
    for j in range(nv + 1):
        th = math.pi * j / nv
        for i in range(nu + 1):
            ph = 2.0 * math.pi * i / nu
            n = (math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th))
            N.append(n); P.append([center[k] + radius * n[k] for k in range(3)]); UV.append((i / nu, j / nv))
    for j in range(nv):
        for i in range(nu):
            a = j * (nu + 1) + i; b = a + 1; c = a + nu + 1; d = c + 1
            if j > 0: idx += [a, c, b]
            if j < nv - 1: idx += [b, c, d]
    return np.array(P, np.float32), np.array(idx, np.uint32), np.array(N, np.float32), np.array(UV, np.float32)


def _quad(o, u, v, n=1):
    o, u, v = (np.asarray(a, np.float64) for a in (o, u, v))
    P = [o + u * (i / n) + v * (j / n) for j in range(n + 1) for i in range(n + 1)]
    UV = [(i / n, j / n) for j in range(n + 1) for i in range(n + 1)]
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            idx += [a, a + 1, a + n + 2, a, a + n + 2, a + n + 1]
    return np.array(P, np.float32), np.array(idx, np.uint32), np.array(UV, np.float32)


def recursion_scene(s, host, sampler="halton", res=48, spp=4, one_light=False):
    """A glass sphere (smooth normals: the refracted differentials use dn/du, dn/dv), a mirror quad with a "none" veil in front of half of it, a mesh cut out by an alpha texture,
    one object instance, an uber surface (diffuse, glossy, specular reflection and transmission in one BSDF) under a checkerboard, a rough-glass panel; a point light, a distant
    light, a constant sky and an emissive quad of 12 triangles: 15 lights, four slices of the light loop."""
    checks = s.add_texture_checkerboard(s.add_texture_constant((0.15, 0.2, 0.6)), s.add_texture_constant((0.8, 0.8, 0.7)), su=6.0, sv=6.0)
    floor = s.add_material_matte_tex(checks)
    glass = s.add_material_glass(kr=(0.9, 0.95, 1.0), kt=(0.95, 0.9, 0.85), eta=1.5)
    rough = s.add_material_glass(kr=(0.8, 0.8, 0.8), kt=(0.9, 0.9, 0.9), uroughness=0.2, vroughness=0.3, eta=1.3)
    mirror = s.add_material_mirror((0.9, 0.8, 0.7))
    veil = s.add_material_none()
    uber = s.add_material_uber(kd=(0.3, 0.2, 0.1), ks=(0.2, 0.2, 0.2), kr=(0.3, 0.3, 0.35), kt=(0.25, 0.3, 0.25), opacity=(0.8, 0.8, 0.8), uroughness=0.15, vroughness=0.15, eta=1.4)
    s.set_material_texture(uber, "Kd", checks)
    matte = s.add_material_matte((0.6, 0.3, 0.2))
    P, idx, UV = _quad((-4, -4, 0), (8, 0, 0), (0, 8, 0))
    s.add_mesh(P, idx, floor, UV=UV)
    P, idx, N, UV = _uv_sphere((-0.9, 0.2, 0.8), 0.8)
    s.add_mesh(P, idx, glass, N=N, UV=UV)
    P, idx, UV = _quad((-3, 2.5, 0), (6, 0, 0), (0, 0.3, 3))
    s.add_mesh(P, idx, mirror, UV=UV)
    P, idx, UV = _quad((-3, 2.2, 0), (3, 0, 0), (0, 0, 3))
    s.add_mesh(P, idx, veil, UV=UV)
    P, idx, UV = _quad((0.6, -0.6, 0.05), (1.6, 0.3, 0), (0, 0.2, 1.6))
    s.add_mesh(P, idx, uber, UV=UV)
    P, idx, UV = _quad((1.0, -1.6, 0.0), (1.4, 0.0, 0), (0, 0.1, 1.2))
    s.add_mesh(P, idx, rough, UV=UV)
    P, idx, UV = _quad((-2.6, -1.2, 0.0), (1.2, 0.2, 0), (0, 0, 1.4), n=2)
    s.add_mesh(P, idx, matte, UV=UV)
    s.set_last_mesh_alpha_textures(alpha=s.add_texture_checkerboard(s.add_texture_constant((0.0,) * 3), s.add_texture_constant((1.0,) * 3), su=3.0, sv=3.0, aa="none"))
    obj = s.object_begin()
    s.add_mesh(R.CUBE_P * 0.3, R.CUBE_IDX, matte)
    s.object_end()
    m = host.compose(host.translate((1.6, 1.2, 0.5)), host.rotate(30.0, (0, 0, 1)))
    s.add_instance(obj, m, host.invert(m))
    s.add_light_point((30.0, 28.0, 25.0), (-2.0, -2.0, 4.0))
    if not one_light: s.add_light_distant((0.8, 0.8, 0.9), host.distant_direction(R._ident(), (3.0, -2.0, 5.0), (0.0, 0.0, 0.0)))
    if not one_light: s.add_light_infinite((0.25, 0.3, 0.4))
    P, idx, UV = _quad((-0.5, -0.5, 4.0), (0.9, 0, 0), (0, 0.6, 0), n=1)
    P = np.concatenate([P + np.float32([k * 0.05, 0, 0]) for k in range(6)]); idx = np.concatenate([idx + 4 * k for k in range(6)]).astype(np.uint32)   # six quads on top of each other's edge: 12 triangles
    first = -1 if one_light else s.add_light_diffuse_area((4.0, 4.0, 3.5), 12)
    s.add_mesh(P, idx, matte, first_area_light=first, reverse_orientation=True)
    _, c2w = host.look_at([0.4, -6.0, 2.6], [0.0, 0.5, 0.8], [0, 0, 1])
    s.set_camera_perspective(host.perspective_raster_to_camera(42.0, res, res), c2w, lens_radius=0.03, focal_distance=6.0)
    cb, table, sb = host.film_box(res, res)
    s.set_film(res, res, cb, (0.5, 0.5), table)
    s.set_sampler(cf.SOBOL if sampler == "sobol" else cf.HALTON, spp, sb)
    if sampler == "sobol":
        s.set_sobol_tables(*cf.sobol_fixture())
    s.build_accel(0, 4)


# (sampler, one light only).  The Sobol tables the repository holds (tests/golden/sobol_subset.npz) have 48 dimensions: the 15-light scene fits them at max_depth 1
# (5 + 30 dimensions), its one-light form up to max_depth 3 (5 + 7 * 2 + 3 * 4 = 31); beyond that the oracle itself runs out of dimensions and returns UNSUPPORTED.
VARIANTS = [("halton", False, 1), ("halton", False, 2), ("halton", False, 3), ("halton", False, 5), ("sobol", False, 1), ("sobol", True, 2), ("sobol", True, 3)]


@pytest.fixture(scope="module")
def recursion_pair(host):
    pairs = {}
    for key in sorted({(s, o) for s, o, _ in VARIANTS}):
        prod, orc = pbrt_hip.Scene(), OracleScene()
        recursion_scene(prod, host, key[0], one_light=key[1]); recursion_scene(orc, host, key[0], one_light=key[1])
        pairs[key] = (prod, orc, {})
    yield pairs
    for prod, orc, _ in pairs.values():
        prod.close(); orc.close()


def _oracle_film(pair, depth):
    prod, orc, cache = pair
    if depth not in cache:
        cache[depth] = oracle_whitted(orc, max_depth=depth)
    return cache[depth]


@pytest.mark.parametrize("sampler,one_light,depth", VARIANTS)
def test_recursion_scene_equals_the_oracle(recursion_pair, sampler, one_light, depth):
    pair = recursion_pair[(sampler, one_light)]
    got = pair[0].render_whitted(max_depth=depth)
    assert_same_film(got, _oracle_film(pair, depth), f"{sampler} depth {depth}")
    assert got[2].shadow_rays > 0 and (depth == 1 or got[2].regular_rays > got[2].camera_rays)


def test_recursion_is_seen_to_run(recursion_pair):
    d1 = recursion_pair[("halton", False)][0].render_whitted(max_depth=1)[0]
    d2 = recursion_pair[("halton", False)][0].render_whitted(max_depth=2)[0]
    assert (d1 != d2).any(-1).mean() > 0.05


def test_recursion_scene_in_chunks_and_tile_parts(recursion_pair, monkeypatch):
    pair = recursion_pair[("halton", False)]
    prod, orc, _ = pair
    want = _oracle_film(pair, 5)
    monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(48 * 48 * 3 // 2))   # four chunks of one sample per pixel
    assert_same_film(prod.render_whitted(max_depth=5), want, "chunked")
    monkeypatch.delenv("PBRT_HIP_MAX_PATHS")
    acc = np.zeros_like(want[0]); accw = np.zeros_like(want[1]); rays = [0, 0, 0]
    for part in range(2):
        got = prod.render_whitted(max_depth=5, tile_part=part, tile_parts=2)
        assert_same_film(got, oracle_whitted(orc, max_depth=5, tile_part=part, tile_parts=2), f"part {part}")
        acc += got[0]; accw += got[1]
        rays = [a + b for a, b in zip(rays, (got[2].camera_rays, got[2].regular_rays, got[2].shadow_rays))]
    assert np.array_equal(accw, want[1]) and np.array_equal(acc.view(np.uint32), want[0].view(np.uint32))   # the parts' tiles are disjoint: the sums are exact
    assert rays == [want[2].camera_rays, want[2].regular_rays, want[2].shadow_rays]


def test_chunk_oom_retry_halves_the_chunk_and_leaves_the_workspace_usable(recursion_pair, monkeypatch):
    """The Whitted driver's side of tests/test_render_gpu.py's retry test (the loop is shared, chunk_plan.h): two forced out-of-memory attempts take the 4 spp to chunks of 1,
    the film does not change and no error text survives; a third exhausts the halving and the call fails; the buffers released on the way are allocated again by the next call."""
    prod = recursion_pair[("halton", False)][0]
    want = prod.render_whitted(max_depth=5)
    monkeypatch.setenv("PBRT_HIP_TEST_CHUNK_OOM", "2")
    assert_same_film(prod.render_whitted(max_depth=5), want, "4 -> 2 -> 1 spp")
    assert prod.last_error() == ""
    monkeypatch.setenv("PBRT_HIP_TEST_CHUNK_OOM", "3")   # 4 -> 2 -> 1 spp and still failing: the call gives up with ERR_OOM
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        prod.render_whitted(max_depth=5)
    assert e.value.code == pbrt_hip.ERR_OOM
    monkeypatch.delenv("PBRT_HIP_TEST_CHUNK_OOM")
    assert_same_film(prod.render_whitted(max_depth=5), want, "after the call that gave up")


# ---- 3. the reference's own pixels --------------------------------------------------------------------------------------------------------------------------------
PIXELS = [(n, s) for n, s in WHITTED if n not in ("samplers_random", "lights_diffuse")] + [("dof", 128), ("six:fbm", 128), ("six:2d-checkerboard", 128), ("mappings", 128)]


@pytest.mark.parametrize("name,spp", PIXELS, ids=[n for n, _ in PIXELS])
def test_device_whitted_reproduces_the_references_render_pixel_for_pixel(host, name, spp):
    """The device equals the oracle in libm mode 1, not the glibc one the oracle tests of tests/test_reference_renders.py run in, so the mode-1 oracle was rendered on the CPU for
    every scene first and held against the reference's PNG (identical pixels, pixels within one level, largest difference):
      triangles_alpha_mask, lights_point, lights_spot, lights_goniometric, lights_distant, samplers_halton, samplers_sobol   1.0, 1.0, 0
      lights_infinite_no_map 0.9999625, 1.0, 1      cameras_perspective 0.9999, 1.0, 1         cameras_orthographic 0.99988125, 0.99999375, 2
      cameras_environment 0.99995, 0.99999375, 5    objects_instances 0.999925, 1.0, 1         materials_bump 0.9992375, 0.99999375, 3
      depth-of-field crop 0.99983668, 0.99998744, 2 six shapes fbm 0.99994709, 1.0, 1          six shapes 2d-checkerboard 0.99998125, 1.0, 1
      2d-mappings 0.99998125, 1.0, 1
    Mode 1 meets the threshold the oracle's own test asserts for every one of them, so those thresholds are asserted here unchanged."""
    with pbrt_hip.Scene() as s, generic_adders():
        if name.startswith("samplers_"): info = R.samplers_scene(s, host, name.split("_")[1], spp=spp)
        elif name == "dof": info = R.cameras_depth_of_field(s, host, spp=spp, crop=(0.25, 0.75, 0.3, 0.8))
        elif name.startswith("six:"): info = R.textures_six_shapes(s, host, name[4:], spp=spp)
        elif name == "mappings": info = R.textures_2d_mappings(s, host, spp=spp)
        else: info = getattr(R, name)(s, host, spp=spp)
        xyz, wt, _ = s.render_whitted(max_depth=5)
        mine = R.to_8bit(s.film_to_rgb(xyz, wt))
    ref = R.reference_render(info["render"])
    if name == "dof":
        cb = info["crop"]; ref = ref[cb[1]:cb[3], cb[0]:cb[2]]
    if name.startswith("six:") and ref.shape[0] != 400:
        r0, r1, c0, c1 = R.TEX_CROP; mine = mine[r0:r1, c0:c1]
    d = np.abs(mine.astype(np.int32) - ref.astype(np.int32)).max(-1)
    same, le1, dmax = (d == 0).mean(), (d <= 1).mean(), d.max()
    print(name, same, le1, dmax)
    if name == "dof": assert same >= 0.999 and le1 >= 0.9999 and dmax <= 4, (same, le1, dmax)
    elif name.startswith("six:") or name == "mappings": assert same >= 0.9995 and dmax <= 2, (same, dmax)
    else: assert same >= 0.999 and le1 >= 0.9999 and dmax <= 6, (same, le1, dmax)


# ---- 4. the front end -----------------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_renders_integrator_whitted_like_the_reference(tmp_path):
    from test_reference_renders_gpu import SCENE_TEXTS
    make, spp, _ = SCENE_TEXTS["lights_spot"]
    text = make(128).replace('Integrator "path" "integer maxdepth" 1\n', 'Integrator "whitted"\n')
    assert 'Integrator "whitted"\n' in text
    (tmp_path / "scene.pbrt").write_text(text)
    r = subprocess.run([ds.RENDER_BIN, "--quiet", str(tmp_path / "scene.pbrt")], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = ds.read_pfm(str(tmp_path / "out.pfm"))
    d = np.abs(R.to_8bit(img).astype(np.int32) - R.reference_render("lights_spot").astype(np.int32)).max(-1)
    assert (d == 0).mean() >= 0.999 and (d <= 1).mean() >= 0.9999 and d.max() <= 6, ((d == 0).mean(), d.max())


# ---- 5. a closed form ------------------------------------------------------------------------------------------------------------------------------------------------
KR = (0.97, 0.85, 0.6)


def test_mirror_corridor_per_pixel(host):
    """tests/closed_form.py, form E: every pixel is exactly Le kr^N if its ray escapes after N reflections and N < max_depth (the N-th mirror vertex sits at depth N - 1 and
    reflects only if depth + 1 < max_depth), else 0 — under Whitted per sample, with nothing stochastic in it."""
    N, ok = cf.corridor_rays(host, pbrt_hip.Scene, KR, 24)
    assert ok.mean() > 0.9 and len(np.unique(N[ok])) >= 4
    with pbrt_hip.Scene() as s:
        cf.mirror_corridor(host, cf.LE, KR, res=24)(s)
        for D in range(1, int(N.max()) + 3):
            xyz, wt, _ = s.render_whitted(max_depth=D)
            want = np.where((N < D)[..., None], np.asarray(cf.LE, np.float64) * np.asarray(KR, np.float64) ** N[..., None], 0.0)
            np.testing.assert_allclose(s.film_to_rgb(xyz, wt)[ok], want[ok], rtol=1e-5, atol=1e-7, err_msg=f"D={D}")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def _raw_whitted(s, max_depth):
    h, w = s.film_shape
    xyz = np.full((h, w, 3), np.nan, np.float32); wt = np.full((h, w), -7.0, np.float32)
    pb = np.ascontiguousarray(s.sample_bounds, dtype=np.int32)
    fp = C.POINTER(C.c_float)
    rc = s.b.fn("render_whitted")(s.h, max_depth, pb.ctypes.data_as(C.POINTER(C.c_int)), 16, 0, 1, xyz.ctypes.data_as(fp), wt.ctypes.data_as(fp), None)
    return rc, xyz, wt


def test_refusals_leave_the_handle_usable(recursion_pair):
    prod, orc, _ = pair = recursion_pair[("sobol", True)]   # one light, specular reflection and transmission, 48 Sobol dimensions: 5 + 31 * 2 + 15 * 4 = 127 at max_depth 5

    def still_renders():
        assert_same_film(prod.render_whitted(max_depth=2), _oracle_film(pair, 2), "whitted after a refusal")
        orc.b.lib.oracle_set_integrator(orc.h, 0)
        set_libm_mode(1)
        try:
            oxyz, owt, ost, _ = orc.render_path_ex(max_depth=2, light_strategy=0)
        finally:
            set_libm_mode(0)
        assert_same_film(prod.render_path(max_depth=2, light_strategy=0), (oxyz, owt, ost), "path after a refusal")

    rc, xyz, wt = _raw_whitted(prod, 17)
    assert rc == pbrt_hip.ERR_INVALID_ARG and np.isnan(xyz).all() and (wt == -7.0).all()
    still_renders()
    rc, xyz, wt = _raw_whitted(prod, 5)   # beyond the tables
    assert rc == pbrt_hip.ERR_UNSUPPORTED and np.isnan(xyz).all() and (wt == -7.0).all(), prod.last_error()
    assert "Sobol" in prod.last_error()
    still_renders()


def test_multi_device_handle_is_refused(host):
    with pbrt_hip.Scene(devices=[0, 0]) as s:
        cf.mirror_corridor(host, cf.LE, KR, res=16)(s)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.render_whitted(max_depth=2)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
        xyz, wt, _ = s.render_path(max_depth=2)   # the handle still renders what it supports
        assert np.isfinite(xyz).all() and (wt > 0).all()
