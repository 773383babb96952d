"""PathIntegrator::li on the device against closed-form radiance (tests/closed_form.py), at sizes the oracle cannot reach: 64 x 64
tessellated faces (49 152 lights), 512^2 frames, forced chunking, tile parts, the Halton depth limit, the null-skip cap.  Each
new scene shape is also held bit for bit against the oracle on a small crop.  What a mean cannot see (eta_scale, where RR starts, q, the order of
the sampler's dimensions) is held sample by sample against the float64 replay of tests/li_replay.py."""

import numpy as np
import pytest

import closed_form as cf
import li_replay as lr
import pbrt_hip
from oracle_binding import OracleScene, set_libm_mode

LE, RHO_RGB, HALTON_MAX_DEPTH = cf.LE, cf.RHO_RGB, cf.HALTON_MAX_DEPTH

pytestmark = pytest.mark.gpu


def render(cap, **kw):
    s = pbrt_hip.Scene()
    cap(s)
    xyz, wt, st = s.render_path(**kw)
    return s.film_to_rgb(xyz, wt), st, s


def assert_crop_bit_exact(cap, crop=(0, 0, 8, 8), **kw):
    prod = pbrt_hip.Scene(); orc = OracleScene()
    cap(prod); cap(orc)
    set_libm_mode(1)
    try:
        oxyz, owt, ost, _ = orc.render_path_ex(pixel_bounds=crop, **kw)
    finally:
        set_libm_mode(0)
    gxyz, gwt, gst = prod.render_path(pixel_bounds=crop, **kw)
    assert (gst.camera_rays, gst.regular_rays, gst.shadow_rays) == (ost.camera_rays, ost.regular_rays, ost.shadow_rays), (gst.as_dict(), ost.as_dict())
    assert np.array_equal(gwt.view(np.uint32), owt.view(np.uint32))
    nb = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    assert nb == 0, f"{nb} pixels differ from the oracle"


@pytest.mark.parametrize("strategy", [0, 1, 2])
@pytest.mark.parametrize("D", [5, 64])
def test_furnace_at_size(host, D, strategy):
    """Form A, 512^2 @ 64 spp, 64 x 64 shared-vertex faces (49 152 lights), per-channel rho, RR on.  Light strategy 2 runs on 4 x 4
    faces (96 lights) instead: SpatialLightDistribution evaluates every light for every voxel a path touches, and 49 152 lights
    times the cube's 64^3 voxels is beyond a test's budget.  At D = 64 depth +- 1 differs by 0.4 0.95^65 (0.2 %), below what a
    frame can resolve: there the power check covers the other wrong answers only."""
    grid = 64 if strategy < 2 else 4
    cap, n_lights = cf.emissive_furnace(host, LE, RHO_RGB, res=512, spp=64, grid=grid)
    assert n_lights == 6 * 2 * grid * grid
    rgb, st, _ = render(cap, max_depth=D, light_strategy=strategy)
    assert st.camera_rays == 512 * 512 * 64
    w = cf.furnace_wrongs(LE, RHO_RGB, D, n_lights)
    if D == 64:
        w = {k: v for k, v in w.items() if not k.startswith("depth")}
    cf.assert_mean(rgb, cf.furnace_expect(LE, RHO_RGB, D), wrongs=w, se_target=0.005, label=f"furnace 512^2 D={D} strategy={strategy}")


@pytest.mark.parametrize("mode", ["general_kernel", "chunks", "tile_parts"])
def test_furnace_paths_through_the_driver(host, mode, monkeypatch):
    """The same closed form through shade_kernel<true, *> (an unused plastic material turns the general-BSDF kernel on), through
    several path-pool chunks (PBRT_HIP_MAX_PATHS), and as 3 tile parts summed."""
    D, res, spp = 5, 256, 32
    cap, n_lights = cf.emissive_furnace(host, LE, RHO_RGB, res=res, spp=spp, grid=8, unused_plastic=(mode == "general_kernel"))
    if mode == "chunks":
        monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(res * res * 6))   # 6 of 32 samples per pixel per chunk: 6 chunks, the last one partial
    s = pbrt_hip.Scene(); cap(s)
    if mode == "tile_parts":
        xyz = np.zeros((res, res, 3), np.float32); wt = np.zeros((res, res), np.float32); rays = 0
        for p in range(3):
            x, w, st = s.render_path(max_depth=D, light_strategy=1, tile_part=p, tile_parts=3)
            xyz += x; wt += w; rays += st.camera_rays
        assert rays == res * res * spp
    else:
        xyz, wt, st = s.render_path(max_depth=D, light_strategy=1)
        assert st.camera_rays == res * res * spp
    rgb = s.film_to_rgb(xyz, wt)
    cf.assert_mean(rgb, cf.furnace_expect(LE, RHO_RGB, D), wrongs=cf.furnace_wrongs(LE, RHO_RGB, D, n_lights), se_target=0.005, label=f"furnace {mode}")


def test_white_furnace_at_halton_depth_limit(host):
    """Form B at D = 123, the deepest Halton path check_render_args accepts (5 + 8 (D + 1) < 1000): E = 124 Le, and enough samples
    to tell it from 123 Le and 125 Le.  D = 124 is refused with ERR_UNSUPPORTED (the reference and the oracle still render it)."""
    D = HALTON_MAX_DEPTH
    cap, n_lights = cf.emissive_furnace(host, LE, 1.0, res=256, spp=16)
    rgb, _, s = render(cap, max_depth=D, rr_threshold=0.0)
    cf.assert_mean(rgb, cf.furnace_expect(LE, 1.0, D), wrongs=cf.furnace_wrongs(LE, 1.0, D, n_lights), se_target=5e-4, label="white furnace D=123")
    rc, xyz, wt, st = cf.raw_render(s, D + 1, [0, 0, 256, 256])
    assert rc == pbrt_hip.ERR_UNSUPPORTED, (rc, s.last_error())
    assert np.isnan(xyz).all() and st.camera_rays == 0


@pytest.mark.parametrize("D", [0, 1, 5])
def test_null_veil_at_size(host, D):
    rgb, _, _ = render(cf.null_veil(host, LE, 0.8, res=256, spp=8), max_depth=D)
    want = np.zeros(3) if D == 0 else np.asarray(LE)
    np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(want, (256 * 256, 3)), rtol=1e-5, atol=1e-7)


def test_null_skip_cap(host):
    """wavefront.hip runs max_depth + 1 rounds plus up to kMaxNullSkips = 1024 more while paths remain, and refuses a path still
    alive in the last one: at max_depth 1 a camera ray that crosses K 'none' quads and ends on the (black) emitter uses K + 1
    rounds, so K = 1024 is the largest stack rendered (L = Le exactly) and K = 1025 is ERR_UNSUPPORTED, not a truncated path."""
    rgb, _, _ = render(cf.null_stack(host, LE, 1024, res=8, spp=1), max_depth=1)
    np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(LE, (64, 3)), rtol=1e-5)
    s = pbrt_hip.Scene(); cf.null_stack(host, LE, 1025, res=8, spp=1)(s)
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        s.render_path(max_depth=1)
    assert e.value.code == pbrt_hip.ERR_UNSUPPORTED


@pytest.mark.parametrize("tilt", [0.0, 40.0])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_glass_slab_at_size(host, D, tilt):
    rgb, _, _ = render(cf.glass_slab(host, LE, tilt_deg=tilt, res=512, spp=16), max_depth=D)
    wrongs = {"depth D-1": cf.glass_slab_expect(LE, D - 1, tilt_deg=tilt), "no emission after specular bounces": np.zeros(3)}
    if D >= 2:
        wrongs["1/eta^2 on entry only"] = cf.glass_slab_expect(LE, D, tilt_deg=tilt, entry_only=True)
    if D <= 2:   # from D = 3 on, D + 1 adds F^(D-1) (1-F)^2, below the noise
        wrongs["depth D+1"] = cf.glass_slab_expect(LE, D + 1, tilt_deg=tilt)
    cf.assert_mean(rgb, cf.glass_slab_expect(LE, D, tilt_deg=tilt), wrongs=wrongs, se_target=0.02, label=f"glass slab 512^2 D={D} tilt={tilt}")


def test_glass_exact_and_radiance_factor_at_size(host):
    for tilt in (0.0, 40.0):
        rgb, _, _ = render(cf.glass_slab(host, LE, tilt_deg=tilt, res=512, spp=4), max_depth=64, rr_threshold=0.0)
        np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(LE, (512 * 512, 3)), rtol=1e-5)
    rgb, _, _ = render(cf.glass_over_emitter(host, LE, res=512, spp=8), max_depth=3)
    cf.assert_mean(rgb, cf.glass_over_emitter_expect(LE, 3), wrongs={"no (eta_i/eta_t)^2 factor": cf.glass_over_emitter_expect(LE, 3, factor=1.0)},
                   se_target=0.005, label="glass over emitter 512^2")


def test_sobol_within_fixture(host):
    """Sobol inside the fixture's range (48 dimensions: D <= 4; 9 VdC matrices: resolution <= 512): form A's mean; beyond it the
    device refuses before launching anything (sentinel outputs untouched)."""
    s = cf.sobol_scene(host, 256, pbrt_hip.Scene)
    xyz, wt, st = s.render_path(max_depth=4, light_strategy=0)
    assert st.camera_rays == 256 * 256 * 4
    cf.assert_mean(s.film_to_rgb(xyz, wt), cf.furnace_expect(LE, 0.5, 4), wrongs={}, se_target=0.01, label="sobol furnace")
    for res, D in ((256, 5), (1024, 1)):
        s = cf.sobol_scene(host, res, pbrt_hip.Scene)
        rc, xyz, wt, st = cf.raw_render(s, D, [0, 0, 4, 4])
        assert rc == pbrt_hip.ERR_UNSUPPORTED, (rc, s.last_error())
        assert np.isnan(xyz).all() and (wt == -7.0).all() and st.camera_rays == 0


KR = (0.97, 0.85, 0.6)


def test_mirror_corridor_at_size(host):
    """Form E at 128^2: exact per pixel at every depth with RR off; with RR on, N <= 4 exact per pixel and the mean of every
    group of equal N >= 5 equal to Le kr^N (and away from the answer without RR's 1/(1-q) weight)."""
    res = 128
    N, ok = cf.corridor_rays(host, pbrt_hip.Scene, KR, res)
    assert ok.mean() > 0.9 and len(np.unique(N[ok])) >= 4, np.unique(N[ok], return_counts=True)
    s = pbrt_hip.Scene(); cf.mirror_corridor(host, LE, KR, res=res)(s)
    for D in range(0, int(N.max()) + 2):
        xyz, wt, _ = s.render_path(max_depth=D, rr_threshold=0.0)
        np.testing.assert_allclose(s.film_to_rgb(xyz, wt)[ok], cf.mirror_expect(LE, KR, N, D)[ok], rtol=1e-5, atol=1e-7, err_msg=f"D={D}")
    D = int(N.max()) + 1
    rgb, _, _ = render(cf.mirror_corridor(host, LE, KR, res=res, spp=64), max_depth=D)
    E = cf.mirror_expect(LE, KR, N, D)
    short = ok & (N <= 4)
    np.testing.assert_allclose(rgb[short], E[short], rtol=1e-5, atol=1e-7)
    for n in [n for n in np.unique(N[ok]) if n >= 5]:
        sel = ok & (N == n)
        En = E[sel][0]
        cf.assert_mean(rgb[sel], En, wrongs={"RR weight 1/(1-q) dropped": En * cf.mirror_rr_survival(KR, n)}, se_target=0.005,
                       label=f"mirror corridor 128^2 N={n}")


@pytest.mark.parametrize("shape", ["furnace_grid", "furnace_lights_tex", "veil", "null_stack", "glass_slab", "glass_tilt", "glass_emitter", "mirror_corridor"])
def test_new_scene_shapes_bit_exact(host, shape):
    caps = {
        "furnace_grid": (lambda: cf.emissive_furnace(host, LE, RHO_RGB, res=32, spp=4, grid=4)[0], dict(max_depth=6, light_strategy=0)),
        "furnace_lights_tex": (lambda: cf.emissive_furnace(host, LE, 0.8, res=32, spp=4, extra_lights=True, textured=True)[0], dict(max_depth=5, light_strategy=1)),
        "veil": (lambda: cf.null_veil(host, LE, 0.8, res=32, spp=4), dict(max_depth=4)),
        "null_stack": (lambda: cf.null_stack(host, LE, 8), dict(max_depth=1)),
        "glass_slab": (lambda: cf.glass_slab(host, LE, res=32, spp=4), dict(max_depth=8)),
        "glass_tilt": (lambda: cf.glass_slab(host, LE, tilt_deg=40.0, res=32, spp=4), dict(max_depth=8)),
        "glass_emitter": (lambda: cf.glass_over_emitter(host, LE, res=32, spp=4), dict(max_depth=3)),
        "mirror_corridor": (lambda: cf.mirror_corridor(host, LE, KR, res=32, spp=4), dict(max_depth=6)),
    }
    mk, kw = caps[shape]
    assert_crop_bit_exact(mk(), **kw)


# ---- the replay, sample by sample (test_closed_form_li.py::test_li_replay proves each case's power on the CPU) --------------------

def _replay_prediction(host, case):
    s = case.scene(host, pbrt_hip.Scene)
    inputs = case.inputs(host, s)     # the device's camera rays and the device's sampler_value_batch
    pred = case.predict(inputs)
    assert float((pred["excluded"] & inputs[3]).mean()) <= lr.EXCLUSION_CAP
    return s, pred


@pytest.mark.parametrize("case", lr.CASES, ids=repr)
def test_li_replay_on_device(host, case):
    """Every pixel of the device's film equals the float64 replay of its samples (zeros exactly, the rest within lr.TOL), and the
    scene's 8 x 8 crop equals the oracle's bit for bit."""
    s, pred = _replay_prediction(host, case)
    xyz, wt, st = s.render_path(max_depth=case.max_depth, rr_threshold=case.rr_threshold)
    assert st.camera_rays == case.res * case.res * case.spp
    rgb = s.film_to_rgb(xyz, wt)
    print(f"{case}: relative deviation {lr.deviation(rgb, pred)[0]:.3g}")
    lr.assert_film_matches(rgb, pred, lr.TOL, label=str(case))
    assert_crop_bit_exact(case.capture(host), max_depth=case.max_depth, rr_threshold=case.rr_threshold)


@pytest.mark.parametrize("mode", ["chunks", "tile_parts"])
def test_li_replay_four_materials_through_the_driver(host, mode, monkeypatch):
    """The stack of four uber materials (four shade-queue keys live in one round) at 4 spp through several path-pool chunks
    (3 samples per pixel, then 1) and as 3 tile parts summed: the same film, sample for sample."""
    case = next(c for c in lr.CASES if c.name == "stack_four_materials_spp4")
    if mode == "chunks":
        monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(case.res * case.res * 3))
    s, pred = _replay_prediction(host, case)
    kw = dict(max_depth=case.max_depth, rr_threshold=case.rr_threshold)
    if mode == "tile_parts":
        xyz = np.zeros((case.res, case.res, 3), np.float32); wt = np.zeros((case.res, case.res), np.float32); rays = 0
        for p in range(3):
            x, w, st = s.render_path(tile_part=p, tile_parts=3, **kw)
            xyz += x; wt += w; rays += st.camera_rays
    else:
        xyz, wt, st = s.render_path(**kw)
        rays = st.camera_rays
    assert rays == case.res * case.res * case.spp
    lr.assert_film_matches(s.film_to_rgb(xyz, wt), pred, lr.TOL, label=f"{case} {mode}")
