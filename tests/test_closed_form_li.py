"""PathIntegrator::li (integrators/src/path.rs:103-284) on the CPU oracle against closed-form radiance (tests/closed_form.py).

The bit-exact suite holds the device to the oracle; these tests hold the oracle to physics written independently in float64, so
a mistake both sides share (depth cut-off, RR weight, MIS halves, emission after specular bounces, the (eta_i/eta_t)^2 radiance
factor, the null-BSDF skip, the light-choice pdf) turns a test red.  Every statistical case also checks that it could tell the
right answer from the plausible wrong ones (closed_form.assert_mean).

What a mean cannot see — eta_scale, the bounce at which Russian roulette starts, the value of q, the order in which a path consumes
sampler dimensions — is held sample by sample by the float64 replay of tests/li_replay.py (section F below)."""
import numpy as np
import pytest

import closed_form as cf
import li_replay as lr
import pbrt_hip
from oracle_binding import OracleScene

LE, RHO_RGB, HALTON_MAX_DEPTH = cf.LE, cf.RHO_RGB, cf.HALTON_MAX_DEPTH


def render(cap, **kw):
    s = OracleScene()
    cap(s)
    xyz, wt, st, _ = s.render_path_ex(**kw)
    return s.film_to_rgb(xyz, wt), st, s


# ---- A: emissive furnace -------------------------------------------------------------------------------------------------

# (rho, D): sizes where the oracle has power against depth D +- 1 at 48 x 48 x 32 samples; the GPU file covers the rest at size
FURNACE_CASES = [(0.5, 1), (0.5, 2), (0.5, 3), (0.8, 4), (0.8, 5), (0.8, 6), (RHO_RGB, 5), (RHO_RGB, 8)]


@pytest.mark.parametrize("rr", [1.0, 0.0])
@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("rho,D", FURNACE_CASES)
def test_furnace_mean(host, rho, D, strategy, rr):
    """Form A: E = Le sum_{k=0..D} rho^k per channel, with and without Russian roulette (which keeps the mean)."""
    cap, n_lights = cf.emissive_furnace(host, LE, rho, res=48, spp=32)
    rgb, st, _ = render(cap, max_depth=D, light_strategy=strategy, rr_threshold=rr)
    assert st.camera_rays == 48 * 48 * 32
    cf.assert_mean(rgb, cf.furnace_expect(LE, rho, D), wrongs=cf.furnace_wrongs(LE, rho, D, n_lights), se_target=0.01,
                   label=f"furnace rho={rho} D={D} strategy={strategy} rr={rr}")


@pytest.mark.parametrize("opts", [dict(grid=8), dict(extra_lights=True), dict(textured=True), dict(grid=4, extra_lights=True, textured=True)],
                         ids=["grid8", "unseen_lights", "imagemap_kd", "all"])
@pytest.mark.parametrize("strategy", [0, 1])
def test_furnace_variants(host, opts, strategy):
    """Tessellated shared-vertex faces (a crack would leak), a point light and an infinite light that are always occluded (the
    light-choice pdf changes, the mean must not), Kd through the image-map texture pass: the closed form is unchanged."""
    rho, D = 0.8, 1   # finer faces make light sampling noisier: a depth where D +- 1 stays well apart at this size
    cap, n_lights = cf.emissive_furnace(host, LE, rho, res=48, spp=16, **opts)
    rgb, _, _ = render(cap, max_depth=D, light_strategy=strategy)
    cf.assert_mean(rgb, cf.furnace_expect(LE, rho, D), wrongs=cf.furnace_wrongs(LE, rho, D, n_lights), se_target=0.03,
                   label=f"furnace {opts} strategy={strategy}")


@pytest.mark.parametrize("rho,D", [(0.8, 1), (RHO_RGB, 3)])
def test_furnace_spatial_strategy(host, rho, D):
    """Light strategy 2 (SpatialLightDistribution) is slow on the oracle: a smaller frame."""
    cap, n_lights = cf.emissive_furnace(host, LE, rho, res=32, spp=32, extra_lights=True)
    rgb, _, _ = render(cap, max_depth=D, light_strategy=2)
    cf.assert_mean(rgb, cf.furnace_expect(LE, rho, D), wrongs=cf.furnace_wrongs(LE, rho, D, n_lights), se_target=0.03,
                   label=f"furnace spatial D={D}")


def test_furnace_depth0_is_le_and_counters(host):
    cap, _ = cf.emissive_furnace(host, LE, 0.8, res=16, spp=4)
    rgb, st, _ = render(cap, max_depth=0)
    np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(LE, (256, 3)), rtol=1e-5)
    assert st.camera_rays == 16 * 16 * 4 and st.regular_rays == st.camera_rays and st.shadow_rays == 0


@pytest.mark.parametrize("D", [0, 1, 3])
def test_furnace_reversed_is_black_and_two_sided_restores(host, D):
    """reverse_orientation turns every one-sided wall outward: nothing inside emits, every pixel is 0 at every D — up to the
    f32 rounding of a light sample on the hit point's own face (wi in the plane, |cos| ~ 1e-8 of either sign: contributions
    ~1e-12).  two_sided=True emits on both sides: form A again."""
    cap, _ = cf.emissive_furnace(host, LE, 0.8, res=16, spp=4, reverse=True)
    rgb, _, _ = render(cap, max_depth=D)
    assert float(np.abs(rgb).max()) < 1e-9, float(np.abs(rgb).max())
    cap, n_lights = cf.emissive_furnace(host, LE, 0.8, res=48, spp=16, reverse=True, two_sided=True)
    rgb, _, _ = render(cap, max_depth=D)
    if D == 0:
        np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(LE, (48 * 48, 3)), rtol=1e-5)
    else:
        cf.assert_mean(rgb, cf.furnace_expect(LE, 0.8, D), wrongs=cf.furnace_wrongs(LE, 0.8, D, n_lights), se_target=0.01,
                       label=f"two-sided reversed D={D}")


# ---- B: white furnace at the depth limit ---------------------------------------------------------------------------------

def test_white_furnace_at_halton_depth_limit(host):
    """Form B: rho = 1, RR off: every bounce adds Le, E = (D + 1) Le, at the deepest path the device accepts for Halton.  The
    reference itself has no such check: HaltonSampler asserts only dim <= 1000, and a path of depth D draws dimensions up to
    8 D + 4, so D = 124 still renders there (and here, on the oracle) with E = 125 Le; the device's bound is one bounce stricter
    (test_closed_form_li_gpu.py checks its refusal).  At this size the oracle cannot tell D from D +- 1 (0.8 %); the GPU file does."""
    D = HALTON_MAX_DEPTH
    for d in (D, D + 1):
        cap, n_lights = cf.emissive_furnace(host, LE, 1.0, res=8, spp=8)
        rgb, st, _ = render(cap, max_depth=d, rr_threshold=0.0)
        w = cf.furnace_wrongs(LE, 1.0, d, n_lights)
        cf.assert_mean(rgb, cf.furnace_expect(LE, 1.0, d), wrongs={k: w[k] for k in ("Le at every hit", "light-choice factor dropped")},
                       se_target=0.01, label=f"white furnace D={d}")


# ---- C: null-BSDF veil ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [0, 1, 2, 5, 9])
def test_null_veil(host, D):
    """Form C (closed_form.null_veil): L = 0 at D = 0 (the depth cut-off precedes the null skip, path.rs:135-150), L = Le exactly
    for D >= 1, every sample."""
    rgb, st, _ = render(cf.null_veil(host, LE, 0.8, res=12, spp=8), max_depth=D)
    want = np.zeros(3) if D == 0 else np.asarray(LE)
    np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(want, (144, 3)), rtol=1e-5, atol=1e-7)
    assert st.camera_rays == 12 * 12 * 8


@pytest.mark.parametrize("K", [1, 7, 40])
def test_null_stack(host, K):
    rgb, _, _ = render(cf.null_stack(host, LE, K), max_depth=1)
    np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(LE, (64, 3)), rtol=1e-5)


# ---- D: glass ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tilt", [0.0, 40.0])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_glass_slab(host, D, tilt):
    """Form D: E = Le sum_{k=1..D} P_k (closed_form.glass_slab_expect).  RR keeps the mean; eta_scale does not even move here: glass builds
    its BSDF without an eta (glass.rs:109), so BSDF::eta is 1 (test_li_replay's glass cases pin that per sample)."""
    rgb, _, _ = render(cf.glass_slab(host, LE, tilt_deg=tilt, res=24, spp=32), max_depth=D)
    E = cf.glass_slab_expect(LE, D, tilt_deg=tilt)
    wrongs = {"depth D-1": cf.glass_slab_expect(LE, D - 1, tilt_deg=tilt), "depth D+1": cf.glass_slab_expect(LE, D + 1, tilt_deg=tilt),
              "no emission after specular bounces": np.zeros(3)}
    if D >= 2:   # at D = 1 no path has been inside the glass
        wrongs["1/eta^2 on entry only"] = cf.glass_slab_expect(LE, D, tilt_deg=tilt, entry_only=True)
    if D >= 3:   # D+1 adds F^(D-1)(1-F)^2, below the noise from here on; D - 1 stays far
        del wrongs["depth D+1"]
    cf.assert_mean(rgb, E, wrongs=wrongs, se_target=0.1, label=f"glass slab D={D} tilt={tilt}")


def test_glass_slab_exact(host):
    """D = 0: nothing (the first hit is glass, which emits nothing).  D = 64, RR off: every path escapes with beta = 1, L = Le."""
    rgb, _, _ = render(cf.glass_slab(host, LE, res=16, spp=4), max_depth=0)
    assert np.all(rgb == 0.0)
    for tilt in (0.0, 40.0):
        rgb, _, _ = render(cf.glass_slab(host, LE, tilt_deg=tilt, res=16, spp=8), max_depth=64, rr_threshold=0.0)
        np.testing.assert_allclose(rgb.reshape(-1, 3), np.broadcast_to(LE, (256, 3)), rtol=1e-5)


@pytest.mark.parametrize("D", [1, 4])
def test_glass_over_emitter_radiance_factor(host, D):
    """Form D2: the emitter seen through one refraction carries (1 - F) / eta^2 — the (eta_i/eta_t)^2 factor of FresnelSpecular's
    transmission in radiance mode, which cancels on any path that leaves the slab of form D and so needs this case."""
    rgb, _, _ = render(cf.glass_over_emitter(host, LE, res=24, spp=16), max_depth=D)
    wrongs = {"no (eta_i/eta_t)^2 factor": cf.glass_over_emitter_expect(LE, D, factor=1.0),
              "inverted factor": cf.glass_over_emitter_expect(LE, D, factor=2.25)}
    if D == 1:
        wrongs["depth D-1"] = cf.glass_over_emitter_expect(LE, 0)
    cf.assert_mean(rgb, cf.glass_over_emitter_expect(LE, D), wrongs=wrongs, se_target=0.05, label=f"glass over emitter D={D}")


# ---- E: mirror corridor --------------------------------------------------------------------------------------------------

KR = (0.97, 0.85, 0.6)   # per channel: a channel mix-up or a grey kr shows; max 0.97 lets RR fire gently from the fifth reflection


def _corridor(host, spp=1, res=24):
    N, ok = cf.corridor_rays(host, OracleScene, KR, res)
    assert ok.mean() > 0.9 and len(np.unique(N[ok])) >= 4, np.unique(N[ok], return_counts=True)
    return cf.mirror_corridor(host, LE, KR, res=res, spp=spp), N, ok


def test_mirror_corridor_per_pixel(host):
    """Form E, RR off: every pixel is exactly Le kr^N if its ray escapes after N <= D reflections, else 0 — the depth cut-off
    checked per pixel at every D from 0 to past the longest path (pixels meet 0, 1, 3, 4 and 5 reflections; the N = 1 ones hit a
    mirror's back from outside the corridor)."""
    cap, N, ok = _corridor(host)
    s = OracleScene(); cap(s)
    for D in range(0, int(N.max()) + 2):
        xyz, wt, _, _ = s.render_path_ex(max_depth=D, rr_threshold=0.0)
        rgb = s.film_to_rgb(xyz, wt)
        np.testing.assert_allclose(rgb[ok], cf.mirror_expect(LE, KR, N, D)[ok], rtol=1e-5, atol=1e-7, err_msg=f"D={D}")


def test_mirror_corridor_rr_groups(host):
    """Form E, RR on: paths of N <= 4 reflections never meet RR (it runs after bounces > 3) and stay exact per pixel; for each
    group of equal N >= 5 the mean over its pixels is Le kr^N, told apart from the answer without RR's 1/(1-q) weight."""
    cap, N, ok = _corridor(host, spp=64)
    D = int(N.max()) + 1
    rgb, _, _ = render(cap, max_depth=D)
    E = cf.mirror_expect(LE, KR, N, D)
    short = ok & (N <= 4)
    np.testing.assert_allclose(rgb[short], E[short], rtol=1e-5, atol=1e-7)
    groups = [n for n in np.unique(N[ok]) if n >= 5]
    assert groups
    for n in groups:
        sel = ok & (N == n)
        En = E[sel][0]
        cf.assert_mean(rgb[sel], En, wrongs={"RR weight 1/(1-q) dropped": En * cf.mirror_rr_survival(KR, n)}, se_target=0.01,
                       label=f"mirror corridor N={n} ({sel.sum()} pixels)")


# ---- F: the replay, sample by sample -------------------------------------------------------------------------------------

def test_replay_against_closed_form():
    """The replay itself, with no renderer and no sampler: RR off, every sample of a Kt-only stack crosses its 8 interfaces and carries
    Le (kt (1 - F))^8 (the 1/eta^2 and eta^2 of each slab cancel); with a max depth of 7 the depth cut-off leaves nothing."""
    faces = lr.slabs([lr.uber(kt=lr.KT, eta=1.5)] * 4)
    u = np.full((5, 5 + 3 * 8), 0.5)
    r = lr.replay(faces, u, np.ones(5), LE, 8, rr_threshold=0.0)
    F = cf.fresnel_dielectric(1.0, 1.5)
    np.testing.assert_allclose(r["L"], np.broadcast_to(np.asarray(LE) * (np.asarray(lr.KT, np.float32).astype(np.float64) * (1 - F)) ** 8, (5, 3)), rtol=1e-12)
    assert (r["fate"] == lr.ESCAPED).all() and (r["vertices"] == 8).all() and not r["excluded"].any()
    r = lr.replay(faces, u, np.ones(5), LE, 7, rr_threshold=0.0)
    assert (r["fate"] == lr.DEPTH).all() and not r["L"].any()


@pytest.mark.parametrize("case", lr.CASES, ids=repr)
def test_li_replay(host, case):
    """Every pixel of the oracle's film equals the float64 replay of its samples (li_replay.py): zeros exactly, the rest within
    lr.TOL.  Before the oracle renders, the case proves from the replay alone that at most 0.5 % of its samples lie within 1e-5 of
    a decision, that samples survive, die by Russian roulette and run longer than 4 vertices (10 % each), and that every misreading
    of li in case.catches would move at least 10 % of its pixels (li_replay.assert_case_sound)."""
    s = case.scene(host, OracleScene)
    inputs = case.inputs(host, s)
    if case.corridor is not None:    # the rim band of closed_form.mirror_bounces, as in test_mirror_corridor_per_pixel
        assert inputs[3].mean() > 0.9 and inputs[2].min() >= 5, np.unique(inputs[2], return_counts=True)
    fig = lr.assert_case_sound(case, inputs, lr.TOL)
    xyz, wt, st, _ = s.render_path_ex(max_depth=case.max_depth, rr_threshold=case.rr_threshold)
    assert st.camera_rays == case.res * case.res * case.spp
    rgb = s.film_to_rgb(xyz, wt)
    print(f"{case}: relative deviation {lr.deviation(rgb, case.predict(inputs))[0]:.3g}, excluded {fig['excluded']:.4%}, fates {fig['fates']}, "
          f"longer than 4 vertices {fig['long']:.1%}, power {fig['power']}")
    lr.assert_film_matches(rgb, case.predict(inputs), lr.TOL, label=str(case))


def test_li_replay_cases_cover_every_misreading():
    """Each misreading the replay can switch on is caught by some case: the floor by the eta 1.1 stacks and the corridor, `<=` by the
    corridor whose kr is 1, BSDF::eta by the glass stacks and the sheet."""
    caught = {w for c in lr.CASES for w in c.catches}
    assert caught == set(lr.WRONGS), set(lr.WRONGS) - caught


# ---- Sobol tables: a render beyond the tables given is refused -----------------------------------------------------------

def test_sobol_tables_length_must_be_multiple_of_52():
    m32, vdc, vdci = cf.sobol_fixture()
    s = OracleScene()
    for a, b, c in ((m32[:-1], vdc, vdci), (m32, vdc[:-3], vdci[:-3]), (m32[:0], vdc, vdci)):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.set_sobol_tables(a, b, c)
        assert e.value.code == pbrt_hip.ERR_INVALID_ARG


@pytest.mark.parametrize("res,D,ok", [(64, 4, True), (256, 4, True), (512, 1, True), (64, 5, False), (64, 30, False), (513, 1, False), (1024, 0, False)])
def test_sobol_render_bounded_by_tables(host, res, D, ok):
    """The fixture holds 48 dimensions and 9 VdC matrices: a path of depth D needs 5 + 8 (D + 1) dimensions (D <= 4) and the
    sample bounds' log2 resolution must not exceed 9 (resolution <= 512).  Beyond, ERR_UNSUPPORTED before anything is rendered."""
    s = cf.sobol_scene(host, res, OracleScene)
    rc, xyz, wt, st = cf.raw_render(s, D, [0, 0, 4, 4])
    if ok:
        assert rc == 0, s.last_error()
        assert st.camera_rays == 4 * 4 * 4 and np.isfinite(xyz[:4, :4]).all()
    else:
        assert rc == pbrt_hip.ERR_UNSUPPORTED, (rc, s.last_error())
        assert np.isnan(xyz).all() and (wt == -7.0).all() and st.camera_rays == 0 and st.regular_rays == 0
        if res > 512:
            with pytest.raises(pbrt_hip.PbrtHipError) as e:
                s.generate_camera_rays([0, 0, 2, 2], 0)
            assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
