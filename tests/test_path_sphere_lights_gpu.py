"""-m gpu: spherical DiffuseAreaLights under the PATH integrator on the device (pbrt_hip_set_path_sphere_lights).  The oracle restates no Sphere::pdf_solid_angle, so the
yardsticks are the ones that exist without it (tests/test_path_sphere_lights_cpu.py proves the first and the third on the CPU):
  - the probe, bit for bit: pdf_li outside against the numpy float32 restatement, inside against distance^2 / (|n . -wi| area) of the oracle's own Sphere::intersect on the
    restated spawn_ray, sample_li against the Whitted light loop's probe (the same function);
  - structure: the oracle's path render of such a scene is the light-sampled half alone, on the same vertices and sampler dimensions — same camera and shadow rays, no fewer
    regular rays, no film value below it;
  - closed forms under closed_form.assert_mean, which the light-sampled half alone, both halves unweighted and depth 0 all miss by more than four tolerance widths;
  - the same bits one way or another: chunks, tile parts, sample-record bands, two contexts, either SAH builder, Sobol;
  - the mean of the Whitted film (bit-pinned to the oracle and to the reference's PNG); the front end; the switch."""
import numpy as np
import pytest

import closed_form as CF
import path_sphere_light_scenes as PS
import pbrt_hip
import sphere_light_scenes as SL
import sphere_pdf_restatement as SP
from oracle_binding import OracleScene
from test_front_end_quadrics_gpu import assert_same_bits, fixture_tree, render

pytestmark = pytest.mark.gpu
F = np.float32
COUNTERS = ("camera_rays", "regular_rays", "shadow_rays", "light_distributions_created")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits_or_both_nan(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


# ---- 4. the probe, bit for bit ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_scene(host):
    s = pbrt_hip.Scene()
    PS.build_probe_lights(s, host)
    yield s
    s.close()


@pytest.fixture(scope="module")
def probe_pdfs(host, probe_scene):
    """op 1 of every probe light on its case set, once"""
    out = {}
    for k in range(len(PS.PROBE_LIGHTS)):
        ref, wi, u = PS.probe_cases(host, k)
        out[k] = (ref, wi, u, probe_scene.sphere_light_probe_batch(k, 1, ref, u, wi))
    return out


@pytest.mark.parametrize("k", range(len(PS.PROBE_LIGHTS)), ids=[p[0] for p in PS.PROBE_LIGHTS])
def test_probe_pdf_li_bit_for_bit(host, probe_pdfs, k):
    name, steps, radius = PS.PROBE_LIGHTS[k][:3]
    ref, wi, u, out = probe_pdfs[k]
    got = out[:, 0]
    assert not out[:, 1:].any()   # the record is zeroed, pdf_li fills slot 0
    centre = SP.centre_of(PS.probe_transform(host, k)[0])
    inside = SP.is_inside(ref, centre, radius)
    assert inside.sum() >= 40 and (~inside).sum() >= 60, (name, int(inside.sum()))
    # outside: uniform_cone_pdf of the restated expression, every bit, infinity included; it does not look at wi
    want = SP.cone_pdf(ref, centre, radius)
    bad = ~same_bits_or_both_nan(got, want) & ~inside
    assert not bad.any(), (name, "outside", int(bad.sum()), [(i, float(got[i]), float(want[i])) for i in np.flatnonzero(bad)[:5]])
    assert np.isinf(got[~inside]).any() and (np.isfinite(got[~inside]) & (got[~inside] > 0)).any(), name
    # inside: the trait's default on the oracle's intersection of the restated spawn_ray with the cut sphere; 0 where it reports no hit
    hit, p, n = PS.oracle_inside_hits(host, k, ref[inside], wi[inside])
    want_in = SP.area_pdf(ref[inside], wi[inside], p, n, hit, PS.probe_light_area(k))
    bad = ~same_bits_or_both_nan(got[inside], want_in)
    assert not bad.any(), (name, "inside", int(bad.sum()), [(i, float(got[inside][i]), float(want_in[i])) for i in np.flatnonzero(bad)[:5]])
    assert (want_in > 0).sum() >= 10, name
    if PS.PROBE_LIGHTS[k][3] is not None:   # a cut sphere: some directions from inside leave through the part that is cut away
        assert (~hit).any() and (got[inside][~hit] == 0).all(), name


def test_probe_pdf_li_ignores_orientation_and_sidedness(probe_pdfs):
    full, rev, two = (probe_pdfs[k][3] for k in range(3))
    assert np.all(same_bits_or_both_nan(full, rev)) and np.all(same_bits_or_both_nan(full, two))


@pytest.mark.parametrize("k", range(len(PS.PROBE_LIGHTS)), ids=[p[0] for p in PS.PROBE_LIGHTS])
def test_probe_sample_li_is_the_whitted_light_loops(host, probe_scene, k):
    ref, wi, u = PS.probe_cases(host, k)
    got = probe_scene.sphere_light_probe_batch(k, 0, ref, u, wi)
    want = probe_scene.light_probe_batch(k, 0, ref, u, wi, variant=2)
    assert np.all(same_bits_or_both_nan(got, want)), PS.PROBE_LIGHTS[k][0]
    assert (got[:, 7] == 1.0).sum() >= 0.8 * len(ref)


def test_probe_refusals(host, probe_scene):
    ref, wi, u = PS.probe_cases(host, 0)
    with pbrt_hip.Scene() as s:   # a triangle light is the other probe's
        m = s.add_material_matte((0.5, 0.5, 0.5))
        lid = s.add_light_diffuse_area((1.0, 1.0, 1.0), 2)
        s.add_mesh(np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F), np.array([0, 1, 2, 0, 2, 3], np.uint32), m, first_area_light=lid)
        s.build_accel(0, 4)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.sphere_light_probe_batch(0, 1, ref[:4], u[:4], wi[:4])
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "spherical" in str(e.value)
    for light, op in ((len(PS.PROBE_LIGHTS), 0), (0, 2), (0, -1)):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            probe_scene.sphere_light_probe_batch(light, op, ref[:4], u[:4], wi[:4])
        assert e.value.code == pbrt_hip.ERR_INVALID_ARG
    # the older probe's refusals stay as they were, whatever the handle's switch says
    probe_scene.set_path_sphere_lights(True)
    try:
        for variant in (0, 1):
            with pytest.raises(pbrt_hip.PbrtHipError) as e:
                probe_scene.light_probe_batch(0, 1, ref[:4], u[:4], wi[:4], variant=variant)
            assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
    finally:
        probe_scene.set_path_sphere_lights(False)


# ---- 5. structure against the oracle's own path render ------------------------------------------------------------------------------------------------------------------------
def pair(build, host):
    prod, orc = pbrt_hip.Scene(), OracleScene()
    try:
        SL.capture(build, prod, host); SL.capture(build, orc, host)
    except Exception:
        prod.close(); orc.close()
        raise
    prod.set_path_sphere_lights(True)
    return prod, orc


def assert_structure(got, want, strategy, label):
    """`want`: the oracle's path render, whose estimate_direct stops after the light-sampled half at a sphere light.  The device walks the same vertices with the same sampler
    dimensions and only adds the BSDF-sampled half: terms >= 0, added at the same places of the same float32 sums, and every later operation is monotone."""
    gxyz, gwt, gst = got
    oxyz, owt, ost = want
    assert np.array_equal(_bits(gwt), _bits(owt)), label
    assert gst.camera_rays == ost.camera_rays and gst.shadow_rays == ost.shadow_rays, (label, gst.as_dict(), ost.as_dict())
    assert gst.regular_rays >= ost.regular_rays, (label, gst.regular_rays, ost.regular_rays)
    if strategy == 2:
        assert gst.light_distributions_created == ost.light_distributions_created, (label, gst.light_distributions_created, ost.light_distributions_created)
    assert np.isfinite(gxyz).all(), label
    below = gxyz < oxyz
    assert not below.any(), (label, int(below.sum()), float((oxyz - gxyz).max()))
    return int((_bits(gxyz) == _bits(oxyz)).all(-1).sum()), int((gxyz > oxyz).any(-1).sum())


@pytest.mark.parametrize("name,build", SL.CASES, ids=[n for n, _ in SL.CASES])
def test_branch_case_is_the_oracles_light_half_plus_more(host, name, build):
    prod, orc = pair(build, host)
    with prod, orc:
        more = 0
        for strategy in (0, 1, 2):
            got = prod.render_path(max_depth=3, light_strategy=strategy)
            same, above = assert_structure(got, PS.oracle_path(orc, max_depth=3, light_strategy=strategy), strategy, f"{name} strategy {strategy}")
            more += above
            assert got[2].shadow_rays > 0
        # Somewhere a BSDF-sampled ray met the light and saw it emit.  Not in `mirrored`: a quadric's normal is flipped for reverse_orientation XOR a handedness-swapping
        # transform in OBJECT space (SurfaceInteraction::new) and then carried to world space, so a mirrored one-sided sphere shows its L to rays that meet it from inside only,
        # while sample_li's normal (flipped for reverse_orientation alone) lights the scene from outside: the reference's behaviour, which the Whitted tests pin.
        assert (more > 0) == (name != "mirrored"), (name, more)


@pytest.mark.parametrize("seed", range(12))
def test_random_scene_is_the_oracles_light_half_plus_more(host, seed):
    build, depth = SL.random_case(host, seed)
    prod, orc = pair(build, host)   # a refusal on either side raises: no seed is skipped
    with prod, orc:
        for strategy in (0, 1, 2):
            got = prod.render_path(max_depth=3, light_strategy=strategy)
            assert_structure(got, PS.oracle_path(orc, max_depth=3, light_strategy=strategy), strategy, f"seed {seed} strategy {strategy}")


def test_small_light_some_pixels_equal_the_oracle_and_some_exceed_it(host):
    prod, orc = pbrt_hip.Scene(), OracleScene()
    with prod, orc:
        PS.small_light_scene(prod, host); PS.small_light_scene(orc, host)
        prod.set_path_sphere_lights(True)
        for strategy in (0, 1, 2):
            got = prod.render_path(max_depth=3, light_strategy=strategy)
            same, above = assert_structure(got, PS.oracle_path(orc, max_depth=3, light_strategy=strategy), strategy, f"small light, strategy {strategy}")
            print("small light, strategy", strategy, ": pixels equal to the oracle", same, ", above it", above)
            assert same > 0 and above > 0, (strategy, same, above)


def test_emission_of_a_sphere_light_at_camera_rays(host):
    """Camera-ray emission indexes first_light correctly for a one-primitive mesh: where every sample of a pixel meets the black light sphere the pixel shows exactly its L"""
    prod, orc = pair(SL.case_visible, host)
    with prod, orc:
        xyz, wt, _ = prod.render_path(max_depth=3, light_strategy=0)
        rgb = prod.film_to_rgb(xyz, wt)
        lit = np.all(np.isclose(rgb, np.float32([3.0, 2.5, 2.0]), rtol=1e-3), -1)
        assert lit.sum() >= 20, int(lit.sum())
        oxyz, owt, _ = PS.oracle_path(orc, max_depth=3, light_strategy=0)
        assert np.array_equal(_bits(xyz[lit]), _bits(oxyz[lit]))   # a black sphere ends the path: these pixels hold nothing else
    prod, orc = pair(lambda s, h: SL.case_inside(s, h, False), host)   # and at specular bounces: the stage's mirror and glass see the enclosing sphere
    with prod, orc:
        xyz, wt, _ = prod.render_path(max_depth=3, light_strategy=0)
        rgb = prod.film_to_rgb(xyz, wt)
        assert np.all(np.isclose(rgb, np.float32([0.9, 0.8, 0.7]), rtol=1e-3), -1).sum() >= 100


# ---- 6. closed forms ----------------------------------------------------------------------------------------------------------------------------------------------------------
RES, SPP = 64, 64


@pytest.fixture(scope="module")
def outside(host):
    """The outside scene on the device (switch on), its per-pixel closed form, and the mean ratio of the oracle's path render (the light-sampled half alone)"""
    prod, orc = pbrt_hip.Scene(), OracleScene()
    PS.outside_scene(host, RES, SPP)(prod); PS.outside_scene(host, RES, SPP)(orc)
    prod.set_path_sphere_lights(True)
    expect = PS.outside_pixel_expect(prod, RES)
    xyz, wt, _ = PS.oracle_path(orc, max_depth=1, light_strategy=0)
    half = CF.frame_stats(orc.film_to_rgb(xyz, wt).astype(np.float64) / expect)[0]
    orc.close()
    yield prod, expect, half
    prod.close()


@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("depth", [1, 5])
def test_outside_closed_form(outside, depth, strategy):
    """ratio = pixel / (rho Le r^2 h / d^3 over the pixel's footprint), expected mean 1 in every channel.  Measured on the MI355X at 64 x 64 @ 64 spp — both depths and both
    strategies give the same bits (one light; nothing a ray from the floor meets reflects): ratio mean (1.0000162, 1.0000145, 1.0000140), se 4.63e-4 in every channel, so the
    tolerance is 2.3e-3; the oracle's path render (the light-sampled half alone) gives 0.98728, 5.5 tolerance widths away; twice the answer and 0 lie hundreds away."""
    prod, expect, half = outside
    xyz, wt, _ = prod.render_path(max_depth=depth, light_strategy=strategy)
    ratio = prod.film_to_rgb(xyz, wt).astype(np.float64) / expect
    print("outside depth", depth, "strategy", strategy, ": ratio mean, se", *CF.frame_stats(ratio), "; light half only", half)
    CF.assert_mean(ratio, 1.0, se_target=PS.SE_TARGET, wrongs=PS.wrongs_from(half, 1.0), label=f"outside, depth {depth}, strategy {strategy}")


@pytest.mark.parametrize("two_sided", [False, True], ids=["reversed", "two_sided"])
def test_inside_closed_form(host, two_sided):
    """L = rho Le = (2, 3.5, 3.8) at depths 1 and 5 under strategies 0 and 1.  Measured on the MI355X at 64 x 64 @ 64 spp, the same bits in all four runs and for both forms of
    the light: mean (2.0000264, 3.5000403, 3.8000417), se (3.39e-4, 5.93e-4, 6.44e-4); the light-sampled half alone (0.39934, 0.69884, 0.75874), 0.2 of the answer."""
    with pbrt_hip.Scene() as prod, OracleScene() as orc:
        PS.inside_scene(host, two_sided, RES, SPP)(prod); PS.inside_scene(host, two_sided, RES, SPP)(orc)
        prod.set_path_sphere_lights(True)
        xyz, wt, _ = PS.oracle_path(orc, max_depth=1, light_strategy=0)
        half = CF.frame_stats(orc.film_to_rgb(xyz, wt))[0]
        for depth in (1, 5):
            for strategy in (0, 1):
                xyz, wt, _ = prod.render_path(max_depth=depth, light_strategy=strategy)
                rgb = prod.film_to_rgb(xyz, wt)
                print("inside", "two-sided" if two_sided else "reversed", "depth", depth, "strategy", strategy, ": mean, se", *CF.frame_stats(rgb), "; light half only", half)
                CF.assert_mean(rgb, PS.INSIDE_EXPECT, se_target=PS.SE_TARGET, wrongs=PS.wrongs_from(half, PS.INSIDE_EXPECT), label=f"inside, depth {depth}, strategy {strategy}")


# ---- 8. the mean of the Whitted film ---------------------------------------------------------------------------------------------------------------------------------------------
def test_path_and_whitted_have_the_same_mean_at_depth_1(outside):
    """The per-pixel difference of the two films against 0, with the Whitted film's se: assert_mean on the Whitted film with the path film's mean as the expectation.  Measured:
    mean of the difference (3.1e-7, 5.4e-7, 6.0e-7), its own se (0.95e-4, 1.66e-4, 1.80e-4); the Whitted film's mean (0.17393, 0.30437, 0.33046), se (1.54e-3, 2.69e-3, 2.92e-3)
    (the film's se is that of the signal's variation over the footprint, which is why the closed form above divides it out first)."""
    prod, expect, half = outside
    xyz, wt, _ = prod.render_path(max_depth=1, light_strategy=0)
    path_rgb = prod.film_to_rgb(xyz, wt).astype(np.float64)
    xyz, wt, _ = prod.render_whitted(max_depth=1)
    whitted_rgb = prod.film_to_rgb(xyz, wt).astype(np.float64)
    d_mean, d_se = CF.frame_stats(path_rgb - whitted_rgb)
    print("path - whitted: mean", d_mean, "se of the difference", d_se, "; whitted film mean, se", *CF.frame_stats(whitted_rgb))
    CF.assert_mean(whitted_rgb, CF.frame_stats(path_rgb)[0], label="whitted film against the path film's mean")


# ---- 7. the same bits every way ----------------------------------------------------------------------------------------------------------------------------------------------------
def film_and_counters(got):
    xyz, wt, st = got
    return xyz, wt, tuple(getattr(st, f) for f in COUNTERS)


def assert_identical(got, want, label):
    """got: a render's (xyz, weight, Stats) or, like want, (xyz, weight, counters)"""
    gx, gw, gc = got if isinstance(got[2], tuple) else film_and_counters(got)
    wx, ww, wc = want
    assert np.array_equal(_bits(gw), _bits(ww)) and np.array_equal(_bits(gx), _bits(wx)), (label, int((_bits(gx) != _bits(wx)).any(-1).sum()))
    assert gc == wc, (label, gc, wc)


def three_forms(prod, want, strategy, monkeypatch, label):
    """forced chunks, three tile parts summed, sample-record bands"""
    monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(48 * 48 * 3 // 2))   # four chunks of one sample per pixel
    assert_identical(prod.render_path(max_depth=3, light_strategy=strategy), want, label + ", chunked")
    monkeypatch.delenv("PBRT_HIP_MAX_PATHS")
    acc = np.zeros_like(want[0]); accw = np.zeros_like(want[1]); cnt = [0, 0, 0]; dists = []
    for part in range(3):
        xyz, wt, st = prod.render_path(max_depth=3, light_strategy=strategy, tile_part=part, tile_parts=3)
        acc += xyz; accw += wt
        cnt = [a + b for a, b in zip(cnt, (st.camera_rays, st.regular_rays, st.shadow_rays))]
        dists.append(st.light_distributions_created)
    # the parts' tiles are disjoint: the sums are exact.  The fourth counter is a count of distinct voxels — each part's render creates the distributions of the voxels ITS
    # paths touch — so over parts it is a union, not a sum: no part exceeds the whole frame's count and together they cover it (0 everywhere where the distribution is not live)
    assert_identical((acc, accw, tuple(cnt)), (want[0], want[1], want[2][:3]), label + ", three tile parts")
    assert max(dists) <= want[2][3] <= sum(dists), (label, dists, want[2][3])
    prod.set_sample_record_budget(2 * 256 * 4 * 20)   # two whole 16 x 16 tiles' records at 4 spp: the 3 x 3 tiles render in several bands
    try:
        assert_identical(prod.render_path(max_depth=3, light_strategy=strategy), want, label + ", bands")
        assert prod.render_footprint()["bands"] > 1
    finally:
        prod.set_sample_record_budget(0)


@pytest.mark.parametrize("name,build", [("six_lights", SL.case_six_lights), ("partial", SL.case_partial)], ids=["six_lights", "partial"])
def test_same_bits_every_way(host, monkeypatch, name, build):
    strategy = 2   # six lights: the spatial light distribution is live and samples the sphere lights too; one light: it falls back to the uniform one
    with pbrt_hip.Scene() as prod:
        SL.capture(build, prod, host)
        prod.set_path_sphere_lights(True)
        want = film_and_counters(prod.render_path(max_depth=3, light_strategy=strategy))
        assert want[2][2] > 0 and float(want[0].max()) > 0.0
        if name == "six_lights":
            assert want[2][3] > 0
        assert_identical(prod.render_path(max_depth=3, light_strategy=strategy), want, name + ", again")
        three_forms(prod, want, strategy, monkeypatch, name)
        # the SAH tree from the device builder
        prod.build_accel_device_shapes(0, 4)
        assert_identical(prod.render_path(max_depth=3, light_strategy=strategy), want, name + ", device-built SAH tree")
        prod.build_accel(0, 4)
        # Sobol with the fixture's tables: one render, and the three forms again
        prod.set_sobol_tables(*CF.sobol_fixture())
        prod.set_sampler(CF.SOBOL, 4, prod.sample_bounds)
        sob = film_and_counters(prod.render_path(max_depth=3, light_strategy=strategy))
        assert not np.array_equal(_bits(sob[0]), _bits(want[0])) and float(sob[0].max()) > 0.0
        three_forms(prod, sob, strategy, monkeypatch, name + ", sobol")
    # a handle over two contexts of the one GPU
    with pbrt_hip.Scene(devices=[0, 0]) as multi:
        SL.capture(build, multi, host)
        multi.set_path_sphere_lights(True)
        assert_identical(multi.render_path(max_depth=3, light_strategy=strategy), want, name + ", two contexts")   # (the handle reports the union of its contexts' voxels)


# ---- 9. the front end ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_renders_lights_diffuse_under_path(tmp_path, host):
    """tests/golden/ref_scenes/lights/diffuse.pbrt with its Integrator line replaced by "path", at 8 spp: the bits of the same scene built call by call through the C ABI"""
    spp = 8
    scene = fixture_tree(tmp_path, "lights/diffuse.pbrt", spp)
    text = scene.read_text()
    lines = [l for l in text.splitlines() if l.strip().startswith("Integrator")]
    assert len(lines) == 1 and "whitted" in lines[0], lines
    scene.write_text(text.replace(lines[0], 'Integrator "path"'))
    got = render(tmp_path, scene, "--path-sphere-lights")
    with pbrt_hip.Scene() as s:
        info = SL.lights_diffuse(s, host, spp=spp)
        s.set_path_sphere_lights(True)
        xyz, wt, _ = s.render_path(max_depth=5)   # the directive's defaults: maxdepth 5, rrthreshold 1, lightsamplestrategy "spatial"
        assert_same_bits(got, np.ascontiguousarray(s.film_to_rgb(xyz, wt), np.float32), "lights/diffuse.pbrt under path")


# ---- 10. the switch ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_switch_on_off_on(host):
    with pbrt_hip.Scene() as s:
        SL.capture(SL.case_cone, s, host)
        whitted = film_and_counters(s.render_whitted(max_depth=3))
        with pytest.raises(pbrt_hip.PbrtHipError) as e:   # off by default
            s.render_path(max_depth=3)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "sphere light" in str(e.value)
        s.set_path_sphere_lights(True)
        on = film_and_counters(s.render_path(max_depth=3, light_strategy=1))
        assert_identical(s.render_path(max_depth=3, light_strategy=1), on, "the switch survives a render")
        s.set_path_sphere_lights(False)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.render_path(max_depth=3, light_strategy=1)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "sphere light" in str(e.value) and "pbrt_hip_render_whitted" in str(e.value)
        assert_identical(s.render_whitted(max_depth=3), whitted, "whitted after the refusal")
        s.set_path_sphere_lights(True)
        assert_identical(s.render_path(max_depth=3, light_strategy=1), on, "on again")
        assert_identical(s.render_whitted(max_depth=3), whitted, "whitted after the path render")
