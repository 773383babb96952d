"""-m gpu: disk and cylinder DiffuseAreaLights (pbrt_hip_add_quadric_light) under both integrators on the device.  The oracle restates neither Disk::sample nor
Cylinder::sample, so the yardsticks are the ones tests/test_quadric_lights_cpu.py proves on the CPU:
  - the probe, bit for bit: sample_li in all 28 floats against tests/quadric_light_restatement.py, the disk's pdf_li against the restated intersection; the cylinder's pdf_li
    against the float64 analytic hit within 4 x what the disk's float32 restatement shows against its own float64 twin;
  - closed forms under closed_form.assert_mean, with the named wrong answers at four tolerance widths;
  - the same bits one way or another: chunks, tile parts, sample-record bands, two contexts, host- and device-built SAH and HLBVH trees, Sobol;
  - the C ABI's refusals, the sphere-light switch next to a disk light, emission at camera rays."""
import numpy as np
import pytest

import closed_form as CF
import pbrt_hip
import quadric_light_restatement as QR
import quadric_light_scenes as QS
import sphere_light_scenes as SL
from test_path_sphere_lights_gpu import assert_identical, film_and_counters, same_bits_or_both_nan, three_forms

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
ALL = range(len(QS.PROBE_LIGHTS))
IDS = [p[0] for p in QS.PROBE_LIGHTS]
RES, SPP = 64, 64
E_RGB = np.asarray(QS.RHO, D) * np.asarray(QS.LE, D)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(host):
    ident = (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY)
    with pbrt_hip.Scene() as s, pbrt_hip.Scene() as fresh:
        QS.case_disk_and_cylinder(fresh, host)
        want = film_and_counters(fresh.render_path(max_depth=3, light_strategy=1))
        m = s.add_material_matte((0.5, 0.5, 0.5))
        for kind, name in ((1, "cone"), (2, "paraboloid")):
            for k in (kind, name):
                with pytest.raises(pbrt_hip.PbrtHipError) as e:
                    s.add_quadric_light(k, ident[0], ident[1], 1.0, 1.0, 0.0, material=m)
                assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "todo!()" in str(e.value), str(e.value)
        for kind in (-1, 4, 5, 17):
            with pytest.raises(pbrt_hip.PbrtHipError) as e:
                s.add_quadric_light(kind, ident[0], ident[1], 1.0, 0.0, 0.0, material=m)
            assert e.value.code == pbrt_hip.ERR_INVALID_ARG
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.add_quadric_light("disk", ident[0], ident[1], 1.0, 0.0, 0.0, material=m + 7)
        assert e.value.code == pbrt_hip.ERR_INVALID_ARG
        s.object_begin()
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.add_quadric_light("disk", ident[0], ident[1], 1.0, 0.0, 0.0, material=m)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object definition" in str(e.value)
        s.add_mesh(np.array([[0, 0, 9], [1, 0, 9], [0, 1, 9]], F), np.array([0, 1, 2], np.uint32), m)
        s.object_end()
        lid = s.add_light_diffuse_area((1.0, 1.0, 1.0), 1)   # triangle area lights that no mesh has claimed yet
        for call in (lambda: s.add_quadric_light("cylinder", ident[0], ident[1], 1.0, -1.0, 1.0, material=m), lambda: s.add_quadric("disk", ident[0], ident[1], 1.0, 0.0, 0.0, material=m)):
            with pytest.raises(pbrt_hip.PbrtHipError) as e:
                call()
            assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "area light" in str(e.value)
    # the handle stays usable and holds nothing of the refused calls: the same refusals in front of a scene leave its film and counters as they are
    with pbrt_hip.Scene() as s:
        for k in ("cone", "paraboloid", 9):
            with pytest.raises(pbrt_hip.PbrtHipError):
                s.add_quadric_light(k, ident[0], ident[1], 1.0, 1.0, 0.0)
        QS.case_disk_and_cylinder(s, host)
        assert_identical(s.render_path(max_depth=3, light_strategy=1), want, "after the refusals")


# ---- 2. sample_li, bit for bit ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_scene(host):
    s = pbrt_hip.Scene()
    QS.build_probe_lights(s, host)
    yield s
    s.close()


@pytest.mark.parametrize("k", ALL, ids=IDS)
def test_probe_sample_li_bit_for_bit(host, probe_scene, k):
    name, kind, steps, radius, a, b, phimax, rev, two = QS.PROBE_LIGHTS[k]
    ref, u = QS.sample_cases(host, k)
    wi = np.zeros((len(ref), 3), F)
    got = probe_scene.sphere_light_probe_batch(k, 0, ref, u, wi)
    want = QR.sample_li(QS.probe_shape(host, k), QS.PROBE_L, two, ref, u)
    bad = ~same_bits_or_both_nan(got, want)
    assert not bad.any(), (name, int(bad.any(1).sum()), [(int(i), np.flatnonzero(bad[i]).tolist(), got[i][bad[i]].tolist(), want[i][bad[i]].tolist()) for i in np.flatnonzero(bad.any(1))[:4]])
    assert (got[:, 7] == 1.0).sum() >= 0.7 * len(ref) and (got[-12:, 7] == 0.0).all()
    whitted = probe_scene.light_probe_batch(k, 0, ref, u, wi, variant=2)
    assert np.all(same_bits_or_both_nan(got, whitted)), name


def test_probe_refusals_stay(host, probe_scene):
    ref, u = QS.sample_cases(host, 0)
    wi = np.zeros((len(ref), 3), F)
    for variant in (0, 1):   # the path integrator's triangle-light code knows no quadric light
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            probe_scene.light_probe_batch(0, 0, ref[:4], u[:4], wi[:4], variant=variant)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        probe_scene.light_probe_batch(0, 1, ref[:4], u[:4], wi[:4], variant=2)
    assert e.value.code == pbrt_hip.ERR_INVALID_ARG
    for light, op in ((len(QS.PROBE_LIGHTS), 0), (0, 2), (0, -1)):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            probe_scene.sphere_light_probe_batch(light, op, ref[:4], u[:4], wi[:4])
        assert e.value.code == pbrt_hip.ERR_INVALID_ARG


# ---- 3. pdf_li -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disk_pdfs(host, probe_scene):
    out = {}
    for k in QS.DISKS:
        ref, wi = QS.disk_pdf_cases(host, k)
        out[k] = (ref, wi, probe_scene.sphere_light_probe_batch(k, 1, ref, np.zeros((len(ref), 2), F), wi))
    return out


@pytest.mark.parametrize("k", QS.DISKS, ids=[IDS[k] for k in QS.DISKS])
def test_probe_disk_pdf_li_bit_for_bit(host, disk_pdfs, k):
    ref, wi, out = disk_pdfs[k]
    q = QS.probe_shape(host, k)
    assert not out[:, 1:].any()   # the record is zeroed, pdf_li fills slot 0
    got = out[:, 0]
    want, hit = QR.disk_pdf_li(q, ref, wi)
    bad = ~same_bits_or_both_nan(got, want)
    assert not bad.any(), (IDS[k], int(bad.sum()), [(int(i), float(got[i]), float(want[i])) for i in np.flatnonzero(bad)[:5]])
    assert (got[~hit] == 0).all() and (~hit).sum() >= 30 and (got > 0).sum() >= 30   # exactly 0 for a miss
    parallel = (wi.astype(D) @ q["w2o"].astype(D).reshape(4, 4)[:3, :3].T)[:, 2] == 0
    assert (got[parallel] == 0).all()
    if k == 0:
        assert parallel.sum() >= 9
    if q["inner_radius"] > 0:   # exactly 0 through the inner hole and the phi cut: rays that meet the full disk of the same plane
        full = dict(q, inner_radius=F(0), phi_max=F(2.0 * np.pi))
        cut_away = QR.disk_pdf_li(full, ref, wi)[1] & ~hit
        assert cut_away.sum() >= 20 and (got[cut_away] == 0).all()


def test_probe_disk_pdf_li_ignores_orientation_and_sidedness(disk_pdfs):
    full, rev, two = (disk_pdfs[k][2] for k in range(3))
    assert np.all(same_bits_or_both_nan(full, rev)) and np.all(same_bits_or_both_nan(full, two))


@pytest.mark.parametrize("k", QS.CYLINDERS, ids=[IDS[k] for k in QS.CYLINDERS])
def test_probe_cylinder_pdf_li_against_the_float64_hit(host, probe_scene, k):
    """Measured on the CPU (tests/test_quadric_lights_cpu.py): the disk's float32 restatement differs from its float64 twin by at most 2.92e-6 relative on probes under the same
    three constraints, so the margin is 1.17e-5.  Measured on the MI355X: 6.75e-6 (full), 4.21e-6 (reversed, cut), 1.03e-5 (mirrored, scaled) — the figures the reference's own
    float32 arithmetic shows on the CPU, because the device equals it bit for bit (the next test)."""
    worst, margin = QS.measured_margin(host)
    ref, wi, p64, keep = QS.cylinder_twin(host, k)
    got = probe_scene.sphere_light_probe_batch(k, 1, ref, np.zeros((len(ref), 2), F), wi)[:, 0].astype(D)
    assert keep.mean() >= 1.0 - QS.COND_CAP
    rel = np.abs(got[keep] - p64[keep]) / p64[keep]
    print(IDS[k], "cylinder pdf_li against the float64 twin: largest relative difference", rel.max(), "margin", margin, "(disk restatement against its twin:", worst, ")")
    assert rel.max() <= margin, (IDS[k], float(rel.max()), margin, int(np.argmax(rel)))


@pytest.mark.parametrize("k", QS.CYLINDERS, ids=[IDS[k] for k in QS.CYLINDERS])
def test_probe_cylinder_pdf_li_is_the_references_arithmetic(host, probe_scene, k):
    """Beyond what the margin asks: on the same probes the device equals, bit for bit, Cylinder::intersect restated in float32 values (the EFloat intervals decide nothing
    where t is far from 0) under the trait's default pdf"""
    ref, wi, want, hit = QS.cylinder_restated(host, k)
    keep = QS.cylinder_twin(host, k)[3]
    got = probe_scene.sphere_light_probe_batch(k, 1, ref, np.zeros((len(ref), 2), F), wi)[:, 0]
    bad = ~same_bits_or_both_nan(got, want) & keep
    assert not bad.any(), (IDS[k], int(bad.sum()), [(int(i), float(got[i]), float(want[i])) for i in np.flatnonzero(bad)[:5]])


def test_probe_cylinder_pdf_li_is_the_references_arithmetic_over_the_whole_band(host, probe_scene):
    """The same bit-for-bit comparison where the margin does not reach: origins out to 19 radii from the wall on the three probe cylinders, and on two cylinders 13 and 18
    units from the origin.  The bits do not depend on the margin."""
    for k in QS.CYLINDERS:
        ref, wi, want, keep = QS.cylinder_wide(host, QS.probe_shape(host, k), k)
        got = probe_scene.sphere_light_probe_batch(k, 1, ref, np.zeros((len(ref), 2), F), wi)[:, 0]
        bad = ~same_bits_or_both_nan(got, want) & keep
        assert keep.sum() >= 380 and not bad.any(), (IDS[k], int(keep.sum()), int(bad.sum()), [(int(i), float(got[i]), float(want[i])) for i in np.flatnonzero(bad)[:5]])
    with pbrt_hip.Scene() as s:
        QS.build_far_cylinders(s, host)
        for k, light in enumerate(QS.FAR_CYLINDERS):
            ref, wi, want, keep = QS.cylinder_wide(host, QS.far_shape(host, k), 20 + k)
            got = s.sphere_light_probe_batch(k, 1, ref, np.zeros((len(ref), 2), F), wi)[:, 0]
            bad = ~same_bits_or_both_nan(got, want) & keep
            assert keep.sum() >= 380 and not bad.any(), (light[0], int(keep.sum()), int(bad.sum()), [(int(i), float(got[i]), float(want[i])) for i in np.flatnonzero(bad)[:5]])


def test_probe_cylinder_pdf_li_misses_are_exactly_zero(host, probe_scene):
    """Rays that leave through the open ends, through the phi cut, or point away"""
    for k in QS.CYLINDERS:
        q = QS.probe_shape(host, k)
        c, M, c_obj = QS._frame(q)
        axis = M @ np.array([0.0, 0.0, 1.0]); axis /= np.linalg.norm(axis)
        ref = QS.LP.mk_ref([c, c + 0.2 * axis, c + 5.0 * axis * float(q["radius"])], n=axis.astype(F))
        wi = np.array([axis, axis, axis], F)
        got = probe_scene.sphere_light_probe_batch(k, 1, ref, np.zeros((3, 2), F), wi)[:, 0]
        assert (got == 0).all(), (IDS[k], got)
    q = QS.probe_shape(host, 6)   # the cut cylinder: through the middle of the phi gap from the axis
    c, M, c_obj = QS._frame(q)
    mid = 0.5 * (float(q["phi_max"]) + 2.0 * np.pi)
    d = M @ np.array([np.cos(mid), np.sin(mid), 0.0]); d /= np.linalg.norm(d)
    got = probe_scene.sphere_light_probe_batch(6, 1, QS.LP.mk_ref([c]), np.zeros((1, 2), F), d.astype(F)[None])[:, 0]
    assert (got == 0).all()


# ---- 4. closed forms -----------------------------------------------------------------------------------------------------------------------------------------------------
def rgb_of(s, got):
    return s.film_to_rgb(got[0], got[1]).astype(D)


@pytest.fixture(scope="module")
def disk_floor(host):
    s = pbrt_hip.Scene()
    QS.disk_over_floor(host, RES, SPP)(s)
    yield s, QS.disk_pixel_expect(s, RES)
    s.close()


# (the third is named on scene (a) as the issue lists it; its disk has no inner radius, so it can only be met there by a pdf that is wrong for every disk — the annulus test
# below is where an inner radius is present)
DISK_WRONGS = {"the MIS weight dropped (both halves unweighted)": 2.0 * np.ones(3), "depth 0": np.zeros(3),
               "1/area of the full disk where inner_radius > 0": np.ones(3) / (1.0 - (QS.DISK_INNER / QS.DISK_R) ** 2)}


@pytest.mark.parametrize("integrator,depth,strategy", [("whitted", 1, 0), ("path", 1, 0), ("path", 1, 1), ("path", 5, 0), ("path", 5, 1)])
def test_disk_above_a_floor(disk_floor, integrator, depth, strategy):
    """(a) ratio = pixel / (rho Le form factor over the pixel's footprint), expected mean 1 in every channel.  Measured on the MI355X at 64 x 64 @ 64 spp: Whitted
    (1.0000141, 1.0000124, 1.0000118), se 1.9e-4; path (1.0000048, 1.0000031, 1.0000025), se 3.6e-4, the same bits at both depths and under both strategies (one light; nothing a
    ray from the floor meets reflects)."""
    s, expect = disk_floor
    got = s.render_whitted(max_depth=depth) if integrator == "whitted" else s.render_path(max_depth=depth, light_strategy=strategy)
    ratio = rgb_of(s, got) / expect
    print("disk above a floor,", integrator, "depth", depth, "strategy", strategy, ": ratio mean, se", *CF.frame_stats(ratio))
    CF.assert_mean(ratio, 1.0, se_target=QS.SE_TARGET, wrongs=DISK_WRONGS, label=f"disk above a floor, {integrator}, depth {depth}, strategy {strategy}")


def test_disk_with_an_inner_radius_under_whitted(host):
    """The reference's Disk::sample ignores inner_radius while area() does not: every sample of the full disk is lit (the shadow ray to a point of the hole meets nothing) with
    pdf 1/area of the annulus, so one light sample per vertex — the Whitted integrator — shows (1 - ri^2 / R^2) of the full disk's radiance.  (Under MIS the BSDF-sampled half
    sees the annulus alone and the sum has no closed form.)"""
    with pbrt_hip.Scene() as s:
        QS.disk_over_floor(host, RES, SPP, inner=QS.DISK_INNER)(s)
        ratio = rgb_of(s, s.render_whitted(max_depth=1)) / QS.disk_pixel_expect(s, RES)
        f = 1.0 - (QS.DISK_INNER / QS.DISK_R) ** 2
        print("annulus under whitted: ratio mean, se", *CF.frame_stats(ratio), "expected", f)
        CF.assert_mean(ratio, f, se_target=QS.SE_TARGET, wrongs={"1/area of the full disk": np.ones(3), "the annulus alone is lit": f * f * np.ones(3)}, label="annulus, whitted")


def test_disk_back_side(host, disk_floor):
    """(b) one-sided and seen from behind the floor is exactly black; two-sided it is (a)"""
    with pbrt_hip.Scene() as s:
        QS.disk_over_floor(host, RES, SPP, reverse=False)(s)
        for got in (s.render_whitted(max_depth=1), s.render_path(max_depth=1, light_strategy=0), s.render_path(max_depth=5, light_strategy=1)):
            assert not got[0].any() and got[2].camera_rays > 0
    with pbrt_hip.Scene() as s:
        QS.disk_over_floor(host, RES, SPP, reverse=False, two_sided=True)(s)
        expect = disk_floor[1]
        for integrator in ("whitted", "path"):
            got = s.render_whitted(max_depth=1) if integrator == "whitted" else s.render_path(max_depth=1, light_strategy=0)
            CF.assert_mean(rgb_of(s, got) / expect, 1.0, se_target=QS.SE_TARGET, wrongs=DISK_WRONGS, label="two-sided disk from behind, " + integrator)


@pytest.mark.parametrize("integrator,depth,strategy", [("whitted", 1, 0), ("path", 1, 0), ("path", 1, 1), ("path", 5, 0), ("path", 5, 1)])
def test_cylinder_wall(host, integrator, depth, strategy):
    """(c) ratio = pixel / (rho Le x the float64 quadrature of the wall at the pixel), expected mean 1; on the axis the quadrature is H^2 / (H^2 + R^2)
    (tests/test_quadric_lights_cpu.py).  Measured on the MI355X: Whitted 0.99997, se 7.2e-4; path 0.99989, se 6.1e-4 (the same bits in all four path runs)."""
    with pbrt_hip.Scene() as s:
        QS.cylinder_wall(host, RES, SPP)(s)
        expect = QS.pixel_expect(s, RES, lambda X, Y: QS.wall_patch_radiance(np.hypot(X, Y), n=1024), k=1)[..., None] * E_RGB
        got = s.render_whitted(max_depth=depth) if integrator == "whitted" else s.render_path(max_depth=depth, light_strategy=strategy)
        ratio = rgb_of(s, got) / expect
        print("cylinder wall,", integrator, "depth", depth, "strategy", strategy, ": ratio mean, se", *CF.frame_stats(ratio))
        wrongs = {"the MIS weight dropped (both halves unweighted)": 2.0 * np.ones(3), "depth 0": np.zeros(3), "the whole sphere of directions lit": np.ones(3) / QS.wall_on_axis()}
        CF.assert_mean(ratio, 1.0, se_target=QS.SE_TARGET, wrongs=wrongs, label=f"cylinder wall, {integrator}, depth {depth}, strategy {strategy}")


@pytest.mark.parametrize("strategy", [0, 1, 2])
def test_closed_can_patch(host, strategy):
    """(d) a Lambertian patch inside the closed can shows rho Le at every depth >= 1 (the walls are black matte), under both integrators.  Measured on the MI355X: strategy 0
    (1.99963, 3.49935, 3.79929), se (0.0025, 0.0044, 0.0048); strategy 1 (1.99954, 3.49920, 3.79913); strategy 2 (1.99908, 3.49838, 3.79824)."""
    with pbrt_hip.Scene() as s:
        QS.cylinder_wall(host, RES, SPP, caps=True)(s)
        wrongs = {"the light-choice pdf dropped": E_RGB / 3.0, "one cap missing": E_RGB * QS.wall_on_axis(), "depth 0": np.zeros(3)}
        for depth in (1, 5):
            rgb = rgb_of(s, s.render_path(max_depth=depth, light_strategy=strategy))
            print("closed can, patch, depth", depth, "strategy", strategy, ": mean, se", *CF.frame_stats(rgb))
            CF.assert_mean(rgb, E_RGB, se_target=QS.SE_TARGET, wrongs=wrongs, label=f"closed can, patch, depth {depth}, strategy {strategy}")
        if strategy == 0:
            wrongs["the light-choice pdf dropped"] = 3.0 * E_RGB   # Whitted sums over the lights: no choice to weight
            CF.assert_mean(rgb_of(s, s.render_whitted(max_depth=1)), E_RGB, se_target=QS.SE_TARGET, wrongs=wrongs, label="closed can, patch, whitted")


@pytest.mark.parametrize("strategy", [0, 1, 2])
def test_closed_can_furnace(host, strategy):
    """(d) every wall of the can matte (rho) and emitting: Le sum_{k <= D} rho^k at depth D, three lights, the camera inside.  Measured on the MI355X under strategy 0: depth 1
    (11.99973, 10.49952, 7.79947) against (12, 10.5, 7.8), se (0.0020, 0.0035, 0.0038); depth 5 (12.49989, 13.78293, 21.18408) against (12.4992, 13.78125, 21.19265),
    se (0.0021, 0.0048, 0.0113)."""
    with pbrt_hip.Scene() as s:
        QS.can_furnace(host, RES, SPP)(s)
        for depth in (1, 5):
            got = s.render_path(max_depth=depth, light_strategy=strategy)
            rgb = rgb_of(s, got)
            print("closed can, furnace, depth", depth, "strategy", strategy, ": mean, se", *CF.frame_stats(rgb), "expected", CF.furnace_expect(QS.LE, QS.RHO, depth))
            CF.assert_mean(rgb, CF.furnace_expect(QS.LE, QS.RHO, depth), se_target=QS.SE_TARGET, wrongs=CF.furnace_wrongs(QS.LE, QS.RHO, depth, 3),
                           label=f"closed can, furnace, depth {depth}, strategy {strategy}")
            if strategy == 2:
                assert got[2].light_distributions_created > 0   # the spatial distribution is live: spatial_compute_kernel<true> sampled the three lights


# ---- 5. integrator agreement -------------------------------------------------------------------------------------------------------------------------------------------------
def test_path_and_whitted_agree_on_the_disk_at_depth_1(disk_floor):
    s, expect = disk_floor
    d = rgb_of(s, s.render_path(max_depth=1, light_strategy=0)) - rgb_of(s, s.render_whitted(max_depth=1))
    mean, se = CF.frame_stats(d)
    print("path - whitted on the disk scene: mean", mean, "se of the difference", se)
    assert (se > 0).all() and np.all(np.abs(mean) < 5.0 * se), (mean, se)


# ---- 6. the same bits every way ------------------------------------------------------------------------------------------------------------------------------------------------
def test_same_bits_every_way(host, monkeypatch):
    strategy = 2
    with pbrt_hip.Scene() as prod:
        QS.case_disk_and_cylinder(prod, host)
        want = film_and_counters(prod.render_path(max_depth=3, light_strategy=strategy))
        assert want[2][2] > 0 and float(want[0].max()) > 0.0
        assert_identical(prod.render_path(max_depth=3, light_strategy=strategy), want, "again")
        three_forms(prod, want, strategy, monkeypatch, "disk and cylinder")
        whitted = film_and_counters(prod.render_whitted(max_depth=3))
        prod.build_accel_device_shapes(0, 4)
        assert_identical(prod.render_path(max_depth=3, light_strategy=strategy), want, "device-built SAH tree")
        assert_identical(prod.render_whitted(max_depth=3), whitted, "whitted, device-built SAH tree")
        prod.build_accel(1, 4)
        hl = film_and_counters(prod.render_path(max_depth=3, light_strategy=strategy))
        prod.build_accel_device_shapes(1, 4)
        assert_identical(prod.render_path(max_depth=3, light_strategy=strategy), hl, "device-built HLBVH tree")
        prod.build_accel(0, 4)
        prod.set_sobol_tables(*CF.sobol_fixture())
        prod.set_sampler(CF.SOBOL, 4, prod.sample_bounds)
        sob = film_and_counters(prod.render_path(max_depth=3, light_strategy=strategy))
        assert not np.array_equal(sob[0].view(np.uint32), want[0].view(np.uint32)) and float(sob[0].max()) > 0.0
        three_forms(prod, sob, strategy, monkeypatch, "disk and cylinder, sobol")
    with pbrt_hip.Scene(devices=[0, 0]) as multi:
        QS.case_disk_and_cylinder(multi, host)
        assert_identical(multi.render_path(max_depth=3, light_strategy=strategy), want, "two contexts")
        assert_identical(multi.render_whitted_devices(max_depth=3), whitted, "whitted on two contexts")


def test_sphere_light_switch_next_to_a_disk_light(host):
    with pbrt_hip.Scene() as s:
        QS.case_sphere_and_disk(s, host)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.render_path(max_depth=3)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "sphere light" in str(e.value) and "pbrt_hip_render_whitted" in str(e.value)
        whitted = s.render_whitted(max_depth=3)
        assert float(whitted[0].max()) > 0.0
        s.set_path_sphere_lights(True)
        on = film_and_counters(s.render_path(max_depth=3, light_strategy=1))
        assert on[2][2] > 0 and float(on[0].max()) > 0.0 and np.isfinite(on[0]).all()
        s.set_path_sphere_lights(False)
        with pytest.raises(pbrt_hip.PbrtHipError):
            s.render_path(max_depth=3)
    with pbrt_hip.Scene() as s:   # a scene whose only shaped lights are disks or cylinders renders with no switch, whatever it says
        QS.case_disk_and_cylinder(s, host)
        off = film_and_counters(s.render_path(max_depth=3, light_strategy=1))
        s.set_path_sphere_lights(True)
        assert_identical(s.render_path(max_depth=3, light_strategy=1), off, "the switch does not matter without a sphere light")


def test_emission_at_camera_rays_shows_on_the_side_the_normal_faces(host):
    res = 32
    with pbrt_hip.Scene() as s:
        QS.emission_scene(host, res)(s)
        masks = QS.emission_masks(s, res)
        for label, got in (("path", s.render_path(max_depth=3, light_strategy=0)), ("whitted", s.render_whitted(max_depth=3))):
            rgb = s.film_to_rgb(got[0], got[1])
            for mask, (centre, kind, rev, lit) in zip(masks, QS.EMITTERS):
                assert mask.sum() >= 8, (centre, int(mask.sum()))
                if lit:
                    assert np.all(np.isclose(rgb[mask], np.float32(QS.EMIT_L), rtol=1e-3)), (label, centre, rgb[mask][:3])
                else:
                    assert not rgb[mask].any(), (label, centre, rgb[mask][:3])
