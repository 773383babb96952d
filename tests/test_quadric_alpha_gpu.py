"""-m gpu: quadric shapes in one scene with alpha-masked triangle meshes — the traversal kernel's rows (quadric, alpha = 1 image-map masks / alpha = 2 any texture class) and their
counting rows, through every entry point: ray batches (host and device forms), the path integrator (three light strategies, both samplers, a thin lens, chunks, tile parts, device
tile buffers, a multi-device handle), the Whitted integrator with a spherical area light whose shadow rays cross a shadow-alpha mask, the work counters, and what stays refused.
Every comparison is against the CPU oracle in libm mode 1 and on bits.  The scenes are those of tests/quadric_alpha_scenes.py; tests/test_quadric_alpha_oracle.py shows on the CPU
that the mask is not inert in them.

(The Sobol film takes its tables from tests/golden/sobol_subset_64.npz: a path of depth 5 draws 5 + 8 * 6 = 53 dimensions, five more than sobol_subset.npz holds.)"""
import numpy as np
import pytest
import torch   # device buffers for the *_device entry points.  At module level: first imported inside a test, after the library had run kernels in the process, torch found no device

import pbrt_hip
import quadric_alpha_scenes as QA
import scenes
from oracle_binding import OracleScene
from sphere_light_scenes import oracle_whitted

pytestmark = pytest.mark.gpu
MISS = QA.MISS


def pair(host, build, **kw):
    """build(scene, host, **kw) on a device scene and, in libm mode 1, on an oracle scene -> (prod, orc, what build returned)"""
    prod = pbrt_hip.Scene(); orc = OracleScene()
    info = build(prod, host, **kw)
    with QA.libm1():
        build(orc, host, **kw)
    return prod, orc, info


def assert_hits_equal(got, want, what):
    bad = ~scenes.hits_equal(got, want)
    assert not bad.any(), (what, int(bad.sum()), got[bad][:3], want[bad][:3])


def check_batches(prod, orc, rays, what):
    with QA.libm1():
        want = orc.intersect_batch(rays); wocc = orc.occluded_batch(rays)
    assert_hits_equal(prod.intersect_batch(rays), want, what)
    gocc = prod.occluded_batch(rays)
    assert np.array_equal(gocc, wocc), (what, int((gocc != wocc).sum()))
    return want, wocc


def in_range(prim, r):
    return (prim >= r[0]) & (prim < r[0] + r[1])


def assert_films_equal(got, want, what=""):
    gxyz, gwt, gst = got[:3]; oxyz, owt, ost = want[:3]
    assert np.array_equal(gwt.view(np.uint32), owt.view(np.uint32)), what
    nd = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    assert nd == 0, (what, nd, float(np.abs(gxyz - oxyz).max()))
    for f in ("camera_rays", "regular_rays", "shadow_rays"):
        assert getattr(gst, f) == getattr(ost, f), (what, f, getattr(gst, f), getattr(ost, f))


# ---- 1. batches, per alpha row ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_prims", [1, 4])
@pytest.mark.parametrize("mask", QA.MASKS)
def test_batches_per_alpha_row(host, mask, max_prims):
    rays = QA.grid_rays()
    assert len(rays) == 4096
    occ = {}
    for shadow in (False, True):
        prod, orc, prims = pair(host, QA.mixed_scene, mask=mask, shadow=shadow, max_prims=max_prims, res=(32, 24), spp=2)
        what = f"{mask} shadow-alpha {shadow} max_prims {max_prims}"
        want, occ[shadow] = check_batches(prod, orc, rays, what + " grid")
        # teeth, on the ORACLE's verdicts: rays that start in front of the grid and cross its outline ...
        o = rays["o"].astype(np.float64); d = rays["d"].astype(np.float64)
        t0 = -o[:, 2] / d[:, 2]
        xy = o[:, :2] + t0[:, None] * d[:, :2]
        crosses = (o[:, 2] > 0) & (np.abs(xy) < QA.GRID - 1e-3).all(1) & ~np.isfinite(rays["t_max"])
        behind = in_range(want["prim"], prims["sphere"]) | in_range(want["prim"], prims["cylinder"]) | in_range(want["prim"], prims["disk"])
        assert (crosses & behind).sum() >= 50, (what, int((crosses & behind).sum()))                      # ... reach a quadric THROUGH a hole of the mask,
        assert (crosses & in_range(want["prim"], prims["mesh"])).sum() >= 200, what                       # ... or are stopped by its opaque part,
        assert (in_range(want["prim"], prims["cone"]) | in_range(want["prim"], prims["paraboloid"])).sum() >= 20, what   # ... or meet a quadric in front of it
        # the rays the oracle's path tracer spawns in this scene (off quadrics and masked triangles), 32 x 24 @ 2 spp
        orc.record_rays(1 << 20)
        with QA.libm1():
            orc.render_path_ex(max_depth=4)
        reg, sh = orc.recorded_rays(False), orc.recorded_rays(True)
        assert len(reg) > 1500 and len(sh) > 500, (what, len(reg), len(sh))
        with QA.libm1():
            rwant = orc.intersect_batch(reg); swant = orc.occluded_batch(sh)
        assert_hits_equal(prod.intersect_batch(reg), rwant, what + " recorded")
        assert np.array_equal(prod.occluded_batch(sh), swant), what + " recorded shadow"
        # the device forms: rays and results stay in device memory
        d_rays = torch.from_numpy(np.ascontiguousarray(reg).view(np.uint8).copy()).cuda()
        d_hits = torch.zeros(len(reg) * pbrt_hip.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        prod.intersect_batch_device(d_rays.data_ptr(), d_hits.data_ptr(), len(reg))
        torch.cuda.synchronize()
        assert_hits_equal(d_hits.cpu().numpy().view(pbrt_hip.HIT_DTYPE), rwant, what + " device form")
        d_sh = torch.from_numpy(np.ascontiguousarray(sh).view(np.uint8).copy()).cuda()
        d_occ = torch.full((len(sh),), 7, dtype=torch.uint8, device="cuda")
        prod.occluded_batch_device(d_sh.data_ptr(), d_occ.data_ptr(), len(sh))
        torch.cuda.synchronize()
        assert np.array_equal(d_occ.cpu().numpy(), swant), what + " device form, shadow"
        prod.close(); orc.close()
    assert (occ[False] != occ[True]).sum() >= 20, int((occ[False] != occ[True]).sum())   # the shadow-alpha mask opens any-hit rays a way the alpha mask alone does not


# ---- 2. tie and order ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_first", [True, False], ids=["mesh-first", "spheres-first"])
@pytest.mark.parametrize("mask", QA.MASKS)
def test_sphere_tangent_to_the_masked_plane(host, mask, mesh_first):
    prod, orc, _ = pair(host, QA.tangent_scene, mask=mask, mesh_first=mesh_first, max_prims=4)
    rays = QA.tangent_rays()
    want, wocc = check_batches(prod, orc, rays, f"tangent {mask} mesh_first {mesh_first}")
    mesh = (0, 32) if mesh_first else (len(QA.TANGENT_CENTRES), 32)
    on_mesh = in_range(want["prim"], mesh); on_sphere = (want["prim"] != MISS) & ~on_mesh
    assert on_mesh.sum() >= 100 and on_sphere.sum() >= 100, (int(on_mesh.sum()), int(on_sphere.sum()))
    # the tie is there: rays that end on a sphere within a few float steps of the plane's own distance
    o = rays["o"].astype(np.float64); d = rays["d"].astype(np.float64)
    t_plane = -o[:, 2] / d[:, 2]
    near = (want["prim"] != MISS) & (np.abs(want["t"] - t_plane) <= 1e-5 * np.abs(t_plane))
    assert (near & on_sphere).sum() >= 10 and (near & on_mesh).sum() >= 10, (int((near & on_sphere).sum()), int((near & on_mesh).sum()))
    prod.close(); orc.close()


# ---- 3. work counters ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", QA.MASKS)
def test_work_counters(host, mask):
    prod, orc, _ = pair(host, QA.mixed_scene, mask=mask, shadow=True, max_prims=4)
    rays = QA.grid_rays()
    with QA.libm1():
        want, wst = orc.intersect_batch_stats(rays); wocc, wost = orc.occluded_batch_stats(rays)
    prod.set_traversal_counting(True)
    prod.traversal_counts()
    got = prod.intersect_batch(rays); cnt_c = prod.traversal_counts()
    gocc = prod.occluded_batch(rays); cnt_a = prod.traversal_counts()
    prod.set_traversal_counting(False)
    assert_hits_equal(got, want, "counting row, closest hit")
    assert np.array_equal(gocc, wocc)
    assert (cnt_c["closest"]["rays"], cnt_c["closest"]["tri_tests"], cnt_c["closest"]["ref_node_visits"]) == (wst.rays, wst.tri_tests, wst.nodes_visited)
    assert (cnt_a["any_hit"]["rays"], cnt_a["any_hit"]["tri_tests"], cnt_a["any_hit"]["ref_node_visits"]) == (wost.rays, wost.tri_tests, wost.nodes_visited)
    assert wst.tri_tests > len(rays) // 2
    assert_hits_equal(prod.intersect_batch(rays), want, "timed row after counting")
    prod.close(); orc.close()


# ---- 4. path films ---------------------------------------------------------------------------------------------------------------------------------------------
PATH_CASES = [("halton", 0.0, 0, 5), ("halton", 0.0, 1, 5), ("halton", 0.0, 2, 5), ("sobol", 0.05, 2, 5)]   # sampler, lens radius, light strategy, depth


@pytest.mark.parametrize("sampler,lens,light_strategy,depth", PATH_CASES, ids=[f"{c[0]}-ls{c[2]}" for c in PATH_CASES])
@pytest.mark.parametrize("mask", QA.MASKS)
def test_path_films(host, monkeypatch, mask, sampler, lens, light_strategy, depth):
    prod, orc, _ = pair(host, QA.mixed_scene, mask=mask, shadow=True, res=(48, 32), spp=4, sampler=sampler, lens=lens)
    kw = dict(max_depth=depth, light_strategy=light_strategy)
    with QA.libm1():
        want = orc.render_path_ex(**kw)
    x, w, st = prod.render_path(**kw)
    assert_films_equal((x, w, st), want, "whole frame")
    assert st.shadow_rays > 0 and st.regular_rays > st.camera_rays
    monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(48 * 32 * 4 // 3 - 100))   # 6 144 paths in chunks of at most 1 948: three full chunks and a ragged fourth; the film must not depend on it
    x2, w2, st2 = prod.render_path(**kw)
    assert_films_equal((x2, w2, st2), want, "chunked")
    # tile parts (0, 2) and (1, 2): each equals the oracle's part, their sum the whole frame; then the same through device tile buffers
    acc = np.zeros_like(x); accw = np.zeros_like(w); bufs = []
    for part in range(2):
        with QA.libm1():
            ox, ow, _, _ = orc.render_path_ex(tile_part=part, tile_parts=2, **kw)
        px, pw, _ = prod.render_path(tile_part=part, tile_parts=2, **kw)
        assert np.array_equal(px.view(np.uint32), ox.view(np.uint32)) and np.array_equal(pw, ow), part
        acc += px; accw += pw
        buf = torch.full((prod.tile_buffer_floats(16, part, 2),), float("nan"), dtype=torch.float32, device="cuda")
        prod.render_path_tiles_device(buf.data_ptr(), tile_part=part, tile_parts=2, **kw)
        bufs.append(buf)
    monkeypatch.delenv("PBRT_HIP_MAX_PATHS")
    assert np.array_equal(accw, w) and np.array_equal(acc.view(np.uint32), x.view(np.uint32))   # the parts' tiles are disjoint: the sums are exact
    mx, mw = prod.merge_tiles_device([b.data_ptr() for b in bufs])
    assert np.array_equal(mw.view(np.uint32), w.view(np.uint32)) and np.array_equal(mx.view(np.uint32), x.view(np.uint32))
    prod.close(); orc.close()


# ---- 5. Whitted films ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", QA.MASKS)
def test_whitted_films_with_a_sphere_light_over_a_shadow_alpha_mask(host, mask):
    prod, orc, _ = pair(host, QA.mixed_scene, mask=mask, shadow=True, whitted=True, res=(32, 24), spp=4)
    want = oracle_whitted(orc, max_depth=3)
    got = prod.render_whitted(max_depth=3)
    assert_films_equal(got, want, "whitted " + mask)
    assert got[2].shadow_rays > 0 and got[2].regular_rays > got[2].camera_rays
    # the shadow-alpha mask matters to this film: without it the oracle's differs
    with OracleScene() as orc2:
        with QA.libm1():
            QA.mixed_scene(orc2, host, mask=mask, shadow=False, whitted=True, res=(32, 24), spp=4)
        assert not np.array_equal(oracle_whitted(orc2, max_depth=3)[0], want[0])
    prod.close(); orc.close()


# ---- 6. the multi-device handle --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", QA.MASKS)
def test_multi_device_film_equals_one_device_film(host, mask):
    one = pbrt_hip.Scene(); multi = pbrt_hip.Scene(devices=[0, 0])
    for s in (one, multi):
        QA.mixed_scene(s, host, mask=mask, shadow=True)
    x1, w1, st1 = one.render_path(max_depth=5)
    xn, wn, stn = multi.render_path(max_depth=5)
    assert np.array_equal(xn.view(np.uint32), x1.view(np.uint32)) and np.array_equal(wn, w1)
    assert (stn.camera_rays, stn.regular_rays, stn.shadow_rays) == (st1.camera_rays, st1.regular_rays, st1.shadow_rays)
    with OracleScene() as orc:
        with QA.libm1():
            QA.mixed_scene(orc, host, mask=mask, shadow=True)
            ox = orc.render_path_ex(max_depth=5)[0]
    assert np.array_equal(xn.view(np.uint32), ox.view(np.uint32))
    one.close(); multi.close()


# ---- 7. what stays refused -------------------------------------------------------------------------------------------------------------------------------------
def _masked_mesh_and_quadric(s, host):
    """the mixed stage's two kinds of shape, not built: a masked mesh, then a sphere as the shape added last"""
    m = s.add_material_matte((0.5, 0.5, 0.5))
    s.add_light_infinite((1, 1, 1))
    P, idx = scenes.grid_mesh(4, z=0.0, size=QA.GRID)
    s.add_mesh(P, idx, m, UV=((P[:, :2] + QA.GRID) / (2 * QA.GRID)).astype(np.float32))
    s.set_last_mesh_alpha_textures(*QA.mask_textures(s, "checkerboard", shadow=True))
    s.add_sphere(*QA.cf_ctm(host, host.translate((0.0, 0.0, -1.0))), 0.5, None, None, 360.0, m, False)
    return m


def test_refusals_that_do_not_depend_on_the_mixed_rows(host):
    """These hold with and without the quadric rows with alpha: a mask ON a quadric, the device builder on a quadric scene, object definitions next to quadrics (the "object"
    message also where the scene has an alpha mask too)."""
    with pbrt_hip.Scene() as s:
        _masked_mesh_and_quadric(s, host)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.set_last_mesh_alpha_textures(s.add_texture_constant(0.0), None)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.build_accel_device(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
    with pbrt_hip.Scene() as s:
        m = _masked_mesh_and_quadric(s, host)
        s.object_begin()
        s.add_mesh(np.array([[-1, -1, 3], [1, -1, 3], [0, 1, 3]], np.float32), np.array([0, 2, 1], np.uint32), m)
        s.object_end()
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.build_accel(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object" in str(e.value)


def test_a_mixed_scene_renders_after_the_refusals(host):
    with pbrt_hip.Scene() as s, OracleScene() as orc:
        QA.mixed_scene(s, host, mask="checkerboard", shadow=True)
        with QA.libm1():
            QA.mixed_scene(orc, host, mask="checkerboard", shadow=True)
        for sc in (s, orc):
            sc.add_sphere(*QA.cf_ctm(host, host.translate((0.0, 0.0, 9.0))), 0.1, None, None, 360.0, 0, False)   # (behind the camera)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:   # an alpha mask ON a quadric
            s.set_last_mesh_alpha_textures(s.add_texture_constant(0.0), None)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:   # the device builders leave quadric scenes to the host builders
            s.build_accel_device(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
        s.build_accel_best(0, 4)                          # ... and the handle still builds and renders
        with QA.libm1():
            orc.build_accel(0, 4)
            want = orc.render_path_ex(max_depth=3)
        assert_films_equal(s.render_path(max_depth=3), want, "after the refusals")
