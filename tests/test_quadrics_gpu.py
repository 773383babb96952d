"""-m gpu: the reference's six quadric shapes (sphere, cylinder, disk, cone, paraboloid, hyperboloid) on the device, through pbrt_hip_add_sphere / _add_quadric /
_add_hyperboloid.  Every comparison is against the CPU oracle in libm mode 1 and on bits (`view(np.uint32)`), never against the device's own output: ray batches per kind,
quadrics mixed into triangle leaves with the traversal work counters, the rays a path tracer spawns off quadric hits (p, p_error, n), films (configs[0] of BASELINE.json, the
reference's textured six-shape and bump-mapped scenes, every material and light strategy, both samplers, chunking, tile parts), a closed form, the reference's own silhouettes of
configs[0], the refusals and the multi-device handle.

The scene builders of tests/reference_scenes.py and tests/test_oracle_sphere.py reach the oracle's entry points directly.  `generic_adders()` swaps their three shape helpers for
the ones below, which go through pbrt_hip.Scene.add_sphere / add_quadric / add_hyperboloid and therefore serve either binding: that is the product-side twin of those scenes."""
import contextlib
import os

import numpy as np
import pytest

import pbrt_hip
import reference_scenes as R
import test_oracle_sphere as TS
from oracle_binding import OracleScene, set_libm_mode

pytestmark = pytest.mark.gpu
IDENT = (pbrt_hip.IDENTITY.copy(), pbrt_hip.IDENTITY.copy())
MISS = 0xFFFFFFFF
KINDS = ("sphere", "cylinder", "disk", "cone", "paraboloid", "hyperboloid")


# ---- one way to add a shape to either binding --------------------------------------------------------------------------------------------------------------
def add_sphere(scene, t, radius=1.0, zmin=None, zmax=None, phimax=360.0, material=0, reverse=False):
    scene.add_sphere(t[0], t[1], radius, zmin, zmax, phimax, material, reverse)


def add_quadric(scene, kind, t, radius, a, b, phimax=360.0, material=0, reverse=False):
    scene.add_quadric(kind, t[0], t[1], radius, a, b, phimax, material, reverse)


def add_hyperboloid(scene, t, p1, p2, phimax=360.0, material=0, reverse=False):
    scene.add_hyperboloid(t[0], t[1], p1, p2, phimax, material, reverse)


@contextlib.contextmanager
def generic_adders():
    saved = (TS.add_sphere, R.add_quadric, R.add_hyperboloid)
    TS.add_sphere, R.add_quadric, R.add_hyperboloid = add_sphere, add_quadric, add_hyperboloid
    try:
        yield
    finally:
        TS.add_sphere, R.add_quadric, R.add_hyperboloid = saved


@contextlib.contextmanager
def libm1():
    set_libm_mode(1)
    try:
        yield
    finally:
        set_libm_mode(0)


def add_shape(scene, kind, partial, t, material, reverse=False):
    """A full shape, or one cut in z and at phi_max 250 degrees"""
    phi = 250.0 if partial else 360.0
    if kind == "sphere":
        add_sphere(scene, t, 1.0, -0.6 if partial else None, 0.7 if partial else None, phi, material, reverse)
    elif kind == "cylinder":
        add_quadric(scene, "cylinder", t, 0.8, -0.6 if partial else -1.0, 0.6 if partial else 1.0, phi, material, reverse)
    elif kind == "cone":
        add_quadric(scene, "cone", t, 0.8, 1.0, 0.0, phi, material, reverse)
    elif kind == "paraboloid":
        add_quadric(scene, "paraboloid", t, 0.8, 0.2 if partial else 0.0, 1.0, phi, material, reverse)
    elif kind == "disk":
        add_quadric(scene, "disk", t, 0.9, 0.1, 0.3 if partial else 0.0, phi, material, reverse)
    else:
        add_hyperboloid(scene, t, (0.6, 0.6, 0.8), (0.6, -0.6, -0.8), phi, material, reverse)


def first_root_f64(kind, partial, w2o, rays):
    """float64 roots of the shape's implicit quadratic along each ray (object space): the smaller one where it is positive, else NaN.  A hit whose t lies clearly beyond it
    is a second-root hit: the first root was clipped away."""
    M = np.asarray(w2o, np.float64).reshape(4, 4)
    o = rays["o"].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    d = rays["d"].astype(np.float64) @ M[:3, :3].T
    ox, oy, oz = o.T; dx, dy, dz = d.T
    if kind == "sphere":
        a = dx * dx + dy * dy + dz * dz; b = 2 * (dx * ox + dy * oy + dz * oz); c = ox * ox + oy * oy + oz * oz - 1.0
    elif kind == "cylinder":
        a = dx * dx + dy * dy; b = 2 * (dx * ox + dy * oy); c = ox * ox + oy * oy - 0.8 ** 2
    elif kind == "cone":
        k = (0.8 / 1.0) ** 2
        a = dx * dx + dy * dy - k * dz * dz; b = 2 * (dx * ox + dy * oy - k * dz * (oz - 1.0)); c = ox * ox + oy * oy - k * (oz - 1.0) ** 2
    elif kind == "paraboloid":
        k = 1.0 / 0.8 ** 2
        a = k * (dx * dx + dy * dy); b = 2 * k * (dx * ox + dy * oy) - dz; c = k * (ox * ox + oy * oy) - oz
    elif kind == "hyperboloid":
        p1, p2 = np.array([0.6, 0.6, 0.8]), np.array([0.6, -0.6, -0.8])
        pp = p1 + 2 * (p2 - p1)
        xy1, xy2 = pp[0] ** 2 + pp[1] ** 2, p2[0] ** 2 + p2[1] ** 2
        ah = (1 / xy1 - pp[2] ** 2 / (xy1 * p2[2] ** 2)) / (1 - xy2 * pp[2] ** 2 / (xy1 * p2[2] ** 2)); ch = (ah * xy2 - 1) / p2[2] ** 2
        a = ah * (dx * dx + dy * dy) - ch * dz * dz; b = 2 * (ah * (dx * ox + dy * oy) - ch * dz * oz); c = ah * (ox * ox + oy * oy) - ch * oz * oz - 1
    else:
        return None
    with np.errstate(all="ignore"):
        disc = b * b - 4 * a * c
        q = np.where(b < 0, -0.5 * (b - np.sqrt(disc)), -0.5 * (b + np.sqrt(disc)))
        t0, t1 = np.minimum(q / a, c / q), np.maximum(q / a, c / q)
    return np.where((disc >= 0) & (t0 > 1e-3), t0, np.nan)


def mk_rays(o, d, t_max=np.inf):
    r = np.zeros(len(o), pbrt_hip.RAY_DTYPE)
    r["o"] = np.asarray(o, np.float32); r["d"] = np.asarray(d, np.float32); r["t_max"] = t_max
    return r


def transforms(host):
    rst = host.compose(host.compose(host.translate((0.1, -0.05, 0.2)), host.rotate(35.0, (1.0, 2.0, 0.5))), host.scale((1.1, 0.7, 1.3)))
    mirror = host.compose(host.rotate(20.0, (0, 1, 0)), host.scale((-1.0, 1.2, 0.9)))
    return [("identity", IDENT, False), ("rotate-scale-translate", rst, False), ("mirror", mirror, False), ("mirror-reversed", mirror, True)]


def object_gradient(kind, q):
    """gradient of the kind's implicit quadratic at the object-space points q (the shapes of add_shape)"""
    x, y, z = q.T; zero = np.zeros_like(x)
    if kind == "sphere": g = (x, y, z)
    elif kind == "cylinder": g = (x, y, zero)
    elif kind == "cone": g = (x, y, -(0.8 / 1.0) ** 2 * (z - 1.0))
    elif kind == "paraboloid": g = (2 * x / 0.8 ** 2, 2 * y / 0.8 ** 2, -np.ones_like(x))
    else:
        p1, p2 = np.array([0.6, 0.6, 0.8]), np.array([0.6, -0.6, -0.8])
        pp = p1 + 2 * (p2 - p1)
        xy1, xy2 = pp[0] ** 2 + pp[1] ** 2, p2[0] ** 2 + p2[1] ** 2
        ah = (1 / xy1 - pp[2] ** 2 / (xy1 * p2[2] ** 2)) / (1 - xy2 * pp[2] ** 2 / (xy1 * p2[2] ** 2)); ch = (ah * xy2 - 1) / p2[2] ** 2
        g = (ah * x, ah * y, -ch * z)
    return np.stack(g, -1)


def tangent_rays(kind, partial, t, hp, rng):
    M = np.asarray(t[0], np.float64).reshape(4, 4); Mi = np.asarray(t[1], np.float64).reshape(4, 4)
    if kind == "disk":   # rays from outside through points a few ulps inside / outside the rim (and the inner radius)
        k = 20_000
        rho = np.where(rng.integers(0, 2, k) == 0, 0.9, 0.3 if partial else 0.9) * (1.0 + rng.integers(-4, 5, k) * 2.0 ** -23)
        phi = rng.uniform(0, np.radians(250.0 if partial else 360.0), k)
        tgt = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(k, 0.1)], -1) @ M[:3, :3].T + M[:3, 3]
        o = rng.normal(size=(k, 3)); o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
        return mk_rays(o, tgt - o)
    q = hp @ Mi[:3, :3].T + Mi[:3, 3]
    nw = object_gradient(kind, q) @ Mi[:3, :3]            # normals transform by the inverse transpose
    nw /= np.linalg.norm(nw, axis=1, keepdims=True)
    tdir = np.cross(nw, rng.normal(size=nw.shape)); tdir /= np.linalg.norm(tdir, axis=1, keepdims=True)
    eps = rng.integers(-4, 5, size=(len(hp), 1)) * 2.0 ** -22
    return mk_rays(hp - 3.0 * tdir + nw * eps, tdir)


def recorded_rays_of(orc, host):
    """The closest-hit and shadow rays of a small path-traced frame of the oracle's scene (its camera, film and sampler are set here; the light was added with the shape)"""
    TS._camera(orc, host, (0.5, -3.0, 2.6), (0, 0, 0), (0, 0, 1), 35.0, 48, 48, 4)   # from above: the disk is not seen edge-on
    orc.record_rays(1 << 20)
    with libm1():
        orc.render_path_ex(max_depth=3)
    return orc.recorded_rays(False), orc.recorded_rays(True)


def check_batches(prod, orc, rays, what, quadric_only=True):
    with libm1():
        want = orc.intersect_batch(rays); wocc = orc.occluded_batch(rays)
    got = prod.intersect_batch(rays); gocc = prod.occluded_batch(rays)
    assert np.array_equal(got["prim"], want["prim"]), what
    assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32)), what
    for f in ("b0", "b1", "b2"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), what
    if quadric_only:
        assert not (got["b0"].view(np.uint32) | got["b1"].view(np.uint32) | got["b2"].view(np.uint32)).any(), what   # a quadric hit reports zero barycentrics
    assert not got["pad"][:, 1].any(), what
    assert np.array_equal(gocc.astype(bool), wocc.astype(bool)), what
    return want, wocc


# ---- 1. batches, per kind -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partial", [False, True], ids=["full", "partial"])
@pytest.mark.parametrize("kind", KINDS)
def test_batches_per_kind(host, kind, partial):
    n = 200_000
    for tname, t, reverse in transforms(host):
        rng = np.random.default_rng(1000 * KINDS.index(kind) + 100 * int(partial) + len(tname))
        prod = pbrt_hip.Scene(); orc = OracleScene()
        for s in (prod, orc):
            m = s.add_material_matte((0.5, 0.5, 0.5))
            s.add_light_infinite((1.0, 1.0, 1.0))
            add_shape(s, kind, partial, t, m, reverse)
            s.build_accel(0, 4)
        M = np.asarray(t[0], np.float64).reshape(4, 4)
        to_world = lambda p: (np.asarray(p, np.float64) @ M[:3, :3].T + M[:3, 3])
        what = f"{kind} {'partial' if partial else 'full'} {tname}"
        # (a) shell: origins on a shell of radius 4 aimed at uniform points of a box slightly larger than the shape
        o = rng.normal(size=(n, 3)); o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
        tgt = to_world(rng.uniform(-1.1, 1.1, size=(n, 3)) * (1.0, 1.0, 1.0))
        shell = mk_rays(o, tgt - o)
        want, wocc = check_batches(prod, orc, shell, what + " shell")
        hit = want["prim"] != MISS
        assert 0.10 <= hit.mean() <= 0.90, (what, float(hit.mean()))               # the case is not empty: asserted on the ORACLE's verdicts
        assert np.array_equal(wocc.astype(bool), hit), what                         # any hit == closest hit on one shape
        if partial and kind != "disk":   # (a disk is a plane: one root, nothing to retry)
            t0 = first_root_f64(kind, partial, t[1], shell)
            second = hit & np.isfinite(t0) & (want["t"] > t0 * (1 + 1e-3))
            assert second.sum() >= 0.01 * hit.sum(), (what, int(second.sum()), int(hit.sum()))
        # (b) finite t_max drawn between and beyond the roots
        tm = np.where(hit, want["t"], 4.0).astype(np.float32) * rng.uniform(0.5, 3.0, n).astype(np.float32)
        check_batches(prod, orc, mk_rays(shell["o"], shell["d"], tm), what + " finite t_max")
        k = n // 4
        # (c) origins inside the shape's box
        oi = to_world(rng.uniform(-0.5, 0.5, size=(k, 3)))
        check_batches(prod, orc, mk_rays(oi, rng.normal(size=(k, 3))), what + " inside")
        # (d) origins ON the surface (a previous hit's point), leaving in every direction; half of them with a short t_max
        hp = (shell["o"].astype(np.float64) + shell["d"].astype(np.float64) * want["t"][:, None].astype(np.float64))[hit][:k]
        on = mk_rays(hp, rng.normal(size=(len(hp), 3)))
        on["t_max"][::2] = np.float32(1.0 - 1e-4)
        check_batches(prod, orc, on, what + " on the surface")
        # (e) tangent within a few ulps: through hit points, along a direction perpendicular to the surface's REAL normal (the gradient of the kind's implicit form in object space,
        #     carried to world space by the inverse transpose), the origin moved off the tangent plane by -4 .. 4 steps of 2^-22 along that normal: the discriminant is a few ulps
        #     either side of zero, the roots nearly double.  The disk is a plane: its rays graze the rim and the inner radius instead.
        tang = tangent_rays(kind, partial, t, hp, rng)
        twant, _ = check_batches(prod, orc, tang, what + " tangent")
        thit = twant["prim"] != MISS
        assert thit.mean() >= 0.01 and (~thit).mean() >= 0.01, (what, "tangent family", float(thit.mean()))   # neither verdict is missing: asserted on the ORACLE's
        # (e') the rays the oracle's own path tracer spawns off this shape (spawn_ray / spawn_ray_to from the refined p, p_error and n): recorded on the oracle, traced by both
        reg, sh = recorded_rays_of(orc, host)
        assert len(reg) > 2000 and len(sh) > 200, (what, len(reg), len(sh))   # the frame does look at the shape
        with libm1():
            rwant = orc.intersect_batch(reg); swant = orc.occluded_batch(sh)
        rgot = prod.intersect_batch(reg)
        assert np.array_equal(rgot["prim"], rwant["prim"]) and np.array_equal(rgot["t"].view(np.uint32), rwant["t"].view(np.uint32)), what + " recorded"
        assert np.array_equal(prod.occluded_batch(sh).astype(bool), swant.astype(bool)), what + " recorded shadow"
        # (f) axis-parallel rays and rays with a zero direction component
        ax = np.zeros((6 * 2000, 3)); oa = rng.uniform(-1.2, 1.2, size=ax.shape)
        for j in range(6):
            ax[j * 2000:(j + 1) * 2000, j % 3] = 1.0 if j < 3 else -1.0
            oa[j * 2000:(j + 1) * 2000, j % 3] = -3.0 if j < 3 else 3.0
        check_batches(prod, orc, mk_rays(to_world(oa), ax), what + " axis-parallel")
        dz = rng.normal(size=(6000, 3)); dz[np.arange(6000), rng.integers(0, 3, 6000)] = 0.0
        check_batches(prod, orc, mk_rays(to_world(rng.uniform(-1.5, 1.5, size=(6000, 3))), dz), what + " zero component")
        prod.close(); orc.close()


# ---- 2. mixed leaves ----------------------------------------------------------------------------------------------------------------------------------------
def scatter_quadrics(s, host, m, n=200, seed=5):
    rng = np.random.default_rng(seed)
    for i in range(n):
        c = rng.uniform(-0.9, 0.9, 3); sc = rng.uniform(0.02, 0.08)
        t = host.compose(host.compose(host.translate(tuple(c)), host.rotate(float(rng.uniform(0, 360)), tuple(rng.normal(size=3)))), host.scale((sc, sc * rng.uniform(0.5, 1.5), sc)))
        add_shape(s, KINDS[i % 6], bool(i & 8), t, m, bool(i & 16))


@pytest.mark.parametrize("max_prims", [4, 1])
def test_mixed_leaves_and_work_counters(host, max_prims):
    P, idx = host.gen_random_tris(50_000, 11)
    prod = pbrt_hip.Scene(); orc = OracleScene()
    for s in (prod, orc):
        m = s.add_material_matte((0.5, 0.5, 0.5))
        half = len(idx) // 6 * 3
        s.add_mesh(P, idx[:half], m)
        scatter_quadrics(s, host, m)                     # quadrics sit between the two meshes in the primitive list
        s.add_mesh(P, idx[half:], m)
        s.build_accel(0, max_prims)
    import scenes
    rays = scenes.random_rays(300_000, 3)
    with libm1():
        want, wst = orc.intersect_batch_stats(rays); wocc, wost = orc.occluded_batch_stats(rays)
    prod.set_traversal_counting(True)
    prod.traversal_counts()
    got = prod.intersect_batch(rays); cnt_c = prod.traversal_counts()
    gocc = prod.occluded_batch(rays); cnt_a = prod.traversal_counts()
    prod.set_traversal_counting(False)
    assert scenes.hits_equal(got, want).all()
    assert np.array_equal(gocc, wocc)
    quad_prims = np.flatnonzero((want["prim"] != MISS) & (want["b0"] == 0) & (want["b1"] == 0) & (want["b2"] == 0))
    assert len(quad_prims) > 100                         # quadrics ARE hit
    assert (cnt_c["closest"]["rays"], cnt_c["closest"]["tri_tests"], cnt_c["closest"]["ref_node_visits"]) == (wst.rays, wst.tri_tests, wst.nodes_visited)
    assert (cnt_a["any_hit"]["rays"], cnt_a["any_hit"]["tri_tests"], cnt_a["any_hit"]["ref_node_visits"]) == (wost.rays, wost.tri_tests, wost.nodes_visited)
    prod.close(); orc.close()


# ---- scenes for the films -----------------------------------------------------------------------------------------------------------------------------------
def materials_scene(s, host, xres=64, yres=48, spp=4, sampler="halton", lens=0.0):
    """glass, mirror, metal, plastic, uber (and matte) quadrics over a triangle floor, under an infinite light and a triangle area light"""
    s.add_light_infinite((0.4, 0.45, 0.5))
    mats = [s.add_material_glass((1, 1, 1), (1, 1, 1), 0.0, 0.0, 1.5), s.add_material_mirror((0.9, 0.9, 0.9)), s.add_material_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.05, 0.05),
            s.add_material_plastic((0.3, 0.1, 0.1), (0.4, 0.4, 0.4), 0.1), s.add_material_uber((0.25, 0.25, 0.25), (0.25, 0.25, 0.25), (0.1, 0.1, 0.1), (0.3, 0.3, 0.3), (0.9, 0.9, 0.9), 0.1, 0.1, 1.4),
            s.add_material_matte((0.5, 0.4, 0.3), 20.0)]
    floor = s.add_material_matte((0.5, 0.5, 0.5))
    s.add_mesh(np.array([[-6, -6, -1], [6, -6, -1], [6, 6, -1], [-6, 6, -1]], np.float32), np.array([0, 1, 2, 0, 2, 3], np.uint32), floor)
    for i, m in enumerate(mats):
        x = -2.5 + i
        t = host.compose(host.translate((x, 0.3 * (i % 2), -0.55)), host.rotate(30.0 * i, (1, 0, 1)))
        if i % 3 == 0: add_sphere(s, t, 0.45, material=m)
        elif i % 3 == 1: add_quadric(s, "cylinder", t, 0.35, -0.4, 0.4, 300.0, m)
        else: add_hyperboloid(s, t, (0.4, 0.0, 0.4), (0.25, 0.3, -0.4), 360.0, m)
    for i, (kind, a, b) in enumerate((("cone", 0.7, 0.0), ("paraboloid", 0.1, 0.6), ("disk", 0.2, 0.1))):   # the other three kinds, behind the first row
        t = host.compose(host.translate((-1.5 + 1.5 * i, 1.6, -0.8)), host.rotate(20.0 * (i + 1), (1, 0.5, 0)))
        add_quadric(s, kind, t, 0.4, a, b, 360.0 if i else 280.0, mats[(2 * i + 1) % 6])
    lid = s.add_light_diffuse_area((8, 8, 8), 2)
    s.add_mesh(np.array([[-1, -1, 2.5], [1, -1, 2.5], [1, 1, 2.5], [-1, 1, 2.5]], np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32), floor, first_area_light=lid)
    w2c, c2w = host.look_at((0, -7, 2.5), (0, 0, -0.4), (0, 0, 1))
    s.set_camera_perspective(host.perspective_raster_to_camera(40.0, xres, yres), c2w, lens_radius=lens, focal_distance=7.0)
    cb, table, sb = host.film_box(xres, yres)
    s.set_film(xres, yres, cb, (0.5, 0.5), table)
    if sampler == "sobol":
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sobol_subset.npz"))
        s.set_sobol_tables(z["m32"], z["vdc"], z["vdc_inv"])
        s.set_sampler(1, spp, sb)
    else:
        s.set_sampler(0, spp, sb)
    s.build_accel(0, 4)


def films_equal(prod, orc, **kw):
    with libm1():
        oxyz, owt, ost, _ = orc.render_path_ex(**kw)
    gxyz, gwt, gst = prod.render_path(**kw)
    assert np.array_equal(gwt.view(np.uint32), owt.view(np.uint32))
    nd = int((gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(axis=2).sum())
    assert nd == 0, (nd, float(np.abs(gxyz - oxyz).max()))
    for f in ("camera_rays", "regular_rays", "shadow_rays"):
        assert getattr(gst, f) == getattr(ost, f), f
    return gxyz, gwt, gst


# ---- 3. recorded path rays ----------------------------------------------------------------------------------------------------------------------------------
def test_recorded_path_rays_bit_exact(host):
    """The rays the oracle's path tracer spawns off quadric hits (bounce, MIS and shadow rays: spawn_ray / spawn_ray_to from p, p_error, n) are the rays the device spawns: the
    films agree bit for bit below; here the oracle's recorded rays are traced by the device, origins ON the quadrics included."""
    prod = pbrt_hip.Scene(); orc = OracleScene()
    for s in (prod, orc):
        materials_scene(s, host, 48, 36, 2)
    orc.record_rays(1 << 20)
    with libm1():
        orc.render_path_ex(max_depth=4)
        reg, sh = orc.recorded_rays(False), orc.recorded_rays(True)
        assert len(reg) > 4000 and len(sh) > 1000
        want, _ = orc.intersect_batch_stats(reg); wocc = orc.occluded_batch_stats(sh)[0]
    import scenes
    assert scenes.hits_equal(prod.intersect_batch(reg), want).all()
    assert np.array_equal(prod.occluded_batch(sh), wocc)
    prod.close(); orc.close()


# ---- 4. films -----------------------------------------------------------------------------------------------------------------------------------------------
def test_film_configs0(host):
    """BASELINE.json configs[0]: scenes/shapes/sphere.pbrt under the path integrator, maxdepth 4, 16 spp"""
    prod = pbrt_hip.Scene(); orc = OracleScene()
    with libm1():   # (the oracle's Sphere::new evaluates acos when the scene is captured)
        TS.configs0_scene(orc, host, 160, 80, 16)
    with generic_adders():
        TS.configs0_scene(prod, host, 160, 80, 16)
    films_equal(prod, orc, max_depth=4)
    prod.close(); orc.close()


@pytest.mark.parametrize("which", ["uv", "marble", "2d-checkerboard", "bump"])
def test_film_textured_shapes(host, which):
    """uv-dependent and 3-D textures on all six shapes, and the bump-mapped sphere: texture context, camera-ray differentials, dn/du and dn/dv"""
    prod = pbrt_hip.Scene(); orc = OracleScene()
    if which == "bump":
        with libm1():
            info = R.materials_bump(orc, host, spp=8, res=96)
        with generic_adders():
            R.materials_bump(prod, host, spp=8, res=96)
    else:
        with libm1():
            info = R.textures_six_shapes(orc, host, which, spp=8)
        with generic_adders():
            R.textures_six_shapes(prod, host, which, spp=8)
        for s in (prod, orc):
            R.camera_film(s, host, (0, 22, 0), (0, 0, 0), (0, 0, 1), 15.0, 96, 96, 8)
    films_equal(prod, orc, max_depth=info["max_depth"])
    prod.close(); orc.close()


@pytest.mark.parametrize("light_strategy", [0, 1, 2])
def test_film_every_material_every_light_strategy(host, light_strategy):
    prod = pbrt_hip.Scene(); orc = OracleScene()
    for s in (prod, orc):
        materials_scene(s, host)
    films_equal(prod, orc, max_depth=5, light_strategy=light_strategy)
    prod.close(); orc.close()


@pytest.mark.parametrize("sampler", ["halton", "sobol"])
def test_film_samplers_thin_lens_chunks_and_tile_parts(host, sampler, monkeypatch):
    """(maxdepth 4: the Sobol tables of tests/golden/sobol_subset.npz hold the 45 dimensions such a path draws)"""
    prod = pbrt_hip.Scene(); orc = OracleScene()
    for s in (prod, orc):
        materials_scene(s, host, 64, 48, 4, sampler=sampler, lens=0.05)
    x, w, st = films_equal(prod, orc, max_depth=4)
    monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(64 * 48 * 3 // 2))   # forced chunking: the film must not depend on it
    x2, w2, st2 = prod.render_path(max_depth=4)
    monkeypatch.delenv("PBRT_HIP_MAX_PATHS")
    assert np.array_equal(x2.view(np.uint32), x.view(np.uint32)) and np.array_equal(w2, w) and st2.regular_rays == st.regular_rays
    acc = np.zeros_like(x); accw = np.zeros_like(w)
    for part in range(3):
        with libm1():
            ox, ow, _, _ = orc.render_path_ex(max_depth=4, tile_part=part, tile_parts=3)
        px, pw, _ = prod.render_path(max_depth=4, tile_part=part, tile_parts=3)
        assert np.array_equal(px.view(np.uint32), ox.view(np.uint32)) and np.array_equal(pw, ow)
        acc += px; accw += pw
    assert np.array_equal(accw, w)                                    # the parts' tiles are disjoint: the sums are exact
    assert np.array_equal(acc.view(np.uint32), x.view(np.uint32))
    prod.close(); orc.close()


# ---- 5. closed form on the device ----------------------------------------------------------------------------------------------------------------------------
def test_white_furnace_on_a_sphere_on_the_device(host):
    """test_oracle_sphere.py::test_white_furnace_on_a_sphere rendered by the device, with that test's tolerances: E = Kd * L on the sphere, exactly L beside it"""
    with pbrt_hip.Scene() as s:
        m = s.add_material_matte((0.6, 0.6, 0.6))
        s.add_light_infinite((1.0, 1.0, 1.0))
        add_sphere(s, IDENT, 1.0, material=m)
        TS._camera(s, host, (0, -4, 0), (0, 0, 0), (0, 0, 1), 35.0, 48, 48, 64)
        s.build_accel(0, 4)
        xyz, wt, st = s.render_path(max_depth=5)
        rgb = s.film_to_rgb(xyz, wt)
    centre = rgb[16:32, 16:32]
    assert abs(centre.mean() - 0.6) < 0.01
    assert np.allclose(rgb[0, 0], 1.0, atol=1e-6) and np.allclose(rgb[47, 47], 1.0, atol=1e-6)
    assert st.shadow_rays > 0 and st.regular_rays > 48 * 48 * 64


# ---- 6. the reference's own pixels ---------------------------------------------------------------------------------------------------------------------------
def test_configs0_silhouettes_equal_the_references_own_render_on_the_device(host):
    """The criterion of test_oracle_sphere.py::test_configs0_silhouettes_equal_the_references_own_render on the device film"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sphere_sky_mask.npz"))
    h, w = (int(v) for v in z["shape"])
    sky = np.unpackbits(z["sky"])[: h * w].reshape(h, w).astype(bool)
    with pbrt_hip.Scene() as s:
        with generic_adders():
            TS.configs0_scene(s, host, w, h, 4)
        xyz, wt, _ = s.render_path(max_depth=1)
        rgb = s.film_to_rgb(xyz, wt)
    mine = np.all(np.abs(rgb - np.array([1.2, 1.2, 1.1], np.float32)) < 1e-4, -1)

    def interior(m):
        p = np.pad(m, 1, mode="edge"); out = np.ones_like(m)
        for dy in range(3):
            for dx in range(3):
                out &= p[dy:dy + h, dx:dx + w]
        return out
    in_sky, in_obj = interior(sky), interior(~sky)
    assert in_sky.sum() + in_obj.sum() > 0.975 * h * w
    assert not np.any(in_sky & ~mine) and not np.any(in_obj & mine)
    assert (sky != mine).mean() < 0.006


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(host):
    with pbrt_hip.Scene() as s:
        m = s.add_material_matte((0.5, 0.5, 0.5))
        s.add_light_infinite((1, 1, 1))
        # a quadric between object_begin and object_end
        s.object_begin()
        for add in (lambda: add_sphere(s, IDENT, 1.0, material=m), lambda: add_quadric(s, "cone", IDENT, 1.0, 1.0, 0.0, material=m), lambda: add_hyperboloid(s, IDENT, (1, 0, 0), (1, 0, 1), material=m)):
            with pytest.raises(pbrt_hip.PbrtHipError) as e:
                add()
            assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object" in str(e.value)
        s.object_end()
        add_sphere(s, IDENT, 1.0, material=m)           # outside the definition it is accepted ...
        with pytest.raises(pbrt_hip.PbrtHipError) as e:   # ... but a scene with object definitions and quadrics is not built
            s.build_accel(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "object" in str(e.value)
    with pbrt_hip.Scene() as s:
        m = s.add_material_matte((0.5, 0.5, 0.5))
        s.add_light_infinite((1, 1, 1))
        # a quadric as the shape of a diffuse area light
        lid = s.add_light_diffuse_area((5, 5, 5), 1)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            add_sphere(s, IDENT, 1.0, material=m)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "area light" in str(e.value)
        s.add_mesh(np.array([[-1, -1, 3], [1, -1, 3], [0, 1, 3]], np.float32), np.array([0, 2, 1], np.uint32), m, first_area_light=lid)
        # alpha textures on a quadric
        add_sphere(s, IDENT, 1.0, material=m)
        tex = s.add_texture_constant(0.0)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.set_last_mesh_alpha_textures(tex, None)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED and "quadric" in str(e.value)
        # the device builders leave quadric scenes to the host builders
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            s.build_accel_device(0, 4)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
        # ... and the handle still works
        s.build_accel_best(0, 4)
        h = s.intersect_batch(mk_rays([[0, -4, 0]], [[0, 1, 0]]))
        assert h["prim"][0] == 1 and abs(float(h["t"][0]) - 3.0) < 1e-5


# ---- 8. the multi-device handle ------------------------------------------------------------------------------------------------------------------------------
def test_multi_device_film_equals_one_device_film(host):
    one = pbrt_hip.Scene(); multi = pbrt_hip.Scene(devices=[0, 0, 0])
    for s in (one, multi):
        materials_scene(s, host)
    x1, w1, st1 = one.render_path(max_depth=5)
    xn, wn, stn = multi.render_path(max_depth=5)
    assert np.array_equal(xn.view(np.uint32), x1.view(np.uint32)) and np.array_equal(wn, w1)
    assert (stn.camera_rays, stn.regular_rays, stn.shadow_rays) == (st1.camera_rays, st1.regular_rays, st1.shadow_rays)
    orc = OracleScene(); materials_scene(orc, host)
    with libm1():
        ox, ow, _, _ = orc.render_path_ex(max_depth=5)
    assert np.array_equal(xn.view(np.uint32), ox.view(np.uint32))
    one.close(); multi.close(); orc.close()
