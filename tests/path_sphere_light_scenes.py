"""Scenes, closed forms and probe cases for spherical DiffuseAreaLights under the PATH integrator (pbrt_hip_set_path_sphere_lights), shared by tests/test_path_sphere_lights_cpu.py
and tests/test_path_sphere_lights_gpu.py.  Built on tests/sphere_light_scenes.py (the light for either binding) and tests/closed_form.py (views, the statistical check).

The oracle's path render of a sphere-light scene is a yardstick of its own kind: its pdf_li knows triangles only and answers 0 for a sphere, so its estimate_direct returns after
the light-sampled half (with its MIS weight) and never traces the BSDF-sampled ray.  On the same vertices and sampler dimensions the device computes that film plus non-negative terms."""
import ctypes as C
import math

import numpy as np

import closed_form as CF
import light_probe_cases as LP
import reference_scenes as R
import sphere_light_scenes as SL
import sphere_pdf_restatement as SP
from oracle_binding import oracle_binding, set_libm_mode

F = np.float32
LE = (10.0, 7.0, 4.0)
RHO = (0.2, 0.5, 0.95)
SE_TARGET = 0.005   # as the furnace tests


def oracle_path(orc, **kw):
    """The oracle's PATH render in libm mode 1 (transcendentals in f64, rounded once: what the device computes)"""
    orc.b.lib.oracle_set_integrator.argtypes = [C.c_void_p, C.c_int]
    assert orc.b.lib.oracle_set_integrator(orc.h, 0) == 0
    set_libm_mode(1)
    try:
        xyz, wt, st, _ = orc.render_path_ex(**kw)
    finally:
        set_libm_mode(0)
    return xyz, wt, st


# ---- closed form, outside: a sphere over a plane ------------------------------------------------------------------------------------------------------------------------
OUT_R, OUT_H, OUT_CAM_X = 1.0, 1.3, 2.2


def outside_scene(host, res=64, spp=64):
    """A sphere of radius 1 at (0, 0, 1.3), L = LE, black matte, over a wide matte (RHO) quad at z = 0; an orthographic camera at (2.2, 0, 5) looks down at the square
    [1.2, 3.2] x [-1, 1] beside the sphere, which no camera ray meets.  The sphere lies above the plane's horizon (h > r), so a floor point at distance d from the centre
    receives E = pi Le r^2 h / d^3 and shows L = rho Le r^2 h / d^3 at every depth >= 1: a ray that leaves the floor meets the black sphere or nothing."""
    def build(s, host_):
        floor = s.add_material_matte(RHO, 0.0)
        black = s.add_material_matte((0.0, 0.0, 0.0), 0.0)
        s.add_mesh(*CF._zquad(0.0, 60.0, c=(33.0, -25.0)), floor)   # (centre off the view: no triangle edge crosses it)
        SL.add_sphere_light(s, R.ctm(host_, host_.translate((0.0, 0.0, OUT_H))), OUT_R, material=black, L=LE)
        CF._setup_view(s, host_, res, spp, CF.HALTON, CF.ortho_down(host_, res, z=5.0, xy=(OUT_CAM_X, 0.0)))
        s.build_accel(0, 4)
    return lambda s: SL.capture(build, s, host)


def outside_pixel_expect(s, res):
    """(res, res, 3) float64: rho Le r^2 h / d^3 averaged over every pixel's footprint (box filter of radius 0.5: a pixel's samples are its own), from the scene's own camera
    rays — film position -> floor position is affine for an orthographic camera looking straight down (image x runs against world x for this look_at)."""
    rays, pf = s.generate_camera_rays([0, 0, res, res], 0)
    A = np.column_stack([np.ones(len(pf)), pf.astype(np.float64)])
    cx, *_ = np.linalg.lstsq(A, rays["o"][:, 0].astype(np.float64), rcond=None)
    cy, *_ = np.linalg.lstsq(A, rays["o"][:, 1].astype(np.float64), rcond=None)
    assert np.abs(A @ cx - rays["o"][:, 0]).max() < 1e-5 and np.abs(A @ cy - rays["o"][:, 1]).max() < 1e-5
    k = 8
    sub = (np.arange(k) + 0.5) / k
    py, px = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    g = np.zeros((res, res))
    for dy in sub:
        for dx in sub:
            fx, fy = px + dx, py + dy
            X = cx[0] + cx[1] * fx + cx[2] * fy; Y = cy[0] + cy[1] * fx + cy[2] * fy
            g += OUT_R ** 2 * OUT_H / (X * X + Y * Y + OUT_H * OUT_H) ** 1.5
    g /= k * k
    assert 1.0 < X.min() and X.max() < 3.4   # the footprint lies beside the sphere
    return g[..., None] * np.asarray(RHO, np.float64) * np.asarray(LE, np.float64)


# ---- closed form, inside: everything inside the light -------------------------------------------------------------------------------------------------------------------
def inside_scene(host, two_sided, res=64, spp=64):
    """A sphere of radius 12 around (0.3, -0.2, 1) that emits inwards (reverse orientation, or two-sided with the normal left outwards), black matte; a matte (RHO) quad of
    half-width 1.5 at z = 0 faces an orthographic camera at z = 5 whose window it fills.  Every direction of the quad's upper hemisphere ends on the sphere: L = rho Le at
    every depth >= 1."""
    def build(s, host_):
        floor = s.add_material_matte(RHO, 0.0)
        black = s.add_material_matte((0.0, 0.0, 0.0), 0.0)
        s.add_mesh(*CF._zquad(0.0, 1.5), floor)
        SL.add_sphere_light(s, R.ctm(host_, host_.translate((0.3, -0.2, 1.0))), 12.0, material=black, reverse=not two_sided, L=LE, two_sided=two_sided)
        CF._setup_view(s, host_, res, spp, CF.HALTON, CF.ortho_down(host_, res, z=5.0))
        s.build_accel(0, 4)
    return lambda s: SL.capture(build, s, host)


INSIDE_EXPECT = np.asarray(RHO, np.float64) * np.asarray(LE, np.float64)


def wrongs_from(light_half_only, expect):
    """The wrong answers both closed forms must be told from: the oracle's path render of the same scene (the light-sampled half alone), both halves unweighted, depth 0"""
    return {"light half only (the oracle's path render)": np.asarray(light_half_only, np.float64), "both halves unweighted": 2.0 * np.asarray(expect, np.float64) * np.ones(3),
            "depth 0": np.zeros(3)}


# ---- one small sphere light: some pixels' BSDF-sampled rays meet it, most do not ----------------------------------------------------------------------------------------
def small_light_scene(s, host):
    """A matte floor and a sphere light of radius 0.35 at height 3.5 above it: radius / distance is about 0.1 from the floor below it"""
    def build(s, host_):
        floor = s.add_material_matte((0.6, 0.55, 0.5), 0.0)
        black = s.add_material_matte((0.0, 0.0, 0.0), 0.0)
        s.add_mesh(*CF._zquad(0.0, 4.0, n=2), floor)
        SL.add_sphere_light(s, R.ctm(host_, host_.translate((0.2, 0.1, 3.5))), 0.35, material=black, L=(40.0, 35.0, 30.0))
        SL._view(s, host_, eye=(0.3, -5.0, 2.2), look=(0.0, 0.3, 0.0))
    SL.capture(build, s, host)


# ---- probe lights and cases ------------------------------------------------------------------------------------------------------------------------------------------------
# name, transform steps (host -> list), radius, zmin, zmax, phimax, reverse_orientation, two_sided.  The first three share everything but orientation and sidedness.
PROBE_LIGHTS = [
    ("full", lambda h: [h.translate((0.0, 0.0, 3.0))], 1.0, None, None, 360.0, False, False),
    ("full_reversed", lambda h: [h.translate((0.0, 0.0, 3.0))], 1.0, None, None, 360.0, True, False),
    ("full_two_sided", lambda h: [h.translate((0.0, 0.0, 3.0))], 1.0, None, None, 360.0, False, True),
    ("partial", lambda h: [h.translate((8.0, 0.0, 3.0)), h.rotate(40.0, (0, 1, 0))], 1.5, -0.7, 2.5, 250.0, False, False),
    ("mirrored_scaled", lambda h: [h.translate((12.0, 0.5, 3.0)), h.rotate(35.0, (1, 2, 3)), h.scale((-1.3, 0.7, 1.0))], 1.4, None, None, 360.0, False, False),
    ("scaled_cut", lambda h: [h.translate((-9.0, 2.0, 4.0)), h.scale((0.5, 2.0, 1.5))], 2.0, -1.0, 1.5, 200.0, True, True),
]


def probe_transform(host, k):
    return R.ctm(host, *PROBE_LIGHTS[k][1](host))


def build_probe_lights(s, host):
    def go(s, host_):
        m = LP.add_floor(s)
        for k, (name, steps, radius, zmin, zmax, phimax, rev, two) in enumerate(PROBE_LIGHTS):
            SL.add_sphere_light(s, probe_transform(host_, k), radius, zmin, zmax, phimax, m, rev, L=(8.0, 7.0, 6.0), two_sided=two)
        s.build_accel(0, 4)
    SL.capture(go, s, host)


def _unit_rows(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def probe_cases(host, k, seed=0):
    """-> (ref (n, 10), wi (n, 3), u (n, 2)) for light k, about 200 probes chosen at the edges; the first three lights get the same arrays (same centre, radius and seed)."""
    name, steps, radius, zmin, zmax, phimax, rev, two = PROBE_LIGHTS[k]
    rng = np.random.default_rng(9100 + seed + (0 if k < 3 else k))
    t = probe_transform(host, k)
    c = SP.centre_of(t[0]).astype(np.float64); r = float(radius)
    M = np.asarray(t[0], np.float64).reshape(4, 4)[:3, :3]
    dirs = np.concatenate([np.eye(3), -np.eye(3), _unit_rows(rng.normal(size=(4, 3)))])
    refs, wis = [], []

    def add(ref_rows, wi_rows):
        """every reference point with every direction"""
        a, b = LP.cross(np.asarray(ref_rows, F).reshape(-1, 10), np.asarray(wi_rows, F).reshape(-1, 3))
        refs.append(a); wis.append(b)

    # (1) one p_error band either side of the surface of the object-radius sphere around the centre (what the predicate measures): the offset is dot(|n|, p_error) ~ 6e-7 |p|
    for d in dirs[:8]:
        for tt in (-3e-6, -6e-7, -1e-7, 0.0, 1e-7, 6e-7, 3e-6):
            p = c + d * r * (1.0 + tt)
            for n in (d, -d):
                add(LP.mk_ref([p], n=n.astype(F)), [(-d).astype(F)])
    # (2) radius / distance so small that cos_theta_max rounds to 1 (or just does not), and coordinates near 1e18
    for ratio in (3e-3, 4e-4, 2.5e-4, 1e-4, 1e-6):
        add(LP.mk_ref([c + dirs[6] * r / ratio, c - dirs[7] * r / ratio]), [(-dirs[6]).astype(F)])
    add(LP.mk_ref([[1e18, 2e18, -1e18]]), [_unit_rows(c - np.array([1e18, 2e18, -1e18])).astype(F)])
    # (3) either side of sin^2(theta_max) = 0.00068523
    dc = r / math.sqrt(float(LP.TAYLOR))
    ax = c - np.array([0.0, 0.0, dc])
    add(LP.mk_ref([[ax[0], ax[1], v] for v in LP.ulps(float(F(ax[2])), range(-3, 4))]), [np.array([0, 0, 1], F)])
    # (4) what every light set gets, and n = 0 with p_error = 0 (what the light-distribution pass hands over)
    add(LP.ref_edges((c - [0.5, 0.3, 2.5 * r]).astype(F), c), [np.array([0, 0, 1], F), _unit_rows([0.5, 0.3, 2.5 * r]).astype(F)])
    add(LP.mk_ref([c + [0.3 * r, -0.2 * r, 0.1 * r], c - [0, 0, 5 * r]], p_error=(0, 0, 0), n=(0, 0, 0)), [np.array([0, 0, 1], F), _unit_rows(rng.normal(size=3)).astype(F)])
    # (5) inside: straight at the surface, at grazing incidence from just below it, at the cut-away part of a cut sphere (object -z and the phi wedge before phi_max closes), random
    cut_dirs = _unit_rows([M @ np.array([0.0, 0.0, -1.0]), M @ np.array([0.0, 0.0, 1.0]), M @ np.array([math.cos(math.radians(-20.0)), math.sin(math.radians(-20.0)), 0.0])])
    inner = [c, c + [0.3 * r, -0.2 * r, 0.1 * r], c + dirs[6] * 0.5 * r, c - dirs[7] * 0.2 * r]
    add(LP.mk_ref(inner), np.concatenate([cut_dirs, dirs[[0, 4, 8]]]).astype(F))
    for d in dirs[6:10]:
        p = c + d * r * 0.999
        tang = _unit_rows(np.cross(d, [0.3, -0.5, 0.8]))
        add(LP.mk_ref([p], n=(-d).astype(F)), np.array([d, tang, _unit_rows(tang + 0.02 * d), _unit_rows(tang - 0.02 * d), -d], F))
    # (6) random fill: outside (half of the normals face the light) and inside
    ro = LP.random_refs(rng, c, 3.0 * r, 24, target=c)
    add(ro[:12], LP.random_dirs(rng, 1)); refs.append(ro[12:]); wis.append(_unit_rows(c - ro[12:, 0:3].astype(np.float64)).astype(F))
    ri = LP.random_refs(rng, c, 0.35 * r, 16)
    refs.append(ri); wis.append(LP.random_dirs(rng, 16))
    ref = np.concatenate(refs).astype(F); wi = np.concatenate(wis).astype(F)
    u = rng.random((len(ref), 2)).astype(F)
    u[:len(LP.SPHERE_U)] = LP.SPHERE_U   # the sample's own edges: 0, 1 - eps, the smallest denormal
    assert 150 <= len(ref) <= 260, (name, len(ref))
    return ref, wi, np.ascontiguousarray(u, F)


def oracle_inside_hits(host, k, ref, wi):
    """For every probe: the oracle's Sphere::intersect (oracle_sphere_probe, libm mode 1) of spawn_ray(ref, wi) with light k's sphere -> (hit mask, p (n, 3) f32, n (n, 3) f32)"""
    name, steps, radius, zmin, zmax, phimax, rev, two = PROBE_LIGHTS[k]
    t = probe_transform(host, k)
    L = oracle_binding().lib
    fp = C.POINTER(C.c_float)
    L.oracle_sphere_probe.argtypes = [fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, fp, fp, C.c_float, fp]
    f = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(fp)
    o = SP.spawn_ray_origin(ref, wi)
    zmin = -radius if zmin is None else zmin; zmax = radius if zmax is None else zmax
    hit = np.zeros(len(ref), bool); p = np.zeros((len(ref), 3), F); n = np.zeros((len(ref), 3), F)
    out = np.zeros(16, F)
    set_libm_mode(1)
    try:
        for i in range(len(ref)):
            if not (np.isfinite(o[i]).all() and np.isfinite(wi[i]).all()):
                continue
            out[:] = 0
            L.oracle_sphere_probe(f(t[0]), f(t[1]), radius, zmin, zmax, phimax, 1 if rev else 0, f(o[i]), f(wi[i]), np.inf, out.ctypes.data_as(fp))
            if out[0] != 0.0:
                hit[i] = True; p[i] = out[2:5]; n[i] = out[5:8]
    finally:
        set_libm_mode(0)
    return hit, p, n


def probe_light_area(k):
    name, steps, radius, zmin, zmax, phimax, rev, two = PROBE_LIGHTS[k]
    return SP.sphere_area(radius, zmin, zmax, phimax)
