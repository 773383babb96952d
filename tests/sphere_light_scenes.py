"""Scenes lit by spherical DiffuseAreaLights, for either binding: the oracle makes the light with oracle_add_sphere + oracle_make_last_sphere_a_light (as
tests/reference_scenes.py::lights_diffuse does), the product with Scene.add_sphere_light.  One scene function then feeds both sides of a bit-for-bit comparison
(tests/test_sphere_light_gpu.py) and the CPU render of tests/test_sphere_light_capi.py."""
import ctypes as C

import numpy as np

import pbrt_hip
import reference_scenes as R
import scenes
from oracle_binding import set_libm_mode


def add_sphere_light(s, t, radius=1.0, zmin=None, zmax=None, phimax=360.0, material=0, reverse=False, L=(1.0, 1.0, 1.0), two_sided=False):
    """t = (object_to_world, world_to_object)"""
    if s.b.prefix != "oracle_":
        s.add_sphere_light(t[0], t[1], radius, zmin, zmax, phimax, material, reverse, L=L, two_sided=two_sided)
        return
    lib = s.b.lib
    fp = C.POINTER(C.c_float)
    lib.oracle_add_sphere.argtypes = [C.c_void_p, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]
    lib.oracle_make_last_sphere_a_light.argtypes = [C.c_void_p, fp, C.c_int]
    zmin = -radius if zmin is None else zmin
    zmax = radius if zmax is None else zmax
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(fp)
    s._chk(lib.oracle_add_sphere(s.h, f(t[0]), f(t[1]), radius, zmin, zmax, phimax, material, 1 if reverse else 0))
    s._chk(lib.oracle_make_last_sphere_a_light(s.h, f(L), 1 if two_sided else 0))


def add_sphere(s, t, radius=1.0, zmin=None, zmax=None, phimax=360.0, material=0, reverse=False):
    if s.b.prefix != "oracle_":
        s.add_sphere(t[0], t[1], radius, zmin, zmax, phimax, material, reverse)
    else:
        from test_oracle_sphere import add_sphere as oracle_add_sphere
        oracle_add_sphere(s, t, radius, zmin, zmax, phimax, material, reverse)


def oracle_whitted(orc, **kw):
    """The oracle's Whitted render in libm mode 1 (transcendentals in f64, rounded once: what the device computes)"""
    orc.b.lib.oracle_set_integrator.argtypes = [C.c_void_p, C.c_int]
    assert orc.b.lib.oracle_set_integrator(orc.h, 1) == 0
    set_libm_mode(1)
    try:
        xyz, wt, st, _ = orc.render_path_ex(**kw)
    finally:
        set_libm_mode(0)
    return xyz, wt, st


def capture(build, s, host):
    """build(s, host) with the oracle's libm in mode 1 for the capture too: Sphere::new evaluates acos for theta_min / theta_max of a cut sphere"""
    if s.b.prefix != "oracle_":
        return build(s, host)
    set_libm_mode(1)
    try:
        return build(s, host)
    finally:
        set_libm_mode(0)


# ---- scenes/lights/diffuse.pbrt ------------------------------------------------------------------------------------------------------------------------------------
def lights_diffuse(s, host, spp=128, res=400, split=0):
    """The numbers of reference_scenes.lights_diffuse: a sphere of radius 3 at (-10, 0, 10), black matte, L = 20, over the cube and the checkered floor"""
    add_sphere_light(s, R.ctm(host, host.translate((-10, 0, 10))), 3.0, material=s.add_material_matte((0.0, 0.0, 0.0)), L=(20.0, 20.0, 20.0))
    R._cube_and_checker_floor(s, host)
    R.camera_film(s, host, (0, 5, 3), (0, 0, 0), (0, 0, 1), 90.0, res, res, spp)
    s.build_accel(split, 4)
    return dict(max_depth=5, render="lights_diffuse")


# ---- the branches of Sphere::sample_solid_angle, by construction -------------------------------------------------------------------------------------------------
def _stage(s, host, floor_z=0.0):
    """A matte floor, one glass and one mirror object made of triangles: the recursion runs"""
    floor = s.add_material_matte((0.6, 0.55, 0.5))
    glass = s.add_material_glass(kr=(0.9, 0.95, 1.0), kt=(0.95, 0.9, 0.85), eta=1.5)
    mirror = s.add_material_mirror((0.9, 0.8, 0.7))
    P, idx = scenes.grid_mesh(2, z=floor_z, size=4.0)
    s.add_mesh(P, idx, floor)
    t = R.ctm(host, host.translate((-0.9, 0.3, floor_z + 0.6)), host.rotate(25.0, (0, 0, 1)), host.scale((0.5, 0.5, 0.6)))
    s.add_mesh(host.transform_points(t[0], R.CUBE_P), R.CUBE_IDX, glass)
    t = R.ctm(host, host.translate((1.0, 0.8, floor_z + 0.9)), host.rotate(-20.0, (0, 0, 1)), host.rotate(80.0, (1, 0, 0)))
    s.add_mesh(host.transform_points(t[0], R.quad(0.9)), R.QUAD_IDX, mirror)
    return floor


def _view(s, host, eye=(0.3, -5.0, 2.2), look=(0.0, 0.3, 0.5), fov=50.0, res=48, spp=4, split=0):
    R.camera_film(s, host, eye, look, (0, 0, 1), fov, res, res, spp)
    s.build_accel(split, 4)


def case_small_angle(s, host):
    """(a) radius / distance < 0.026 from everywhere on the stage: sin^2(theta_max) < 0.00068523, the Taylor form"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    _stage(s, host)
    add_sphere_light(s, R.ctm(host, host.translate((-20.0, -30.0, 50.0))), 1.2, material=black, L=(9000.0, 8500.0, 8000.0))   # >= 55 units from every surface: ratio <= 0.022
    _view(s, host)


def case_cone(s, host):
    """(b) a near, large sphere: the plain cone form"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    _stage(s, host)
    add_sphere_light(s, R.ctm(host, host.translate((-1.5, -0.5, 4.5))), 2.0, material=black, L=(6.0, 6.0, 5.5))
    _view(s, host)


def case_inside(s, host, two_sided=False):
    """(c) the camera and the whole stage inside the light sphere: uniform_sample_sphere over its area.  reverse=True turns the normal inwards; the two-sided form keeps it outwards"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    _stage(s, host)
    add_sphere_light(s, R.ctm(host, host.translate((0.2, -0.5, 1.0)), host.rotate(30.0, (1, 1, 0))), 12.0, material=black, reverse=not two_sided, L=(0.9, 0.8, 0.7), two_sided=two_sided)
    _view(s, host)


def case_partial(s, host):
    """(d) z_min, z_max (one of them beyond the radius: clamped) and phi_max 250 degrees: `area` is that of the clamped cut, samples also land on the missing part"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    _stage(s, host)
    add_sphere_light(s, R.ctm(host, host.translate((1.0, -1.0, 3.6)), host.rotate(40.0, (0, 1, 0))), 1.5, -0.7, 2.5, 250.0, material=black, L=(14.0, 13.0, 12.0))
    _view(s, host)


def case_mirrored(s, host):
    """(e) object_to_world scales non-uniformly, rotates and has a negative determinant"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    _stage(s, host)
    t = R.ctm(host, host.translate((-1.0, 0.5, 3.8)), host.rotate(35.0, (1, 2, 3)), host.scale((-1.3, 0.7, 1.0)))
    assert host.swaps_handedness(t[0])
    add_sphere_light(s, t, 1.4, material=black, L=(10.0, 11.0, 12.0))
    _view(s, host)


def case_six_lights(s, host):
    """(f) sphere, point, an area light of 2 triangles (2 lights), sphere, distant: six lights, PH_WH_SLICE = 4 crossed, a sphere light at positions 0 and 4"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    floor = _stage(s, host)
    add_sphere_light(s, R.ctm(host, host.translate((-2.0, -1.0, 4.0))), 0.8, material=black, L=(12.0, 10.0, 8.0))
    s.add_light_point((6.0, 7.0, 8.0), (2.5, -2.0, 3.0))
    first = s.add_light_diffuse_area((5.0, 5.0, 4.0), 2)
    t = R.ctm(host, host.translate((0.5, 2.5, 3.5)), host.rotate(150.0, (1, 0, 0)))
    s.add_mesh(host.transform_points(t[0], R.quad(0.6)), R.QUAD_IDX, floor, first_area_light=first)
    add_sphere_light(s, R.ctm(host, host.translate((2.2, 1.0, 3.0)), host.scale((1.0, 1.0, 1.0))), 0.6, -0.3, 0.6, 300.0, material=black, L=(4.0, 9.0, 6.0), two_sided=True)
    s.add_light_distant((0.5, 0.5, 0.6), host.distant_direction(R._ident(), (3.0, -2.0, 5.0), (0.0, 0.0, 0.0)))
    _view(s, host)


def case_visible(s, host):
    """(g) the light sphere in front of the camera: `L += isect.le(wo)` at the camera rays that meet it"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    _stage(s, host)
    add_sphere_light(s, R.ctm(host, host.translate((-0.2, -0.8, 2.0))), 0.6, material=black, L=(3.0, 2.5, 2.0))
    _view(s, host)


CASES = [("small_angle", case_small_angle), ("cone", case_cone), ("inside_reversed", lambda s, host: case_inside(s, host, False)),
         ("inside_two_sided", lambda s, host: case_inside(s, host, True)), ("partial", case_partial), ("mirrored", case_mirrored), ("six_lights", case_six_lights),
         ("visible", case_visible)]


# ---- randomised scenes -----------------------------------------------------------------------------------------------------------------------------------------------
def _material(s, g):
    k = int(g.integers(0, 4))
    c = lambda lo=0.05, hi=0.95: tuple(g.uniform(lo, hi, 3).astype(np.float32))
    if k == 0: return s.add_material_matte(c(), float(g.choice([0.0, g.uniform(1, 60)])))
    if k == 1: return s.add_material_glass(c(0.5, 1), c(0.5, 1), 0.0, 0.0, float(g.uniform(1.1, 1.8)), True)
    if k == 2: return s.add_material_mirror(c(0.3, 1.0))
    return s.add_material_plastic(c(), c(0.05, 0.5), float(g.uniform(0.01, 0.4)), bool(g.integers(0, 2)))


def _rigid_or_scaled(host, g, centre, spread):
    t = R.ctm(host, host.translate(tuple(np.asarray(centre) + g.uniform(-spread, spread, 3))), host.rotate(float(g.uniform(0, 360)), tuple(g.normal(size=3) + 1e-3)))
    if g.integers(0, 2):
        t = host.compose(t, host.scale(tuple(g.uniform(0.6, 1.4, 3) * g.choice([1.0, 1.0, -1.0], 3))))
    return t


def random_case(host, seed):
    """-> (build(s, host), max_depth).  1-3 sphere lights (random radius, placement, cut, orientation, two_sided; now and then one that encloses the scene), 0-2 other lights, at most
    5 lights in all: with smooth glass and mirrors in the scene the recursion may draw 5 + 7 * 2 * 5 + 3 * 4 = 87 dimensions at depth 3, far below Halton's 1000."""
    rng = np.random.default_rng(1000 + seed)
    depth = int(rng.integers(1, 4))
    geo_seed = int(rng.integers(0, 2 ** 31))
    max_prims = int(rng.choice([1, 4, 8]))   # SAH: the reference's HLBVH asserts on some random scenes (hlbvh.rs:338), and tests/test_sphere_light_gpu.py builds the reference scene with it

    def build(s, host_):
        g = np.random.default_rng(geo_seed)
        mats = [_material(s, g) for _ in range(4)]
        black = s.add_material_matte((0.0, 0.0, 0.0))
        n_sphere = int(g.integers(1, 4)); n_other = int(g.integers(0, 3))
        kinds = ["sphere"] * n_sphere + ["other"] * n_other
        g.shuffle(kinds)
        P, idx = scenes.grid_mesh(3, z=-1.3, size=3.0)
        s.add_mesh(P, idx, s.add_material_matte(tuple(g.uniform(0.3, 0.8, 3))))
        for kind in kinds:
            if kind == "sphere":
                enclosing = g.integers(0, 5) == 0
                r = float(g.uniform(9.0, 14.0)) if enclosing else float(g.uniform(0.2, 1.5))
                t = _rigid_or_scaled(host_, g, (0, 0, 0) if enclosing else (0, 0, 2.0), 0.5 if enclosing else 1.5)
                cut = bool(g.integers(0, 2)) and not enclosing
                rev = g.integers(0, 4) == 0; two = bool(g.integers(0, 2))   # reversed and one-sided, a small sphere emits into itself only: the less frequent draw
                if enclosing and not two: rev = True   # the sampled normal points inwards: the sphere lights what it encloses
                scale = 1.0 if enclosing else float(g.uniform(3, 25))
                add_sphere_light(s, t, r, float(g.uniform(-r, 0)) if cut else None, float(g.uniform(0, 1.3 * r)) if cut else None,
                                 float(g.choice([360.0, g.uniform(40, 340)])) if cut else 360.0, black if g.integers(0, 2) else mats[int(g.integers(0, 4))], bool(rev),
                                 tuple(g.uniform(0.3, 1.0, 3) * scale), two)
            elif g.integers(0, 2):
                s.add_light_point(tuple(g.uniform(2, 12, 3)), g.uniform(-1.5, 1.5, 3).astype(np.float32) + np.float32([0, 0, 2.5]))
            else:
                w = g.normal(size=3); w /= np.linalg.norm(w)
                s.add_light_distant(tuple(g.uniform(0.3, 2, 3)), np.float32(w))
            # geometry between the lights: triangles and quadrics that do not emit
            Pt, it = host_.gen_random_tris(int(g.integers(1, 30)), int(g.integers(1, 1000)))
            s.add_mesh(Pt, it, mats[int(g.integers(0, 4))])
            t = _rigid_or_scaled(host_, g, (0, 0, 0), 1.2)
            q = int(g.integers(0, 3))
            if q == 0: add_sphere(s, t, float(g.uniform(0.3, 0.8)), None, None, 360.0, mats[int(g.integers(0, 4))], bool(g.integers(0, 2)))
            elif q == 1: s.add_quadric("cylinder", t[0], t[1], float(g.uniform(0.2, 0.6)), -0.5, 0.5, float(g.choice([360.0, 270.0])), mats[int(g.integers(0, 4))], bool(g.integers(0, 2)))
            else: s.add_quadric("disk", t[0], t[1], float(g.uniform(0.4, 1.0)), float(g.uniform(-0.5, 0.5)), 0.0, 360.0, mats[int(g.integers(0, 4))], bool(g.integers(0, 2)))
        eye = g.uniform(-0.5, 0.5, 3) + np.array([0, -4.5, 0.5])
        R.camera_film(s, host_, tuple(eye), (0, 0, 0), (0, 0, 1), float(g.uniform(35, 60)), 48, 48, 4)
        s.build_accel(0, max_prims)

    return build, depth
