"""Scenes that hold quadric shapes NEXT TO alpha-masked triangle meshes, for either binding (pbrt_hip.Scene on the device library or tests/oracle_binding.OracleScene): one builder
feeds both sides of the bit-for-bit comparisons of tests/test_quadric_alpha_gpu.py and tests/test_fuzz_quadric_alpha_gpu.py and the CPU render of tests/test_quadric_alpha_oracle.py.

The stage (`mixed_scene`): the camera looks down -z at a 4 x 4 grid of quads (32 triangles) in the plane z = 0 that carries the mask; three quadrics lie behind the grid (z < 0: a
red sphere, a blue partial cylinder, a yellow disk), two in front of it (a mirror cone, a plastic paraboloid), a grey wall closes the view at z = -2.2.  MASKS names the alpha
textures: "imagemap" keeps the scene in the traversal kernel's lean alpha row, "checkerboard" (and the "dots" shadow mask that goes with it) needs the general evaluator's row."""
import contextlib
import os

import numpy as np

import closed_form as cf
import pbrt_hip
import scenes
from oracle_binding import set_libm_mode
from sphere_light_scenes import add_sphere_light

MISS = 0xFFFFFFFF
MASKS = ("imagemap", "checkerboard")
GRID = 2.0            # the masked grid spans [-GRID, GRID]^2 at z = 0; uv = (xy + GRID) / (2 GRID)
CHECKS = 4.0          # checkerboard mask: uscale = vscale
MESH_KD, SPHERE_KD, CYL_KD, DISK_KD, WALL_KD = (0.1, 0.8, 0.1), (0.8, 0.1, 0.1), (0.1, 0.1, 0.8), (0.8, 0.8, 0.1), (0.4, 0.4, 0.4)
SPHERE_C, SPHERE_R = (-0.9, 0.6, -1.0), 0.7


@contextlib.contextmanager
def libm1():
    """The oracle's transcendentals in f64, rounded once: what the device computes.  Held while an oracle scene is captured too (Sphere::new evaluates acos)."""
    set_libm_mode(1)
    try:
        yield
    finally:
        set_libm_mode(0)


def block_image(seed, blocks=4, px=4):
    """(blocks px)^2 texels of exactly 0 / 1 in square blocks: a bilinear look-up is exactly 0 inside a zero block, so the mask has holes, and exactly 1 inside a one block"""
    g = np.random.default_rng(seed)
    m = (g.uniform(0, 1, (blocks, blocks)) > 0.5).astype(np.float32)
    m[0, 0] = 0.0; m[-1, -1] = 1.0
    m = np.kron(m, np.ones((px, px), np.float32))
    return np.repeat(m[..., None], 3, axis=2)


def mask_textures(s, mask, shadow=False, inert=False):
    """-> (alpha texture, shadow-alpha texture or None).  inert: the same texture classes with the value 1 everywhere"""
    c = s.add_texture_constant
    if mask == "imagemap":
        img = lambda seed: np.ones_like(block_image(seed)) if inert else block_image(seed)
        a = s.add_texture_imagemap(s.add_mipmap(img(3), as_float=True, trilinear=True, wrap="clamp"))
        sa = s.add_texture_imagemap(s.add_mipmap(img(8), as_float=True, trilinear=True, wrap="repeat"), su=2.0, sv=2.0) if shadow else None
    else:
        a = s.add_texture_checkerboard(c(1.0), c(1.0 if inert else 0.0), su=CHECKS, sv=CHECKS, aa="none")
        sa = s.add_texture_dots(c(1.0 if inert else 0.0), c(1.0), su=3.0, sv=3.0) if shadow else None   # (the constructor swaps inside / outside: 0 INSIDE the dots)
    return a, sa


def checker_opaque(x, y):
    """The "checkerboard" alpha mask at the point (x, y, 0) of the grid, restated: checkerboard.rs with aa none takes tex1 (1) where floor(s) + floor(t) is even"""
    u = (np.asarray(x, np.float64) + GRID) / (2 * GRID) * CHECKS; v = (np.asarray(y, np.float64) + GRID) / (2 * GRID) * CHECKS
    return (np.floor(u).astype(np.int64) + np.floor(v).astype(np.int64)) % 2 == 0


def _quad_mesh(z, size, flip=False):
    P = np.array([[-size, -size, z], [size, -size, z], [size, size, z], [-size, size, z]], np.float32)
    return P, np.array([0, 2, 1, 0, 3, 2] if flip else [0, 1, 2, 0, 2, 3], np.uint32)


def mixed_scene(s, host, mask="imagemap", shadow=False, inert=False, max_prims=4, res=(48, 32), spp=4, sampler="halton", lens=0.0, whitted=False, plain=False):
    """-> {name: (first primitive, count)}.  whitted: plus a glass sphere in front of the grid and a spherical area light in front of it (its shadow rays cross the masked grid).
    plain: matte surfaces and the sky only (the CPU test reads material colours off the film)."""
    prims, n = {}, [0]

    def took(name, count=1):
        prims[name] = (n[0], count); n[0] += count
    T = lambda *steps: cf_ctm(host, *steps)
    green = s.add_material_matte(MESH_KD); red = s.add_material_matte(SPHERE_KD); yellow = s.add_material_matte(DISK_KD); grey = s.add_material_matte(WALL_KD)
    blue = s.add_material_matte(CYL_KD) if plain else s.add_material_plastic(CYL_KD, (0.3, 0.3, 0.3), 0.1)
    mirror = grey if plain else s.add_material_mirror((0.9, 0.9, 0.9))
    plastic = grey if plain else s.add_material_plastic((0.5, 0.2, 0.5), (0.4, 0.4, 0.4), 0.05)
    s.add_light_infinite((0.5, 0.55, 0.6))
    # two quadrics ahead of the mesh in the primitive list, three after it
    s.add_sphere(*T(host.translate(SPHERE_C)), SPHERE_R, None, None, 360.0, red, False); took("sphere")
    s.add_quadric("cone", *T(host.translate((-1.2, -1.0, 0.3)), host.rotate(20.0, (1, 0, 0))), 0.4, 0.8, 0.0, 360.0, mirror, False); took("cone")
    P, idx = scenes.grid_mesh(4, z=0.0, size=GRID)
    s.add_mesh(P, idx, green, UV=((P[:, :2] + GRID) / (2 * GRID)).astype(np.float32))
    s.set_last_mesh_alpha_textures(*mask_textures(s, mask, shadow, inert)); took("mesh", len(idx) // 3)
    s.add_quadric("cylinder", *T(host.translate((1.0, 0.5, -1.2)), host.rotate(70.0, (1, 1, 0))), 0.45, -0.6, 0.6, 270.0, blue, False); took("cylinder")
    s.add_quadric("disk", *T(host.translate((0.1, -1.0, -0.6)), host.rotate(15.0, (0, 1, 0))), 0.7, 0.0, 0.2, 360.0, yellow, False); took("disk")
    s.add_quadric("paraboloid", *T(host.translate((1.2, -0.9, 0.4)), host.rotate(-30.0, (1, 0, 0))), 0.4, 0.1, 0.7, 300.0, plastic, True); took("paraboloid")
    s.add_mesh(*_quad_mesh(-2.2, 4.0), grey); took("wall", 2)
    if not plain:
        s.add_light_point((20.0, 19.0, 18.0), (1.5, -1.0, 5.0))
        lid = s.add_light_diffuse_area((9.0, 9.0, 8.0), 2)
        s.add_mesh(*_quad_mesh(4.5, 0.7, flip=True), grey, first_area_light=lid); took("emitter", 2)
    if whitted:
        glass = s.add_material_glass(kr=(0.9, 0.95, 1.0), kt=(0.95, 0.9, 0.85), eta=1.5)
        s.add_sphere(*T(host.translate((-0.2, 0.3, 1.0))), 0.8, None, None, 360.0, glass, False); took("glass")
        add_sphere_light(s, T(host.translate((0.6, 0.9, 3.5))), 0.4, material=s.add_material_matte((0.0, 0.0, 0.0)), L=(14.0, 13.0, 12.0)); took("sphere light")
    w2c, c2w = host.look_at((0.4, -0.6, 7.0), (0.0, 0.0, -0.3), (0, 1, 0))
    s.set_camera_perspective(host.perspective_raster_to_camera(40.0, res[0], res[1]), c2w, lens_radius=lens, focal_distance=7.0)
    cb, table, sb = host.film_box(res[0], res[1])
    s.set_film(res[0], res[1], cb, (0.5, 0.5), table)
    if sampler == "sobol":
        s.set_sobol_tables(*sobol_fixture_64())
    s.set_sampler(cf.SOBOL if sampler == "sobol" else cf.HALTON, spp, sb)
    s.build_accel(0, max_prims)
    return prims


def sobol_fixture_64():
    """tests/golden/sobol_subset_64.npz: 64 dimensions and 9 VdC matrices of the reference's Sobol tables — a path of depth 5 draws 53"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sobol_subset_64.npz"))
    return z["m32"], z["vdc"], z["vdc_inv"]


def cf_ctm(host, *steps):
    t = (pbrt_hip.IDENTITY.copy(), pbrt_hip.IDENTITY.copy())
    for st in steps:
        t = host.compose(t, st)
    return t


def tangent_scene(s, host, mask, mesh_first, max_prims=4):
    """Four small spheres that TOUCH the masked plane z = 0, two from behind and two from the front, each inside one cell of the grid: a ray through a point of tangency meets the
    sphere and a masked triangle at equal or nearly equal t, in one leaf.  mesh_first: the order of the directives, hence of the primitives in a leaf."""
    green = s.add_material_matte(MESH_KD); red = s.add_material_matte(SPHERE_KD)
    P, idx = scenes.grid_mesh(4, z=0.0, size=GRID)

    def mesh():
        s.add_mesh(P, idx, green, UV=((P[:, :2] + GRID) / (2 * GRID)).astype(np.float32))
        s.set_last_mesh_alpha_textures(*mask_textures(s, mask, shadow=True))

    def spheres():
        for c in TANGENT_CENTRES:
            s.add_sphere(*cf_ctm(host, host.translate(c)), abs(c[2]), None, None, 360.0, red, False)
    if mesh_first: mesh(); spheres()
    else: spheres(); mesh()
    s.add_light_infinite((1.0, 1.0, 1.0))
    s.build_accel(0, max_prims)


# (x, y) chosen so that the tangent points fall on an opaque and on a cut-out part of both masks' grids; z = -r behind, +r in front
TANGENT_CENTRES = ((0.45, 0.3, -0.25), (-0.55, -0.7, 0.25), (-1.5, 0.5, -0.25), (1.3, -1.4, 0.25))


def tangent_rays(seed=4, per_point=600):
    g = np.random.default_rng(seed)
    o, d = [], []
    for c in TANGENT_CENTRES:
        # through points a few float steps around the point of tangency (c.x, c.y, 0), from both sides of the plane, steep and grazing
        tgt = np.array([c[0], c[1], 0.0]) + np.c_[g.integers(-6, 7, (per_point, 2)) * 2.0 ** -20, np.zeros(per_point)]
        org = np.c_[g.uniform(-2.5, 2.5, (per_point, 2)), g.choice([-3.0, -0.8, 0.8, 3.0], per_point)]
        org[::3, :2] = tgt[::3, :2]   # a third straight along z: equal t on the sphere and on the plane up to rounding
        o.append(org); d.append(tgt - org)
    r = np.zeros(len(TANGENT_CENTRES) * per_point, pbrt_hip.RAY_DTYPE)
    r["o"] = np.concatenate(o).astype(np.float32); r["d"] = np.concatenate(d).astype(np.float32); r["t_max"] = np.inf
    r["t_max"][1::4] = np.float32(1.0 + 1e-3)   # a quarter ends just beyond the target (shadow-ray style)
    return r


def grid_rays(n_side=64, seed=9):
    """n_side^2 rays from a jittered grid: three quarters start in front of the masked grid (z = 5) and look down through it, a quarter starts behind the wall's side of it (z = -2)
    and looks up; a fifth of them end at a finite t_max"""
    g = np.random.default_rng(seed)
    k = n_side * n_side
    ij = np.stack(np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="xy"), -1).reshape(-1, 2)
    xy = (ij + g.uniform(0, 1, (k, 2))) / n_side * 4.8 - 2.4
    up = (np.arange(k) % 4) == 3
    o = np.c_[xy, np.where(up, -2.0, 5.0)]
    tgt = np.c_[xy + g.normal(0, 0.35, (k, 2)), np.where(up, 1.5, -2.0)]
    r = np.zeros(k, pbrt_hip.RAY_DTYPE)
    r["o"] = o.astype(np.float32); r["d"] = (tgt - o).astype(np.float32); r["t_max"] = np.inf
    r["t_max"][::5] = g.uniform(0.3, 1.2, len(r["t_max"][::5])).astype(np.float32)
    return r
