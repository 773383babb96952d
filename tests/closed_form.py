"""Closed-form radiance for PathIntegrator::li (integrators/src/path.rs:103-284): scene builders, float64 expectations written from
the physics with numpy alone (they never call the oracle or the library), and the statistical check the closed-form tests share.

Every builder takes a pbrt_hip.Scene or an OracleScene.  The scenes are chosen so that every pixel has the same expected value.  What a mean cannot see: `eta_scale` (path.rs:192-203),
the bounce at which Russian roulette starts (`bounces > 3`), the value of q (the 0.05 floor, the max component, `<` against rr_threshold)
and the order in which a path consumes sampler dimensions only steer which samples die and what the survivors weigh; the `1/(1-q)`
weight keeps the mean.  Those are pinned sample by sample by tests/li_replay.py, a float64 replay of li on specular chains, in
test_closed_form_li.py::test_li_replay (the oracle) and test_closed_form_li_gpu.py::test_li_replay_on_device: eta_scale and the start of RR
by the stack_* cases, eta_scale staying out of reflections and the RR dimension being consumed only when RR runs by the walk_* cases,
the floor by stack_eta1.1_* and corridor, `<` by corridor_kr1, BSDF::eta = 1 for glass (glass.rs:109) and for uber with opacity < 1
(uber.rs:133) by glass_* and sheet_*.
"""
import ctypes as C
import math
import os

import numpy as np

import pbrt_hip

HALTON, SOBOL = 0, 1
LE = (1.0, 0.7, 0.4)                 # the emitters' and the sky's radiance in every case
RHO_RGB = (0.2, 0.5, 0.95)           # per channel: RR's max-component is driven by one channel
HALTON_MAX_DEPTH = 123               # check_render_args: 5 + 8 (D + 1) < 1000 (HaltonSampler's prime table, halton.rs:106-110)


# ---- geometry ---------------------------------------------------------------------------------------------------------

def _face(center, u, v, n):
    """An n x n shared-vertex grid over center + a u + b v, a, b in [-1, 1]; every triangle's geometric normal is u x v."""
    a = np.linspace(-1.0, 1.0, n + 1)
    A, B = np.meshgrid(a, a, indexing="xy")
    P = np.asarray(center, np.float64) + A.reshape(-1, 1) * np.asarray(u, np.float64) + B.reshape(-1, 1) * np.asarray(v, np.float64)
    idx = []
    for j in range(n):
        for i in range(n):
            p0 = j * (n + 1) + i
            idx += [p0, p0 + 1, p0 + n + 2, p0, p0 + n + 2, p0 + n + 1]
    return P.astype(np.float32), np.array(idx, np.uint32)


def cube_faces(half=1.0, n=1):
    """The six faces of [-half, half]^3 as n x n grids whose normals point INTO the cube."""
    h = float(half)
    X, Y, Z = np.eye(3) * h
    faces = []
    for axis, (u, v) in enumerate(((Y, Z), (Z, X), (X, Y))):
        c = np.eye(3)[axis] * h
        faces.append(_face(-c, u, v, n))     # at -h: u x v = +axis, inward
        faces.append(_face(c, v, u, n))      # at +h: v x u = -axis, inward
    return faces


def _setup_view(s, host, res, spp, sampler, camera, at_center=False, sobol_tables=None):
    kind, r2c, c2w = camera
    if kind == "persp":
        s.set_camera_perspective(r2c, c2w)
    else:
        s.set_camera_orthographic(r2c, c2w)
    cb, table, sb = host.film_box(res, res)
    s.set_film(res, res, cb, (0.5, 0.5), table)
    if sampler == SOBOL:
        s.set_sobol_tables(*sobol_tables)
    s.set_sampler(sampler, spp, sb, sample_at_pixel_center=at_center)


def inside_camera(host, res):
    """A perspective camera inside the unit cube, off-centre and oblique, so its pixels see every kind of wall point."""
    _, c2w = host.look_at([0.13, -0.21, 0.07], [0.4, 1.0, 0.25], [0, 0, 1])
    return ("persp", host.perspective_raster_to_camera(70.0, res, res), c2w)


def ortho_down(host, res, z=5.0, xy=(0.0, 0.0), up=(0.0, 1.0, 0.0)):
    _, c2w = host.look_at([xy[0], xy[1], z], [xy[0], xy[1], 0.0], list(up))
    return ("ortho", host.orthographic_raster_to_camera(res, res), c2w)


def emissive_furnace(host, Le, rho, res=16, spp=16, grid=1, reverse=False, two_sided=False, extra_lights=False, textured=False,
                     unused_plastic=False, sampler=HALTON, sobol_tables=None):
    """Form A: a closed cube whose every triangle is a one-sided DiffuseAreaLight facing inward (Le) and Lambertian (Kd = rho),
    the camera inside.  reverse flips every triangle's orientation (the walls then face out); extra_lights adds a point light and
    an infinite light that are always occluded; textured takes Kd from a constant image map; unused_plastic adds a plastic material no mesh uses.  Returns (capture, n_lights)."""
    faces = cube_faces(1.0, grid)
    rho = tuple(float(r) for r in np.broadcast_to(np.asarray(rho, np.float64), (3,)))
    n_lights = sum(len(idx) // 3 for _, idx in faces) + (2 if extra_lights else 0)

    def capture(s):
        if textured:
            mm = s.add_mipmap(np.broadcast_to(np.asarray(rho, np.float32), (4, 4, 3)).copy())
            mat = s.add_material_matte_tex(s.add_texture_imagemap(mm))
        else:
            mat = s.add_material_matte(rho, 0.0)
        if unused_plastic:
            s.add_material_plastic((0.3, 0.3, 0.3), (0.2, 0.2, 0.2), 0.1)
        for P, idx in faces:
            lid = s.add_light_diffuse_area(Le, len(idx) // 3, two_sided=two_sided)
            s.add_mesh(P, idx, mat, first_area_light=lid, reverse_orientation=reverse)
        if extra_lights:
            s.add_light_point((0.5, 0.4, 0.3), (3.0, 0.5, -0.2))
            s.add_light_infinite((0.02, 0.03, 0.04))
        _setup_view(s, host, res, spp, sampler, inside_camera(host, res), sobol_tables=sobol_tables)
        s.build_accel(0, 4)
    return capture, n_lights


def furnace_expect(Le, rho, D):
    """E = Le * sum_{k=0..D} rho^k per channel: the camera hit's Le, then each of the D vertices adds beta * rho * Le by direct
    lighting (beta = rho^k: cosine sampling of a Lambertian lobe has f cos / pdf = rho)."""
    Le = np.asarray(Le, np.float64) * np.ones(3); rho = np.asarray(rho, np.float64) * np.ones(3)
    if D < 0:
        return np.zeros(3)
    return Le * sum(rho ** k for k in range(D + 1))


def furnace_wrongs(Le, rho, D, n_lights):
    """The plausible wrong answers of form A (closed forms of the mistakes the tests must be able to see)."""
    E = furnace_expect(Le, rho, D)
    Le3 = np.asarray(Le, np.float64) * np.ones(3)
    w = {"depth D+1": furnace_expect(Le, rho, D + 1),
         "Le at every hit": E + (E - Le3),                             # each later vertex adds beta * Le on top of its direct light
         "light-choice factor dropped": Le3 + (E - Le3) / n_lights}    # direct light divided by n_lights (uniform / equal-power choice)
    if D >= 1:
        w["depth D-1"] = furnace_expect(Le, rho, D - 1)
    return w


def fresnel_dielectric(cos_i, eta):
    """Unpolarised Fresnel reflectance of a smooth dielectric (f64), incidence from the side with index 1."""
    cos_i = abs(cos_i)
    sin_t = math.sqrt(max(0.0, 1.0 - cos_i * cos_i)) / eta
    if sin_t >= 1.0:
        return 1.0
    cos_t = math.sqrt(1.0 - sin_t * sin_t)
    r_par = (eta * cos_i - cos_t) / (eta * cos_i + cos_t)
    r_perp = (cos_i - eta * cos_t) / (cos_i + eta * cos_t)
    return 0.5 * (r_par * r_par + r_perp * r_perp)


def glass_slab(host, Le, eta=1.5, tilt_deg=0.0, res=16, spp=16, thickness=0.5):
    """Form D: a slab of smooth glass (Kr = Kt = 1: the FresnelSpecular lobe) between two parallel faces, wider than the view,
    under a constant infinite light Le, seen by an orthographic camera looking down -z; the slab is tilted by tilt_deg about x."""
    t = math.radians(tilt_deg)
    n = np.array([0.0, -math.sin(t), math.cos(t)])          # the front face's outward normal
    u = np.array([1.0, 0.0, 0.0]); v = np.cross(n, u)       # u x v = n
    W = 60.0

    def quad(c, a, b):
        P = np.array([c - W * a - W * b, c + W * a - W * b, c + W * a + W * b, c - W * a + W * b], np.float32)
        return P, np.array([0, 1, 2, 0, 2, 3], np.uint32)

    def capture(s):
        glass = s.add_material_glass((1, 1, 1), (1, 1, 1), 0.0, 0.0, eta)
        s.add_mesh(*quad(np.zeros(3), u, v), glass)                   # normal +n: faces the camera
        s.add_mesh(*quad(-thickness * n, v, u), glass)                # normal -n: faces away
        s.add_light_infinite(Le)
        _setup_view(s, host, res, spp, HALTON, ortho_down(host, res))
        s.build_accel(0, 4)
    return capture


def glass_slab_expect(Le, D, eta=1.5, tilt_deg=0.0, entry_only=False):
    """E = Le * sum_{k=1..D} P_k: the path escapes after k interface events with P_1 = F, P_k = (1-F)^2 F^(k-2), k >= 2, and every
    escaping path carries beta = 1 (its one entry's 1/eta^2 and one exit's eta^2 cancel).  The faces are parallel, so the inner
    incidence angle is the refracted one and F is the same at every event (no total internal reflection).  entry_only: the wrong
    answer where 1/eta^2 is applied on entry and nothing on exit."""
    F = fresnel_dielectric(math.cos(math.radians(tilt_deg)), eta)
    tr = 1.0 / (eta * eta) if entry_only else 1.0
    tot = sum((F if k == 1 else tr * (1 - F) ** 2 * F ** (k - 2)) for k in range(1, D + 1))
    return np.asarray(Le, np.float64) * np.ones(3) * tot


def glass_over_emitter(host, Le, eta=1.5, res=16, spp=16):
    """Form D2: one smooth-glass interface (facing the camera) over a black one-sided emitter facing up; nothing else emits.  A
    camera ray refracts in with probability 1 - F and meets the emitter with beta = 1/eta^2 (radiance is compressed entering the
    denser medium: the (eta_i/eta_t)^2 factor of FresnelSpecular in TransportMode::Radiance); the reflected part sees nothing."""
    def quad(z, flip=False):
        W = 60.0
        P = np.array([[-W, -W, z], [W, -W, z], [W, W, z], [-W, W, z]], np.float32)
        return P, np.array([0, 2, 1, 0, 3, 2] if flip else [0, 1, 2, 0, 2, 3], np.uint32)

    def capture(s):
        glass = s.add_material_glass((1, 1, 1), (1, 1, 1), 0.0, 0.0, eta)
        black = s.add_material_matte((0, 0, 0), 0.0)
        s.add_mesh(*quad(0.0), glass)
        lid = s.add_light_diffuse_area(Le, 2)
        s.add_mesh(*quad(-1.0), black, first_area_light=lid)
        _setup_view(s, host, res, spp, HALTON, ortho_down(host, res))
        s.build_accel(0, 4)
    return capture


def glass_over_emitter_expect(Le, D, eta=1.5, factor=None):
    F = fresnel_dielectric(1.0, eta)
    f = 1.0 / (eta * eta) if factor is None else factor
    return np.asarray(Le, np.float64) * np.ones(3) * ((1 - F) * f if D >= 1 else 0.0)


def _zquad(z, W, down=False, n=1, c=(0.0, 0.0)):
    P, idx = _face((c[0], c[1], z), (W, 0.0, 0.0), (0.0, W, 0.0), n)
    if down:
        idx = idx.reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)
    return P, np.ascontiguousarray(idx)


def null_veil(host, Le, rho, res=16, spp=16, W=60.0):
    """Form C: two wide parallel Lambertian (Kd = rho) emitters facing each other (floor z = 0 facing up, ceiling z = 1 facing
    down, one-sided, Le) with a wide 'none'-material veil at z = 0.5 between them; an orthographic camera at z = 0.9 looks down
    through the veil.  Reading of path.rs:120-150 and estimate_direct: the camera ray's first hit is the veil, where the emission
    check (bounces == 0, nothing emitted) and then the depth cut-off run BEFORE the null-BSDF skip — so at max_depth 0 the path
    ends on the veil and L = 0.  For D >= 1 the ray skips the veil without spending a bounce and adds the floor's Le; every shadow
    ray and every MIS-BSDF ray from the floor is stopped by the veil (intersect_p / intersect do not consult the material, and a
    BSDF ray whose first hit is not the sampled light gets no Le); the continuation ray meets the veil at bounces >= 1, where
    nothing is added.  So L = Le exactly, for every sample and every D >= 1.  (A veil cube inset in a closed emissive cube would
    not do: wall-to-wall segments near the cube's edges run outside the veil.)"""
    rho = tuple(float(r) for r in np.broadcast_to(np.asarray(rho, np.float64), (3,)))

    def capture(s):
        mat = s.add_material_matte(rho, 0.0)
        none = s.add_material_none()
        # every quad's centre lies off the view so that no triangle edge crosses it: a camera ray landing exactly on a shared
        # edge is not what this case is about
        for z, down in ((0.0, False), (1.0, True)):
            P, idx = _zquad(z, W, down, c=(33.0, -25.0))
            lid = s.add_light_diffuse_area(Le, len(idx) // 3)
            s.add_mesh(P, idx, mat, first_area_light=lid)
        s.add_mesh(*_zquad(0.5, W, c=(33.0, -25.0)), none)
        _setup_view(s, host, res, spp, HALTON, ortho_down(host, res, z=0.9))
        s.build_accel(0, 4)
    return capture


def null_stack(host, Le, K, res=8, spp=2):
    """K parallel 'none' quads between an orthographic camera and a black one-sided emitter facing it.  At max_depth 1 every
    camera ray skips the K quads (no bounce spent), adds the emitter's Le and ends there (a black matte has no lobe): L = Le."""
    def capture(s):
        none = s.add_material_none()
        black = s.add_material_matte((0, 0, 0), 0.0)
        for k in range(K):
            s.add_mesh(*_zquad(1.0 + 3.0 * k / max(K, 1), 4.0), none)
        lid = s.add_light_diffuse_area(Le, 2)
        s.add_mesh(*_zquad(0.0, 4.0), black, first_area_light=lid)
        _setup_view(s, host, res, spp, HALTON, ortho_down(host, res, z=6.0))
        s.build_accel(0, 4)
    return capture


# ---- E: mirror corridor ------------------------------------------------------------------------------------------------------

CORRIDOR = dict(g=0.5, y0=-2.0, y1=2.0, h=1.0)   # mirrors at x = +-g, spanning y in [y0, y1] and z in [-h, h]


def mirror_corridor(host, Le, kr, res=24, spp=1, angle_deg=50.0):
    """Form E: two parallel finite mirrors (add_material_mirror: SpecularReflection with FresnelNoOp, per-channel kr) facing
    each other across a corridor, under a constant sky Le.  An orthographic camera inside the corridor near one end looks down
    it at angle_deg from its axis, every sample at its pixel's centre, so each pixel's ray zig-zags between the mirrors a number
    of times N that depends on where it starts, then escapes through the far end (or over the top) to the sky."""
    c = CORRIDOR
    t = math.radians(angle_deg)
    d = np.array([math.sin(t), math.cos(t), 0.04])

    def capture(s):
        m = s.add_material_mirror(kr)
        for x in (-c["g"], c["g"]):
            P = np.array([[x, c["y0"], -c["h"]], [x, c["y1"], -c["h"]], [x, c["y1"], c["h"]], [x, c["y0"], c["h"]]], np.float32)
            s.add_mesh(P, np.array([0, 1, 2, 0, 2, 3], np.uint32), m)
        s.add_light_infinite(Le)
        eye = np.array([0.0, -1.3, 0.0])
        _, c2w = host.look_at(list(eye), list(eye + d), [0, 0, 1])
        s.set_camera_orthographic(host.orthographic_raster_to_camera(res, res, screen=(-0.8, 0.8, -0.3, 0.3)), c2w)
        cb, table, sb = host.film_box(res, res)
        s.set_film(res, res, cb, (0.5, 0.5), table)
        s.set_sampler(HALTON, spp, sb, sample_at_pixel_center=True)
        s.build_accel(0, 4)
    return capture


def mirror_bounces(rays, edge=1e-4, max_n=10000):
    """float64 reflect loop against the corridor's two mirrors for the rays generate_camera_rays returned: (N reflections before
    the ray escapes, usable mask).  A ray that meets a mirror plane within `edge` of the mirror's rim is unusable: f32 decides
    those hits, not the closed form."""
    c = CORRIDOR
    N = np.zeros(len(rays), np.int64); ok = np.ones(len(rays), bool)
    for i in range(len(rays)):
        p = rays["o"][i].astype(np.float64); v = rays["d"][i].astype(np.float64)
        n = 0
        while n < max_n and v[0] != 0.0:
            ts = [t for t in ((x - p[0]) / v[0] for x in (-c["g"], c["g"])) if t > 1e-9]   # either plane, from either side
            if not ts:
                break
            q = p + min(ts) * v
            dy = min(q[1] - c["y0"], c["y1"] - q[1]); dz = c["h"] - abs(q[2])
            if abs(dy) < edge or abs(dz) < edge:
                ok[i] = False
            if dy < 0.0 or dz < 0.0:
                break
            p = q; v = v * np.array([-1.0, 1.0, 1.0]); n += 1
        N[i] = n
    return N, ok


def mirror_expect(Le, kr, N, D):
    """Per pixel: Le kr^N if the ray escapes after N <= D reflections (the N-th one happens at bounces = N - 1 < D; the sky is
    added at the escape because every vertex was specular), else 0.  N: array of reflection counts; returns (..., 3)."""
    kr = np.asarray(kr, np.float64)
    N = np.asarray(N)
    return np.where((N <= D)[..., None], np.asarray(Le, np.float64) * kr ** N[..., None], 0.0)


def corridor_rays(host, Scene, kr, res, angle_deg=50.0):
    """The corridor's capture, its pixels' reflection counts N (res x res) and usable mask, from the scene's own camera rays."""
    cap = mirror_corridor(host, LE, kr, res=res, angle_deg=angle_deg)
    s = Scene(); cap(s)
    rays, _ = s.generate_camera_rays([0, 0, res, res], 0)
    N, ok = mirror_bounces(rays)
    return N.reshape(res, res), ok.reshape(res, res)


def mirror_rr_survival(kr, N, rr_threshold=1.0):
    """Probability that Russian roulette lets a path of N mirror reflections reach the sky: after the vertex at bounces = b
    (eta_scale = 1) RR runs if max(beta) < rr_threshold and b > 3, and stops the path with q = max(0.05, 1 - max(beta)).  beta is kr^(b+1)
    over the 1 - q of every RR the path has survived: the weights already applied feed the next q.
    The mean is kept by the 1/(1-q) weight; survival * E is the wrong answer where that weight is dropped."""
    m = float(np.max(kr))
    p = 1.0; beta = 1.0
    for b in range(N):
        beta *= m
        if b > 3 and beta < rr_threshold:
            q = max(0.05, 1.0 - beta)
            p *= 1.0 - q
            beta /= 1.0 - q
    return p


# ---- Sobol tables and the raw render entry point ---------------------------------------------------------------------------

def sobol_fixture():
    """tests/golden/sobol_subset.npz: 48 dimensions and 9 VdC matrices of the reference's Sobol tables."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sobol_subset.npz"))
    return z["m32"], z["vdc"], z["vdc_inv"]


def sobol_scene(host, res, Scene):
    """Form A (rho 0.5, 4 spp) with the Sobol sampler and the fixture's tables, captured into a new Scene (product or oracle)."""
    s = Scene()
    cap, _ = emissive_furnace(host, LE, 0.5, res=res, spp=4, sampler=SOBOL, sobol_tables=sobol_fixture())
    cap(s)
    return s


def raw_render(s, max_depth, pb):
    """The C entry point with sentinel-filled outputs: a refusal must leave them untouched (nothing was rendered)."""
    h, w = s.film_shape
    xyz = np.full((h, w, 3), np.nan, np.float32); wt = np.full((h, w), -7.0, np.float32)
    pb = np.ascontiguousarray(pb, dtype=np.int32)
    st = pbrt_hip.Stats()
    fp = C.POINTER(C.c_float)
    rc = s.b.fn("render_path")(s.h, max_depth, C.c_float(1.0), 0, pb.ctypes.data_as(C.POINTER(C.c_int)), 16, 0, 1,
                               xyz.ctypes.data_as(fp), wt.ctypes.data_as(fp), C.byref(st))
    return rc, xyz, wt, st


# ---- the statistical check ------------------------------------------------------------------------------------------------

def frame_stats(rgb):
    px = np.asarray(rgb, np.float64).reshape(-1, 3)
    return px.mean(axis=0), px.std(axis=0) / math.sqrt(len(px))


def assert_mean(rgb, expected, k=5.0, se_target=0.02, wrongs=None, label=""):
    """|mean - E| <= k se + 1e-6 E per channel (se = std(pixels) / sqrt(n_pixels)), se / E below se_target wherever E > 0, and
    (power) every wrong answer in `wrongs` lies at least 4 tolerance widths from E in some channel — a case too noisy to tell
    the right answer from the wrong ones fails loudly instead of passing."""
    E = np.asarray(expected, np.float64) * np.ones(3)
    mean, se = frame_stats(rgb)
    tol = k * se + 1e-6 * np.abs(E)
    wrongs = wrongs or {}
    near = min(wrongs.items(), key=lambda kv: np.max(np.abs(np.asarray(kv[1]) - E) / np.maximum(tol, 1e-30)), default=None)
    msg = (f"{label}: E={E}, mean={mean}, se={se}, nearest wrong answer: "
           + (f"{near[0]}={np.asarray(near[1])}" if near else "none"))
    pos = E > 0
    assert np.all(se[pos] / E[pos] < se_target), "too noisy to mean anything (se/E >= %g): " % se_target + msg
    for name, W in wrongs.items():
        dist = np.max(np.abs(np.asarray(W, np.float64) - E) / np.maximum(tol, 1e-30))
        assert dist >= 4.0, f"no power against '{name}' ({dist:.2f} tolerance widths away): " + msg
    assert np.all(np.abs(mean - E) <= tol), msg
    return mean, se
