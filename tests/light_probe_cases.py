"""Case generators for the light probe (light_probe_batch), shared by the CPU test that measures what the cases reach on the oracle and the GPU test that compares
the device with the oracle bit for bit.

One small scene per light set — a matte quad under the lights, accelerator built, so that the world radius is a real number — captured into both sides by
`LightSet.capture`.  A set's cases are batches {light, op, ref (n, 10) = p, p_error, n, time, u (n, 2), wi (n, 3), tag}: a deterministic edge list (the reference point
edges every set gets, the light's own branch boundaries) crossed with a seeded random fill.  Everything is float32 from the start, so that both sides receive the same
bits; where an edge depends on what the light holds (the CDF entries of a Distribution2D, the point a sample lands on, reference points whose cosine equals a spot's
cut-off) it is taken from the oracle's own answers."""
import ctypes as C
import math

import numpy as np

import pbrt_hip
import sphere_light_scenes as SL
from probe_cases import F, MAX_PROBES, NAN_SHARE, ONE_MINUS_EPS, dn, hexf, up

STRIDE = 28
WI, PDF, VAL, VALID, VP, VPERR, VN, RO, RD, TMAX = slice(0, 3), 3, slice(4, 7), 7, slice(8, 11), slice(11, 14), slice(14, 17), slice(17, 20), slice(20, 23), 23
TIME = F(0.25)
# Offsets from a light at the origin whose distance_squared is a nonzero float32 denormal (below 1.1755e-38): the first three near 1e-38, where I / d^2 of an intensity of a few
# units is still finite, the others further down, where it overflows.  (1e-23 squares to 0: such a point is *at* the light.)  They survive only where light space is world space.
DENORMAL_D2 = [[0, 0, 1e-19], [1e-20, 1e-20, 1e-19], [0, 0, 1.05e-19], [6e-20, 0, 8e-20], [1e-20, 0, 2e-20], [0, 0, 3e-22], [0, 2e-21, 1e-21]]
TAYLOR = F(0.00068523)   # sphere.rs: sin^2(1.5 deg), below which the cone sample switches to its Taylor form


def ulps(x, ks):
    """x moved by each k of ks float32 steps (x != 0, no sign change)."""
    b = np.array([x], F).view(np.int32).astype(np.int64)[0]
    s = 1 if x > 0 else -1
    return (b + s * np.asarray(ks, np.int64)).astype(np.int32).view(F)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


def mk_ref(p, p_error=None, n=None):
    """(k, 10) reference points from (k, 3) positions; p_error and n broadcast."""
    p = np.asarray(p, F).reshape(-1, 3)
    r = np.zeros((len(p), 10), F)
    r[:, 0:3] = p
    r[:, 3:6] = (np.abs(p) * F(6e-7) if p_error is None else np.asarray(p_error, F))
    r[:, 6:9] = (np.array([0, 0, 1], F) if n is None else np.asarray(n, F))
    r[:, 9] = TIME
    return r


def ref_edges(canonical, target):
    """The reference-point edges every light set gets: the canonical point; n = 0 and p_error = 0 (what spatial_compute_kernel passes); a large p_error with n towards the
    light and away from it; coordinates near 1e-30, near 1e18 and denormal.  `target`: a point of the light, for the two normals."""
    c = np.asarray(canonical, F); t = unit(np.asarray(target, np.float64) - c.astype(np.float64))
    return np.concatenate([
        mk_ref(c, n=t),
        mk_ref(c, p_error=(0, 0, 0), n=(0, 0, 0)),
        mk_ref(c, p_error=(0.5, 0.25, 0.75), n=t),
        mk_ref(c, p_error=(0.5, 0.25, 0.75), n=-t),
        mk_ref([1e-30, -2e-30, 3e-30], n=t),
        mk_ref([1e18, 2e18, -1e18], n=t),
        mk_ref([1e-40, 0, -1e-41], p_error=(1e-42, 0, 1e-45), n=t),
    ])


def random_refs(rng, centre, spread, k, target=None):
    p = (np.asarray(centre, np.float64) + rng.normal(size=(k, 3)) * spread).astype(F)
    n = rng.normal(size=(k, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    if target is not None:   # half of them face the light
        t = np.asarray(target, np.float64) - p
        n[::2] = (t / np.linalg.norm(t, axis=1, keepdims=True))[::2]
    return mk_ref(p, n=n.astype(F))


def cross(a, b):
    """every row of a with every row of b"""
    return np.repeat(a, len(b), axis=0), np.tile(b, (len(a), 1))


def batch(light, op, ref, u=None, wi=None, tag=""):
    ref = np.ascontiguousarray(ref, F).reshape(-1, 10); n = len(ref)
    u = np.full((n, 2), 0.5, F) if u is None else np.ascontiguousarray(u, F).reshape(-1, 2)
    wi = np.tile(np.array([0, 0, 1], F), (n, 1)) if wi is None else np.ascontiguousarray(wi, F).reshape(-1, 3)
    assert len(u) == n and len(wi) == n, (tag, n, len(u), len(wi))
    return dict(light=light, op=op, ref=ref, u=u, wi=wi, tag=tag)


def sample_batch(light, refs, us, tag):
    a, b = cross(refs, np.asarray(us, F).reshape(-1, 2))
    return batch(light, 0, a, u=b, tag=tag)


def dir_batches(light, refs, dirs, tag):
    a, b = cross(refs, np.asarray(dirs, F).reshape(-1, 3))
    return [batch(light, 1, a, wi=b, tag=tag + " pdf_li"), batch(light, 2, a, wi=b, tag=tag + " le")]


def random_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def around(values):
    """each value, one float32 below and one above, clipped to a sample's range [0, 1 - eps]"""
    v = np.asarray(values, F).reshape(-1)
    return np.unique(np.clip(np.concatenate([v, np.nextafter(v, F(-1)), np.nextafter(v, F(2))]), F(0), ONE_MINUS_EPS))


def light_distribution(orc, light):
    """(dw, dh, marginal cdf (dh + 1), conditional cdfs (dh, dw + 1)) of an infinite light, as the oracle holds them."""
    fn = orc.b.lib.oracle_light_distribution
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_float), C.c_uint64]
    buf = np.zeros(1 << 16, F)
    get = lambda what: buf[:fn(orc.h, light, what, buf.ctypes.data_as(C.POINTER(C.c_float)), len(buf))].copy()
    dims = get(0)
    assert len(dims) == 2, "oracle_light_distribution refused"
    dw, dh = int(dims[0]), int(dims[1])
    return dw, dh, get(1), get(2).reshape(dh, dw + 1)


def add_floor(s):
    """the few triangles every probe scene carries; returns the material"""
    m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
    P = np.array([[-2, -2, -1], [2, -2, -1], [2, 2, -1], [-2, 2, -1]], F)
    s.add_mesh(P, np.array([0, 1, 2, 0, 2, 3], np.uint32), m)
    return m


class LightSet:
    """name; build(s, host): adds the set's lights (the floor and the accelerator come from capture); cases(orc, host): its batches; variant: 0 (compared under 0 and, for
    lights without a map, 1) or 2; mapped: the lights that hold a map."""

    def __init__(self, name, build, cases, variant=0, mapped=()):
        self.name, self.build, self._cases, self.variant, self.mapped = name, build, cases, variant, set(mapped)

    def capture(self, s, host):
        def go(s, host):
            add_floor(s)
            self.build(s, host)
            s.build_accel(0, 4)
        SL.capture(go, s, host)   # the oracle's libm in mode 1 while it captures, as for every scene with a sphere

    def cases(self, orc, host, seed=0):
        batches = thin_nans(orc, self._cases(orc, host, np.random.default_rng(7000 + seed)), self.variant)
        total = sum(len(b["ref"]) for b in batches)
        assert 0 < total <= MAX_PROBES, (self.name, total)
        return batches


def run_batches(scene, batches, variant=0):
    return [scene.light_probe_batch(b["light"], b["op"], b["ref"], b["u"], b["wi"], variant=variant) for b in batches]


def thin_nans(orc, batches, variant):
    """The reference's formulas give NaN for a reference point at a point light's position, for le of a zero vector, for a zero-area triangle.  Such probes stay in the set,
    where both sides must put a NaN in the same slots, but thinned at a fixed stride until they are at most NAN_SHARE of the set.  Decided on the oracle's output only."""
    outs = run_batches(orc, batches, variant)
    total = sum(len(b["ref"]) for b in batches)
    n_nan = sum(int(np.isnan(o).any(axis=1).sum()) for o in outs)
    if n_nan <= NAN_SHARE * total:
        return batches
    keep_every = int(math.ceil(n_nan / (NAN_SHARE * (total - n_nan) / (1.0 - NAN_SHARE))))
    thinned, seen = [], 0
    for b, o in zip(batches, outs):
        nan = np.isnan(o).any(axis=1)
        order = seen + np.cumsum(nan) - 1
        keep = ~nan | (order % keep_every == 0)
        seen += int(nan.sum())
        thinned.append(dict(light=b["light"], op=b["op"], ref=b["ref"][keep], u=b["u"][keep], wi=b["wi"][keep], tag=b["tag"]))
    return thinned


def describe(set_name, b, i):
    """One probe's inputs as hex floats, for a failure message."""
    return f"set {set_name} light {b['light']} op {b['op']} ({b['tag']}) probe {i}: ref {hexf(b['ref'][i])} u {hexf(b['u'][i])} wi {hexf(b['wi'][i])}"


# ---------------------------------------------------------------- infinite lights -----------------------------------------------------------------------------------
def light_space_dirs(dw, dh):
    """Directions of light space for pdf_li and le: the poles, the seam with y = +0 and y = -0 and just under 2 pi, the cell boundaries k / dw and k / dh from either side,
    a zero vector and vectors that are not unit length."""
    d = [[0, 0, 1], [0, 0, -1], [1, 0, 0.0], [1, -0.0, 0.0], [1, -1e-45, 0.2], [1, -1e-40, 0], [1, -1e-10, 0], [1, -1e-8, 0.3], [1, -3e-8, 0], [1, -6e-8, 0], [1, -1e-7, 0],
         [-1, 0.0, 0], [-1, -0.0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0], [0.0, 0.0, 1e-30], [1e-20, 2e-20, -1e-20], [3e19, 1e19, 2e19], [0.3, -0.4, 3.7],
         [1e-4, 0, -1], [0, 1e-7, -1], [1e-4, 1e-4, 1], [0, -0.0, -1]]
    for k in range(dw + 1):   # phi = 2 pi k / dw
        for e in (-2e-7, 0.0, 2e-7):
            a = 2.0 * math.pi * k / dw * (1.0 + e)
            d.append([math.cos(a), math.sin(a), 0.3])
    for k in range(1, dh):    # theta = pi k / dh
        for e in (-2e-7, 0.0, 2e-7):
            t = math.pi * k / dh * (1.0 + e)
            d.append([math.sin(t) * 0.8, math.sin(t) * 0.6, math.cos(t)])
    return np.array(d, F)


def infinite_cases(orc, host, rng, lights, l2w, canonical=(0.3, -0.2, 0.1)):
    """lights: the infinite lights' numbers; l2w[k]: light k's light_to_world matrix."""
    out = []
    edges = ref_edges(canonical, (0.3, -0.2, 5.0))
    for li in lights:
        dw, dh, marg, cond = light_distribution(orc, li)
        tiny = [0, 1e-45, 1e-42, 1e-40, 1e-38, 1e-30, 1e-20, 1e-10, 1e-8, ONE_MINUS_EPS, 0.3137, 0.6871]
        uy = np.unique(np.concatenate([around(marg), np.array(tiny, F)]))
        ux_few = np.array([0, 0.3137, ONE_MINUS_EPS], F)
        # every marginal entry against a few u.x, on a few reference points
        refs = np.concatenate([edges[:3], edges[5:6]]) if dh > 8 else edges
        a, b = cross(uy.reshape(-1, 1), ux_few.reshape(-1, 1))
        out.append(sample_batch(li, refs, np.concatenate([b, a], axis=1), "marginal cdf entries"))
        # rows: the first, the last, and every row next to a flat stretch of the marginal cdf (a black row), at most six; u.y in the row's own interval
        flat = np.flatnonzero(np.diff(marg) == 0)
        rows = sorted(set([0, dh - 1] + [int(r) for r in np.concatenate([flat - 1, flat, flat + 1]) if 0 <= r < dh]))[:6]
        for r in rows:
            lo, hi = float(marg[r]), float(marg[r + 1])
            uys = np.unique(np.clip(np.array([lo, 0.5 * (lo + hi), dn(hi) if hi > 0 else 0], F), F(0), ONE_MINUS_EPS))
            ux = np.unique(np.concatenate([around(cond[r]), np.array([0, 1e-45, 1e-30, ONE_MINUS_EPS, 0.77], F)]))
            a, b = cross(ux.reshape(-1, 1), uys.reshape(-1, 1))
            out.append(sample_batch(li, edges[:2], np.concatenate([a, b], axis=1), f"conditional cdf entries of row {r}"))
        out.append(sample_batch(li, random_refs(rng, canonical, 2.0, 6), rng.random((40, 2)).astype(F), "random"))
        # pdf_li and le: the light-space edge directions carried to world space, the same vectors taken as world directions, random ones
        ls = light_space_dirs(dw, dh)
        dirs = np.concatenate([host.transform_vectors(l2w[li], ls), ls, random_dirs(rng, 40)]).astype(F)
        out += dir_batches(li, edges[:3], dirs, "edge directions")
    return out


ROT = dict(theta=37.0, axis=(1.0, 2.0, 3.0))


def _const_transforms(host):
    mirror = host.compose(host.scale((-1.0, 1.0, 1.0)), host.rotate(20.0, (0.0, 1.0, 0.5)))
    return [(pbrt_hip.IDENTITY, pbrt_hip.IDENTITY), host.rotate(ROT["theta"], ROT["axis"]), host.scale((2.0, 0.5, 3.0)), mirror]


def _build_infinite_const(s, host):
    for k, t in enumerate(_const_transforms(host)):
        s.add_light_infinite((0.4 + k, 0.8, 1.3), t[0], t[1])


def _cases_infinite_const(orc, host, rng):
    ts = _const_transforms(host)
    return infinite_cases(orc, host, rng, range(len(ts)), [t[0] for t in ts])


def _map_images():
    rng = np.random.default_rng(41)
    img = lambda h, w: (rng.random((h, w, 3)) * 2.0 + 0.05).astype(F)
    black_rows = img(8, 4); black_rows[2:5] = 0          # three black rows: the scalar image is filtered between rows, two of its rows in between come out black
    black_texels = img(4, 8)
    for r in range(4):                                   # per row a pair of black texels (one alone would be filtered away), at an offset that moves with the row and wraps
        black_texels[r, [(3 * r) % 8, (3 * r + 1) % 8]] = 0
    return [("1x1", img(1, 1)), ("2x64", img(64, 2)), ("64x2", img(2, 64)), ("5x3", img(3, 5)), ("black_rows", black_rows), ("black_texels", black_texels),
            ("black", np.zeros((2, 2, 3), F))]


def _build_infinite_map(s, host):
    rot = host.rotate(ROT["theta"], ROT["axis"])
    for k, (_, image) in enumerate(_map_images()):
        t = rot if k % 2 else (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY)
        s.add_light_infinite_map((1.0, 0.9, 0.8), image, t[0], t[1])


def _cases_infinite_map(orc, host, rng):
    rot = host.rotate(ROT["theta"], ROT["axis"])
    n = len(_map_images())
    return infinite_cases(orc, host, rng, range(n), [rot[0] if k % 2 else pbrt_hip.IDENTITY for k in range(n)])


# ---------------------------------------------------------------- spot ----------------------------------------------------------------------------------------------
SPOT_TOTAL, SPOT_START = F(math.cos(math.radians(30.0))), F(math.cos(math.radians(25.0)))
# lights 0..4 share position (the origin), axis (+z) and the identity transform, so that one reference point has one cos_theta under all of them: 0 the cone with a falloff,
# 1 / 2 cone_delta = 0 at SPOT_TOTAL and one float32 above it, 3 / 4 the same at SPOT_START; 5 a point light there (its value is I / d^2: a spot's where fall == 1);
# 6 / 7 a rotated, translated cone with a falloff and one with cone_delta = 0
SPOT_FROM, SPOT_TO = (1.0, 2.0, 3.0), (0.2, -0.1, 0.3)
SPOT_I = (3.0, 2.0, 1.5)


def _build_spot(s, host):
    I = pbrt_hip.IDENTITY
    s.add_light_spot(SPOT_I, I, I, SPOT_TOTAL, SPOT_START)
    for c in (SPOT_TOTAL, up(SPOT_TOTAL), SPOT_START, up(SPOT_START)):
        s.add_light_spot(SPOT_I, I, I, c, c)
    s.add_light_point(SPOT_I, (0.0, 0.0, 0.0))
    ident = (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY)
    l2w, w2l, ct, cs = host.spot(ident, SPOT_FROM, SPOT_TO, 30.0, 5.0)
    s.add_light_spot(SPOT_I, l2w, w2l, ct, cs)
    l2w, w2l, ct, cs = host.spot(ident, SPOT_FROM, SPOT_TO, 20.0, 0.0)
    s.add_light_spot(SPOT_I, l2w, w2l, ct, cs)


def cone_points(cos_cut, radii=(0.5, 1.0, 3.0, 7.5), azimuths=(0.0, 0.9, 2.2, 4.1, 5.5), steps=range(-24, 25)):
    """points around the cone of half-angle acos(cos_cut) about +z from the origin, a few float32 of angle either side of it"""
    tc = math.acos(float(cos_cut))
    p = [[r * math.sin(tc + k * 3e-8) * math.cos(a), r * math.sin(tc + k * 3e-8) * math.sin(a), r * math.cos(tc + k * 3e-8)] for r in radii for a in azimuths for k in steps]
    return np.array(p, F)


def spot_equal_points(orc, cos_cut, light_at, light_above):
    """Among cone_points(cos_cut), those whose cos_theta equals cos_cut in float32, found on the oracle: the cone_delta = 0 light at the cut-off lights them (cos_theta >= cut),
    the one a float32 above it does not.  Returns (all the points, the mask of the equal ones)."""
    p = cone_points(cos_cut)
    r = mk_ref(p)
    at = orc.light_probe_batch(light_at, 0, r)[:, VAL]; above = orc.light_probe_batch(light_above, 0, r)[:, VAL]
    return p, (at[:, 0] > 0) & (above[:, 0] == 0)


def _cases_spot(orc, host, rng):
    out = []
    pt, eq_t = spot_equal_points(orc, SPOT_TOTAL, 1, 2)
    ps, eq_s = spot_equal_points(orc, SPOT_START, 3, 4)
    edges = ref_edges((0.3, -0.2, 2.0), (0, 0, 0))
    special = mk_ref([[0, 0, 0], [1e20, 1e20, 3e20], [0, 0, 3e19], [1e-23, 0, 2e-23], [0, 0, 1e-23], [0, 0, 5], [0, 0, -5], [1e-30, 0, 1e-30]] + DENORMAL_D2)
    for li in range(5):
        out.append(batch(li, 0, mk_ref(pt), tag="around cos_total_width")); out.append(batch(li, 0, mk_ref(ps), tag="around cos_falloff_start"))
        out.append(batch(li, 0, mk_ref(pt[eq_t]), tag="cos_theta == SPOT_TOTAL")); out.append(batch(li, 0, mk_ref(ps[eq_s]), tag="cos_theta == SPOT_START"))
        out.append(batch(li, 0, np.concatenate([edges, special, random_refs(rng, (0, 0, 2), 1.0, 1200)]), tag="edges and random"))
    out.append(batch(5, 0, np.concatenate([mk_ref(pt), mk_ref(ps), edges, special]), tag="point light at the spots' position"))
    # the rotated cones: the same rings carried to their frame (rounding moves them by a few float32: the nearest values on each side), their own position, far and near
    ident = (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY)
    for li, (angle, delta) in ((6, (30.0, 5.0)), (7, (20.0, 0.0))):
        l2w, _, ct, cs = host.spot(ident, SPOT_FROM, SPOT_TO, angle, delta)
        rings = np.concatenate([cone_points(c, radii=(1.0, 4.0), azimuths=(0.3, 2.0, 4.4)) for c in sorted({ct, cs})])
        pos = np.array(SPOT_FROM, F)
        sp = mk_ref([pos, pos + F(1e-23), pos * F(1e19), [0, 0, 0]])
        out.append(batch(li, 0, np.concatenate([mk_ref(host.transform_points(l2w, rings)), ref_edges((0.3, -0.2, 0.1), SPOT_FROM), sp, random_refs(rng, SPOT_TO, 1.5, 300)]),
                         tag="rotated cone"))
    for li in (0, 6):
        out += dir_batches(li, edges[:2], random_dirs(rng, 8), "a delta light")
    return out


# ---------------------------------------------------------------- projection ------------------------------------------------------------------------------------------
# (fov, image shape (H, W) or None, rotated): no image / aspect 2 / aspect 0.5 / a frustum so wide that the near plane, not the screen window, decides
PROJECTIONS = [(45.0, None, False), (60.0, (2, 4), True), (90.0, (4, 2), False), (179.9, None, False), (179.9, (2, 2), True)]
PROJ_POS = (0.5, -1.0, 2.0)


def _proj_transform(host, rotated):
    """the rotated lights sit at PROJ_POS; the others at the origin under the identity, so that light space is world space and a ladder of float32 steps stays one"""
    return host.compose(host.translate(PROJ_POS), host.rotate(ROT["theta"], ROT["axis"])) if rotated else (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY)


def _build_projection(s, host):
    rng = np.random.default_rng(43)
    for fov, shape, rotated in PROJECTIONS:
        t = _proj_transform(host, rotated)
        s.add_light_projection((2.0, 3.0, 4.0), t[0], t[1], fov, None if shape is None else (rng.random(shape + (3,)) + 0.1).astype(F))


def _cases_projection(orc, host, rng):
    out = []
    ks = list(range(-6, 7))
    for li, (fov, shape, rotated) in enumerate(PROJECTIONS):
        t = _proj_transform(host, rotated)
        aspect = 1.0 if shape is None else shape[1] / shape[0]
        sx, sy = (aspect, 1.0) if aspect > 1 else (1.0, 1.0 / aspect)
        tan = math.tan(math.radians(fov) / 2.0)
        pts = [[0, 0, 5], [0, 0, 1], [0, 0, -5], [0.3, 0.2, -1], [1, 0, 0], [0, 1, 0.0], [0, 0, 0], [0, 0, 1e20], [1e19, 0, 2e19], [0, 0, 1e-23], [1e-23, 0, 1e-23]] + DENORMAL_D2   # on the axis: wp == 1
        for z in (1.0, 3.0):   # light-space points whose projection lands on each screen edge, and a few float32 either side of it
            for sgn in (-1.0, 1.0):
                pts += [[x, 0.1 * z * tan * sy, z] for x in ulps(sgn * sx * tan * z, ks)]
                pts += [[0.1 * z * tan * sx, y, z] for y in ulps(sgn * sy * tan * z, ks)]
                pts.append([sgn * sx * tan * z, sgn * sy * tan * z, z])   # a corner
        zc = 1e-3 / math.sqrt(1.0 - 1e-6)   # wl.z = z / |p| either side of 1e-3, where the wide frustums still have the point inside the window
        for x, y in ((1.0, 0.0), (-0.6, 0.8), (0.0, -1.0)):
            pts += [[x, y, z] for z in ulps(zc, range(-12, 13))] + [[x, y, -zc], [x, y, 0.0]]
        pts = np.array(pts, F)
        world = host.transform_points(t[0], pts)
        refs = np.concatenate([mk_ref(world), ref_edges((0.3, -0.2, 0.1), host.transform_points(t[0], [[0, 0, 0]])[0]), random_refs(rng, host.transform_points(t[0], [[0, 0, 2]])[0], 1.5, 500)])
        out.append(batch(li, 0, refs, tag="screen edges, near plane, axis"))
        out += dir_batches(li, refs[:2], random_dirs(rng, 6), "a delta light")
    return out


# ---------------------------------------------------------------- goniometric, point, distant --------------------------------------------------------------------------
def _delta_transforms(host):
    """at the origin under the identity (light space is world space: the seam's -0 and denormals survive), and rotated away from it"""
    return [(pbrt_hip.IDENTITY, pbrt_hip.IDENTITY), host.compose(host.translate((0.5, 1.0, 2.0)), host.rotate(ROT["theta"], ROT["axis"]))]


def _build_gonio(s, host):
    rng = np.random.default_rng(44)
    image = (rng.random((4, 8, 3)) + 0.1).astype(F)
    for t in _delta_transforms(host):
        s.add_light_goniometric((2.0, 3.0, 4.0), t[0], t[1], None)
        s.add_light_goniometric((2.0, 3.0, 4.0), t[0], t[1], image)


def _cases_gonio(orc, host, rng):
    out = []
    # light-space offsets from the light: the poles of the swapped axes (+-y), their seam (z = +-0 with x > 0), the opposite meridian, texel boundaries of the 8 x 4 diagram
    pts = [[0, 3, 0], [0, -3, 0], [1e-8, 3, 0], [0, 3, 1e-8], [2, 0.5, 0.0], [2, 0.5, -0.0], [2, 0.5, -1e-40], [2, 0.5, -1e-8], [2, 0.5, 1e-8], [-2, 0.5, 0.0], [-2, 0.5, -0.0],
           [0, 0, 0], [2e19, 2e19, 2e19], [1e19, 0, 0], [0, 3e19, 0], [1e-23, 0, 0], [0, 0, 2], [0, 0, -2]] + DENORMAL_D2
    for k in range(8):
        for e in (-1e-7, 0.0, 1e-7):
            a = 2.0 * math.pi * k / 8 * (1.0 + e)
            pts.append([math.cos(a), 0.4, math.sin(a)])
    for k in range(1, 4):
        for e in (-1e-7, 0.0, 1e-7):
            th = math.pi * k / 4 * (1.0 + e)
            pts.append([math.sin(th), math.cos(th), 0.3 * math.sin(th)])
    pts = np.array(pts, F)
    for k, t in enumerate(_delta_transforms(host)):
        pos = host.transform_points(t[0], [[0, 0, 0]])[0]
        refs = np.concatenate([mk_ref(host.transform_points(t[0], pts)), ref_edges((0.3, -0.2, 0.1), pos), random_refs(rng, pos, 2.0, 400)])
        for li in (2 * k, 2 * k + 1):
            out.append(batch(li, 0, refs, tag="poles, seam, texel boundaries"))
            out += dir_batches(li, refs[:2], random_dirs(rng, 6), "a delta light")
    return out


POINT_POS, DISTANT_W = (0.5, 1.0, 2.0), (0.3, 0.4, 0.86)


def _build_point_distant(s, host):
    s.add_light_point((5.0, 4.0, 3.0), POINT_POS)
    s.add_light_distant((1.0, 2.0, 3.0), DISTANT_W)
    s.add_light_point((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))


def _cases_point_distant(orc, host, rng):
    out = []
    pos = np.array(POINT_POS, F)
    special = mk_ref([pos, pos + F(1e-23), up(pos[0]) * np.array([1, 0, 0], F) + pos * np.array([0, 1, 1], F), pos * F(1e19), [1e20, -1e20, 1e20], [3e38, 0, 0], [0, 0, 0],
                      [1e-23, 1e-23, 0], [1e-30, 0, 0]] + DENORMAL_D2)   # the last: denormal d^2 from the point light at the origin
    refs = np.concatenate([ref_edges((0.3, -0.2, 0.1), POINT_POS), special, random_refs(rng, POINT_POS, 2.0, 600, target=POINT_POS)])
    for li in range(3):
        out.append(batch(li, 0, refs, tag="at the light, overflow, random"))
        out += dir_batches(li, refs[:2], random_dirs(rng, 6), "a delta light")
    return out


# ---------------------------------------------------------------- triangle area lights --------------------------------------------------------------------------------
BASE_TRI = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2]], np.float64)   # geometric normal +z, area 0.5
# name, two_sided, N (per-vertex normals or None), reverse_orientation, swaps_handedness, scale about the centroid, the triangle (None: BASE_TRI)
TRIANGLES = [
    ("one_sided", False, None, False, False, 1.0, None),
    ("two_sided", True, None, False, False, 1.0, None),
    ("normals_agree", False, [[0.1, 0, 1], [0, 0.1, 1], [-0.1, 0, 1]], False, False, 1.0, None),
    ("normals_oppose", False, [[0.1, 0, -1], [0, 0.1, -1], [-0.1, 0, -1]], False, False, 1.0, None),
    ("normals_perpendicular", False, [[1, 0, 0], [1, 0, 0], [1, 0, 0]], False, False, 1.0, None),
    ("normals_oppose_reversed", True, [[0.1, 0, -1], [0, 0.1, -1], [-0.1, 0, -1]], True, False, 1.0, None),
    ("reversed", False, None, True, False, 1.0, None),
    ("swapped", False, None, False, True, 1.0, None),
    ("reversed_swapped", False, None, True, True, 1.0, None),
    ("huge", False, None, False, False, 1e6, None),
    ("tiny", False, None, False, False, 1e-6, None),
    ("tilted", True, None, False, False, 1.0, [[0.2, -0.3, 1.5], [1.4, 0.1, 2.2], [-0.1, 0.9, 2.6]]),
    ("zero_area", False, None, False, False, 1.0, [[0, 0, 2], [0.5, 0.5, 2], [1, 1, 2]]),
]


def tri_points(k):
    name, _, _, _, _, scale, tri = TRIANGLES[k]
    t = BASE_TRI if tri is None else np.array(tri, np.float64)
    if scale < 1.0:   # the very small triangle sits at the origin, where float32 still resolves it
        return (t * scale).astype(F)
    c = t.mean(axis=0)
    return ((t - c) * scale + c + np.array([4.0 * k, 0, 0])).astype(F)


def _build_triangles(s, host):
    m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
    for k, (name, two_sided, N, rev, swap, _, _) in enumerate(TRIANGLES):
        lid = s.add_light_diffuse_area((8.0, 7.0, 6.0), 1, two_sided=two_sided)
        assert lid == k
        s.add_mesh(tri_points(k), np.array([0, 1, 2], np.uint32), m, N=None if N is None else np.array(N, F), first_area_light=lid, reverse_orientation=rev, swaps_handedness=swap)


TRI_U = np.array([[0, 0], [0, ONE_MINUS_EPS], [ONE_MINUS_EPS, 0], [ONE_MINUS_EPS, ONE_MINUS_EPS], [ONE_MINUS_EPS, 0.5], [0.3, ONE_MINUS_EPS], [0, 0.7], [0.25, 0.5], [1e-45, 1e-45], [1e-12, 0.5],
                  [0.5, 0.5], [0.81, 0.13]], F)


def _cases_triangles(orc, host, rng):
    out = []
    for k, (name, two_sided, N, rev, swap, scale, tri) in enumerate(TRIANGLES):
        P = tri_points(k).astype(np.float64)
        c = P.mean(axis=0); size = float(np.linalg.norm(P[1] - P[0]))
        nrm = np.cross(P[1] - P[0], P[2] - P[0]); ln = np.linalg.norm(nrm)
        nrm = nrm / ln if ln > 0 else np.array([0.0, 0.0, 1.0])
        below, above = c - nrm * 1.5 * size + (P[1] - P[0]) * 0.2, c + nrm * 1.5 * size + (P[2] - P[0]) * 0.1
        us = np.concatenate([TRI_U, rng.random((12, 2)).astype(F)])
        # in the triangle's plane, outside it, and one float32 off the plane on either side (the base triangles lie in z = 2)
        inplane = c + (P[1] - P[0]) * 2.0 + (P[2] - P[0]) * 1.5
        offs = np.array([inplane, inplane, inplane], F)
        axis = int(np.argmax(np.abs(nrm)))
        offs[1, axis] = up(offs[1, axis]); offs[2, axis] = dn(offs[2, axis])
        refs = np.concatenate([ref_edges(below.astype(F), c), mk_ref([below, above, c]), mk_ref(offs, p_error=(0, 0, 0), n=(0, 0, 0)), mk_ref(offs),
                               mk_ref(c * 1e19 + 1e19), mk_ref([below], p_error=np.array([3, 3, 3], F) * F(size), n=nrm.astype(F)),
                               random_refs(rng, c, 2.0 * size, 40, target=c)])
        sb = sample_batch(k, refs, us, f"{name}: corners, plane, both sides")
        out.append(sb)
        # the reference point exactly on the sampled point: the oracle's own vp for each u, fed back as p with the same u
        on = orc.light_probe_batch(k, 0, np.tile(mk_ref([below]), (len(us), 1)), us)
        ok = on[:, VALID] == 1
        if ok.any():
            out.append(batch(k, 0, mk_ref(on[ok][:, VP]), u=us[ok], tag=f"{name}: reference point on the sampled point"))
        # pdf_li
        targets = [P[0], P[1], P[2], 0.5 * (P[0] + P[1]), 0.5 * (P[1] + P[2]), 0.5 * (P[2] + P[0]), c]
        for a, b2 in ((0, 1), (1, 2), (2, 0)):   # just outside and just inside each edge
            mid = 0.5 * (P[a] + P[b2]); outward = mid - c
            targets += [mid + outward * 1e-6, mid - outward * 1e-6, mid + outward * 1e-3]
        dirs = []
        for origin in (below, above):
            o32 = origin.astype(F).astype(np.float64)
            for t in targets:
                d = t - o32
                dirs += [(d / np.linalg.norm(d)).astype(F), d.astype(F)]
        e1 = (P[1] - P[0]) / max(np.linalg.norm(P[1] - P[0]), 1e-30)
        dirs += [e1.astype(F), (-e1).astype(F), nrm.astype(F), (-nrm).astype(F), np.zeros(3, F)]
        dirs = np.concatenate([np.array(dirs, F), random_dirs(rng, 10)])
        prefs = np.concatenate([mk_ref([below, above]), mk_ref([below], p_error=(0, 0, 0), n=(0, 0, 0)), mk_ref([below], p_error=np.array([3, 3, 3], F) * F(size), n=nrm.astype(F)),
                                mk_ref([below], p_error=np.array([3, 3, 3], F) * F(size), n=(-nrm).astype(F)), mk_ref(offs[:1]), mk_ref([c])])
        out += dir_batches(k, prefs, dirs, f"{name}: vertices, edges, plane, back")
    return out


# ---------------------------------------------------------------- sphere lights (the Whitted light loop) ----------------------------------------------------------------
# name, centre, radius, zmin, zmax, phimax, reverse_orientation, two_sided, scale
SPHERES = [
    ("full", (0.0, 0.0, 3.0), 1.0, None, None, 360.0, False, False, None),
    ("reversed", (4.0, 0.0, 3.0), 0.75, None, None, 360.0, True, False, None),
    ("partial", (8.0, 0.0, 3.0), 1.0, -0.3, 0.7, 200.0, False, False, None),
    ("scaled", (12.0, 0.0, 3.0), 1.0, None, None, 360.0, False, False, (1.0, 2.0, 0.5)),
    ("two_sided", (16.0, 0.0, 3.0), 0.5, None, None, 360.0, False, True, None),
]


def _sphere_transform(host, centre, scale):
    t = host.translate(centre)
    return host.compose(t, host.scale(scale)) if scale is not None else t


def _build_spheres(s, host):
    m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
    for name, centre, radius, zmin, zmax, phimax, rev, two_sided, scale in SPHERES:
        SL.add_sphere_light(s, _sphere_transform(host, centre, scale), radius, zmin, zmax, phimax, m, rev, L=(8.0, 7.0, 6.0), two_sided=two_sided)


SPHERE_U = np.array([[0, 0], [0, 0.5], [ONE_MINUS_EPS, 0.5], [ONE_MINUS_EPS, ONE_MINUS_EPS], [0, ONE_MINUS_EPS], [0.5, 0], [0.5, 0.25], [0.25, 0.75], [1e-45, 0.1], [0.999, 0.3]], F)


def _cases_spheres(orc, host, rng):
    out = []
    for k, (name, centre, radius, zmin, zmax, phimax, rev, two_sided, scale) in enumerate(SPHERES):
        c = np.array(centre, np.float64); r = float(radius)
        us = np.concatenate([SPHERE_U, rng.random((10, 2)).astype(F)])
        pts = [c, c + [0.3 * r, -0.2 * r, 0.1 * r], c + [0, 0, 0.999 * r], c - [0, 0, 5 * r], c + [2 * r, 1 * r, -3 * r], c * 1e18 + 1e18, c + [1e-20, 0, 0]]
        # distance^2 (p_origin, centre) below, equal to and above radius^2 through p: on the axis below the centre, a few float32 either side of the surface
        for ax in (0, 2):
            base = np.array(centre, F)
            for v in ulps(float(F(centre[ax]) - F(radius)), range(-4, 5)):
                q = base.copy(); q[ax] = v; pts.append(q)
        # sin_theta_max2 = (radius / dc)^2 either side of the Taylor switch
        dc = r / math.sqrt(float(TAYLOR))
        for v in ulps(float(F(centre[2] - dc)), range(-6, 7)):
            pts.append([centre[0], centre[1], v])
        pts += [c - [0, 0, 0.5 * dc], c - [0, 0, 2 * dc], c - [0.6 * dc, 0, 0.8 * dc]]
        refs = [ref_edges((c - [0.5, 0.3, 2.5 * r]).astype(F), c), mk_ref(np.array(pts, F)), mk_ref(np.array(pts, F), p_error=(0, 0, 0), n=(0, 0, 0))]
        # ... and through p_error and n: a point just outside whose offset origin falls inside.  offset_origin turns the offset into the hemisphere of (centre - p) whatever the sign
        # of n, so both signs carry a point outside inwards, and a point inside only moves further in (until a p_error of more than a diameter takes it out on the far side: the case after these)
        for d, sgn in ((1.001, 1.0), (0.999, -1.0), (1.05, 1.0), (0.95, -1.0)):
            p = c - np.array([0, 0, d * r])
            for pe in (1e-3 * r, 2e-2 * r, 0.2 * r):
                refs.append(mk_ref([p], p_error=(pe, pe, pe), n=(0, 0, sgn)))
                refs.append(mk_ref([p], p_error=(pe, pe, pe), n=(0, 0, -sgn)))
        for sgn in (1.0, -1.0):   # inside, with a p_error of three radii: the offset origin overshoots the far side and the cone branch runs with sin_theta_max = 2
            refs.append(mk_ref([c - np.array([0, 0, 0.5 * r])], p_error=(0, 0, 3 * r), n=(0, 0, sgn)))
        refs.append(random_refs(rng, c, 3.0 * r, 60, target=c))
        refs.append(random_refs(rng, c, 0.4 * r, 20))
        out.append(sample_batch(k, np.concatenate(refs), us, f"{name}: inside, outside, surface, Taylor switch"))
    return out


LIGHT_SETS = [
    LightSet("infinite_constant", _build_infinite_const, _cases_infinite_const),
    LightSet("infinite_map", _build_infinite_map, _cases_infinite_map, mapped=range(len(_map_images()))),
    LightSet("spot", _build_spot, _cases_spot),
    LightSet("projection", _build_projection, _cases_projection, mapped=[i for i, p in enumerate(PROJECTIONS) if p[1] is not None]),
    LightSet("goniometric", _build_gonio, _cases_gonio, mapped=[1, 3]),
    LightSet("point_distant", _build_point_distant, _cases_point_distant),
    LightSet("triangle", _build_triangles, _cases_triangles),
    LightSet("sphere", _build_spheres, _cases_spheres, variant=2),
]
LIGHT_SET_BY_NAME = {s.name: s for s in LIGHT_SETS}
