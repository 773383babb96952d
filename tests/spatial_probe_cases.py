"""Case sets for the spatial light distribution's probe (spatial_probe_begin / _batch / _voxel against oracle_spatial_lookup_batch / oracle_spatial_voxel), shared by the CPU
test that measures what the sets reach on the oracle and the GPU test that compares the device with the oracle bit for bit.

A set is a list of cases; a case is one small scene (a box mesh that fixes the world bound, the lights, accelerator built) with its probe points p (n, 3) and samples u (n,):
deterministic edges first, seeded random ones after.  Everything is float32 from the start, so that both sides receive the same bits.  Where an edge depends on what the
distribution holds (the float at which lookup's voxel index changes, the entries of a voxel's CDF) it is taken from the oracle's own answers, never from the device.
A set also names the branch flags it must reach; `flags_of` computes them from the inputs and the oracle's answers."""
import numpy as np

import light_probe_cases as LP
import pbrt_hip
import quadric_light_restatement as QR
import quadric_light_scenes as QL
import sphere_light_scenes as SL
from probe_cases import F, ONE_MINUS_EPS, hexf

# ---- branch flags ------------------------------------------------------------------------------------------------------------------------------------------------------
ON_LO_FACE, ON_HI_FACE, BELOW_LO, ABOVE_HI, NAN_COORD, INF_COORD, NEG_ZERO, FLAT_AXIS, BOUNDARY_CROSSED, ALL_BOUNDARIES = (1 << k for k in range(10))
U_ZERO, U_ON_CDF, U_TOP, U_CLAMPED, FLAT_RUN, ONE_LIGHT = (1 << k for k in range(10, 16))
FLOOR_AVG, FLOOR_ONE, SECOND_CHUNK, SECOND_STRIDE = (1 << k for k in range(16, 20))
Q_OUTSIDE, Q_STRADDLES, Q_CONTAINS, Q_INSIDE = (1 << k for k in range(20, 24))   # a voxel against a disk or cylinder light: apart from it, crossed by its surface, holding all of it, inside the cylinder's wall
FLAG_NAMES = {ON_LO_FACE: "on_lo_face", ON_HI_FACE: "on_hi_face", BELOW_LO: "below_lo", ABOVE_HI: "above_hi", NAN_COORD: "nan_coord", INF_COORD: "inf_coord", NEG_ZERO: "neg_zero",
              FLAT_AXIS: "flat_axis", BOUNDARY_CROSSED: "boundary_crossed", ALL_BOUNDARIES: "all_boundaries", U_ZERO: "u_zero", U_ON_CDF: "u_on_cdf", U_TOP: "u_top",
              U_CLAMPED: "u_clamped", FLAT_RUN: "flat_run", ONE_LIGHT: "one_light", FLOOR_AVG: "floor_avg", FLOOR_ONE: "floor_one", SECOND_CHUNK: "second_chunk",
              SECOND_STRIDE: "second_stride", Q_OUTSIDE: "quadric_outside", Q_STRADDLES: "quadric_straddles", Q_CONTAINS: "quadric_contains", Q_INSIDE: "quadric_inside"}


def flag_names(mask):
    return [n for f, n in FLAG_NAMES.items() if mask & f]


def step(x, k):
    """float32 x moved by k representable steps (through zero if need be)"""
    x = F(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def box_mesh(s, lo, hi, material):
    """12 triangles spanning [lo, hi]; an axis with lo == hi gives a flat box (its side triangles are degenerate and lie in the same plane)."""
    lo = np.asarray(lo, F); hi = np.asarray(hi, F)
    P = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], F)
    idx = np.array([0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3], np.uint32)
    s.add_mesh(P, idx, material)


class Case:
    """name; lo, hi: the box that the scene's meshes span together (the world bound, checked against the oracle's resolution); lights(s, host, material) adds the lights
    and any emitter meshes, returning the number of lights; points(case, orc, rng) -> (p, u); strategy: 2, or 0 / 1 for the scene-wide tables; sphere: the scene holds
    quadric lights (set_path_sphere_lights on the product); voxels: points whose voxel's whole distribution is read back."""

    def __init__(self, name, lo, hi, lights, points, strategy=2, sphere=False, voxels=()):
        self.name, self.lo, self.hi, self._lights, self._points, self.strategy, self.sphere = name, np.asarray(lo, F), np.asarray(hi, F), lights, points, strategy, sphere
        self.voxels = np.asarray(voxels, F).reshape(-1, 3)
        self.n_lights = None

    def capture(self, s, host):
        def go(s, host):
            m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
            self.n_lights = self._lights(s, host, m)
            box_mesh(s, self.lo, self.hi, m)
            s.build_accel(0, 4)
        SL.capture(go, s, host)
        if self.sphere and s.b.prefix != "oracle_":
            s.set_path_sphere_lights(True)

    def points(self, orc, seed=0):
        p, u = self._points(self, orc, np.random.default_rng(9000 + seed))
        p = np.ascontiguousarray(p, F).reshape(-1, 3); u = np.ascontiguousarray(u, F).reshape(-1)
        assert len(p) == len(u) > 0, self.name
        return p, u


def describe(set_name, case, p, u, i):
    return f"set {set_name} case {case.name} (strategy {case.strategy}) point {i}: p {hexf(p[i])} u {hexf(u[i:i + 1])}"


def two_points(s, host, m):
    s.add_light_point((5.0, 4.0, 3.0), (0.3, 0.2, 9.0))
    s.add_light_point((1.0, 2.0, 3.0), (-4.0, 6.0, -5.0))
    return 2


# ---- look-up points ----------------------------------------------------------------------------------------------------------------------------------------------------
def mid_point(case):
    return ((case.lo.astype(np.float64) + case.hi.astype(np.float64)) * 0.5 + (case.hi - case.lo) * 0.013).astype(F)


def face_points(case):
    """every corner and face centre of the bound; +-1, +-2, +-8 steps around each face; +-1e30, +-inf, NaN and -0.0 in each coordinate"""
    lo, hi = case.lo, case.hi
    mid = mid_point(case)
    pts = [[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    for a in range(3):
        for face in (lo[a], hi[a]):
            for k in (0, 1, -1, 2, -2, 8, -8):
                q = mid.copy(); q[a] = step(face, k); pts.append(q)
        for v in (1e30, -1e30, np.inf, -np.inf, np.nan, -0.0, 0.0):
            q = mid.copy(); q[a] = F(v); pts.append(q)
    pts.append([np.nan, np.nan, np.nan]); pts.append([np.inf, -np.inf, np.nan])
    return np.array(pts, F)


def boundary_points(case, orc, nv, every=1):
    """Every interior voxel boundary k / nv of each axis (every `every`-th of them), found on the oracle: the two neighbouring float32 values between which lookup's index goes
    k - 1 -> k (the other coordinates mid-box; the index is monotonic in the coordinate, so the pair is bisected from a bracket of 64 steps of the bound's magnitude around the
    float64 position), with the two floats below the pair and the two above it: six points per boundary."""
    lo, hi = case.lo.astype(np.float64), case.hi.astype(np.float64)
    mid = mid_point(case)
    axis, ks, below, above = [], [], [], []
    for a in range(3):
        w = 64.0 * float(np.spacing(F(max(abs(lo[a]), abs(hi[a])))))
        for k in range(1, nv[a], every):
            x0 = lo[a] + (hi[a] - lo[a]) * k / nv[a]
            axis.append(a); ks.append(k); below.append(F(x0 - w)); above.append(F(x0 + w))
    if not axis:
        return np.zeros((0, 3), F)
    axis, ks, below, above = np.array(axis), np.array(ks), np.array(below, F), np.array(above, F)

    def index_at(x):
        q = np.tile(mid, (len(x), 1)); q[np.arange(len(x)), axis] = x
        return orc.spatial_lookup_batch(q, np.full(len(x), 0.5, F))[0][np.arange(len(x)), axis]
    assert (index_at(below) == ks - 1).all() and (index_at(above) == ks).all(), "the bracket holds the boundary"
    while True:
        m = ((below.astype(np.float64) + above.astype(np.float64)) * 0.5).astype(F)
        open_ = (m > below) & (m < above)
        if not open_.any():
            break
        up = index_at(m) >= ks
        above = np.where(open_ & up, m, above); below = np.where(open_ & ~up, m, below)
    assert (np.nextafter(below, F(np.inf)) == above).all()
    pts = []
    for a, b, c in zip(axis, below, above):
        for x in (step(b, -2), step(b, -1), b, c, step(c, 1), step(c, 2)):
            q = mid.copy(); q[a] = x; pts.append(q)
    return np.array(pts, F)


def lookup_points(case, orc, rng):
    nv = orc.spatial_lookup_batch(mid_point(case).reshape(1, 3), [0.5])[3]
    bp = boundary_points(case, orc, nv)
    ext = (case.hi - case.lo).astype(np.float64)
    rnd = (case.lo + (rng.random((400, 3)) * 1.2 - 0.1) * ext).astype(F)   # a tenth of them outside the bound
    p = np.concatenate([face_points(case), bp, rnd])
    return p, np.full(len(p), 0.5, F)


GRID_LO, GRID_HI = (-1.3, 0.7, 2.1), (2.9, 1.75, 3.1)
FLAT_LO, FLAT_HI = (0.25, -1.5, 0.5), (2.25, -0.5, 0.5)           # zero extent in z
FAR_LO, FAR_HI = (1000.0, 1000.0, 1000.0), (1001.0, 1001.0, 1001.0)   # p - lo loses 10 bits


def far_points(case, orc, rng):
    """the off-origin cube has 3 * 63 boundaries: every seventh of them, all the faces"""
    nv = orc.spatial_lookup_batch(mid_point(case).reshape(1, 3), [0.5])[3]
    bp = boundary_points(case, orc, nv, every=7)
    p = np.concatenate([face_points(case), bp, (case.lo + rng.random((200, 3)) * (case.hi - case.lo)).astype(F)])
    return p, np.full(len(p), 0.5, F)


# ---- resolution ----------------------------------------------------------------------------------------------------------------------------------------------------------
RESOLUTION_EXTENTS = [(64.0, 2.5, 4.5), (64.0, 0.5, 1.5), (1.0, 1.0, 1.0), (4.0, 2.0, 0.01)]


def resolution_rule(extent):
    """SpatialLightDistribution::new's voxel counts in float32 NumPy: round-half-away of diag / max * 64, at least 1 -> (nv, the three ratios before rounding)"""
    d = np.asarray(extent, F)
    r = d / d.max() * F(64.0)
    assert r.dtype == F
    nv = np.maximum(np.floor(np.abs(r) + F(0.5)), 1).astype(np.int64)   # r >= 0: floor(r + 0.5) is round-half-away wherever r + 0.5 is exact, as it is for r < 2^22
    return tuple(int(v) for v in nv), r


def few_points(case, orc, rng):
    p = np.concatenate([case.lo.reshape(1, 3), case.hi.reshape(1, 3), (case.lo + rng.random((30, 3)) * (case.hi - case.lo)).astype(F)])
    return p, rng.random(len(p)).astype(F)


# ---- many voxels -----------------------------------------------------------------------------------------------------------------------------------------------------------
MANY_LATTICE = 15   # 15^3 = 3375 voxels of the 64^3 grid in the first pass: more than three rounds of the distribution pass's 1024 blocks


def three_points(s, host, m):
    s.add_light_point((5.0, 4.0, 3.0), (0.3, 0.2, 3.0))
    s.add_light_point((1.0, 2.0, 3.0), (-2.0, 0.6, -1.5))
    s.add_light_distant((0.5, 0.25, 1.0), (0.0, 0.0, 1.0))
    return 3


def voxel_centre(idx, nv=64):
    return ((np.asarray(idx, np.float64) + 0.5) / nv).astype(F)


def many_voxel_batches(seed=0):
    """Three batches in the unit cube: the centres of MANY_LATTICE^3 distinct voxels; the same with one point in a new voxel; 5000 points inside one further voxel."""
    k = np.arange(MANY_LATTICE) * 4 + 1
    first = voxel_centre(np.array([[x, y, z] for x in k for y in k for z in k]))
    second = np.concatenate([first, voxel_centre([[62, 3, 7]])])
    rng = np.random.default_rng(9100 + seed)
    third = ((np.array([40, 41, 42]) + 0.05 + 0.9 * rng.random((5000, 3))) / 64.0).astype(F)
    return [first, second, third]


# ---- light counts ------------------------------------------------------------------------------------------------------------------------------------------------------------
LIGHT_COUNTS = [2, 255, 256, 257, 2047, 2048, 2049]
COUNT_LO, COUNT_HI = (0.0, 0.0, 0.0), (4.0, 2.0, 1.0)
COUNT_VOXELS = np.array([[0.1, 0.1, 0.1], [3.9, 1.9, 0.9], [2.03, 1.01, 0.51], [1.3, 0.4, 0.77]], F)


def count_light_arrays(n):
    """(positions (n, 3), intensities (n, 3)) of count_lights(n): above the box, no two alike; the middle one has zero intensity"""
    rng = np.random.default_rng(9200 + n)
    pos = np.stack([rng.random(n) * 6.0 - 1.0, rng.random(n) * 4.0 - 1.0, 1.5 + rng.random(n) * 2.0], axis=1).astype(F)
    inten = (0.2 + rng.random((n, 3)) * 5.0).astype(F)
    inten[n // 2] = 0
    return pos, inten


def count_lights(n):
    def build(s, host, m):
        pos, inten = count_light_arrays(n)
        for k in range(n):
            s.add_light_point(inten[k], pos[k])
        return n
    return build


def pick_samples(cdf, rng, n_random=200, most=64):
    """0; up to `most` interior entries of the CDF with the float32 either side of each; 1 - 2^-24; what a sampler never gives but the function must survive (1, 1.5, -1, NaN);
    seeded random values"""
    inner = np.unique(cdf[1:-1])
    if len(inner) > most:
        inner = inner[np.linspace(0, len(inner) - 1, most).astype(np.int64)]
    edge = np.concatenate([inner, np.nextafter(inner, F(-1)), np.nextafter(inner, F(2))]) if len(inner) else np.zeros(0, F)
    return np.concatenate([np.array([0.0, -0.0], F), edge.astype(F), np.array([ONE_MINUS_EPS, 1.0, 1.5, -1.0, np.nan], F), rng.random(n_random).astype(F)])


def voxel_pick_points(case, orc, rng):
    """per voxel of the case: the pick samples made from the oracle's CDF of that voxel"""
    pi, _, _, _ = orc.spatial_lookup_batch(case.voxels, np.full(len(case.voxels), 0.5, F))
    ps, us = [], []
    for v, q in zip(case.voxels, pi):
        _, cdf, _ = orc.spatial_voxel(q, case.n_lights)
        u = pick_samples(cdf, rng)
        ps.append(np.tile(v, (len(u), 1))); us.append(u)
    return np.concatenate(ps), np.concatenate(us)


# ---- kinds ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
KIND_LO, KIND_HI = (-2.0, -2.0, 2.5), (2.0, 2.0, 6.5)


def _lp(build, n):
    def lights(s, host, m):
        build(s, host)
        return n
    return lights


def distant_infinite(s, host, m):
    s.add_light_distant((1.0, 2.0, 3.0), LP.DISTANT_W)
    s.add_light_infinite((0.4, 0.8, 1.3))
    s.add_light_point((5.0, 4.0, 3.0), (0.5, 1.0, 1.0))
    return 3


# a one-sided emitter facing the box from below (+z), one facing away (-z), a two-sided one, and one in the middle of the box: its voxel contains it
EMITTERS = [("towards", False, False, (0.0, 0.0, 2.0)), ("away", False, True, (1.0, 0.5, 2.0)), ("two_sided", True, True, (-1.0, -0.5, 2.0)), ("inside", False, False, (0.3, 0.2, 4.03))]


def emitters(s, host, m):
    for k, (name, two_sided, flip, at) in enumerate(EMITTERS):
        lid = s.add_light_diffuse_area((8.0, 7.0, 6.0), 1, two_sided=two_sided)
        assert lid == k
        tri = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]], np.float64) + np.array(at)
        s.add_mesh(tri.astype(F), np.array([0, 2, 1] if flip else [0, 1, 2], np.uint32), m, first_area_light=lid)
    return len(EMITTERS)


def facing_away(s, host, m):
    """two one-sided emitters under the box whose normals point down: no light reaches any voxel"""
    for k, at in enumerate(((0.0, 0.0, 1.0), (1.0, -1.0, 0.5))):
        lid = s.add_light_diffuse_area((4.0, 4.0, 4.0), 1, two_sided=False)
        tri = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0]], np.float64) + np.array(at)   # normal -z
        s.add_mesh(tri.astype(F), np.array([0, 1, 2], np.uint32), m, first_area_light=lid)
    return 2


def quadric_lights(s, host, m):
    """A sphere light in the box (voxels outside, straddling and inside it), a small reversed two-sided one, a cut one.  The oracle has spherical area lights only: disk and
    cylinder lights run the same instantiation of the distribution pass (wh_light_sample_li) but have no oracle to be compared with here."""
    SL.add_sphere_light(s, host.translate((0.0, 0.0, 4.5)), 1.0, None, None, 360.0, m, False, L=(8.0, 7.0, 6.0), two_sided=False)
    SL.add_sphere_light(s, host.translate((1.2, 1.2, 5.8)), 0.4, None, None, 360.0, m, True, L=(3.0, 2.0, 1.0), two_sided=True)
    SL.add_sphere_light(s, host.translate((-1.2, 0.8, 3.4)), 0.5, -0.2, 0.4, 250.0, m, False, L=(6.0, 5.0, 4.0), two_sided=False)
    s.add_light_point((1.0, 2.0, 3.0), (1.0, -1.2, 1.0))
    return 4


SPOT_VOXELS = [[0.03, 0.02, 6.0], [3.0 * 0.52, 0.02, 3.0], [1.9, 1.9, 2.6], [0.5, 1.0, 3.2]]   # inside the cones about +z; across their falloff (25..30 degrees); outside every cone about +z; near the rotated cones
KINDS = [
    Case("spot", KIND_LO, KIND_HI, _lp(LP._build_spot, 8), voxel_pick_points, voxels=SPOT_VOXELS),
    Case("projection", KIND_LO, KIND_HI, _lp(LP._build_projection, len(LP.PROJECTIONS)), voxel_pick_points, voxels=[[0.03, 0.02, 5.0], [1.5, -1.2, 2.7], [-1.9, 1.9, 6.4]]),
    Case("goniometric", KIND_LO, KIND_HI, _lp(LP._build_gonio, 4), voxel_pick_points, voxels=[[0.03, 0.02, 5.0], [0.6, 1.1, 2.6], [-1.9, 1.9, 6.4]]),
    Case("distant_infinite", KIND_LO, KIND_HI, distant_infinite, voxel_pick_points, voxels=[[0.03, 0.02, 5.0], [0.5, 1.0, 2.55]]),
    Case("infinite_map", KIND_LO, KIND_HI, _lp(LP._build_infinite_map, len(LP._map_images())), voxel_pick_points, voxels=[[0.03, 0.02, 5.0], [-1.9, 1.9, 6.4]]),
    Case("triangles", KIND_LO, KIND_HI, emitters, voxel_pick_points, voxels=[[0.1, 0.1, 3.0], [0.4, 0.3, 4.03], [-1.9, 1.9, 6.4], [1.1, 0.6, 2.6]]),
    Case("quadrics", KIND_LO, KIND_HI, quadric_lights, voxel_pick_points, sphere=True,
         voxels=[[0.02, 0.03, 4.5], [0.02, 0.03, 3.5], [0.02, 0.03, 2.6], [0.7, 0.7, 5.2], [1.2, 1.2, 5.8], [-1.2, 0.8, 3.4], [-1.2, 0.8, 3.95]]),
    Case("facing_away", KIND_LO, KIND_HI, facing_away, voxel_pick_points, voxels=[[0.03, 0.02, 5.0], [1.5, -0.5, 2.6]]),
]


# ---- the power and uniform tables ----------------------------------------------------------------------------------------------------------------------------------------------
def zero_power_between(s, host, m):
    s.add_light_point((1.0, 1.0, 1.0), (0.0, 0.0, 9.0))
    s.add_light_point((0.0, 0.0, 0.0), (1.0, 0.0, 9.0))
    s.add_light_point((0.0, 0.0, 0.0), (1.0, 1.0, 9.0))
    s.add_light_point((2.0, 2.0, 2.0), (2.0, 0.0, 9.0))
    s.add_light_spot((3.0, 2.0, 1.0), pbrt_hip.IDENTITY, pbrt_hip.IDENTITY, LP.SPOT_TOTAL, LP.SPOT_START)
    return 5


def one_light(s, host, m):
    s.add_light_point((1.0, 1.0, 1.0), (0.0, 0.0, 9.0))
    return 1


def table_points(case, orc, rng):
    """the scene-wide table's CDF is not read back: its entries are found as the samples at which the oracle's pick changes, by bisection between k / 4096 neighbours"""
    grid = (np.arange(4097) / 4096.0).astype(F); grid[-1] = ONE_MINUS_EPS
    z = np.zeros((len(grid), 3), F)
    _, light, _, _ = orc.spatial_lookup_batch(z, grid, case.strategy)
    edges = []
    for i in np.flatnonzero(light[1:] != light[:-1]):
        a, b = grid[i], grid[i + 1]
        while np.nextafter(a, F(2)) < b:
            mid = F((np.float64(a) + np.float64(b)) * 0.5)
            lm = orc.spatial_lookup_batch(z[:1], [mid], case.strategy)[1][0]
            if lm == light[i]: a = mid
            else: b = mid
        edges += [a, b, np.nextafter(b, F(2)), np.nextafter(a, F(-1))]   # b: the first sample of the next interval = a CDF entry
    u = np.concatenate([np.array([0.0, -0.0, ONE_MINUS_EPS, 1.0, 1.5, -1.0, np.nan], F), np.array(edges, F), rng.random(200).astype(F)])
    case.table_edges = np.array(edges[1::4], F)
    return np.zeros((len(u), 3), F) + mid_point(case), u


SETS = {
    "grid": [Case("awkward_bounds", GRID_LO, GRID_HI, two_points, lookup_points)],
    "flat": [Case("flat_z", FLAT_LO, FLAT_HI, two_points, lookup_points), Case("far_from_origin", FAR_LO, FAR_HI, two_points, far_points)],
    "resolution": [Case("extent_%g_%g_%g" % e, (0.0, 0.0, 0.0), e, two_points, few_points) for e in RESOLUTION_EXTENTS],
    "many_voxels": [Case("unit_cube", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), three_points, lambda c, o, r: (many_voxel_batches()[0], np.full(MANY_LATTICE ** 3, 0.5, F)))],
    "light_counts": [Case("lights_%d" % n, COUNT_LO, COUNT_HI, count_lights(n), voxel_pick_points, voxels=COUNT_VOXELS) for n in LIGHT_COUNTS],
    "kinds": KINDS,
    "pick": [Case("power_zero_between", COUNT_LO, COUNT_HI, zero_power_between, table_points, strategy=1),
             Case("uniform_five", COUNT_LO, COUNT_HI, zero_power_between, table_points, strategy=0),
             Case("single_light", COUNT_LO, COUNT_HI, one_light, table_points, strategy=0)],
}
# what each set must reach (flags_of); "pick" counts the samples of light_counts and kinds too, whose cases carry pick_samples on every voxel
MUST_REACH = {
    "grid": ON_LO_FACE | ON_HI_FACE | BELOW_LO | ABOVE_HI | NAN_COORD | INF_COORD | NEG_ZERO | BOUNDARY_CROSSED | ALL_BOUNDARIES,
    "flat": ON_LO_FACE | ON_HI_FACE | BELOW_LO | ABOVE_HI | NAN_COORD | INF_COORD | NEG_ZERO | FLAT_AXIS | BOUNDARY_CROSSED,
    "resolution": 0,
    "many_voxels": SECOND_STRIDE,
    "light_counts": U_ZERO | U_ON_CDF | U_TOP | U_CLAMPED | FLOOR_AVG | SECOND_CHUNK,
    "kinds": U_ZERO | U_ON_CDF | U_TOP | U_CLAMPED | FLOOR_AVG | FLOOR_ONE | Q_OUTSIDE | Q_STRADDLES | Q_CONTAINS | Q_INSIDE,   # the Q flags: DISK_CYLINDER below
    "pick": U_ZERO | U_ON_CDF | U_TOP | U_CLAMPED | FLAT_RUN | ONE_LIGHT,
}


def boundaries_crossed(case, p, pi, nv):
    """per axis, the k whose boundary k / nv the points cross between two neighbouring float32 values (the other two coordinates mid-box): the oracle's index goes k - 1 -> k"""
    mid = mid_point(case); found = {}
    for a in range(3):
        o = [b for b in range(3) if b != a]
        sel = (p[:, o[0]] == mid[o[0]]) & (p[:, o[1]] == mid[o[1]]) & np.isfinite(p[:, a])
        x = p[sel, a]; v = pi[sel, a]
        order = np.argsort(x, kind="stable"); x = x[order]; v = v[order]
        found[a] = {int(v[i + 1]) for i in np.flatnonzero(v[1:] != v[:-1]) if np.nextafter(x[i], F(np.inf)) == x[i + 1] and v[i + 1] == v[i] + 1}
    return found


def flags_of(case, p, u, pi, light, nv, voxel_tables=None):
    """The branch flags one case reaches, from its inputs (p, u), the oracle's voxels and picks (pi, light, nv) and, for cases with voxels, the oracle's tables
    {voxel: (func, cdf, func_int)}."""
    m = 0
    if case.strategy != 2:
        ok = (u >= 0) & (u < 1)
        order = np.argsort(u[ok], kind="stable")
        if np.any(np.diff(light[ok][order].astype(np.int64)) > 1): m |= FLAT_RUN          # the pick steps over a light: a run of equal CDF entries
        if len(getattr(case, "table_edges", ())) and np.isin(case.table_edges, u).all(): m |= U_ON_CDF
    if case.strategy == 2:
        crossed = boundaries_crossed(case, p, pi, nv)
        if any(crossed.values()): m |= BOUNDARY_CROSSED
        if all(crossed[a] == set(range(1, nv[a])) for a in range(3)) and max(nv) > 1: m |= ALL_BOUNDARIES
        lo, hi = case.lo, case.hi
        for a in range(3):
            x = p[:, a]
            flat = not hi[a] > lo[a]
            if flat: m |= FLAT_AXIS
            if np.any((x == lo[a]) & (pi[:, a] == 0)): m |= ON_LO_FACE
            if np.any((x == hi[a]) & (pi[:, a] == nv[a] - 1)): m |= ON_HI_FACE     # offset 1 -> index nv, clamped (flat: offset p - lo = 0)
            if np.any((x < lo[a]) & (pi[:, a] == 0)): m |= BELOW_LO
            if np.any((x > hi[a]) & (pi[:, a] == nv[a] - 1)): m |= ABOVE_HI
            if np.any(np.isnan(x) & (pi[:, a] == 0)): m |= NAN_COORD
            if np.any(np.isinf(x)): m |= INF_COORD
            if np.any((x == 0) & np.signbit(x)): m |= NEG_ZERO
        if nv[0] * nv[1] * nv[2] > 1024 and len(np.unique(pi, axis=0)) > 2048: m |= SECOND_STRIDE
    if case.n_lights == 1: m |= ONE_LIGHT
    if np.any((u == 0) & ~np.signbit(u)): m |= U_ZERO
    if np.any(u == ONE_MINUS_EPS): m |= U_TOP
    if np.any(u >= 1): m |= U_CLAMPED
    if case.n_lights > 2048: m |= SECOND_CHUNK
    for func, cdf, func_int in (voxel_tables or {}).values():
        if np.isin(u, cdf[1:-1]).any(): m |= U_ON_CDF
        if func_int == 1 and np.all(func == 1): m |= FLOOR_ONE
        elif np.sum(func == func.min()) >= 1 and func.min() < func.max() and np.isclose(func.min(), 0.001 * _avg_before_floor(func), rtol=1e-3): m |= FLOOR_AVG
    return m


def _avg_before_floor(func):
    """the average contribution per light and sample, from a floored table: the floored entries held 0 before (exact where at least one light is floored)"""
    floor = func.min()
    return func[func > floor].sum(dtype=np.float64) / (128.0 * len(func))


# ---- disk and cylinder lights: part of `kinds`, against a float32 restatement --------------------------------------------------------------------------------------------------
# The oracle has no Disk::sample or Cylinder::sample.  quadric_light_restatement.sample_li is the NumPy restatement of DiffuseAreaLight::sample_li on both shapes that
# test_quadric_lights_gpu.py holds the device to bit for bit; a voxel's func[j] is the sequential float32 sum over the 128 Halton points of y(Li) / pdf of that sample_li, and
# cdf, func_int and the floor follow from Distribution1D (distribution_1d.rs:30-60): restated below in float32, operation by operation, so the comparison is bit for bit too.
# kind, centre (translation only: the classification below is axis-aligned), radius, a, b, reverse_orientation, L, two_sided
_VOX = 4.0 / 64.0
QUADRIC_LIGHTS = [
    (QR.DISK, (0.03, 0.02, 4.02), 0.5, 0.0, 0.0, False, (8.0, 7.0, 6.0), False),                                                              # emits towards +z
    (QR.DISK, (-2.0 + 20.5 * _VOX, -2.0 + 40.5 * _VOX, 2.5 + 50.5 * _VOX), 0.02, 0.0, 0.0, True, (6.0, 5.0, 4.0), True),                     # fits inside voxel (20, 40, 50)
    (QR.CYLINDER, (1.0, -1.0, 5.0), 0.4, -0.3, 0.3, False, (2.0, 3.0, 4.0), False),                                                          # emits outwards
    (QR.CYLINDER, (-2.0 + 44.5 * _VOX, -2.0 + 12.5 * _VOX, 2.5 + 10.5 * _VOX), 0.015, -0.015, 0.015, False, (3.0, 2.0, 1.0), True),          # fits inside voxel (44, 12, 10)
]
# apart from every light; crossed by the large disk; above it (lit) and below it (dark); holding the small disk; crossed by the cylinder's wall; on its axis; holding the small cylinder
QUADRIC_VOXELS = np.array([[-1.9, 1.9, 6.4], [0.2, 0.1, 4.02], [0.2, 0.1, 5.0], [0.2, 0.1, 3.0], QUADRIC_LIGHTS[1][1], [1.4, -1.0, 5.0], [1.0, -1.0, 5.0], QUADRIC_LIGHTS[3][1]], F)


def disk_cylinder_lights(s, host, m):
    for kind, centre, radius, a, b, rev, L, two in QUADRIC_LIGHTS:
        QL.add_light(s, kind, host.translate(centre), radius, a, b, 360.0, m, rev, L=L, two_sided=two)
    return len(QUADRIC_LIGHTS)


def quadric_shapes(host):
    return [(QR.shape(kind, host.translate(centre), radius, a, b, 360.0, rev), L, two) for kind, centre, radius, a, b, rev, L, two in QUADRIC_LIGHTS]


DISK_CYLINDER = Case("disk_cylinder", KIND_LO, KIND_HI, disk_cylinder_lights, None, voxels=QUADRIC_VOXELS)   # the product alone captures it; its points come from restated_points


def halton_128(radical_inverse):
    """the distribution pass's table: radical_inverse(0 .. 4, i) for i < 128 (spatial.rs:113-117); radical_inverse(base_index, i) -> float32"""
    return np.array([[radical_inverse(d, i) for d in range(5)] for i in range(128)], F)


def lerp32(t, a, b):
    return F(F(F(1.0) - t) * a) + F(t * b)


def voxel_of_f32(case, p, nv):
    """lookup's voxel (spatial.rs:170-181) in float32"""
    out = np.zeros((len(p), 3), np.int32)
    for a in range(3):
        o = (p[:, a] - case.lo[a]).astype(F)
        if case.hi[a] > case.lo[a]:
            o = (o / F(case.hi[a] - case.lo[a])).astype(F)
        v = (o * F(nv[a])).astype(F)
        with np.errstate(invalid="ignore"):
            out[:, a] = np.clip(np.where(np.isnan(v), 0, np.trunc(np.clip(v, -2e9, 2e9))), 0, nv[a] - 1).astype(np.int32)
    return out


def voxel_bounds_f32(case, q, nv):
    lo, hi = np.zeros(3, F), np.zeros(3, F)
    for a in range(3):
        p0, p1 = F(F(q[a]) / F(nv[a])), F(F(q[a] + 1) / F(nv[a]))
        x, y = lerp32(p0, case.lo[a], case.hi[a]), lerp32(p1, case.lo[a], case.hi[a])
        lo[a], hi[a] = min(x, y), max(x, y)
    return lo, hi


def distribution_f32(contrib):
    """the floor (spatial.rs:141-150) and Distribution1D::new (distribution_1d.rs:30-60) in float32, sums left to right -> (func, cdf, func_int)"""
    n = len(contrib)
    total = F(0)
    for c in contrib:
        total = F(total + c)
    avg = F(total / F(128 * n))
    floor = F(F(0.001) * avg) if avg > 0 else F(1.0)
    func = np.maximum(contrib, floor).astype(F)
    cdf = np.zeros(n + 1, F)
    for i in range(1, n + 1):
        cdf[i] = F(cdf[i - 1] + F(func[i - 1] / F(n)))
    func_int = cdf[n]
    cdf[1:] = (np.arange(1, n + 1, dtype=F) / F(n)) if func_int == 0 else (cdf[1:] / func_int).astype(F)
    return func, cdf, func_int


def restated_table(case, shapes, q, nv, halton):
    """compute_distribution (spatial.rs:90-160) for voxel q of a scene whose lights are all `shapes`, in float32"""
    lo, hi = voxel_bounds_f32(case, q, nv)
    ref = np.zeros((128, 10), F)
    for a in range(3):
        ref[:, a] = lerp32(halton[:, a], lo[a], hi[a])
    contrib = np.zeros(len(shapes), F)
    for j, (shape, L, two) in enumerate(shapes):
        o = QR.sample_li(shape, L, two, ref, halton[:, 3:5])
        y = (F(0.212671) * o[:, 4] + F(0.715160) * o[:, 5]).astype(F) + (F(0.072169) * o[:, 6]).astype(F)
        acc = F(0)
        for i in np.flatnonzero((o[:, 7] == 1) & (o[:, 3] > 0)):
            acc = F(acc + F(y[i] / o[i, 3]))
        contrib[j] = acc
    return distribution_f32(contrib)


def pick_f32(func, cdf, func_int, u):
    """Distribution1D::sample_discrete (distribution_1d.rs:83-95) in float32: find_interval's answer is the count of entries <= u, less one, clamped to [0, n - 1]"""
    n = len(func)
    with np.errstate(invalid="ignore"):
        count = (cdf[None, :] <= u[:, None]).sum(axis=1)
    k = np.clip(count - 1, 0, n - 1)
    pdf = (func[k] / F(func_int * F(n))).astype(F) if func_int > 0 else np.zeros(len(u), F)
    return k.astype(np.uint32), pdf


def classify_voxel(light, vlo, vhi):
    """Q_* of one voxel against one axis-aligned disk or cylinder light, in float64"""
    kind, c, r, a, b = light[0], np.array(light[1], np.float64), float(light[2]), float(light[3]), float(light[4])
    z0, z1 = (c[2] + a, c[2] + a) if kind == QR.DISK else (c[2] + min(a, b), c[2] + max(a, b))
    blo, bhi = np.array([c[0] - r, c[1] - r, z0]), np.array([c[0] + r, c[1] + r, z1])
    if (vlo <= blo).all() and (bhi <= vhi).all():
        return Q_CONTAINS
    near = np.clip(c[:2], vlo[:2], vhi[:2]); dmin = float(np.linalg.norm(near - c[:2]))
    dmax = float(np.linalg.norm(np.maximum(np.abs(vlo[:2] - c[:2]), np.abs(vhi[:2] - c[:2]))))
    z_overlap = vlo[2] <= z1 and z0 <= vhi[2]
    if kind == QR.DISK:
        return Q_STRADDLES if z_overlap and dmin <= r else Q_OUTSIDE
    if z_overlap and dmin <= r <= dmax:
        return Q_STRADDLES
    return Q_INSIDE if z_overlap and dmax < r and vlo[2] >= z0 and vhi[2] <= z1 else Q_OUTSIDE


def restated_points(case, host, radical_inverse, seed=0):
    """-> (p, u, {voxel: (func, cdf, func_int)}, want pi, want light, want pdf, Q flags reached): everything the device is compared with for DISK_CYLINDER"""
    nv = (64, 64, 64)
    shapes = quadric_shapes(host)
    halton = halton_128(radical_inverse)
    rng = np.random.default_rng(9500 + seed)
    vpi = voxel_of_f32(case, case.voxels, nv)
    tables, ps, us, lights, pdfs, reached = {}, [], [], [], [], 0
    for v, q in zip(case.voxels, vpi):
        key = tuple(int(x) for x in q)
        tables[key] = restated_table(case, shapes, key, nv, halton)
        u = pick_samples(tables[key][1], rng)
        k, pdf = pick_f32(*tables[key], u)
        ps.append(np.tile(v, (len(u), 1))); us.append(u); lights.append(k); pdfs.append(pdf)
        vlo, vhi = voxel_bounds_f32(case, key, nv)
        kinds = [classify_voxel(l, vlo.astype(np.float64), vhi.astype(np.float64)) for l in QUADRIC_LIGHTS]
        reached |= Q_OUTSIDE if all(c == Q_OUTSIDE for c in kinds) else 0
        for c in kinds:
            if c != Q_OUTSIDE: reached |= c
    p, u = np.concatenate(ps).astype(F), np.concatenate(us).astype(F)
    return p, u, tables, voxel_of_f32(case, p, nv), np.concatenate(lights), np.concatenate(pdfs), reached
