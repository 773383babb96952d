"""Scenes, closed forms and probe cases for disk and cylinder DiffuseAreaLights (pbrt_hip_add_quadric_light), shared by tests/test_quadric_lights_cpu.py,
tests/test_quadric_lights_gpu.py and tests/test_front_end_quadric_lights.py.  The oracle restates neither Disk::sample nor Cylinder::sample, so nothing here goes through it: the
yardsticks are tests/quadric_light_restatement.py (proved on the CPU) and float64 radiometry written from the physics with numpy alone."""
import math

import numpy as np

import closed_form as CF
import light_probe_cases as LP
import quadric_light_restatement as QR
import reference_scenes as R
import sphere_light_scenes as SL

F = np.float32
D = np.float64
LE = (10.0, 7.0, 4.0)
RHO = (0.2, 0.5, 0.95)
SE_TARGET = 0.005
KIND_NAME = {QR.CYLINDER: "cylinder", QR.DISK: "disk"}


def add_light(s, kind, t, radius, a, b, phimax=360.0, material=0, reverse=False, L=(1.0, 1.0, 1.0), two_sided=False):
    """t = (object_to_world, world_to_object); a, b = zmin, zmax of a cylinder, height, innerradius of a disk"""
    s.add_quadric_light(KIND_NAME[kind], t[0], t[1], radius, a, b, phimax, material, reverse, L=L, two_sided=two_sided)


# ---- probe lights --------------------------------------------------------------------------------------------------------------------------------------------------------
# name, kind, transform steps (host -> list), radius, a, b, phimax, reverse_orientation, two_sided.  The first three share everything but orientation and sidedness.
_MIRROR = lambda at: (lambda h: [h.translate(at), h.rotate(35.0, (1, 2, 3)), h.scale((-1.3, 0.7, 1.0))])
PROBE_LIGHTS = [
    ("disk_full", QR.DISK, lambda h: [h.translate((0.0, 0.0, 3.0))], 1.0, 0.0, 0.0, 360.0, False, False),
    ("disk_reversed", QR.DISK, lambda h: [h.translate((0.0, 0.0, 3.0))], 1.0, 0.0, 0.0, 360.0, True, False),
    ("disk_two_sided", QR.DISK, lambda h: [h.translate((0.0, 0.0, 3.0))], 1.0, 0.0, 0.0, 360.0, False, True),
    ("disk_annulus_cut", QR.DISK, lambda h: [h.translate((8.0, 0.0, 3.0)), h.rotate(40.0, (0, 1, 0))], 1.5, 0.4, 0.5, 250.0, False, False),
    ("disk_mirrored_scaled", QR.DISK, _MIRROR((12.0, 0.5, 3.0)), 1.4, -0.2, 0.0, 360.0, False, False),
    ("cylinder_full", QR.CYLINDER, lambda h: [h.translate((-4.0, 0.0, 3.0))], 1.0, -1.0, 1.0, 360.0, False, False),
    ("cylinder_reversed_cut", QR.CYLINDER, lambda h: [h.translate((-5.0, 1.0, 4.0)), h.rotate(25.0, (1, 0, 1))], 1.2, -0.5, 1.5, 200.0, True, False),
    ("cylinder_mirrored_scaled", QR.CYLINDER, _MIRROR((-3.0, 0.5, 3.0)), 0.8, -1.0, 0.5, 360.0, False, True),
]
# Where the cylinders stand: Cylinder::intersect rounds the quadratic's coefficients to float32 and carries the hit back to world space, so its pdf loses digits with
# |translation| / distance and with (|origin| / radius)^2 where the disk's plane test loses them with the first alone.  The margin of the cylinder's pdf_li is the disk's figure
# (measured_margin), so the cylinders stand within 5 units of the origin and their probes start within 1.5 radii of the wall (conditioned_probes): there the reference's own
# float32 arithmetic, restated in quadric_light_restatement.cylinder_intersect, stays inside that margin against the float64 hit (tests/test_quadric_lights_cpu.py measures it:
# 6.7e-6, 4.2e-6 and 1.03e-5 against 1.17e-5), and what the margin then measures on the device is the device.
# Cylinders further out, for the bit-for-bit comparison alone (the bits do not depend on the margin): where the first session's layout had them
FAR_CYLINDERS = [
    ("far_cylinder_reversed_cut", QR.CYLINDER, lambda h: [h.translate((-12.0, 1.0, 4.0)), h.rotate(25.0, (1, 0, 1))], 1.2, -0.5, 1.5, 200.0, True, False),
    ("far_cylinder_mirrored_scaled", QR.CYLINDER, _MIRROR((-18.0, 0.5, 3.0)), 0.8, -1.0, 0.5, 360.0, False, True),
]
PROBE_L = (8.0, 7.0, 6.0)
DISKS = [k for k, p in enumerate(PROBE_LIGHTS) if p[1] == QR.DISK]
CYLINDERS = [k for k, p in enumerate(PROBE_LIGHTS) if p[1] == QR.CYLINDER]


def probe_transform(host, k):
    return R.ctm(host, *PROBE_LIGHTS[k][2](host))


def probe_shape(host, k):
    name, kind, steps, radius, a, b, phimax, rev, two = PROBE_LIGHTS[k]
    return QR.shape(kind, probe_transform(host, k), radius, a, b, phimax, rev)


def far_shape(host, k):
    name, kind, steps, radius, a, b, phimax, rev, two = FAR_CYLINDERS[k]
    return QR.shape(kind, R.ctm(host, *steps(host)), radius, a, b, phimax, rev)


def build_far_cylinders(s, host):
    m = LP.add_floor(s)
    for name, kind, steps, radius, a, b, phimax, rev, two in FAR_CYLINDERS:
        add_light(s, kind, R.ctm(host, *steps(host)), radius, a, b, phimax, m, rev, L=PROBE_L, two_sided=two)
    s.build_accel(0, 4)


def build_probe_lights(s, host):
    m = LP.add_floor(s)
    for k, (name, kind, steps, radius, a, b, phimax, rev, two) in enumerate(PROBE_LIGHTS):
        add_light(s, kind, probe_transform(host, k), radius, a, b, phimax, m, rev, L=PROBE_L, two_sided=two)
    s.build_accel(0, 4)


def _unit_rows(v):
    v = np.asarray(v, D)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(q):
    """(world centre of the shape, linear part of object_to_world, object-space centre) in float64"""
    M4 = q["o2w"].astype(D).reshape(4, 4)
    c_obj = np.array([0.0, 0.0, float(q["height"]) if q["kind"] == QR.DISK else 0.5 * (float(q["z_min"]) + float(q["z_max"]))])
    return M4[:3, :3] @ c_obj + M4[:3, 3], M4[:3, :3], c_obj


def to_world(q, p_obj):
    M4 = q["o2w"].astype(D).reshape(4, 4)
    return np.asarray(p_obj, D) @ M4[:3, :3].T + M4[:3, 3]


def sample_cases(host, k, seed=0):
    """-> (ref (n, 10), u (n, 2)) for probe light k, about 200 probes: both sides, in the disk's plane / on the cylinder's axis, beyond 10^3 radii, ON the sampled point
    (the direction has length zero), the reference-point edges every light set gets, a random fill; the sample's own edges (0, 1 - eps, a denormal) in front."""
    q = probe_shape(host, k)
    rng = np.random.default_rng(9300 + seed + (0 if k < 3 else k))
    c, M, c_obj = _frame(q)
    r = float(q["radius"])
    axis = _unit_rows(M @ np.array([0.0, 0.0, 1.0])); ex = _unit_rows(M @ np.array([1.0, 0.0, 0.0]))
    refs = []
    for s in (1.0, -1.0):   # both sides of the disk / both ends of the cylinder, near and off the axis
        for dist in (0.05, 0.5, 2.0, 7.0):
            p = c + s * axis * dist * r
            refs.append(LP.mk_ref([p, p + ex * 0.7 * r, p - ex * 2.5 * r], n=(-s * axis).astype(F)))
            refs.append(LP.mk_ref([p + ex * 0.3 * r], n=(s * axis).astype(F)))
    # in the disk's plane (|n . wi| = 0 or next to it: the pdf is infinite or huge) / on the cylinder's axis and in its end planes
    flat = np.array([[0.0, 0.0, 0.0], [0.4, 0.1, 0.0], [1.0, 0.0, 0.0], [1.7, -0.6, 0.0], [-3.0, 2.0, 0.0], [0.0, 0.0, 0.3], [0.0, 0.0, -0.45]]) * r + c_obj
    if q["kind"] == QR.CYLINDER:
        flat = np.concatenate([flat, np.array([[0.3 * r, 0.2 * r, float(q["z_min"])], [1.5 * r, 0.0, float(q["z_max"])], [0.999 * r, 0.0, c_obj[2]], [1.001 * r, 0.0, c_obj[2]]])])
    refs.append(LP.mk_ref(to_world(q, flat), n=axis.astype(F)))
    refs.append(LP.mk_ref(to_world(q, flat[:4]), p_error=(0, 0, 0), n=(0, 0, 0)))
    # far away: beyond 10^3 radii
    far = _unit_rows(rng.normal(size=(6, 3)))
    refs.append(LP.mk_ref(np.concatenate([c + far[:3] * r * 2.5e3, c + far[3:] * r * 4e5, [c + axis * r * 1e4, c + ex * r * 1e4]])))
    refs.append(LP.ref_edges((c - axis * 2.5 * r + ex * 0.4 * r).astype(F), c))
    refs.append(LP.random_refs(rng, c, 3.0 * r, 110, target=c))
    refs.append(LP.random_refs(rng, c, 0.5 * r, 20))
    ref = np.concatenate(refs).astype(F)
    u = rng.random((len(ref), 2)).astype(F)
    u[:len(LP.SPHERE_U)] = LP.SPHERE_U
    # touching: the reference point IS the point its own u samples (float32 bits of the restatement)
    n_touch = 12
    ut = rng.random((n_touch, 2)).astype(F)
    pt, _, nt = QR.sample(q, ut)
    ref = np.concatenate([ref, LP.mk_ref(pt, n=-nt)]).astype(F); u = np.concatenate([u, ut]).astype(F)
    assert 150 <= len(ref) <= 260, (PROBE_LIGHTS[k][0], len(ref))
    return np.ascontiguousarray(ref), np.ascontiguousarray(u)


def disk_pdf_cases(host, k, seed=0):
    """-> (ref (n, 10), wi (n, 3)) for disk light k: from points on both sides towards the annulus, the inner hole, the phi cut, just inside and outside the rim, past the
    disk, away from it; parallel to the disk's plane (exactly so where the transform is a translation); the reference-point edges; a random fill"""
    q = probe_shape(host, k)
    rng = np.random.default_rng(9400 + seed + (0 if k < 3 else k))
    c, M, c_obj = _frame(q)
    r, ri, pm, h = float(q["radius"]), float(q["inner_radius"]), float(q["phi_max"]), float(q["height"])
    axis = _unit_rows(M @ np.array([0.0, 0.0, 1.0])); ex = _unit_rows(M @ np.array([1.0, 0.0, 0.0]))
    origins = [c + axis * 1.5 * r + ex * 0.3 * r, c - axis * 0.8 * r - ex * 0.6 * r, c + axis * 0.2 * r, c - axis * 6.0 * r + ex * 2.0 * r]
    rho = sorted({0.0, 0.5 * ri, 0.98 * ri, 1.02 * ri if ri > 0 else 0.1 * r, 0.5 * (ri + r), 0.75 * r, 0.999 * r, 1.001 * r, 1.6 * r})
    phis = sorted({0.05 * pm, 0.5 * pm, 0.97 * pm, min(1.03 * pm, 6.2), 0.5 * (pm + 2.0 * math.pi)})
    targets = to_world(q, np.array([[a * math.cos(p), a * math.sin(p), h] for a in rho for p in phis]))
    refs, wis = [], []
    for o in origins:
        d = _unit_rows(targets - o)
        a, b = LP.mk_ref(np.tile(o, (len(d), 1)), n=_unit_rows(c - o).astype(F)), d.astype(F)
        refs += [a, a[:8]]; wis += [b, -b[:8]]
    par = _unit_rows(np.array([M @ v for v in ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, 0.8, 0.0], [-0.28, 0.96, 0.0])])).astype(F)
    a, b = LP.cross(LP.mk_ref([origins[0], origins[1], c]), par)
    refs.append(a); wis.append(b)
    a, b = LP.cross(LP.ref_edges((c - axis * 2.5 * r + ex * 0.4 * r).astype(F), c), np.concatenate([_unit_rows([axis, axis + 0.3 * ex]).astype(F), LP.random_dirs(rng, 1)]))
    refs.append(a); wis.append(b)
    ro = LP.random_refs(rng, c, 2.5 * r, 40, target=c)
    refs.append(ro); wis.append(_unit_rows(to_world(q, np.column_stack([rng.uniform(-r, r, 40), rng.uniform(-r, r, 40), np.full(40, h)])) - ro[:, 0:3].astype(D)).astype(F))
    ref = np.concatenate(refs).astype(F); wi = np.concatenate(wis).astype(F)
    assert 150 <= len(ref) <= 330, (PROBE_LIGHTS[k][0], len(ref))
    return np.ascontiguousarray(ref), np.ascontiguousarray(wi)


# ---- the conditioned probes: float64 yardsticks for pdf_li -----------------------------------------------------------------------------------------------------------------
COND_MIN_COS, COND_MIN_DIST, COND_MAX_DIST, COND_RIM = 0.1, 0.2, 20.0, 1e-3
COND_CAP = 0.02   # the three constraints may set aside at most this share of the probes


def conditioned_probes(host, k, n=400, seed=0, q=None, wide=False):
    """-> (ref (n, 10), wi (n, 3)) for probe light k, aimed at the shape so that nearly every probe keeps |n . wi| >= 0.1, a distance between 0.2 and 20 radii and a hit point
    at least 10^-3 radii from a rim: origins between 0.6 and 8 radii from the target along a direction within 70 degrees of the surface normal at it (either side).
    q: another shape than probe light k's; wide: a cylinder's outside origins 0.3 to 19 radii from the wall, the whole band the constraints name."""
    q = probe_shape(host, k) if q is None else q
    rng = np.random.default_rng(9500 + seed + k)
    M4 = q["o2w"].astype(D).reshape(4, 4); M = M4[:3, :3]
    r, pm = float(q["radius"]), float(q["phi_max"])
    phi = rng.uniform(0.03, 0.97, n) * pm
    if q["kind"] == QR.DISK:
        ri = float(q["inner_radius"])
        rho = np.sqrt(rng.uniform((ri + 0.03 * r) ** 2, (0.97 * r) ** 2, n))
        t_obj = np.column_stack([rho * np.cos(phi), rho * np.sin(phi), np.full(n, float(q["height"]))])
        n_obj = np.tile([0.0, 0.0, 1.0], (n, 1))
    else:
        zlo, zhi = float(q["z_min"]), float(q["z_max"])
        z = zlo + rng.uniform(0.03, 0.97, n) * (zhi - zlo)
        t_obj = np.column_stack([r * np.cos(phi), r * np.sin(phi), z])
        n_obj = np.column_stack([np.cos(phi), np.sin(phi), np.zeros(n)])
    target = to_world(q, t_obj)
    nw = _unit_rows(n_obj @ np.linalg.inv(M))   # (M^-T n) as rows
    # a direction within 70 degrees of +-n
    side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    tang = _unit_rows(np.cross(nw, rng.normal(size=(n, 3))))
    ang = rng.uniform(0.0, math.radians(70.0), n)
    out = side[:, None] * nw * np.cos(ang)[:, None] + tang * np.sin(ang)[:, None]
    scale = np.linalg.norm(M, 2)   # the object-space radius against world-space distances: keep the world distance inside the band whatever the transform scales
    dist = rng.uniform(0.6, 8.0, n) * r * min(1.0, scale)
    if q["kind"] == QR.CYLINDER:
        # The quadratic's coefficients are rounded to float32 before the discriminant is taken (Quadratic::solve_efloat): b^2 - 4ac cancels to (r^2 - m^2) / |o|^2 of its terms
        # (m: the ray's distance from the axis), so t carries (|o| / r)^2 roundings where the disk's one division carries one.  The disk's figure is the yardstick only where
        # that factor is near 1: origins within 1.5 radii of the wall.  From inside the near wall must be the one aimed at: 0.5 radii on the inner side.
        dist = np.where(side < 0, 0.5 * r, rng.uniform(0.3, 19.0 if wide else 1.5, n) * r * min(1.0, scale))
    o = target + out * dist[:, None]
    ref = LP.mk_ref(o, n=(-out).astype(F))
    wi = _unit_rows(target - ref[:, 0:3].astype(D)).astype(F)
    return np.ascontiguousarray(ref, F), np.ascontiguousarray(wi, F)


def cylinder_hit_f64(q, o, d):
    """The float64 analytic intersection of the world-space ray (o, d) with the cut cylinder, in the roles the device gives the matrices (world_to_object for the ray,
    object_to_world for the point, the transpose of world_to_object for the normal) -> (hit mask, p world, n world (unit), rim distance in radii)"""
    W = q["w2o"].astype(D).reshape(4, 4); O = q["o2w"].astype(D).reshape(4, 4)
    oo = o @ W[:3, :3].T + W[:3, 3]; dd = d @ W[:3, :3].T
    r, zlo, zhi, pm = float(q["radius"]), float(q["z_min"]), float(q["z_max"]), float(q["phi_max"])
    a = dd[:, 0] ** 2 + dd[:, 1] ** 2; b = 2.0 * (dd[:, 0] * oo[:, 0] + dd[:, 1] * oo[:, 1]); c = oo[:, 0] ** 2 + oo[:, 1] ** 2 - r * r
    with np.errstate(all="ignore"):
        disc = b * b - 4.0 * a * c
        root = np.sqrt(np.maximum(disc, 0.0))
        qq = np.where(b < 0, -0.5 * (b - root), -0.5 * (b + root))
        t0, t1 = qq / a, c / qq
        t0, t1 = np.minimum(t0, t1), np.maximum(t0, t1)

        def at(t):
            p = oo + dd * t[:, None]
            phi = np.arctan2(p[:, 1], p[:, 0]); phi = np.where(phi < 0, phi + 2.0 * math.pi, phi)
            ok = (t > 0) & (p[:, 2] >= zlo) & (p[:, 2] <= zhi) & (phi <= pm)
            rim = np.minimum(p[:, 2] - zlo, zhi - p[:, 2])
            if pm < 6.28:
                rim = np.minimum(rim, np.minimum(phi, pm - phi) * r)
            return ok, p, rim / r
        ok0, p0, rim0 = at(t0); ok1, p1, rim1 = at(t1)
    hit = (disc >= 0) & (ok0 | ok1)
    p = np.where(ok0[:, None], p0, p1); rim = np.where(ok0, rim0, rim1)
    n_obj = np.column_stack([p[:, 0], p[:, 1], np.zeros(len(p))])
    nw = _unit_rows(n_obj @ W[:3, :3])   # transpose of world_to_object applied to n
    return hit, p @ O[:3, :3].T + O[:3, 3], nw, rim


def disk_rim_f64(q, hit_p_world):
    """distance of a float64 hit point on the disk from its nearest rim (outer, inner, the two phi edges), in radii"""
    W = q["w2o"].astype(D).reshape(4, 4)
    p = hit_p_world @ W[:3, :3].T + W[:3, 3]
    r, ri, pm = float(q["radius"]), float(q["inner_radius"]), float(q["phi_max"])
    rho = np.hypot(p[:, 0], p[:, 1])
    rim = r - rho
    if ri > 0:
        rim = np.minimum(rim, rho - ri)
    if pm < 6.28:
        phi = np.arctan2(p[:, 1], p[:, 0]); phi = np.where(phi < 0, phi + 2.0 * math.pi, phi)
        rim = np.minimum(rim, np.minimum(phi, pm - phi) * rho)
    return rim / r


def conditioned_keep(q, ref, wi, hit, p, n, rim):
    """the three constraints, evaluated on float64 values alone"""
    dist = np.linalg.norm(p - ref[:, 0:3].astype(D), axis=1) / float(q["radius"])
    cos = np.abs(np.einsum("ij,ij->i", n, wi.astype(D)))
    with np.errstate(invalid="ignore"):
        return hit & (cos >= COND_MIN_COS) & (dist >= COND_MIN_DIST) & (dist <= COND_MAX_DIST) & (rim >= COND_RIM)


def disk_twin(host, k, n=400):
    """Disk light k on its conditioned probes: (ref, wi, float32 restatement, float64 twin, keep mask decided by the twin alone)"""
    q = probe_shape(host, k)
    ref, wi = conditioned_probes(host, k, n)
    p32, _ = QR.disk_pdf_li(q, ref, wi, F)
    hit, p, nn = QR.disk_intersect(q, QR.spawn_origin(ref, wi, D), wi.astype(D), D)
    p64 = QR.area_pdf(q, ref, wi, p, nn, hit, D)
    keep = conditioned_keep(q, ref, wi, hit, p, nn, disk_rim_f64(q, p))
    return ref, wi, p32, p64, keep


def cylinder_twin(host, k, n=400):
    """Cylinder light k on its conditioned probes: (ref, wi, float64 twin of area_pdf on the float64 analytic hit, keep mask)"""
    q = probe_shape(host, k)
    ref, wi = conditioned_probes(host, k, n)
    hit, p, nn, rim = cylinder_hit_f64(q, QR.spawn_origin(ref, wi, D), wi.astype(D))
    p64 = QR.area_pdf(q, ref, wi, p, nn, hit, D)
    return ref, wi, p64, conditioned_keep(q, ref, wi, hit, p, nn, rim)


def cylinder_restated(host, k, n=400):
    """Cylinder light k on its conditioned probes: the float32 restatement of the reference's own arithmetic (ref, wi, pdf, hit mask)"""
    ref, wi = conditioned_probes(host, k, n)
    pdf, hit = QR.cylinder_pdf_li(probe_shape(host, k), ref, wi, F)
    return ref, wi, pdf, hit


def cylinder_wide(host, q, k):
    """Cylinder q on probes over the whole band (origins out to 19 radii): (ref, wi, float32 restatement, where |t| is far from 0 and the float64 hit keeps the constraints)"""
    ref, wi = conditioned_probes(host, k, 400, seed=50, q=q, wide=True)
    pdf, hit = QR.cylinder_pdf_li(q, ref, wi, F)
    h64, p, nn, rim = cylinder_hit_f64(q, QR.spawn_origin(ref, wi, D), wi.astype(D))
    return ref, wi, pdf, conditioned_keep(q, ref, wi, h64, p, nn, rim)


def measured_margin(host):
    """-> (largest relative difference of the disk's float32 restatement against its float64 twin over the five disk lights' conditioned probes, 4 x that): the cylinder's
    device pdf is held to its float64 twin within the second.  Nothing of the library's device code enters this figure."""
    worst = 0.0
    for k in DISKS:
        ref, wi, p32, p64, keep = disk_twin(host, k)
        assert keep.mean() >= 1.0 - COND_CAP, (PROBE_LIGHTS[k][0], float(keep.mean()))
        worst = max(worst, float(np.max(np.abs(p32[keep].astype(D) - p64[keep]) / p64[keep])))
    return worst, 4.0 * worst


# ---- closed forms --------------------------------------------------------------------------------------------------------------------------------------------------------
DISK_R, DISK_H, DISK_CAM_X, DISK_INNER = 0.7, 1.3, 1.8, 0.35
CYL_R, CYL_H, PATCH, WINDOW = 1.0, 0.8, 0.3, 0.2


def ortho_window(host, res, z, xy=(0.0, 0.0), half=1.0):
    _, c2w = host.look_at([xy[0], xy[1], z], [xy[0], xy[1], 0.0], [0.0, 1.0, 0.0])
    return ("ortho", host.orthographic_raster_to_camera(res, res, screen=(-half, half, -half, half)), c2w)


def disk_over_floor(host, res=64, spp=64, reverse=True, two_sided=False, inner=0.0):
    """(a) A disk of radius 0.7 at height 1.3 that faces down (reverse orientation; (b): left facing up), L = LE, black matte, over a wide matte (RHO) quad at z = 0; an
    orthographic camera at (1.8, 0, 5) looks down at the square [0.8, 2.8] x [-1, 1] beside the disk, which no camera ray meets.  A ray that leaves the floor meets the black
    disk or nothing: the same radiance at every depth >= 1."""
    def build(s):
        floor = s.add_material_matte(RHO, 0.0)
        black = s.add_material_matte((0.0, 0.0, 0.0), 0.0)
        s.add_mesh(*CF._zquad(0.0, 60.0, c=(33.0, -25.0)), floor)
        add_light(s, QR.DISK, R.ctm(host, host.translate((0.0, 0.0, DISK_H))), DISK_R, 0.0, inner, 360.0, black, reverse, L=LE, two_sided=two_sided)
        CF._setup_view(s, host, res, spp, CF.HALTON, CF.ortho_down(host, res, z=5.0, xy=(DISK_CAM_X, 0.0)))
        s.build_accel(0, 4)
    return build


def disk_floor_radiance(d, R_=DISK_R, h=DISK_H):
    """radiance / (rho Le) of a Lambertian floor at distance d from the axis of a disk of radius R_ that faces it from height h: the disk's form factor"""
    return 0.5 * (1.0 - (h * h + d * d - R_ * R_) / np.sqrt((h * h + d * d + R_ * R_) ** 2 - 4.0 * R_ * R_ * d * d))


def pixel_expect(s, res, fn, k=4):
    """(res, res) float64: fn(X, Y) averaged over every pixel's footprint (box filter of radius 0.5: a pixel's samples are its own), from the scene's own camera rays — film
    position -> world position is affine for an orthographic camera looking straight down"""
    rays, pf = s.generate_camera_rays([0, 0, res, res], 0)
    A = np.column_stack([np.ones(len(pf)), pf.astype(D)])
    cx, *_ = np.linalg.lstsq(A, rays["o"][:, 0].astype(D), rcond=None)
    cy, *_ = np.linalg.lstsq(A, rays["o"][:, 1].astype(D), rcond=None)
    assert np.abs(A @ cx - rays["o"][:, 0]).max() < 1e-5 and np.abs(A @ cy - rays["o"][:, 1]).max() < 1e-5
    sub = (np.arange(k) + 0.5) / k
    py, px = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    g = np.zeros((res, res))
    for dy in sub:
        for dx in sub:
            fx, fy = px + dx, py + dy
            g += fn(cx[0] + cx[1] * fx + cx[2] * fy, cy[0] + cy[1] * fx + cy[2] * fy)
    return g / (k * k)


def disk_pixel_expect(s, res):
    """(res, res, 3): rho Le times the form factor over every pixel's footprint"""
    g = pixel_expect(s, res, lambda X, Y: disk_floor_radiance(np.hypot(X, Y)))
    return g[..., None] * np.asarray(RHO, D) * np.asarray(LE, D)


def wall_patch_radiance(rr, R_=CYL_R, H=CYL_H, n=4096):
    """radiance / (rho Le) of a horizontal Lambertian patch in the plane z = 0 at distance rr from the axis of an inward-emitting cylinder wall of radius R_, z in [-H, H]:
    (1 / pi) int cos cos' / d^2 dA over the wall's upper half, the z integral done in closed form, the phi integral by the midpoint rule in float64"""
    rr = np.asarray(rr, D)
    phi = (np.arange(n) + 0.5) * (2.0 * math.pi / n)
    cp = np.cos(phi)
    a2 = R_ * R_ + rr[..., None] ** 2 - 2.0 * R_ * rr[..., None] * cp
    f = (R_ - rr[..., None] * cp) * 0.5 * (1.0 / a2 - 1.0 / (a2 + H * H))
    return R_ * f.sum(-1) * (2.0 * math.pi / n) / math.pi


def wall_on_axis(R_=CYL_R, H=CYL_H):
    return H * H / (H * H + R_ * R_)


def cylinder_wall(host, res=64, spp=64, caps=False, cam_z=3.0):
    """(c) An inward-emitting (reverse orientation) cylinder of radius 1, z in [-0.8, 0.8], L = LE, black matte, around a matte (RHO) patch of half-width 0.3 in the plane
    z = 0 that faces +z; an orthographic camera on the axis looks down at the patch's middle [-0.2, 0.2]^2.  caps: (d) two disks close the can, both emitting inwards, and the
    camera sits inside it: three lights."""
    def build(s):
        rho = s.add_material_matte(RHO, 0.0)
        black = s.add_material_matte((0.0, 0.0, 0.0), 0.0)
        s.add_mesh(*CF._zquad(0.0, PATCH), rho)
        ident = R.ctm(host)
        add_light(s, QR.CYLINDER, ident, CYL_R, -CYL_H, CYL_H, 360.0, black, True, L=LE)
        if caps:
            add_light(s, QR.DISK, ident, CYL_R, -CYL_H, 0.0, 360.0, black, False, L=LE)
            add_light(s, QR.DISK, ident, CYL_R, CYL_H, 0.0, 360.0, black, True, L=LE)
        CF._setup_view(s, host, res, spp, CF.HALTON, ortho_window(host, res, 0.5 if caps else cam_z, half=WINDOW))
        s.build_accel(0, 4)
    return build


def can_furnace(host, res=64, spp=64):
    """(d) The closed can alone, every wall matte (RHO) and emitting LE inwards, a perspective camera inside it: Le sum_{k <= D} rho^k at depth D (closed_form.furnace_expect)"""
    def build(s):
        rho = s.add_material_matte(RHO, 0.0)
        ident = R.ctm(host)
        add_light(s, QR.CYLINDER, ident, CYL_R, -CYL_H, CYL_H, 360.0, rho, True, L=LE)
        add_light(s, QR.DISK, ident, CYL_R, -CYL_H, 0.0, 360.0, rho, False, L=LE)
        add_light(s, QR.DISK, ident, CYL_R, CYL_H, 0.0, 360.0, rho, True, L=LE)
        _, c2w = host.look_at([0.13, -0.21, 0.07], [0.4, 1.0, 0.25], [0, 0, 1])
        CF._setup_view(s, host, res, spp, CF.HALTON, ("persp", host.perspective_raster_to_camera(70.0, res, res), c2w))
        s.build_accel(0, 4)
    return build


# ---- scenes for the same-bits and emission tests ------------------------------------------------------------------------------------------------------------------------------
def case_disk_and_cylinder(s, host, split=0):
    """The stage of the sphere-light cases (a matte floor, a glass and a mirror object) under a disk light with an inner radius that faces down and a two-sided cut cylinder"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    SL._stage(s, host)
    add_light(s, QR.DISK, R.ctm(host, host.translate((0.4, 0.2, 2.6)), host.rotate(20.0, (1, 0, 0))), 0.8, 0.0, 0.2, 300.0, black, True, L=(14.0, 12.0, 10.0))
    add_light(s, QR.CYLINDER, R.ctm(host, host.translate((-1.2, 1.0, 1.2)), host.rotate(70.0, (0, 1, 0))), 0.25, -0.6, 0.6, 270.0, black, False, L=(9.0, 10.0, 12.0), two_sided=True)
    SL._view(s, host, split=split)


def case_sphere_and_disk(s, host):
    black = s.add_material_matte((0.0, 0.0, 0.0))
    SL._stage(s, host)
    SL.add_sphere_light(s, R.ctm(host, host.translate((-1.0, -0.5, 2.5))), 0.3, material=black, L=(20.0, 18.0, 16.0))
    add_light(s, QR.DISK, R.ctm(host, host.translate((0.4, 0.2, 2.6))), 0.8, 0.0, 0.0, 360.0, black, True, L=(14.0, 12.0, 10.0))
    SL._view(s, host)


EMIT_L = (3.0, 2.5, 2.0)
# centre, kind, reverse: seen from +z by an orthographic camera.  A disk shows L on the side its normal faces (+z unless reversed); a cylinder lying along y shows L on its
# outside unless reversed
EMITTERS = [((-0.5, 0.5), QR.DISK, False, True), ((0.5, 0.5), QR.DISK, True, False), ((-0.5, -0.5), QR.CYLINDER, False, True), ((0.5, -0.5), QR.CYLINDER, True, False)]


def emission_scene(host, res=32, spp=4):
    def build(s):
        black = s.add_material_matte((0.0, 0.0, 0.0), 0.0)
        s.add_mesh(*CF._zquad(-2.0, 3.0), black)
        for (x, y), kind, rev, lit in EMITTERS:
            if kind == QR.DISK:
                add_light(s, kind, R.ctm(host, host.translate((x, y, 0.0))), 0.4, 0.0, 0.0, 360.0, black, rev, L=EMIT_L)
            else:
                add_light(s, kind, R.ctm(host, host.translate((x, y, 0.0)), host.rotate(90.0, (1, 0, 0))), 0.3, -0.4, 0.4, 360.0, black, rev, L=EMIT_L)
        CF._setup_view(s, host, res, spp, CF.HALTON, CF.ortho_down(host, res, z=5.0))
        s.build_accel(0, 4)
    return build


def emission_masks(s, res):
    """per emitter: the pixels whose whole footprint lies on the shape as the camera sees it, with a margin"""
    rays, pf = s.generate_camera_rays([0, 0, res, res], 0)
    X = rays["o"][:, 0].astype(D).reshape(res, res); Y = rays["o"][:, 1].astype(D).reshape(res, res)
    m = 2.0 * 2.0 / res
    out = []
    for (x, y), kind, rev, lit in EMITTERS:
        if kind == QR.DISK:
            out.append(np.hypot(X - x, Y - y) < 0.4 - m)
        else:
            out.append((np.abs(X - x) < 0.3 - m) & (np.abs(Y - y) < 0.4 - m))
    return out


# ---- the front end ---------------------------------------------------------------------------------------------------------------------------------------------------------------
FRONT_END_WORLD = """
  AttributeBegin
    Material "matte" "color Kd" [0 0 0]
    Translate -4 0 6
    ReverseOrientation
    AreaLightSource "diffuse" "color L" [20 20 20] "integer nsamples" [8]
    Shape "disk" "float radius" [3] "float innerradius" [0.5] "float phimax" [300]
  AttributeEnd

  AttributeBegin
    Material "matte" "color Kd" [0 0 0]
    Translate 3 0 2
    Rotate 90 0 1 0
    AreaLightSource "area" "color L" [6 5 4] "rgb scale" [2 2 2] "bool twosided" "true"
    Shape "cylinder" "float radius" [0.5] "float zmin" [-1] "float zmax" [1.5] "float phimax" [270]
  AttributeEnd
"""


def front_end_scene_text(text, integrator, res=64, spp=8):
    """tests/golden/ref_scenes/lights/diffuse.pbrt with its sphere light replaced by FRONT_END_WORLD, at res x res and spp samples"""
    import re
    text, n = re.subn(r"  AttributeBegin\n    Material \"matte\" \"color Kd\" \[0 0 0\]\n.*?AttributeEnd\n", lambda m: FRONT_END_WORLD, text, count=1, flags=re.S)
    assert n == 1
    text, n = re.subn(r'"integer pixelsamples" \d+', '"integer pixelsamples" %d' % spp, text); assert n == 1
    text, n = re.subn(r'"integer xresolution" \[\d+\] "integer yresolution" \[\d+\]', '"integer xresolution" [%d] "integer yresolution" [%d]' % (res, res), text); assert n == 1
    text, n = re.subn(r'Integrator "whitted"', 'Integrator "%s"' % integrator, text); assert n == 1
    return text


def front_end_scene_abi(s, host, res=64, spp=8):
    """FRONT_END_WORLD and the rest of lights/diffuse.pbrt call by call"""
    black = s.add_material_matte((0.0, 0.0, 0.0))
    add_light(s, QR.DISK, R.ctm(host, host.translate((-4, 0, 6))), 3.0, 0.0, 0.5, 300.0, black, True, L=(20.0, 20.0, 20.0))
    add_light(s, QR.CYLINDER, R.ctm(host, host.translate((3, 0, 2)), host.rotate(90.0, (0, 1, 0))), 0.5, -1.0, 1.5, 270.0, black, False, L=(12.0, 10.0, 8.0), two_sided=True)
    R._cube_and_checker_floor(s, host)
    R.camera_film(s, host, (0, 5, 3), (0, 0, 0), (0, 0, 1), 90.0, res, res, spp)
    s.build_accel(0, 4)
