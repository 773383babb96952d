"""Disk and Cylinder as the shapes of a DiffuseAreaLight, restated in numpy with one operation per ufunc call (numpy fuses nothing), in the reference's expression order:
Disk::sample (shapes/src/disk.rs:214-234), Cylinder::sample (shapes/src/cylinder.rs:322-348), the trait's default Shape::sample_solid_angle (core/src/geometry/shape.rs:64-80),
the tail of DiffuseAreaLight::sample_li (lights/src/diffuse.rs:114-129) with the shadow ray Interaction::spawn_ray_to_hit makes of it, and Disk::intersect (disk.rs:85-156) up to the
world-space p and n that Shape::pdf_solid_angle (shape.rs:86-107) reads.  Every function takes the number type T: numpy.float32 is the restatement the device is held to bit for
bit, numpy.float64 its twin (the same expressions; the float32 inputs are widened exactly).  Sine, cosine and atan2 are evaluated in float64 and rounded once to T, as the
library does.  tests/test_quadric_lights_cpu.py proves this file without the device."""
import numpy as np

F = np.float32
D = np.float64
CYLINDER, DISK = 0, 3
STRIDE = 28


def _c(T):
    """the constants of core/src/pbrt/common.rs in T (the float32 ones as dmath.h spells them)"""
    pi = T(F(np.pi)) if T is F else T(np.pi)
    eps = T(2.0 ** -24) if T is F else T(2.0 ** -53)
    g3 = (T(3) * eps) / (T(1) - T(3) * eps)
    return dict(pi=pi, pi2=pi * T(0.5), pi4=pi * T(0.25), two_pi=pi * T(2), g3=g3, inf=T(np.inf))


def _a(x, T):
    return np.asarray(x, T)


def pabs(x):
    """abs as `n < 0 ? -n : n` (common.rs:66-72): -0 stays -0, a NaN stays"""
    return np.where(x < 0, -x, x)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def length_squared(a):
    return dot(a, a)


def div_vec(v, f):
    """Vector3 / Float (vector3.rs:406-418): one reciprocal, three products"""
    inv = v.dtype.type(1) / f
    return inv[..., None] * v


def normalize(v):
    return div_vec(v, np.sqrt(length_squared(v)))


def sincos(x, T):
    x64 = np.asarray(x, D)
    return np.sin(x64).astype(T), np.cos(x64).astype(T)


def xf_normal(w2o, n, T):
    """Transform::transform_normal (transform.rs:439-446): the transpose of the inverse"""
    mi = _a(w2o, T).reshape(16)
    return np.stack([(mi[0] * n[..., 0] + mi[4] * n[..., 1]) + mi[8] * n[..., 2], (mi[1] * n[..., 0] + mi[5] * n[..., 1]) + mi[9] * n[..., 2],
                     (mi[2] * n[..., 0] + mi[6] * n[..., 1]) + mi[10] * n[..., 2]], -1)


def xf_point_abs_err(o2w, p, pe, T):
    """Transform::transform_point_with_abs_error (transform.rs:338-368) -> (point, absolute error)"""
    m = _a(o2w, T).reshape(16)
    g3 = _c(T)["g3"]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    row = lambda r: (m[4 * r] * x + m[4 * r + 1] * y) + (m[4 * r + 2] * z + m[4 * r + 3])
    err = lambda r: ((g3 + T(1)) * ((pabs(m[4 * r]) * pe[..., 0] + pabs(m[4 * r + 1]) * pe[..., 1]) + pabs(m[4 * r + 2]) * pe[..., 2])
                     + g3 * (((pabs(m[4 * r] * x) + pabs(m[4 * r + 1] * y)) + pabs(m[4 * r + 2] * z)) + pabs(m[4 * r + 3])))
    xyz = np.stack([row(0), row(1), row(2)], -1)
    wp = row(3)
    with np.errstate(all="ignore"):
        xyz = np.where((wp == T(1))[..., None], xyz, div_vec(xyz, wp))
    return xyz.astype(T), np.stack([err(0), err(1), err(2)], -1).astype(T)


def concentric_sample_disk(u, T):
    """core/src/sampling/common.rs:138-155"""
    c = _c(T)
    ux = T(2) * u[..., 0] - T(1); uy = T(2) * u[..., 1] - T(1)
    with np.errstate(all="ignore"):
        first = pabs(ux) > pabs(uy)
        r = np.where(first, ux, uy)
        theta = np.where(first, c["pi4"] * (uy / ux), c["pi2"] - c["pi4"] * (ux / uy))
    sn, cs = sincos(theta, T)
    zero = (ux == 0) & (uy == 0)
    return np.where(zero, T(0), r * cs).astype(T), np.where(zero, T(0), r * sn).astype(T)


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------------------------------------------
def shape(kind, t, radius, a, b, phimax_deg=360.0, reverse=False):
    """The constructor's values (Cylinder::new cylinder.rs:21-42, a, b = zmin, zmax; Disk::new disk.rs:21-40, a, b = height, innerradius) in float32, and area();
    t = (object_to_world, world_to_object) as 16 floats each"""
    q = dict(kind=kind, o2w=np.asarray(t[0], F).reshape(16), w2o=np.asarray(t[1], F).reshape(16), radius=F(radius), reverse=bool(reverse))
    q["phi_max"] = F(np.clip(F(phimax_deg), F(0), F(360)) * (F(np.pi) / F(180)))   # f32::to_radians
    m = q["o2w"].astype(D).reshape(4, 4)[:3, :3]
    q["swaps"] = bool(np.linalg.det(m) < 0)
    if kind == CYLINDER:
        q["z_min"], q["z_max"] = F(min(a, b)), F(max(a, b))
        q["area"] = F(F(F(q["z_max"] - q["z_min"]) * q["radius"]) * q["phi_max"])
    else:
        q["height"], q["inner_radius"] = F(a), F(b)
        q["area"] = F(F(q["phi_max"] * F(0.5)) * F(F(q["radius"] * q["radius"]) - F(q["inner_radius"] * q["inner_radius"])))
    return q


def area(q, T):
    """area() again in T, from the float32 constructor values"""
    if q["kind"] == CYLINDER:
        return ((T(q["z_max"]) - T(q["z_min"])) * T(q["radius"])) * T(q["phi_max"])
    return (T(q["phi_max"]) * T(0.5)) * (T(q["radius"]) * T(q["radius"]) - T(q["inner_radius"]) * T(q["inner_radius"]))


def object_point(q, u, T=F):
    """the object-space point of ::sample (the cylinder's before its re-projection): what lies on the shape"""
    u = _a(u, T).reshape(-1, 2)
    r = T(q["radius"])
    if q["kind"] == DISK:
        px, py = concentric_sample_disk(u, T)
        return np.stack([px * r, py * r, np.full(len(u), T(q["height"]), T)], -1)
    z = (T(1) - u[:, 0]) * T(q["z_min"]) + u[:, 0] * T(q["z_max"])   # lerp (common.rs:167-173)
    sn, cs = sincos(u[:, 1] * T(q["phi_max"]), T)
    return np.stack([r * cs, r * sn, z], -1)


def cylinder_reproject(q, p_obj, T=F):
    """cylinder.rs:337-339: the sampled point scaled back to the radius in x and y"""
    r = T(q["radius"])
    with np.errstate(all="ignore"):
        hit_rad = np.sqrt(p_obj[:, 0] * p_obj[:, 0] + p_obj[:, 1] * p_obj[:, 1])
        return np.stack([p_obj[:, 0] * (r / hit_rad), p_obj[:, 1] * (r / hit_rad), p_obj[:, 2]], -1)


def sample(q, u, T=F):
    """Disk::sample / Cylinder::sample -> (p, p_error, n) in world space, (k, 3) each"""
    u = _a(u, T).reshape(-1, 2)
    p_obj = object_point(q, u, T)
    if q["kind"] == DISK:   # the sample ignores inner_radius and phi_max
        n_obj = np.broadcast_to(np.array([0, 0, 1], T), p_obj.shape)
        pe_obj = np.zeros_like(p_obj)
    else:
        n_obj = np.stack([p_obj[:, 0], p_obj[:, 1], np.zeros(len(u), T)], -1)   # before the re-projection
        p_obj = cylinder_reproject(q, p_obj, T)
        pe_obj = _c(T)["g3"] * pabs(np.stack([p_obj[:, 0], p_obj[:, 1], np.zeros(len(u), T)], -1))
    with np.errstate(all="ignore"):
        n = normalize(xf_normal(q["w2o"], n_obj, T))
    if q["reverse"]:
        n = n * T(-1)
    p, pe = xf_point_abs_err(q["o2w"], p_obj, pe_obj, T)
    return p, pe, n.astype(T)


def sample_solid_angle(q, ref_p, u, T=F):
    """The trait's default (shape.rs:64-80) over sample -> (p, p_error, n, pdf)"""
    ref_p = _a(ref_p, T)
    p, pe, n = sample(q, u, T)
    pdf = T(1) / area(q, T)
    wi = p - ref_p
    with np.errstate(all="ignore"):
        zero = length_squared(wi) == 0
        wn = normalize(wi)
        d = ref_p - p
        conv = pdf * (length_squared(d) / pabs(dot(n, -wn)))
    conv = np.where(np.isinf(conv), T(0), conv)
    return p, pe, n, np.where(zero, T(0), conv).astype(T)


def next_up(v):
    return np.nextafter(v, v.dtype.type(np.inf))


def next_down(v):
    return np.nextafter(v, v.dtype.type(-np.inf))


def offset_origin(p, p_error, n, w):
    """Ray::offset_origin (core/src/geometry/ray.rs:107-127)"""
    d = dot(pabs(n), p_error)
    offset = d[..., None] * n
    offset = np.where((dot(w, n) < 0)[..., None], -offset, offset)
    po = p + offset
    with np.errstate(over="ignore"):
        return np.where(offset > 0, next_up(po), np.where(offset < 0, next_down(po), po))


def sample_li(q, L, two_sided, ref, u, T=F):
    """DiffuseAreaLight::sample_li on the shape and the shadow ray of its VisibilityTester, in the light probe's layout (STRIDE floats per probe, zeros where no sample is made)"""
    ref = _a(ref, T).reshape(-1, 10)
    hp, hpe, hn = ref[:, 0:3], ref[:, 3:6], ref[:, 6:9]
    p, pe, n, pdf = sample_solid_angle(q, hp, u, T)
    out = np.zeros((len(ref), STRIDE), T)
    wi = p - hp
    with np.errstate(all="ignore"):
        l2 = length_squared(wi)
        valid = ~((pdf == 0) | (l2 == 0))
        wi = div_vec(wi, np.sqrt(l2))
        lit = (dot(n, -wi) > 0) | bool(two_sided)
        origin = offset_origin(hp, hpe, hn, p - hp)
        target = offset_origin(p, pe, n, origin - p)
    out[:, 0:3] = wi; out[:, 3] = pdf
    out[:, 4:7] = np.where(lit[:, None], _a(L, T), T(0))
    out[:, 7] = 1
    out[:, 8:11] = p; out[:, 11:14] = pe; out[:, 14:17] = n
    out[:, 17:20] = origin; out[:, 20:23] = target - origin
    out[:, 23] = T(1) - T(F(0.0001)) if T is F else T(1) - T(0.0001)
    out[~valid] = 0
    return out


# ---- Disk::intersect and the trait's default pdf ------------------------------------------------------------------------------------------------------------------------
def object_ray(q, o, d, T):
    """Transform::transform_ray_with_error (transform.rs:481-510) by world_to_object, values only: the origin is pushed along d by its error bound"""
    c = _a(q["w2o"], T); k = _c(T)
    x, y, z = o[:, 0], o[:, 1], o[:, 2]
    row = lambda r: (c[4 * r] * x + c[4 * r + 1] * y) + (c[4 * r + 2] * z + c[4 * r + 3])
    ab = lambda r: ((pabs(c[4 * r] * x) + pabs(c[4 * r + 1] * y)) + pabs(c[4 * r + 2] * z)) + pabs(c[4 * r + 3])
    oo = np.stack([row(0), row(1), row(2)], -1); ow = row(3)
    o_err = k["g3"] * np.stack([ab(0), ab(1), ab(2)], -1)
    oo = np.where((ow == T(1))[:, None], oo, div_vec(oo, ow))
    dd = np.stack([(c[4 * r] * d[:, 0] + c[4 * r + 1] * d[:, 1]) + c[4 * r + 2] * d[:, 2] for r in range(3)], -1)
    l2 = length_squared(dd)
    dt = dot(pabs(dd), o_err) / l2
    return np.where((l2 > 0)[:, None], oo + dd * dt[:, None], oo), dd


def cylinder_intersect(q, o, d, T=F):
    """Cylinder::intersect (cylinder.rs:64-196) of the world-space ray (o, d), t_max = infinity, in VALUES: the EFloat intervals only decide hits whose t lies within its own
    error bound of 0, which callers keep away from.  The coefficients are rounded in T, the discriminant is taken in float64 from them (Quadratic::solve_efloat), the hit point
    is re-projected to the radius -> (hit mask, p, n) in world space."""
    assert q["kind"] == CYLINDER
    o, d = _a(o, T), _a(d, T)
    k = _c(T)
    r, zlo, zhi, pm = T(q["radius"]), T(q["z_min"]), T(q["z_max"]), T(q["phi_max"])
    with np.errstate(all="ignore"):
        oo, dd = object_ray(q, o, d, T)
        ox, oy, dx, dy = oo[:, 0], oo[:, 1], dd[:, 0], dd[:, 1]
        a = dx * dx + dy * dy
        b = T(2) * (dx * ox + dy * oy)
        c = (ox * ox + oy * oy) - r * r
        disc = b.astype(D) * b.astype(D) - D(4) * a.astype(D) * c.astype(D)
        root = np.sqrt(disc).astype(T)
        qq = np.where(b < 0, T(-0.5) * (b - root), T(-0.5) * (b + root))
        t0, t1 = qq / a, c / qq
        swap = t0 > t1
        t0, t1 = np.where(swap, t1, t0), np.where(swap, t0, t1)

        def at(t):
            p = oo + dd * t[:, None]
            hit_rad = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
            p = np.stack([p[:, 0] * (r / hit_rad), p[:, 1] * (r / hit_rad), p[:, 2]], -1)
            phi = np.arctan2(p[:, 1].astype(D), p[:, 0].astype(D)).astype(T)
            phi = np.where(phi < 0, phi + k["two_pi"], phi)
            return p, (p[:, 2] < zlo) | (p[:, 2] > zhi) | (phi > pm)
        hit = ~(disc < 0) & ~(t1 <= 0)
        first = ~(t0 <= 0)
        th = np.where(first, t0, t1)
        p, clipped = at(th)
        p2, clipped2 = at(t1)
        retry = clipped & first & ~(t0 == t1)
        hit &= ~clipped | (retry & ~clipped2)
        p = np.where((clipped & retry)[:, None], p2, p)
        dpdu = np.stack([-pm * p[:, 1], pm * p[:, 0], np.zeros(len(p), T)], -1)
        dz = zhi - zlo
        cr = np.stack([dpdu[:, 1] * dz - dpdu[:, 2] * T(0), dpdu[:, 2] * T(0) - dpdu[:, 0] * dz, dpdu[:, 0] * T(0) - dpdu[:, 1] * T(0)], -1)
        n = normalize(cr)
        if q["reverse"] != q["swaps"]:
            n = n * T(-1)
        pw, _ = xf_point_abs_err(q["o2w"], p, np.zeros_like(p), T)
        nw = normalize(xf_normal(q["w2o"], n, T))
    return hit, pw.astype(T), nw.astype(T)


def cylinder_pdf_li(q, ref, wi, T=F):
    hit, p, n = cylinder_intersect(q, spawn_origin(ref, wi, T), wi, T)
    return area_pdf(q, ref, wi, p, n, hit, T), hit


def disk_intersect(q, o, d, T=F):
    """Disk::intersect of the world-space ray (o, d), t_max = infinity -> (hit mask, p, n) in world space.  transform_ray_with_error (transform.rs:481-510) pushes the origin
    along d by its error bound; the normal is the cross product of dpdu and dpdv, flipped for reverse_orientation XOR a handedness-swapping transform, carried to world space
    by transform_surface_interaction (transform.rs:566-590)."""
    assert q["kind"] == DISK
    o, d = _a(o, T), _a(d, T)
    k = _c(T)
    with np.errstate(all="ignore"):
        oo, dd = object_ray(q, o, d, T)
        t = (T(q["height"]) - oo[:, 2]) / dd[:, 2]
        hit = (dd[:, 2] != 0) & ~(t <= 0) & ~(t >= k["inf"])
        p = oo + dd * t[:, None]
        dist2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
        hit &= ~(dist2 > T(q["radius"]) * T(q["radius"])) & ~(dist2 < T(q["inner_radius"]) * T(q["inner_radius"]))
        phi = np.arctan2(p[:, 1].astype(D), p[:, 0].astype(D)).astype(T)
        phi = np.where(phi < 0, phi + k["two_pi"], phi)
        hit &= ~(phi > T(q["phi_max"]))
        r_hit = np.sqrt(dist2)
        pm = T(q["phi_max"])
        dpdu = np.stack([-pm * p[:, 1], pm * p[:, 0], np.zeros(len(p), T)], -1)
        dpdv = div_vec(np.stack([p[:, 0], p[:, 1], np.zeros(len(p), T)], -1) * (T(q["inner_radius"]) - T(q["radius"])), r_hit)
        p = np.stack([p[:, 0], p[:, 1], np.full(len(p), T(q["height"]), T)], -1)   # refine (disk.rs:134)
        cr = np.stack([dpdu[:, 1] * dpdv[:, 2] - dpdu[:, 2] * dpdv[:, 1], dpdu[:, 2] * dpdv[:, 0] - dpdu[:, 0] * dpdv[:, 2], dpdu[:, 0] * dpdv[:, 1] - dpdu[:, 1] * dpdv[:, 0]], -1)
        n = normalize(cr)
        if q["reverse"] != q["swaps"]:
            n = n * T(-1)
        pw, _ = xf_point_abs_err(q["o2w"], p, np.zeros_like(p), T)
        nw = normalize(xf_normal(q["w2o"], n, T))
    return hit, pw.astype(T), nw.astype(T)


def area_pdf(q, ref, wi, hit_p, hit_n, hit_mask, T=F):
    """shape.rs:98-103 from an intersection (p, n) of spawn_ray(ref, wi) with the shape: distance_squared / (abs_dot(n, -wi) * area), 0 for a miss and for an infinite value"""
    ref, wi = _a(ref, T).reshape(-1, 10), _a(wi, T)
    with np.errstate(all="ignore"):
        pdf = length_squared(ref[:, 0:3] - _a(hit_p, T)) / (pabs(dot(_a(hit_n, T), -wi)) * area(q, T))
    pdf = np.where(np.isinf(pdf), T(0), pdf)
    return np.where(hit_mask, pdf, T(0)).astype(T)


def spawn_origin(ref, wi, T=F):
    """Interaction::spawn_ray (interaction/mod.rs:189-192): the origin of the ray from reference points (k, 10) = p, p_error, n, time towards wi"""
    ref = _a(ref, T).reshape(-1, 10)
    return offset_origin(ref[:, 0:3], ref[:, 3:6], ref[:, 6:9], _a(wi, T))


def disk_pdf_li(q, ref, wi, T=F):
    """DiffuseAreaLight::pdf_li on a disk: Shape::pdf_solid_angle's default, whole"""
    hit, p, n = disk_intersect(q, spawn_origin(ref, wi, T), wi, T)
    return area_pdf(q, ref, wi, p, n, hit, T), hit
