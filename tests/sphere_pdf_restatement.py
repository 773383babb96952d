"""Sphere::pdf_solid_angle (shapes/src/sphere.rs:462-475) restated in numpy float32, one operation per ufunc call (numpy fuses nothing), in the reference's expression order:
Ray::offset_origin (core/src/geometry/ray.rs:107-127), the inside predicate, the outside (cone) value, and the trait default's last line (core/src/geometry/shape.rs:98) that the
inside branch evaluates on an intersection found elsewhere.  No intersection routine and no transcendental lives here.  tests/test_path_sphere_lights_cpu.py holds this file to
the oracle's own sample_li on the probe case set; the GPU probe test then holds the device to it bit for bit."""
import numpy as np

F = np.float32
TWO_PI = F(F(np.pi) * F(2.0))   # dmath.h: kTwoPi = kPi * 2.0f
INF = F(np.inf)


def _f(a):
    return np.asarray(a, F)


def dot(a, b):
    a, b = _f(a), _f(b)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]   # left to right, as `a.x * b.x + a.y * b.y + a.z * b.z` parses


def distance_squared(a, b):
    d = _f(a) - _f(b)
    return dot(d, d)


def next_up(v):
    """next_float_up (core/src/pbrt/common.rs:205-222): +inf stays, -0 counts as +0"""
    return np.nextafter(_f(v), INF)


def next_down(v):
    return np.nextafter(_f(v), -INF)


def offset_origin(p, p_error, n, w):
    """(k, 3) each -> (k, 3)"""
    p, p_error, n, w = _f(p), _f(p_error), _f(n), _f(w)
    d = dot(np.abs(n), p_error)
    offset = d[..., None] * n
    offset = np.where((dot(w, n) < F(0))[..., None], -offset, offset)
    po = p + offset
    with np.errstate(over="ignore"):
        return np.where(offset > F(0), next_up(po), np.where(offset < F(0), next_down(po), po)).astype(F)


def spawn_ray_origin(ref, wi):
    """Interaction::spawn_ray (interaction/mod.rs:189-192): origin of the ray from the probe reference points `ref` (k, 10) = p, p_error, n, time towards wi"""
    ref = _f(ref)
    return offset_origin(ref[:, 0:3], ref[:, 3:6], ref[:, 6:9], wi)


def centre_of(o2w):
    """object_to_world.transform_point(Point3f::ZERO) of an affine transform: its translation column"""
    m = _f(o2w).reshape(4, 4)
    assert m[3, 3] == F(1) and not m[3, :3].any()
    return np.array([m[0, 3], m[1, 3], m[2, 3]], F)


def is_inside(ref, centre, radius):
    """sphere.rs:466-467 on probe reference points (k, 10): does the point, offset towards the centre, lie in or on the sphere of the OBJECT-space radius?"""
    ref = _f(ref); c = _f(centre)
    with np.errstate(all="ignore"):
        po = offset_origin(ref[:, 0:3], ref[:, 3:6], ref[:, 6:9], c - ref[:, 0:3])
        return distance_squared(po, c) <= F(radius) * F(radius)


def cone_pdf(ref, centre, radius):
    """sphere.rs:472-474: uniform_cone_pdf of the cone the full sphere subtends from hit.p.  Whatever the float32 expression gives, infinity (cos_theta_max rounded to 1) included"""
    ref = _f(ref); c = _f(centre)
    with np.errstate(all="ignore"):
        sin2 = (F(radius) * F(radius)) / distance_squared(ref[:, 0:3], c)
        x = F(1) - sin2
        cos_max = np.sqrt(np.where(F(0) > x, F(0), x))   # max(0, x) as `0 > x ? 0 : x`: a NaN stays
        return (F(1) / (TWO_PI * (F(1) - cos_max))).astype(F)


def sampled_cone_pdf(ref, centre, radius):
    """The same pdf as Sphere::sample_solid_angle's outside branch spells it (sphere.rs:373-409): sin_theta_max = radius * (1 / distance), squared — not radius^2 / distance^2, so
    the two differ in the last bit now and then.  Here only so that the oracle's sample_li can show which branch it took."""
    ref = _f(ref); c = _f(centre)
    with np.errstate(all="ignore"):
        d = ref[:, 0:3] - c
        inv_dc = F(1) / np.sqrt(dot(d, d))
        s = F(radius) * inv_dc
        x = F(1) - s * s
        cos_max = np.sqrt(np.where(F(0) > x, F(0), x))
        return (F(1) / (TWO_PI * (F(1) - cos_max))).astype(F)


def sphere_area(radius, zmin=None, zmax=None, phimax=360.0):
    """Sphere::area of the constructor's clamped values (sphere.rs:21-44): phi_max * radius * (z_max - z_min)"""
    r = F(radius)
    a = -r if zmin is None else F(zmin); b = r if zmax is None else F(zmax)
    lo, hi = np.clip(min(a, b), -r, r), np.clip(max(a, b), -r, r)
    phi = np.clip(F(phimax), F(0), F(360)) * (F(np.pi) / F(180))
    return F(F(phi * r) * F(hi - lo))


def area_pdf(ref, wi, hit_p, hit_n, hit_mask, area):
    """shape.rs:98-103 from an intersection (p, n) of spawn_ray(ref, wi) with the shape: distance_squared / (abs_dot(n, -wi) * area), 0 for a miss and for an infinite value"""
    ref, wi = _f(ref), _f(wi)
    with np.errstate(all="ignore"):
        pdf = distance_squared(ref[:, 0:3], hit_p) / (np.abs(dot(hit_n, -wi)) * F(area))
    pdf = np.where(np.isinf(pdf), F(0), pdf)
    return np.where(hit_mask, pdf, F(0)).astype(F)
