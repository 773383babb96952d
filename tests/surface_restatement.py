"""Float64 restatement of the hit-to-interaction stage, in numpy, written from the reference's sources — the tail of Triangle::intersect (shapes/src/triangle.rs:547-724),
Ray::offset_origin (core/src/geometry/ray.rs:107-127), Interaction::spawn_ray / spawn_ray_to_hit (core/src/interaction/mod.rs:189-223), Transform::transform_surface_interaction
(core/src/geometry/transform.rs:566-590) and SurfaceInteraction::compute_differentials (core/src/interaction/surface_interaction.rs:203-278) — and not from the oracle.  It does not
reproduce float32 rounding: it supplies the exact quantities (the point sum b_i p_i, the triangle's plane, the interpolated shading frame) that properties of the oracle's float32
outputs are checked against in test_surface_probe_cases_cpu.py.  A misreading of the reference shared by the oracle and the device breaks these properties; rounding does not.

RESIDUALS: the largest residual of each approximate condition that the ORACLE leaves on the case sets of surface_probe_cases.py, relative to the norms of the operands, with the
set it came from.  The test asserts 8 x the value: room for another libm or compiler, not for a wrong formula (the smallest of which — a swapped pair of uv differences, a
missing transpose — leaves residuals of order 1)."""
import numpy as np

# measured 2026-10-21 on the oracle, libm mode 0; (largest relative residual, the set that gave it)
RESIDUALS = {
    "unit_ns": (1.279e-07, "quadrics_and_curves"),          # | |ns| - 1 |
    "unit_ss": (2.438e-07, "quadrics_and_curves"),          # | |ss| - 1 |, hits outside instances on meshes with N or S
    "ss_dot_ns": (1.230e-07, "instances"),                  # |ss . ns| / (|ss| |ns|)
    "dpdu_dpdv_span": (2.119e-07, "instances"),             # p_i - p_2 - (dpdu (u_i - u_2) + dpdv (v_i - v_2)), |uv determinant| >= 1e-2
    "dndu_dndv_span": (2.658e-07, "instances"),             # the same for N_i - N_2 with dn/du, dn/dv
    "n_dot_dpdx": (2.104e-07, "quadrics_and_curves"),       # n . dpdx, n . dpdy against p, the offset rays' origins and dpdx
    "dpdx_solved": (1.768e-07, "instances"),                # dpdx - (dudx dpdu + dvdx dpdv) in the two solved coordinates
    "n_matches_plane": (1.367e-07, "instances"),            # n against the restated, oriented plane normal
}
FACTOR = 8.0


def f64(a):
    return np.asarray(a, np.float64)


def norm(v):
    return np.sqrt((v * v).sum(axis=-1))


def normalize(v):
    return v / norm(v)[..., None]


def apply_point(m, p):
    """Transform::transform_point with the float32 matrix entries taken as exact (w = 1 for the affine matrices used here)"""
    m = f64(m)
    return p @ m[:3, :3].T + m[:3, 3]


def apply_vector(m, v):
    return v @ f64(m)[:3, :3].T


def apply_normal(m, n):
    """transform_normal: the transpose of the inverse (transform.rs:441-448)"""
    inv = np.linalg.inv(f64(m)[:3, :3])
    return n @ inv   # (inv^T n)^T = n^T inv


def exact_point(P, b, m=None):
    """sum b_i p_i in float64 (every product and sum of float32 operands here is exact or rounds far below float32's resolution), carried through an instance's matrix"""
    p = f64(b) @ f64(P)
    return p if m is None else apply_point(m, p)


def plane_normal(P, m=None):
    """the unit normal cross(p0 - p2, p1 - p2) of the triangle's plane (triangle.rs:625), of its world-space image under an instance"""
    P = f64(P)
    if m is not None:
        P = apply_point(m, P)
    return normalize(np.cross(P[0] - P[2], P[1] - P[2])), P


def coordinate_system(v1):
    """core/src/geometry/coordinate_system.rs:12-20"""
    if abs(v1[0]) > abs(v1[1]):
        v2 = np.array([-v1[2], 0.0, v1[0]]) / np.sqrt(v1[0] * v1[0] + v1[2] * v1[2])
    else:
        v2 = np.array([0.0, v1[2], -v1[1]]) / np.sqrt(v1[1] * v1[1] + v1[2] * v1[2])
    return v2, np.cross(v1, v2)


DEFAULT_UV = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])   # get_uvs without per-vertex uv (triangle.rs:384-394)


def uvs_of(tri):
    return DEFAULT_UV if tri["UV"] is None else f64(tri["UV"])


def uv_determinant(tri):
    uv = uvs_of(tri)
    d02, d12 = uv[0] - uv[2], uv[1] - uv[2]
    return d02[0] * d12[1] - d02[1] * d12[0]


def shading_frame(tri, b, m=None):
    """The tail of Triangle::intersect in float64 for one probe: returns dict(n, ns, ss, margin) in world space, n and ns as the reference orients them — reverse_orientation ^
    transform_swaps_handedness, then set_shading_geometry's face_forward of n towards the shading normal, then (instances) transform_surface_interaction's face_forward of the
    shading normal towards n.  margin = the smallest |dot| a sign decision rested on: a probe whose margin is tiny may legitimately round to the other side in float32."""
    P = f64(tri["P"]); b = f64(b)
    uv = uvs_of(tri)
    duv02, duv12 = uv[0] - uv[2], uv[1] - uv[2]
    dp02, dp12 = P[0] - P[2], P[1] - P[2]
    det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
    degenerate = abs(np.float32(det)) < np.float32(1e-8)
    dpdu = dpdv = np.zeros(3)
    if not degenerate:
        dpdu = (duv12[1] * dp02 - duv02[1] * dp12) / det
        dpdv = (-duv12[0] * dp02 + duv02[0] * dp12) / det
    if degenerate or (np.cross(dpdu, dpdv).astype(np.float32) ** 2).sum() == 0:
        dpdu, dpdv = coordinate_system(normalize(np.cross(P[2] - P[0], P[1] - P[0])))
    n = normalize(np.cross(dp02, dp12))
    if tri["rev"] != tri["swp"]:
        n = -n
    ns, ss, margin = n, normalize(dpdu), np.inf
    if tri["N"] is not None or tri["S"] is not None:
        if tri["N"] is not None:
            ns2 = b @ f64(tri["N"])
            ns = normalize(ns2) if (ns2 * ns2).sum() > 0 else n
        if tri["S"] is not None:
            ss2 = b @ f64(tri["S"])
            if (ss2 * ss2).sum() > 0:
                ss = normalize(ss2)
        ts = np.cross(ss, ns)
        if (ts * ts).sum() > 1e-24:
            ts = normalize(ts); ss = np.cross(ts, ns)
        else:
            ss, ts = coordinate_system(ns)
        if tri["rev"]:
            ts = -ts
        ns = normalize(np.cross(ss, ts))
        margin = abs(np.dot(n, ns))
        if np.dot(n, ns) < 0:
            n = -n
    if m is not None:
        n = normalize(apply_normal(m, n)); ns = normalize(apply_normal(m, ns)); ss = apply_vector(m, ss)
        margin = min(margin, abs(np.dot(ns, n)))
        if np.dot(ns, n) < 0:
            ns = -ns
    return dict(n=n, ns=ns, ss=ss, margin=margin)


def rel(residual, *operands):
    """|residual| relative to the largest operand norm (0 where every operand is 0)"""
    scale = max([float(np.max(np.abs(o))) for o in operands] + [0.0])
    r = float(np.max(np.abs(residual)))
    return r / scale if scale > 0 else r
