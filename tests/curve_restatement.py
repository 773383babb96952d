"""The reference's Curve shape (shapes/src/curve.rs) restated in NumPy float32, written from curve.rs and the geometry code it calls — not from the device code.

Every operation is one f32 operation in the reference's expression order (NumPy never fuses a multiply and an add); sin, cos and acos go through f64 and are rounded
once.  The functions take N rays at once, each with the parameters of its own curve segment, and follow the reference's control flow ray by ray through
masks: `recursive_intersect` below IS a recursion, one call per (node, set of rays that reach it), with the reference's two quirks spelled as the reference spells them
(`hit = ...` assigned unconditionally; `cps += 3` skipped by `continue`).

    curve_data(type, cp, width, n)             CurveData::new (:743-762)
    create_segments(...)                       Curve::create_segments (:105-140): the (u_min, u_max) of each segment
    object_bound(curve, u_min, u_max)          Curve::object_bound (:660-674)
    intersect(seg, o, d, t_max, shadow)        Curve::intersect(r, is_shadow_ray) (:543-645), (N, 20): hit flag, t, u, v, world-space p, p_error, dpdu, dpdv, n, pad
    intersect_p(...)                           Curve::intersect_p (:689-691)
    from_props(params)                         Curve::from_props (:149-316): the list of (cp, width, n, type, split_depth) it hands create_segments
    log2int(x)                                 Log2Int<u32> for f32 (core/src/pbrt/log2int.rs:12-26)

Where the reference would panic (assert!(dpdu != 0), :501; LookAt's "pointing in the same direction", transform.rs:195-198) the restatement reports a miss of that
evaluation: the library's documented departure."""
import numpy as np

F = np.float32
FLAT, CYLINDER, RIBBON = 0, 1, 2
TYPES = {"flat": FLAT, "cylinder": CYLINDER, "ribbon": RIBBON}
STRIDE = 20
_PI = F(3.14159265358979323846)
_GAMMA3 = F(F(3) * F(5.9604644775390625e-08)) / F(F(1) - F(3) * F(5.9604644775390625e-08))   # gamma(3), common.rs:132-134


def _f(x):
    return np.asarray(x, dtype=np.float32)


def pmax(a, b):   # common.rs:99-108
    return np.where(a > b, a, b)


def pmin(a, b):   # common.rs:83-92
    return np.where(a < b, a, b)


def pabs(a):      # common.rs:67-76
    return np.where(a < F(0), -a, a)


def clamp(x, lo, hi):   # clamp.rs:14-25
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(np.float32)


def lerp(t, a, b):      # common.rs:167-173
    return (F(1) - t) * a + t * b


def lerp3(t, a, b):     # the same on points: Float * Point3 + Float * Point3
    t = _f(t)[..., None]
    return (F(1) - t) * a + t * b


def sin64(x):
    return np.sin(_f(x).astype(np.float64)).astype(np.float32)


def cos64(x):
    return np.cos(_f(x).astype(np.float64)).astype(np.float32)


def acos64(x):
    return np.arccos(_f(x).astype(np.float64)).astype(np.float32)


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross(a, b):   # vector3.rs:211-217
    return np.stack([(a[..., 1] * b[..., 2]) - (a[..., 2] * b[..., 1]), (a[..., 2] * b[..., 0]) - (a[..., 0] * b[..., 2]),
                     (a[..., 0] * b[..., 1]) - (a[..., 1] * b[..., 0])], axis=-1)


def length_squared(a):
    return a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]


def length(a):
    return np.sqrt(length_squared(a))


def div3(a, f):   # Vector3 / Point3 / Normal3 `/ f`: a product with 1 / f (vector3.rs:412-417)
    inv = F(1) / _f(f)
    return inv[..., None] * a


def normalize(a):
    return div3(a, length(a))


def log2int(x):
    """f32::log2int as it runs: 0 below 1, else the exponent plus the mantissa's LOWEST bit; +inf and NaN fail `< 1.0` and come out at 128 or above."""
    x = _f(x)
    bits = x.view(np.uint32).astype(np.int64)
    return np.where(x < F(1), 0, ((bits >> 23) - 127) + (bits & 1))


def max_depth_of(l0, eps):
    """clamp(log2int(1.41421356237 * 6 * l0 / (8 * eps)) / 2, 0, 10) (:628-632)"""
    with np.errstate(all="ignore"):
        r0 = log2int(F(1.41421356237) * F(6.0) * _f(l0) / (F(8.0) * _f(eps))) // 2
    return np.clip(r0, 0, 10)


# ---- geometry the curve calls ------------------------------------------------------------------------------------------------------------------------------
def m4_inverse(a):
    """Matrix4x4::inverse (matrix4x4.rs:67-143) on (N, 4, 4)"""
    m = np.array(a, dtype=np.float32, copy=True)
    n = len(m)
    ar = np.arange(n)
    ipiv = np.zeros((n, 4), np.int64)
    indxr = np.zeros((4, n), np.int64)
    indxc = np.zeros((4, n), np.int64)
    for i in range(4):
        irow = np.zeros(n, np.int64); icol = np.zeros(n, np.int64); big = np.zeros(n, np.float32)
        for j in range(4):
            for k in range(4):
                v = pabs(m[:, j, k])
                upd = (ipiv[:, j] != 1) & (ipiv[:, k] == 0) & (v >= big)
                big = np.where(upd, v, big); irow = np.where(upd, j, irow); icol = np.where(upd, k, icol)
        ipiv[ar, icol] += 1
        ri = m[ar, irow, :].copy(); rc = m[ar, icol, :].copy()
        m[ar, irow, :] = rc; m[ar, icol, :] = ri      # (irow == icol: both rows are the same row)
        indxr[i] = irow; indxc[i] = icol
        pivinv = F(1) / m[ar, icol, icol]
        m[ar, icol, icol] = F(1)
        m[ar, icol, :] = m[ar, icol, :] * pivinv[:, None]
        for j in range(4):
            other = icol != j
            save = m[ar, j, icol].copy()
            row = m[:, j, :].copy()
            row[ar, icol] = F(0)
            row = row - m[ar, icol, :] * save[:, None]
            m[:, j, :] = np.where(other[:, None], row, m[:, j, :])
    for j in range(3, -1, -1):
        a_, b_ = indxr[j], indxc[j]
        ca = m[ar, :, a_].copy(); cb = m[ar, :, b_].copy()
        m[ar, :, a_] = cb; m[ar, :, b_] = ca
    return m


def transform_point(m, p):   # transform.rs:288-302
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    xp = m[..., 0, 0] * x + m[..., 0, 1] * y + m[..., 0, 2] * z + m[..., 0, 3]
    yp = m[..., 1, 0] * x + m[..., 1, 1] * y + m[..., 1, 2] * z + m[..., 1, 3]
    zp = m[..., 2, 0] * x + m[..., 2, 1] * y + m[..., 2, 2] * z + m[..., 2, 3]
    wp = m[..., 3, 0] * x + m[..., 3, 1] * y + m[..., 3, 2] * z + m[..., 3, 3]
    q = np.stack([xp, yp, zp], axis=-1)
    return np.where((wp == F(1))[..., None], q, div3(q, wp))


def transform_vector(m, v):  # transform.rs:373-380
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([m[..., 0, 0] * x + m[..., 0, 1] * y + m[..., 0, 2] * z, m[..., 1, 0] * x + m[..., 1, 1] * y + m[..., 1, 2] * z,
                     m[..., 2, 0] * x + m[..., 2, 1] * y + m[..., 2, 2] * z], axis=-1)


def transform_normal(m_inv, n):  # transform.rs:439-448
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return np.stack([m_inv[..., 0, 0] * x + m_inv[..., 1, 0] * y + m_inv[..., 2, 0] * z, m_inv[..., 0, 1] * x + m_inv[..., 1, 1] * y + m_inv[..., 2, 1] * z,
                     m_inv[..., 0, 2] * x + m_inv[..., 1, 2] * y + m_inv[..., 2, 2] * z], axis=-1)


def transform_ray_with_error(m, o, d):
    """transform.rs:481-513: (o', d'); the origin is pushed along d' by its error bound; t_max is kept"""
    x, y, z = o[..., 0], o[..., 1], o[..., 2]
    xp = (m[..., 0, 0] * x + m[..., 0, 1] * y) + (m[..., 0, 2] * z + m[..., 0, 3])   # transform_point_with_error (:307-334)
    yp = (m[..., 1, 0] * x + m[..., 1, 1] * y) + (m[..., 1, 2] * z + m[..., 1, 3])
    zp = (m[..., 2, 0] * x + m[..., 2, 1] * y) + (m[..., 2, 2] * z + m[..., 2, 3])
    wp = (m[..., 3, 0] * x + m[..., 3, 1] * y) + (m[..., 3, 2] * z + m[..., 3, 3])
    xs = pabs(m[..., 0, 0] * x) + pabs(m[..., 0, 1] * y) + pabs(m[..., 0, 2] * z) + pabs(m[..., 0, 3])
    ys = pabs(m[..., 1, 0] * x) + pabs(m[..., 1, 1] * y) + pabs(m[..., 1, 2] * z) + pabs(m[..., 1, 3])
    zs = pabs(m[..., 2, 0] * x) + pabs(m[..., 2, 1] * y) + pabs(m[..., 2, 2] * z) + pabs(m[..., 2, 3])
    o_err = _GAMMA3 * np.stack([xs, ys, zs], axis=-1)
    q = np.stack([xp, yp, zp], axis=-1)
    o2 = np.where((wp == F(1))[..., None], q, div3(q, wp))
    d2 = transform_vector(m, d)
    l2 = length_squared(d2)
    dt = dot(pabs(d2), o_err) / l2
    return np.where((l2 > F(0))[..., None], o2 + d2 * dt[..., None], o2), d2


def coordinate_system(v1):   # coordinate_system.rs:12-20 (the first of the two vectors)
    x, y, z = v1[..., 0], v1[..., 1], v1[..., 2]
    zero = np.zeros_like(x)
    a = div3(np.stack([-z, zero, x], axis=-1), np.sqrt(x * x + z * z))
    b = div3(np.stack([zero, z, -y], axis=-1), np.sqrt(y * y + z * z))
    return np.where((pabs(x) > pabs(y))[..., None], a, b)


def look_at(pos, look, up):
    """Transform::look_at (transform.rs:191-214): (m, m_inv, panics) — m_inv is the matrix the function writes down, m its Gauss-Jordan inverse"""
    dir_ = normalize(look - pos)
    right = cross(normalize(up), dir_)
    panics = length(right) == F(0)
    right = normalize(right)
    new_up = cross(dir_, right)
    n = len(pos)
    c2w = np.zeros((n, 4, 4), np.float32)
    c2w[:, :3, 0] = right; c2w[:, :3, 1] = new_up; c2w[:, :3, 2] = dir_; c2w[:, :3, 3] = pos
    c2w[:, 3, 3] = F(1)
    return m4_inverse(c2w), c2w, panics


def rotate_axis_matrix(theta_deg, axis):   # transform.rs:155-183 (the 3x3 block of m)
    a = normalize(axis)
    r = _f(theta_deg) * (_PI / F(180.0))      # f32::to_radians
    s, c = sin64(r), cos64(r)
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    m = np.zeros(a.shape[:-1] + (4, 4), np.float32)
    m[..., 0, 0] = ax * ax + (F(1) - ax * ax) * c
    m[..., 0, 1] = ax * ay * (F(1) - c) - az * s
    m[..., 0, 2] = ax * az * (F(1) - c) + ay * s
    m[..., 1, 0] = ax * ay * (F(1) - c) + az * s
    m[..., 1, 1] = ay * ay + (F(1) - ay * ay) * c
    m[..., 1, 2] = ay * az * (F(1) - c) - ax * s
    m[..., 2, 0] = ax * az * (F(1) - c) - ay * s
    m[..., 2, 1] = ay * az * (F(1) - c) + ax * s
    m[..., 2, 2] = az * az + (F(1) - az * az) * c
    m[..., 3, 3] = F(1)
    return m


def swaps_handedness(m):   # transform.rs:593-599
    m = _f(m).reshape(4, 4)
    det = m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])
    return bool(det < F(0))


def transform_bounds(m, lo, hi):   # transform.rs:552-561
    m = _f(m).reshape(4, 4)
    corners = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 1), (1, 1, 1)]
    b = [lo, hi]
    pts = [transform_point(m, _f([b[c[0]][0], b[c[1]][1], b[c[2]][2]])) for c in corners]
    blo, bhi = pts[0].copy(), pts[0].copy()
    for p in pts[1:]:
        blo = pmin(blo, p); bhi = pmax(bhi, p)
    return blo, bhi


# ---- Bezier helpers (curve.rs:765-812) -----------------------------------------------------------------------------------------------------------------------
def blossom_bezier(p, u0, u1, u2):
    a = [lerp3(u0, p[..., 0, :], p[..., 1, :]), lerp3(u0, p[..., 1, :], p[..., 2, :]), lerp3(u0, p[..., 2, :], p[..., 3, :])]
    b = [lerp3(u1, a[0], a[1]), lerp3(u1, a[1], a[2])]
    return lerp3(u2, b[0], b[1])


def subdivide_bezier(cp):
    c0, c1, c2, c3 = cp[..., 0, :], cp[..., 1, :], cp[..., 2, :], cp[..., 3, :]
    return np.stack([c0, (c0 + c1) * (F(1) / F(2)), (c0 + F(2) * c1 + c2) * (F(1) / F(4)), (c0 + F(3) * c1 + F(3) * c2 + c3) * (F(1) / F(8)),
                     (c1 + F(2) * c2 + c3) * (F(1) / F(4)), (c2 + c3) * (F(1) / F(2)), c3], axis=-2)


def eval_bezier(cp, u):
    c0, c1, c2, c3 = cp[..., 0, :], cp[..., 1, :], cp[..., 2, :], cp[..., 3, :]
    cp1 = [lerp3(u, c0, c1), lerp3(u, c1, c2), lerp3(u, c2, c3)]
    cp2 = [lerp3(u, cp1[0], cp1[1]), lerp3(u, cp1[1], cp1[2])]
    diff = cp2[1] - cp2[0]
    deriv = np.where((length_squared(diff) > F(0))[..., None], F(3) * diff, c3 - c0)
    return lerp3(u, cp2[0], cp2[1]), deriv


# ---- the shape -----------------------------------------------------------------------------------------------------------------------------------------------
def curve_data(curve_type, cp, width, n=None):
    """CurveData::new: a dict with cp_obj (4,3), width (2,), n (2,3), normal_angle, inv_sin_normal_angle, type"""
    t = TYPES[curve_type] if isinstance(curve_type, str) else int(curve_type)
    nn = np.zeros((2, 3), np.float32)
    with np.errstate(all="ignore"):
        if n is not None:
            nn = normalize(_f(n).reshape(2, 3))
        angle = acos64(clamp(dot(nn[0], nn[1]), F(0), F(1)))
        inv_sin = F(1) / sin64(angle)
    return dict(cp_obj=_f(cp).reshape(4, 3), width=_f(width).reshape(2), n=nn, normal_angle=F(angle), inv_sin_normal_angle=F(inv_sin), type=t)


def create_segments(split_depth):
    """[(u_min, u_max)] of Curve::create_segments (:117-132)"""
    num = 1 << split_depth
    f = F(1) / F(num)
    return [(F(i) * f, F(i + 1) * f) for i in range(num)]


def segment_cp(cd_cp, u_min, u_max):   # Curve::blossom_bezier (:319-326)
    return np.stack([blossom_bezier(cd_cp, u_min, u_min, u_min), blossom_bezier(cd_cp, u_min, u_min, u_max), blossom_bezier(cd_cp, u_min, u_max, u_max),
                     blossom_bezier(cd_cp, u_max, u_max, u_max)], axis=-2)


def object_bound(cd, u_min, u_max):
    """Curve::object_bound (:660-674): (lo, hi)"""
    q = segment_cp(cd["cp_obj"], F(u_min), F(u_max))
    w = [lerp(F(u_min), cd["width"][0], cd["width"][1]), lerp(F(u_max), cd["width"][0], cd["width"][1])]
    lo = pmin(pmin(q[0], q[1]), pmin(q[2], q[3])); hi = pmax(pmax(q[0], q[1]), pmax(q[2], q[3]))
    delta = pmax(w[0], w[1]) * F(0.5)
    return (lo - delta).astype(np.float32), (hi + delta).astype(np.float32)


def world_bound(cd, u_min, u_max, o2w):
    lo, hi = object_bound(cd, u_min, u_max)
    return transform_bounds(o2w, lo, hi)


class _Ctx:
    pass


def _box_culled(c4, max_width, z_max):
    """the three box tests of :370-411 (and :592-612): True where a `continue` / `return None` is taken"""
    hw = F(0.5) * max_width
    out = np.zeros(len(c4), bool)
    for axis, upper in ((1, None), (0, None), (2, z_max)):
        a = c4[:, :, axis]
        mx = pmax(pmax(a[:, 0], a[:, 1]), pmax(a[:, 2], a[:, 3])); mn = pmin(pmin(a[:, 0], a[:, 1]), pmin(a[:, 2], a[:, 3]))
        out |= (mx + hw < F(0)) | (mn - hw > (F(0) if upper is None else upper))
    return out


def _recursive_intersect(cx, idx, cp, u0, u1, depth, shadow):
    """recursive_intersect (:339-536) for the rays `idx` of the context, all at the same `depth`: (len(idx), STRIDE) rows, column 0 the hit flag"""
    n = len(idx)
    res = np.zeros((n, STRIDE), np.float32)
    if n == 0:
        return res
    w0, w1 = cx.w0[idx], cx.w1[idx]
    z_max = cx.z_max[idx]
    if depth > 0:
        cp_split = subdivide_bezier(cp)
        u = [u0, (u0 + u1) / F(2.0), u1]
        cps = np.zeros(n, np.int64)
        running = np.ones(n, bool)     # False once the ray has `return`ed (shadow rays)
        ar = np.arange(n)
        for seg in range(2):
            c4 = cp_split[ar[:, None], cps[:, None] + np.arange(4)[None, :]]
            max_width = pmax(lerp(u[seg], w0, w1), lerp(u[seg + 1], w0, w1))
            go = running & ~_box_culled(c4, max_width, z_max)          # the others `continue`
            sub = _recursive_intersect(cx, idx[go], c4[go], u[seg][go], u[seg + 1][go], depth - 1, shadow)
            res[go] = sub                                               # `hit = self.recursive_intersect(..)`: unconditional
            if shadow:
                returned = np.zeros(n, bool); returned[go] = sub[:, 0] != 0
                running &= ~returned
            cps = np.where(go, cps + 3, cps)                            # `cps += 3` is not reached after a `continue`
        return res

    # the leaf (:437-535)
    c0, c1, c2, c3 = cp[:, 0], cp[:, 1], cp[:, 2], cp[:, 3]
    ok = np.ones(n, bool)
    edge = (c1[:, 1] - c0[:, 1]) * -c0[:, 1] + c0[:, 0] * (c0[:, 0] - c1[:, 0])
    ok &= ~(edge < F(0))
    edge = (c2[:, 1] - c3[:, 1]) * -c3[:, 1] + c3[:, 0] * (c3[:, 0] - c2[:, 0])
    ok &= ~(edge < F(0))
    sdx, sdy = c3[:, 0] - c0[:, 0], c3[:, 1] - c0[:, 1]
    denom = sdx * sdx + sdy * sdy
    ok &= ~(denom == F(0))
    w = (-c0[:, 0] * sdx + -c0[:, 1] * sdy) / denom
    uu = clamp(lerp(w, u0, u1), u0, u1)
    hit_width = lerp(uu, w0, w1)
    ribbon = cx.type[idx] == RIBBON
    ray_d, ray_length = cx.d[idx], cx.ray_length[idx]
    sin0 = sin64((F(1) - uu) * cx.normal_angle[idx]) * cx.inv_sin[idx]
    sin1 = sin64(uu * cx.normal_angle[idx]) * cx.inv_sin[idx]
    n_hit = np.where(ribbon[:, None], sin0[:, None] * cx.n0[idx] + sin1[:, None] * cx.n1[idx], F(0)).astype(np.float32)
    hit_width = np.where(ribbon, hit_width * (pabs(dot(n_hit, ray_d)) / ray_length), hit_width)
    pc, dpcdw = eval_bezier(cp, clamp(w, F(0), F(1)))
    pt_curve_dist2 = pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]
    ok &= ~(pt_curve_dist2 > hit_width * hit_width * F(0.25))
    ok &= ~((pc[:, 2] < F(0)) | (pc[:, 2] > z_max))
    pt_curve_dist = np.sqrt(pt_curve_dist2)
    edge_func = dpcdw[:, 0] * -pc[:, 1] + pc[:, 0] * dpcdw[:, 1]
    v = np.where(edge_func > F(0), F(0.5) + pt_curve_dist / hit_width, F(0.5) - pt_curve_dist / hit_width)
    t_hit = pc[:, 2] / ray_length
    p_error = F(2.0) * hit_width
    _, dpdu = eval_bezier(cx.cp_common[idx], uu)
    ok &= ~((dpdu[:, 0] == F(0)) & (dpdu[:, 1] == F(0)) & (dpdu[:, 2] == F(0)))      # assert!(dpdu != 0): the reference panics; a miss (module docstring)
    dpdv_ribbon = normalize(cross(n_hit, dpdu)) * hit_width[:, None]
    o2r, r2o = cx.o2r[idx], cx.r2o[idx]
    dpdu_plane = transform_vector(o2r, dpdu)                                          # ray_to_object.inverse()
    dpdv_plane = normalize(np.stack([-dpdu_plane[:, 1], dpdu_plane[:, 0], np.zeros(n, np.float32)], axis=-1)) * hit_width[:, None]
    theta = lerp(v, F(-90.0), F(90.0))
    rot = rotate_axis_matrix(-theta, dpdu_plane)
    dpdv_plane = np.where((cx.type[idx] == CYLINDER)[:, None], transform_vector(rot, dpdv_plane), dpdv_plane)
    dpdv = np.where(ribbon[:, None], dpdv_ribbon, transform_vector(r2o, dpdv_plane))
    p = cx.o[idx] + ray_d * t_hit[:, None]                                            # ray.at(t_hit), the object-space ray
    # SurfaceInteraction::new (surface_interaction.rs:69-98), then object_to_world.transform_surface_interaction (transform.rs:566-590)
    nn = normalize(cross(dpdu, dpdv))
    nn = np.where(cx.flip[idx][:, None], nn * F(-1.0), nn)
    m, mi = cx.o2w[idx], cx.w2o[idx]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rows = []
    errs = []
    for r in range(4):
        rows.append((m[:, r, 0] * x + m[:, r, 1] * y) + (m[:, r, 2] * z + m[:, r, 3]))
    for r in range(3):
        errs.append((_GAMMA3 + F(1)) * (pabs(m[:, r, 0]) * p_error + pabs(m[:, r, 1]) * p_error + pabs(m[:, r, 2]) * p_error)
                    + _GAMMA3 * (pabs(m[:, r, 0] * x) + pabs(m[:, r, 1] * y) + pabs(m[:, r, 2] * z) + pabs(m[:, r, 3])))
    q = np.stack(rows[:3], axis=-1)
    pw = np.where((rows[3] == F(1))[:, None], q, div3(q, rows[3]))
    res[:, 0] = 1.0
    res[:, 1] = t_hit; res[:, 2] = uu; res[:, 3] = v
    res[:, 4:7] = pw; res[:, 7:10] = np.stack(errs, axis=-1)
    res[:, 10:13] = transform_vector(m, dpdu); res[:, 13:16] = transform_vector(m, dpdv)
    res[:, 16:19] = normalize(transform_normal(mi, nn))
    res[~ok] = 0.0
    return res


def intersect(seg, o, d, t_max, shadow=False):
    """Curve::intersect(r, is_shadow_ray) for N rays.  `seg`: dict of per-ray arrays (or arrays that broadcast to N): cp_obj (4,3), width (2,), n (2,3), normal_angle,
    inv_sin_normal_angle, type, u_min, u_max, o2w (4,4), w2o (4,4), flip.  Returns (N, STRIDE); rows of a miss are zero."""
    o = _f(o).reshape(-1, 3); d = _f(d).reshape(-1, 3); t_max = _f(t_max).reshape(-1)
    n = len(o)

    def bc(key, shape, dtype=np.float32):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(seg[key], dtype=dtype), (n,) + shape))
    with np.errstate(all="ignore"):
        cx = _Ctx()
        cx.cp_common = bc("cp_obj", (4, 3)); width = bc("width", (2,)); nrm = bc("n", (2, 3))
        cx.w0, cx.w1 = width[:, 0].copy(), width[:, 1].copy(); cx.n0, cx.n1 = nrm[:, 0].copy(), nrm[:, 1].copy()
        cx.normal_angle = bc("normal_angle", ()); cx.inv_sin = bc("inv_sin_normal_angle", ()); cx.type = bc("type", (), np.int64)
        u_min, u_max = bc("u_min", ()), bc("u_max", ())
        cx.o2w, cx.w2o, cx.flip = bc("o2w", (4, 4)), bc("w2o", (4, 4)), bc("flip", (), bool)
        # :546-583
        cx.o, cx.d = transform_ray_with_error(cx.w2o, o, d)
        cp_obj = segment_cp(cx.cp_common, u_min, u_max)
        dx = cross(cx.d, cp_obj[:, 3] - cp_obj[:, 0])
        dx = np.where((length_squared(dx) == F(0))[:, None], coordinate_system(cx.d), dx)
        cx.o2r, cx.r2o, panics = look_at(cx.o, cx.o + cx.d, dx)
        cp = np.stack([transform_point(cx.o2r, cp_obj[:, k]) for k in range(4)], axis=1)
        # :588-612
        max_width = pmax(lerp(u_min, cx.w0, cx.w1), lerp(u_max, cx.w0, cx.w1))
        cx.ray_length = length(cx.d)
        cx.z_max = cx.ray_length * t_max
        alive = ~panics & ~_box_culled(cp, max_width, cx.z_max)
        # :614-632
        l0 = np.zeros(n, np.float32)
        for i in range(2):
            l0 = pmax(l0, pmax(pmax(pabs(cp[:, i, 0] - F(2.0) * cp[:, i + 1, 0] + cp[:, i + 2, 0]), pabs(cp[:, i, 1] - F(2.0) * cp[:, i + 1, 1] + cp[:, i + 2, 1])),
                               pabs(cp[:, i, 2] - F(2.0) * cp[:, i + 1, 2] + cp[:, i + 2, 2])))
        eps = pmax(cx.w0, cx.w1) * F(0.05)
        depth = max_depth_of(l0, eps)
        out = np.zeros((n, STRIDE), np.float32)
        for dep in range(11):
            idx = np.nonzero(alive & (depth == dep))[0]
            if len(idx):
                out[idx] = _recursive_intersect(cx, idx, cp[idx], u_min[idx], u_max[idx], dep, shadow)
    return out


def intersect_p(seg, o, d, t_max):
    return intersect(seg, o, d, t_max, shadow=True)[:, 0] != 0


def segment(cd, u_min, u_max, o2w=None, w2o=None, reverse_orientation=False):
    """The per-ray parameter dict of one Curve (:75-93)"""
    o2w = np.eye(4, dtype=np.float32) if o2w is None else _f(o2w).reshape(4, 4)
    w2o = np.eye(4, dtype=np.float32) if w2o is None else _f(w2o).reshape(4, 4)
    return dict(cp_obj=cd["cp_obj"], width=cd["width"], n=cd["n"], normal_angle=cd["normal_angle"], inv_sin_normal_angle=cd["inv_sin_normal_angle"], type=cd["type"],
                u_min=F(u_min), u_max=F(u_max), o2w=o2w, w2o=w2o, flip=bool(reverse_orientation) != swaps_handedness(o2w))


def stack_segments(segs, counts):
    """One parameter dict for sum(counts) rays: segs[k] repeated counts[k] times"""
    return {key: np.concatenate([np.broadcast_to(np.asarray(s[key]), (c,) + np.asarray(s[key]).shape) for s, c in zip(segs, counts)]) for key in segs[0]}


# ---- Curve::from_props (:149-316) ------------------------------------------------------------------------------------------------------------------------------
class CurvePanic(Exception):
    pass


def from_props(P, width=1.0, width0=None, width1=None, degree=3, basis="bezier", curve_type="flat", N=None, splitdepth=3):
    """Returns (list of dict(cp (4,3), width (2,), n (2,3) or None, type, split_depth), warnings).  Raises CurvePanic where the reference panics."""
    warnings = []
    width0 = F(width if width0 is None else width0); width1 = F(width if width1 is None else width1)
    if degree not in (2, 3):
        raise CurvePanic(f"Invalid degree {degree}: only degree 2 and 3 curves are supported.")
    if basis not in ("bezier", "bspline"):
        raise CurvePanic(f"Invalid basis '{basis}': only ''bezier' and 'bspline' are supported.")
    cp = _f(P).reshape(-1, 3)
    ncp = len(cp)
    if basis == "bezier":
        if ncp < degree + 1 or ((ncp - 1 - degree) % degree) != 0:
            raise CurvePanic(f"Invalid number of control points {ncp}")
        n_segments = (ncp - 1) // degree
    else:
        if ncp < degree + 1:
            raise CurvePanic(f"Invalid number of control points {ncp}")
        n_segments = ncp - degree
    if curve_type in TYPES:
        t = TYPES[curve_type]
    else:
        warnings.append(f"Unknown curve type '{curve_type}'.  Using 'cylinder'.")
        t = CYLINDER
    n = None if N is None else _f(N).reshape(-1, 3)
    if n is not None and len(n) > 0:
        if t != RIBBON:
            warnings.append("Curve normals are only used with 'ribbon' type curves.")
            n = None
        elif len(n) != n_segments + 1:
            raise CurvePanic(f"Invalid number of normals {len(n)}")
    elif t == RIBBON:
        raise CurvePanic("Must provide normals 'N' at curve endpoints with ribbon curves.")
    else:
        n = None
    sd = int(splitdepth)
    out = []
    base = 0
    third, two_thirds = F(1.0) / F(3.0), F(2.0) / F(3.0)
    for seg in range(n_segments):
        if basis == "bezier":
            if degree == 2:
                b = [cp[base], lerp3(two_thirds, cp[base], cp[base + 1]), lerp3(third, cp[base + 1], cp[base + 2]), cp[base + 2]]
            else:
                b = [cp[base + i] for i in range(4)]
            base += degree
        else:
            if degree == 2:
                p01, p12, p23 = cp[base], cp[base + 1], cp[base + 2]
                p11 = lerp3(F(0.5), p01, p12); p22 = lerp3(F(0.5), p12, p23)
                b = [p11, lerp3(two_thirds, p11, p12), lerp3(third, p12, p22), p22]
            else:
                p012, p123, p234, p345 = cp[base], cp[base + 1], cp[base + 2], cp[base + 3]
                p122 = lerp3(two_thirds, p012, p123); p223 = lerp3(third, p123, p234); p233 = lerp3(two_thirds, p123, p234); p334 = lerp3(third, p234, p345)
                b = [lerp3(F(0.5), p122, p223), p223, p233, lerp3(F(0.5), p233, p334)]
            base += 1
        w = [lerp(F(seg) / F(n_segments), width0, width1), lerp(F(seg + 1) / F(n_segments), width0, width1)]
        out.append(dict(cp=np.stack(b).astype(np.float32), width=_f(w), n=None if n is None else n[seg:seg + 2], type=t, split_depth=sd))
    return out, warnings
