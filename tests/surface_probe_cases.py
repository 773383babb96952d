"""Case generators for the surface probe (surface_probe_batch), shared by the CPU test that measures what the cases reach on the oracle and checks the oracle against a
float64 restatement, and the GPU test that compares the device with the oracle bit for bit.

One tiny scene per set, captured into either backend by `SurfaceSet.capture` — tens of triangles, a 16 x 16 film, a camera and a Halton sampler, the accelerator built.  A
set's cases are batches {op, prim (n,), inst (n,), b (n,3), t (n,), rays (n,) RAY_DTYPE, aux (n,48), texture, camera_ray, camera, tag}: a deterministic edge list followed by a
seeded random fill.  A hit record is made per backend: `learn_templates` obtains one real hit per (primitive, instance) from intersect_batch — which is where pad[0] and pad[1]
come from — and `hits_of` overwrites t, b0, b1, b2 with the batch's.  Everything is float32 from the start, so that both sides receive the same bits.

The oracle's word 39 of every record is the probe's branch mask; BITS below names one bit per line."""
import math

import numpy as np

import pbrt_hip
import sphere_light_scenes as SL
from probe_cases import F, dn, hexf, up

STRIDE, AUX, MASK = 40, 48, 39
TIME = F(0.25)

# ---------------------------------------------------------------- the branch mask (oracle/oracle_capi.cpp: ORC_SB_*) -------------------------------------------------
BITS = dict(
    UV_DEGENERATE=1 << 0,       # |uv determinant| < 1e-8: dpdu, dpdv from coordinate_system(n)
    DPDU_CROSS_ZERO=1 << 1,     # determinant fine but dpdu x dpdv == 0: the same fallback
    N_ZERO=1 << 2,              # interpolated N of zero length: ns = n
    S_ZERO=1 << 3,              # interpolated S of zero length: ss = normalize(dpdu)
    TS_ZERO=1 << 4,             # S parallel to the interpolated N: coordinate_system(ns)
    FLIP_N=1 << 5,              # reverse_orientation != swaps_handedness: n negated
    REV_TS=1 << 6,              # reverse_orientation: ts negated
    FACE_FORWARD=1 << 7,        # set_shading_geometry's face_forward turned n
    INST_IDENTITY=1 << 8,       # an instance under the identity: transform_surface_interaction skipped
    INST_TRANSFORM=1 << 9,      # any other instance: the interaction carried to world space
    INST_NS_FLIP=1 << 10,       # face_forward(ns, n) after the instance transform turned ns
    WO_ZERO=1 << 11,            # a ray direction of length 0: wo stays as given
    TX_EARLY_OUT=1 << 12,       # tx or ty infinite or NaN: all differentials zero
    DIFF_DET_SMALL=1 << 13,     # |det| < 1e-10 in compute_differentials' 2 x 2 solve
    AXIS_X=1 << 14,             # compute_differentials drops x (|n.x| strictly largest)
    AXIS_Y=1 << 15,             # ... drops y
    AXIS_Z=1 << 16,             # ... drops z (the fall-through: every tie ends here or at y)
    OFFSET_ZERO=1 << 17,        # a zero component of offset_origin's offset: the coordinate stays
    OFFSET_NEG=1 << 18,         # dot(w, n) < 0: offset_origin negates the offset
    DN_UV_DEGENERATE=1 << 19,   # dn/du, dn/dv from coordinate_system(dn) under a degenerate uv determinant
    DN_ZERO=1 << 20,            # ... with dn == 0: dn/du = dn/dv = 0
    BUMP_DU_DEFAULT=1 << 21,    # Material::bump's du or dv == 0 -> 0.0005
    SPEC_FLIP=1 << 22,          # specular_transmit with dot(wo, ns) < 0: eta inverted, normal and derivatives negated
    SPEC_TRANSMIT=1 << 23,      # the refracted ray's differentials
    SPEC_REFLECT=1 << 24,       # the reflected ray's differentials
    QUADRIC=1 << 25,            # the hit lies on a quadric shape
    CAMERA_LENS=1 << 26,        # the camera's differentials come through a lens sample
    DIFF_SOLVED=1 << 27,        # compute_differentials ran to its end and solved both systems
)
ALL_BITS = 0
for _v in BITS.values():
    ALL_BITS |= _v


def bits_of(outs):
    m = 0
    for o in outs:
        m |= int(np.bitwise_or.reduce(o[:, MASK].view(np.uint32))) if len(o) else 0
    return m


def bit_names(mask):
    return [k for k, v in BITS.items() if mask & v]


# ---------------------------------------------------------------- scene building ---------------------------------------------------------------------------------------
CAM_EYE, CAM_LOOK, CAM_UP = (0.5, 0.4, 9.0), (0.5, 0.4, 0.0), (0.0, 1.0, 0.0)
RES = 16
# name -> (kind, lens_radius, focal_distance, spp, eye, look, up)
CAMERAS = {
    "pinhole": ("perspective", 0.0, 1e6, 4, CAM_EYE, CAM_LOOK, CAM_UP),
    "pinhole_spp1": ("perspective", 0.0, 1e6, 1, CAM_EYE, CAM_LOOK, CAM_UP),
    "pinhole_spp16": ("perspective", 0.0, 1e6, 16, CAM_EYE, CAM_LOOK, CAM_UP),
    "thinlens_spp1": ("perspective", 0.3, 8.5, 1, CAM_EYE, CAM_LOOK, CAM_UP),
    "thinlens_spp16": ("perspective", 0.3, 8.5, 16, CAM_EYE, CAM_LOOK, CAM_UP),
    "ortho_spp1": ("orthographic", 0.0, 1e6, 1, CAM_EYE, CAM_LOOK, CAM_UP),
    "ortho_spp16": ("orthographic", 0.0, 1e6, 16, CAM_EYE, CAM_LOOK, CAM_UP),
    "ortho_lens_spp1": ("orthographic", 0.2, 8.0, 1, CAM_EYE, CAM_LOOK, CAM_UP),
    "ortho_lens_spp16": ("orthographic", 0.2, 8.0, 16, CAM_EYE, CAM_LOOK, CAM_UP),
    "environment_spp1": ("environment", 0.0, 1e6, 1, (0.5, 0.4, 3.0), (0.5, 0.4, 0.0), CAM_UP),
    "environment_spp16": ("environment", 0.0, 1e6, 16, (0.5, 0.4, 3.0), (0.5, 0.4, 0.0), CAM_UP),
    # looks along +x with z up: its rays' direction lies in every plane z = const, where dot(n, rx_direction) is an exact zero
    "ortho_along_x": ("orthographic", 0.0, 1e6, 1, (-5.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
}


def apply_camera(s, host, name):
    kind, lens_radius, focal, spp, eye, look, upv = CAMERAS[name]
    w2c, c2w = host.look_at(eye, look, upv)
    if kind == "perspective":
        s.set_camera_perspective(host.perspective_raster_to_camera(40.0, RES, RES), c2w, lens_radius=lens_radius, focal_distance=focal)
    elif kind == "orthographic":
        s.set_camera_orthographic(host.orthographic_raster_to_camera(RES, RES), c2w, lens_radius=lens_radius, focal_distance=focal)
    else:
        s.set_camera_environment(c2w, RES, RES)
    cb, table, sb = host.film_box(RES, RES)
    s.set_film(RES, RES, cb, (0.5, 0.5), table)
    s.set_sampler(0, spp, sb)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def rot_about(v, axis, deg):
    """v rotated about `axis` by `deg` degrees (Rodrigues), float64"""
    v = np.asarray(v, np.float64); k = unit(axis); a = math.radians(deg)
    return v * math.cos(a) + np.cross(k, v) * math.sin(a) + k * np.dot(k, v) * (1.0 - math.cos(a))


class Geo:
    """Records what is added to a scene, in primitive order: tris[prim] = dict(P (3,3), N, S, UV (or None), rev, swp, obj), instances[k] = (object, i2w (4,4) float32),
    targets = the (prim, inst) pairs a probe may name.  The same calls build either backend."""

    def __init__(self, s, host):
        self.s, self.host = s, host
        self.tris, self.instances, self.targets, self.quadrics = [], [], [], {}
        self.mat = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        self.obj = None
        # the displacement textures of op 2: constant 0, constant 1, uv, a scaled bilerp
        self.tex = dict(zero=s.add_texture_constant(0.0), one=s.add_texture_constant(1.0), uv=s.add_texture_uv(1.0, 1.0, 0.0, 0.0))
        self.tex["bilerp"] = s.add_texture_scale(s.add_texture_bilerp(0.1, 0.9, 0.4, 0.2, 3.0, 2.0, 0.25, 0.5), s.add_texture_constant(2.5))

    def mesh(self, P, N=None, S=None, UV=None, rev=False, swp=False, idx=None, name=""):
        P = np.ascontiguousarray(P, F).reshape(-1, 3)
        idx = np.arange(len(P), dtype=np.uint32) if idx is None else np.asarray(idx, np.uint32)
        f = lambda a, k: None if a is None else np.ascontiguousarray(a, F).reshape(-1, k)
        N, S, UV = f(N, 3), f(S, 3), f(UV, 2)
        base = len(self.tris)
        self.s.add_mesh(P, idx, self.mat, N=N, S=S, UV=UV, reverse_orientation=rev, swaps_handedness=swp)
        for t in range(len(idx) // 3):
            i = idx[3 * t:3 * t + 3]
            g = lambda a: None if a is None else a[i].copy()
            self.tris.append(dict(P=P[i].copy(), N=g(N), S=g(S), UV=g(UV), rev=rev, swp=swp, obj=self.obj, name=name))
            if self.obj is None:
                self.targets.append((base + t, 0))
        return list(range(base, base + len(idx) // 3))

    def object_begin(self):
        self.obj = self.s.object_begin()
        return self.obj

    def object_end(self):
        self.s.object_end(); self.obj = None

    def instance(self, obj, xf):
        self.s.add_instance(obj, xf[0], xf[1])
        self.instances.append((obj, np.asarray(xf[0], F).reshape(4, 4).copy()))
        k = len(self.instances)
        for p, t in enumerate(self.tris):
            if t["obj"] == obj:
                self.targets.append((p, k))
        return k

    def quadric_slot(self, name):
        """a quadric takes one slot of the primitive list"""
        self.quadrics[name] = len(self.tris)
        self.tris.append(dict(P=None, N=None, S=None, UV=None, rev=False, swp=False, obj=None, name=name))
        return self.quadrics[name]

    def world_verts(self, prim, inst):
        """float64 images of the triangle's float32 vertices under the instance's float32 matrix"""
        P = self.tris[prim]["P"].astype(np.float64)
        if inst:
            m = self.instances[inst - 1][1].astype(np.float64)
            P = P @ m[:3, :3].T + m[:3, 3]
        return P


# the four triangles every flags mesh holds: one in the plane z = 0, three tilted; three vertices each, nothing shared
BASE_TRIS = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]],
                      [[1, 0, 0], [1.1, 1, 0.3], [0.1, 1.2, 0]],
                      [[0, 0, 0], [0, 1, 0], [-0.7, 0.4, 0.5]],
                      [[0, 0, 0], [0.2, -0.9, 0.1], [1, 0, 0]]], np.float64)
BASE_UV = np.array([[[0.1, 0.2], [0.9, 0.15], [0.2, 0.8]], [[0, 0], [2, 0.5], [0.5, 1.5]], [[0.3, 0.3], [0.35, 0.9], [-0.4, 0.5]], [[1, 1], [0.2, 0.7], [0.4, 0.1]]], np.float64)


def base_normals():
    """Per-vertex N for BASE_TRIS: the geometric normal (of dp02 x dp12) tilted by 20 .. 40 degrees about an in-plane axis, a different angle per vertex, not unit length; in
    triangles 1 and 3 on the opposite side, so that face_forward turns n.  S: an in-plane direction mixed with a little of the normal."""
    N, S = np.zeros((4, 3, 3)), np.zeros((4, 3, 3))
    for t in range(4):
        p0, p1, p2 = BASE_TRIS[t]
        ng = unit(np.cross(p0 - p2, p1 - p2))
        e = unit(p1 - p0)
        for v, deg in enumerate((20.0, 30.0, 40.0)):
            n = rot_about(ng, rot_about(e, ng, 50.0 * v), deg) * (1.0 + 0.3 * v)
            N[t, v] = -n if t in (1, 3) else n
            S[t, v] = rot_about(e, ng, 25.0 * v + 10.0 * t) * (0.7 + 0.2 * v) + 0.15 * ng
    return N, S


def add_flags_mesh(g, origin, flags, name=""):
    """flags = (N, S, UV, reverse_orientation, swaps_handedness)"""
    N, S = base_normals()
    has_n, has_s, has_uv, rev, swp = flags
    P = (BASE_TRIS + np.asarray(origin, np.float64)).reshape(-1, 3)
    return g.mesh(P, N=N if has_n else None, S=S if has_s else None, UV=BASE_UV if has_uv else None, rev=rev, swp=swp, name=name or f"flags{flags}")


def all_flags():
    return [tuple(bool(k >> j & 1) for j in range(5)) for k in range(32)]


def build_flags32(g, origin=(0.25, 0.5, 0.75)):   # off the coordinate planes: no p_error component is an exact zero here
    for k, fl in enumerate(all_flags()):
        add_flags_mesh(g, np.asarray(origin) + [3.0 * (k % 8), 3.0 * (k // 8), 0.0], fl)


TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)   # geometric normal of dp02 x dp12: +z
UV_OK = np.array([[0, 0], [1, 0], [0, 1]], np.float64)
N_OK = np.array([[0.2, 0.1, 1], [-0.1, 0.3, 1], [0.1, -0.2, 1]], np.float64)


def det_edge_uvs():
    """UV triangles (0,0), (a,0), (0,a) whose float32 determinant a * a is the nearest float32 below and the first at or above 1e-8"""
    lim = F(1e-8)
    a = F(math.sqrt(1e-8))
    while a * a >= lim:
        a = dn(a)
    below = a
    above = up(a)
    assert below * below < lim <= above * above
    return [np.array([[0, 0], [x, 0], [0, x]], F) for x in (below, above)]


def build_degenerate(g, origin=(0.0, 0.0, 0.0)):
    """one triangle per case, side by side; returns {name: prim}"""
    o = np.asarray(origin, np.float64)
    out = {}
    k = [0]

    def add(name, **kw):
        P = TRI + o + [2.0 * (k[0] % 8), 2.0 * (k[0] // 8), 0.0]; k[0] += 1
        out[name] = g.mesh(P, name=name, **kw)[0]

    below, above = det_edge_uvs()
    denorm = np.array([[1e-40, 0, 1e-39], [0, 1e-41, 1e-39], [1e-42, 1e-42, 1e-39]], F)
    add("uv_all_equal", UV=[[0.3, 0.7]] * 3, N=N_OK)
    add("uv_collinear", UV=[[0, 0], [0.5, 0.5], [1, 1]], N=N_OK, S=[[1, 0, 0.2]] * 3)
    add("uv_det_below_1e-8", UV=below, N=N_OK)
    add("uv_det_above_1e-8", UV=above, N=N_OK)
    add("uv_1e6", UV=UV_OK * 1e6, N=N_OK)             # dpdu ~ 1e-6 long: compute_differentials' determinant ~ 1e-12 < 1e-10
    add("uv_1e12", UV=UV_OK * 1e12)                   # dpdu ~ 1e-12 long: dpdu x dpdv underflows to zero
    add("n_opposed", N=[[0, 0, 1], [0, 0, -1], [0.3, 0, 1]], UV=UV_OK)     # b = (0.5, 0.5, 0): N interpolates to zero
    add("s_opposed", S=[[1, 0, 0], [-1, 0, 0], [0, 1, 0]], N=N_OK, UV=UV_OK)
    add("s_opposed_no_n", S=[[1, 0, 0], [-1, 0, 0], [0, 1, 0]])
    add("s_parallel_n", N=[[0.2, 0.1, 1]] * 3, S=[[0.4, 0.2, 2]] * 3, UV=UV_OK)   # S = 2 N: ts of length 0
    add("n_len_1e-3", N=N_OK * 1e-3, UV=UV_OK)
    add("n_len_1e3", N=N_OK * 1e3, UV=UV_OK)
    add("n_denormal", N=denorm, UV=UV_OK)
    add("n_all_equal", N=[[0.2, 0.1, 1]] * 3, UV=UV_OK)                    # dn1 = dn2 = 0: dndu = dndv = 0 through the regular branch
    add("n_all_equal_uv_degenerate", N=[[0.2, 0.1, 1]] * 3, UV=[[0.3, 0.7]] * 3)   # dn = 0 under a degenerate determinant: both stay zero
    add("n_uv_degenerate", N=N_OK, UV=[[0, 0], [0.5, 0.5], [1, 1]])        # coordinate_system(dn, ..)
    add("n_uv_degenerate_rev", N=N_OK, UV=[[0.3, 0.7]] * 3, rev=True, S=[[1, 0.5, 0]] * 3)
    return out


def instance_transforms(host):
    rot = host.rotate(37.0, (1.0, 2.0, 3.0))
    sc = host.scale((3.0, 0.25, 1.0))
    mir = host.scale((-1.0, 1.0, 1.0))
    comp = host.compose(host.translate((40.0, -3.0, 2.0)), host.compose(rot, host.compose(mir, sc)))
    return [("identity", (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY)), ("translate_1e4", host.translate((1e4, 0.0, 0.0))),
            ("rotate", host.compose(host.translate((0.0, 20.0, 0.0)), rot)), ("scale", host.compose(host.translate((0.0, 40.0, 0.0)), sc)),
            ("mirror", host.compose(host.translate((0.0, 60.0, 0.0)), mir)), ("composition", comp)]


def build_instances(g, origin=(0.0, 0.0, 0.0)):
    """The N + S + UV flags mesh — and its reverse_orientation twin — plus one triangle whose N leans 40 degrees across y (under the scale (3, 0.25, 1) its image and the
    geometric normal's end up on opposite sides: face_forward(ns, n) turns it), in an object instanced six times."""
    obj = g.object_begin()
    add_flags_mesh(g, origin, (True, True, True, False, False), name="inst_nsuv")
    add_flags_mesh(g, np.asarray(origin) + [3.0, 0.0, 0.0], (True, True, True, True, False), name="inst_nsuv_rev")
    ng = np.array([0.0, math.sin(math.radians(20.0)), math.cos(math.radians(20.0))])
    e = np.array([1.0, 0.0, 0.0]); f = np.cross(ng, e)
    P = np.array([[0, 0, 0], e, f]) + np.asarray(origin) + [6.0, 0.0, 0.0]
    lean = np.array([0.0, -math.sin(math.radians(20.0)), math.cos(math.radians(20.0))])
    g.mesh(P, N=[lean] * 3, UV=UV_OK, name="inst_lean")
    g.object_end()
    return [g.instance(obj, xf) for _, xf in instance_transforms(g.host)]


# ---------------------------------------------------------------- hits and batches -------------------------------------------------------------------------------------
def learn_templates(scene, g):
    """{(prim, inst): a HIT_DTYPE record of a real hit on it}, from intersect_batch: rays at the triangle's centroid along its normal, from either side, three distances and two direction lengths;
    the first that reports this primitive and this instance is kept."""
    want, rays = [], []
    for prim, inst in g.targets:
        if g.tris[prim]["P"] is None:
            continue
        P = g.world_verts(prim, inst)
        c = P.mean(axis=0); n = np.cross(P[1] - P[0], P[2] - P[0])
        edge = min(np.linalg.norm(P[1] - P[0]), np.linalg.norm(P[2] - P[1]), np.linalg.norm(P[0] - P[2]))
        n = n / np.linalg.norm(n)
        for sgn in (1.0, -1.0):
            for L in (0.3 * edge, 0.03 * edge, 3.0 * edge):
                L = max(L, 64.0 * float(np.spacing(F(np.abs(c).max()))))
                for k in (1.0, 1000.0):   # (Triangle::intersect's error bound on t grows with the square of the ray parameter: a very small triangle is met only at a small t)
                    r = np.zeros(1, pbrt_hip.RAY_DTYPE)
                    r["o"] = (c + sgn * L * n).astype(F); r["d"] = (-sgn * L * k * n).astype(F); r["t_max"] = np.inf
                    rays.append(r); want.append((prim, inst))
    rays = np.concatenate(rays)
    hits = scene.intersect_batch(rays)
    out = {}
    for (prim, inst), h in zip(want, hits):
        if (prim, inst) not in out and h["prim"] == prim and h["pad"][1] == inst:
            out[(prim, inst)] = h.copy()
    missing = [t for t in g.targets if g.tris[t[0]]["P"] is not None and t not in out]
    assert not missing, f"no ray of learn_templates reached {missing}"
    return out


def hits_of(templates, b):
    """the batch's hit records on the backend `templates` came from"""
    if "hits" in b:   # real hits (quadrics, curve segments): taken as intersect_batch gave them on this backend
        return templates["real"][b["hits"]]
    h = np.zeros(len(b["prim"]), pbrt_hip.HIT_DTYPE)
    for i, key in enumerate(zip(b["prim"].tolist(), b["inst"].tolist())):
        h[i] = templates[key]
    h["t"] = b["t"]; h["b0"] = b["b"][:, 0]; h["b1"] = b["b"][:, 1]; h["b2"] = b["b"][:, 2]
    return h


def default_aux(n, rng):
    a = np.zeros((n, AUX), F)
    a[:, 0:2] = (rng.random((n, 2)) * RES).astype(F)
    a[:, 2:4] = rng.random((n, 2)).astype(F)
    v = rng.normal(size=(n, 3)); a[:, 4:7] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    a[:, 7:10] = rng.normal(size=(n, 3)).astype(F) * F(3)
    a[:, 10:13] = np.abs(rng.normal(size=(n, 3))).astype(F) * F(1e-5)
    v = rng.normal(size=(n, 3)); a[:, 13:16] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    return a


def rays_through(g, prim, inst, b, d):
    """rays with direction d[i] that pass through the point b[i] of (prim[i], inst[i]) at t = 1, t_max = inf"""
    n = len(prim)
    r = np.zeros(n, pbrt_hip.RAY_DTYPE)
    for i in range(n):
        P = g.world_verts(int(prim[i]), int(inst[i]))
        p = b[i].astype(np.float64) @ P
        with np.errstate(invalid="ignore", over="ignore"):
            r["o"][i] = (p - np.nan_to_num(d[i].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)).astype(F)
    r["d"] = d; r["t_max"] = np.inf; r["time"] = TIME
    return r


def batch(g, op, prim, inst, b, d, rng, tag, aux=None, texture=0, camera_ray=False, camera="pinhole"):
    prim = np.asarray(prim, np.int64).reshape(-1); n = len(prim)
    inst = np.broadcast_to(np.asarray(inst, np.int64), (n,)).copy()
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(b, F), (n, 3)))
    d = np.ascontiguousarray(np.broadcast_to(np.asarray(d, F), (n, 3)))
    aux = default_aux(n, rng) if aux is None else np.ascontiguousarray(aux, F).reshape(n, AUX)
    return dict(op=op, prim=prim, inst=inst, b=b, t=np.ones(n, F), rays=rays_through(g, prim, inst, b, d), aux=aux, texture=texture, camera_ray=camera_ray, camera=camera, tag=tag)


def run_batches(scene, host, templates, batches, variant=1):
    out, cam = [], None
    for b in batches:
        if b["camera"] != cam:
            cam = b["camera"]; apply_camera(scene, host, cam)
        out.append(scene.surface_probe_batch(b["op"], b["rays"], hits_of(templates, b), b["aux"], variant=b.get("variant", variant), texture=b["texture"], camera_ray=b["camera_ray"]))
    return out


def describe(set_name, b, i):
    return (f"set {set_name} ({b['tag']}) op {b['op']} probe {i}: prim {int(b['prim'][i]) if 'prim' in b else '?'} inst {int(b['inst'][i]) if 'inst' in b else 0} "
            f"b {hexf(b['b'][i]) if 'b' in b else ''} ray o {hexf(b['rays']['o'][i])} d {hexf(b['rays']['d'][i])} camera {b['camera']} camera_ray {b['camera_ray']} aux {hexf(b['aux'][i][:16])}")


def random_b(rng, n):
    b = rng.dirichlet((1.0, 1.0, 1.0), size=n).astype(F)
    b[:, 2] = F(1) - b[:, 0] - b[:, 1]
    return b


def random_d(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(F)


CENTROID = np.array([1, 1, 1], F) / F(3)
B_EDGES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [F(1) / F(3), F(1) / F(3), F(1) - F(1) / F(3) - F(1) / F(3)],
                    [1e-30, 0.5, 0.5], [0.25, 1e-40, 0.75], [-0.0, 0.5, 0.5], [0.5, -0.0, 0.5], [0.25, 0.75, -0.0], [0.25, 0.25, up(F(0.5))], [0.25, 0.25, dn(F(0.5))],
                    [up(F(0.3)), 0.2, 0.5], [dn(F(0.3)), 0.2, 0.5], [0.7, up(F(0.3)), 0.0], [1.0, 1e-30, 1e-30]], F)


def edge_then_random(g, op, targets, rng, tag, n_random, b_edges=B_EDGES, **kw):
    """every target at every edge barycentric triple with a fixed direction, then n_random random (target, b, d)"""
    targets = list(targets)
    pe = np.repeat(np.arange(len(targets)), len(b_edges)); be = np.tile(b_edges, (len(targets), 1))
    pr = rng.integers(0, len(targets), n_random)
    idx = np.concatenate([pe, pr])
    prim = np.array([targets[i][0] for i in idx]); inst = np.array([targets[i][1] for i in idx])
    b = np.concatenate([be, random_b(rng, n_random)])
    d = np.concatenate([np.tile(np.array([[0.3, -0.2, -1.0]], F), (len(pe), 1)), random_d(rng, n_random)])
    return batch(g, op, prim, inst, b, d, rng, tag, **kw)


# ---------------------------------------------------------------- the sets -----------------------------------------------------------------------------------------------
class SurfaceSet:
    """name; build(g): fills the scene through a Geo and returns what cases() needs; cases(orc, host, g, info, templates, rng): the batches; expect: the branch bits the set
    exists to reach; ops: the ops it exercises (each with at least 500 probes)."""

    def __init__(self, name, build, cases, expect, ops, variant=1):
        self.name, self.build, self._cases, self.expect, self.ops, self.variant = name, build, cases, expect, ops, variant

    def capture(self, s, host):
        def go(s, host):
            g = Geo(s, host)
            info = self.build(g)
            apply_camera(s, host, "pinhole")
            s.build_accel(0, 4)
            return g, info
        return SL.capture(go, s, host)   # the oracle's libm in mode 1 while it captures, as for every scene that may hold a sphere

    def cases(self, orc, host, g, info, templates, seed=0):
        return self._cases(orc, host, g, info, templates, np.random.default_rng(9000 + seed))


def oracle_op0(orc, host, templates, b):
    """the oracle's interaction of a batch's probes (p, p_error, n: what the spawn targets are placed around)"""
    b0 = dict(b); b0["op"] = 0; b0["camera_ray"] = False
    return run_batches(orc, host, templates, [b0])[0]


def _mask(names):
    m = 0
    for k in names:
        m |= BITS[k]
    return m


# ---- flags32
def _build_flags32(g):
    build_flags32(g)
    return {}


def _cases_flags32(orc, host, g, info, templates, rng):
    out = []
    for op, kw in ((0, {}), (1, dict(camera_ray=True)), (1, dict(camera_ray=False)), (3, {})):
        out.append(edge_then_random(g, op, g.targets, rng, f"all 32 flag combinations{' camera ray' if kw.get('camera_ray') else ''}", 640, b_edges=B_EDGES[[3, 6, 0]], **kw))
    return out


# ---- degenerate_frames
def _build_degenerate(g):
    return build_degenerate(g)


def _cases_degenerate(orc, host, g, info, templates, rng):
    out = []
    for op, kw in ((0, {}), (1, dict(camera_ray=True)), (1, dict(camera_ray=False))):
        out.append(edge_then_random(g, op, g.targets, rng, "degenerate frames" + (" camera ray" if kw.get("camera_ray") else ""), 400, b_edges=B_EDGES[[3, 6, 0, 1, 2, 4]], **kw))
    return out


# ---- barycentric_edges
def _build_barycentric(g):
    info = {}
    info["ordinary"] = g.mesh(np.array([[0.3, -0.2, 0.1], [1.4, 0.1, 0.6], [-0.1, 0.9, -0.4]]) + [0.0, 3.0, 0.0], N=N_OK, UV=UV_OK, name="ordinary")[0]
    info["sliver"] = g.mesh(np.array([[0, 0, 0], [1, 0, 0], [0.5, 1e-5, 0]]) + [4.0, 0.5, 0.25], UV=UV_OK, name="sliver")[0]   # aspect 1e5
    # float32 resolves 2^-10 at 1e4: the smallest triangle that exists there has edges of a few such steps (an edge of 1e-6 at that offset is three equal vertices)
    h = float(np.spacing(F(1e4)))
    info["tiny_far"] = g.mesh(np.array([[0, 0, 0], [2 * h, 0, 0], [0, 3 * h, 0]]) + [1e4, 1e4, 0.0], UV=UV_OK, name="tiny_far")[0]
    info["tiny"] = g.mesh(np.array([[0, 0, 0], [1e-6, 0, 0], [0, 1e-6, 0]]) + [0.0, -1e-3, 0.0], N=N_OK, name="tiny")[0]          # the 1e-6 edge itself, near the origin, where float32 resolves it
    info["huge"] = g.mesh(np.array([[-5e5, -3e5, 0], [5e5, -3e5, 0], [0, 6e5, 0]]) + [0.0, 0.0, -1e3], N=N_OK, UV=UV_OK, name="huge")[0]   # edges of ~1e6
    info["zero_coords"] = g.mesh(TRI, name="zero_coords")[0]   # in z = 0 with a vertex at the origin: coordinates, and so p_error components, that are exactly 0
    return info


def _cases_barycentric(orc, host, g, info, templates, rng):
    # zero_coords lies in z = 0 with a vertex at the origin: p_error.z = 0 everywhere, p_error = 0 at that vertex, and n = (0, 0, 1) makes the x, y offsets zero
    out = []
    for op in (0, 3):
        out.append(edge_then_random(g, op, g.targets, rng, "vertices, edges, centroid, tiny and signed-zero components, sums of 1 +- 1 ulp", 500))
    return out


# ---- instances
def _build_instances(g):
    return dict(inst=build_instances(g))


def spec_aux(rng, n, transmit, eta=None):
    """op 4's inputs on top of the default ones"""
    a = default_aux(n, rng)
    a[:, 16:22] = (a[:, [4, 5, 6, 4, 5, 6]] * F(-1) + rng.normal(size=(n, 6)).astype(F) * F(0.02))   # the parent's offset directions: near -wi, as a camera ray's are near its own
    a[:, 22:26] = rng.normal(size=(n, 4)).astype(F) * F(0.05)
    a[:, 26:32] = rng.normal(size=(n, 6)).astype(F) * F(0.03)
    a[:, 32:38] = rng.normal(size=(n, 6)).astype(F) * F(0.5)
    a[:, 38] = rng.choice(np.array([1.0, 1.5, 1.0 / 1.5], F), n) if eta is None else F(eta)
    a[:, 39] = F(1) if transmit else F(0)
    return a


def _cases_instances(orc, host, g, info, templates, rng):
    out = []
    tg = g.targets
    out.append(edge_then_random(g, 0, tg, rng, "six instances", 500, b_edges=B_EDGES[[3, 6, 0]]))
    out.append(edge_then_random(g, 1, tg, rng, "six instances camera ray", 500, b_edges=B_EDGES[[3, 6]], camera_ray=True))
    out.append(edge_then_random(g, 1, tg, rng, "six instances", 300, b_edges=B_EDGES[[6]], camera_ray=False))
    for name in ("one", "bilerp"):
        out.append(edge_then_random(g, 2, tg, rng, f"six instances bump {name}", 400, b_edges=B_EDGES[[6]], texture=g.tex[name], camera_ray=True))
    out.append(edge_then_random(g, 2, tg, rng, "six instances bump uv, no camera ray", 300, b_edges=B_EDGES[[6]], texture=g.tex["uv"], camera_ray=False))
    out.append(edge_then_random(g, 3, tg, rng, "six instances", 500, b_edges=B_EDGES[[3, 6]]))
    for tr in (False, True):
        b = edge_then_random(g, 4, tg, rng, f"six instances {'transmit' if tr else 'reflect'}", 300, b_edges=B_EDGES[[6]])
        b["aux"] = spec_aux(rng, len(b["prim"]), tr)
        out.append(b)
    return out


# ---- rays
def _build_rays(g):
    info = dict(flat=g.mesh(TRI + [0.0, 0.0, 0.0], N=N_OK, UV=UV_OK, name="flat")[0])
    info["tilted"] = add_flags_mesh(g, (3.0, 0.0, 0.0), (True, True, True, False, False), name="tilted")
    obj = g.object_begin()
    g.mesh(TRI + [0.0, 3.0, 0.0], N=N_OK, UV=UV_OK, name="flat_inst")
    g.object_end()
    info["inst"] = g.instance(obj, g.host.compose(g.host.translate((0.0, 0.0, 1.0)), g.host.scale((2.0, 0.5, 1.5))))
    return info


def _cases_rays(orc, host, g, info, templates, rng):
    nan = F(np.nan)
    d_edges = np.array([[0, 0, 0], [0.0, -0.0, 0.0], [3e-4, -5e-4, -8e-4], [3e2, -5e2, -8e2], [1e-30, 0, -1e-30], [1e19, 1e19, -1e19],
                        [1, 0.5, 0.0], [1, 0.5, 1e-45], [1, 0.5, -1e-45], [0.6, -0.8, float(np.spacing(F(0)))], [0, 0, -1], [0, 0, 1],
                        [nan, 0, -1], [0.3, nan, -1], [nan, nan, nan]], F)
    out = []
    tg = g.targets
    for op, kw in ((0, {}), (1, dict(camera_ray=True)), (1, dict(camera_ray=False))):
        t_idx = np.repeat(np.arange(len(tg)), len(d_edges)); de = np.tile(d_edges, (len(tg), 1))
        nr = 450
        pr = rng.integers(0, len(tg), nr)
        idx = np.concatenate([t_idx, pr])
        prim = [tg[i][0] for i in idx]; inst = [tg[i][1] for i in idx]
        b = np.concatenate([np.tile(B_EDGES[6], (len(t_idx), 1)), random_b(rng, nr)])
        d = np.concatenate([de, random_d(rng, nr)])
        out.append(batch(g, op, prim, inst, b, d, rng, "direction of length 0, 1e-3, 1e3, in the plane and one step off it, NaN" + (" camera ray" if kw.get("camera_ray") else ""), **kw))
    # the orthographic camera that looks along the plane z = 0 of `flat`: its differential rays are parallel to the surface, the probe's main ray is not
    n = 200
    out.append(batch(g, 1, [info["flat"]] * n, 0, random_b(rng, n), random_d(rng, n), rng, "orthographic camera along the surface, main ray across it", camera_ray=True, camera="ortho_along_x"))
    return out


# ---- cameras
TIE_NORMALS = [("n110", [[0, 0, 0], [1, -1, 0], [0, 0, 1]]), ("n101", [[0, 0, 0], [0, 1, 0], [1, 0, -1]]), ("n011", [[0, 0, 0], [1, 0, 0], [0, 1, -1]]),
               ("n111", [[1, 0, 0], [0, 1, 0], [0, 0, 1]]), ("nx", [[0, 0, 0], [0, 1, 0], [0, 0, 1]]), ("ny", [[0, 0, 0], [0, 0, 1], [1, 0, 0]]), ("nz", [[0, 0, 0], [1, 0, 0], [0, 1, 0]])]


def _build_cameras(g):
    info = {}
    for k, (name, P) in enumerate(TIE_NORMALS):   # small integer coordinates: the cross product's components tie exactly
        info[name] = g.mesh(np.array(P, np.float64) + [2.0 * (k % 4) - 3.0, 2.0 * (k // 4) - 1.0, 0.0], UV=UV_OK, N=None, name=name)[0]
    info["backdrop"] = g.mesh(np.array([[-6, -6, -1], [6, -6, -1], [6, 6, -1], [-6, 6, -1]], np.float64), idx=[0, 1, 2, 0, 2, 3], UV=[[0, 0], [1, 0], [1, 1], [0, 1]], name="backdrop")
    return info


P_FILM_EDGES = np.array([[0, 0], [RES, 0], [0, RES], [RES, RES], [RES / 2, RES / 2], [0.5, 0.5], [7.3, 11.9]], F)
LENS_EDGES = np.array([[0, 0], [0.5, 0.5], [np.nextafter(F(1), F(0)), 0], [0.25, 0.8]], F)


def _cases_cameras(orc, host, g, info, templates, rng):
    out = []
    tg = g.targets
    for cam in CAMERAS:
        if cam in ("pinhole", "ortho_along_x"):
            continue
        pf, ln = np.repeat(P_FILM_EDGES, len(LENS_EDGES), axis=0), np.tile(LENS_EDGES, (len(P_FILM_EDGES), 1))
        n_e = len(pf) * len(tg)
        nr = 120
        idx = np.concatenate([np.repeat(np.arange(len(tg)), len(pf)), rng.integers(0, len(tg), nr)])
        prim = [tg[i][0] for i in idx]; inst = [0] * len(idx)
        n = len(idx)
        aux = default_aux(n, rng)
        aux[:n_e, 0:2] = np.tile(pf, (len(tg), 1)); aux[:n_e, 2:4] = np.tile(ln, (len(tg), 1))
        # directions about the camera's own: towards -z with a spread
        d = (np.array([0.0, 0.0, -1.0]) + rng.normal(size=(n, 3)) * 0.15).astype(F)
        out.append(batch(g, 1, prim, inst, random_b(rng, n), d, rng, f"film corners and centre, lens centre and rim, normals that tie the dominant axis: {cam}", aux=aux, camera_ray=True, camera=cam))
    # genuine camera rays of the lens-less cameras: the oracle's own rays of all 256 pixels, where they meet the scene
    for cam in ("pinhole_spp1", "pinhole_spp16", "ortho_spp16"):
        apply_camera(orc, host, cam)
        rays, pf = orc.generate_camera_rays((0, 0, RES, RES), 0)
        hits = orc.intersect_batch(rays)
        ok = hits["prim"] != 0xFFFFFFFF
        rays, pf, hits = rays[ok], pf[ok], hits[ok]
        n = len(rays)
        aux = default_aux(n, rng); aux[:, 0:2] = pf
        out.append(dict(op=1, prim=hits["prim"].astype(np.int64), inst=hits["pad"][:, 1].astype(np.int64), b=np.stack([hits["b0"], hits["b1"], hits["b2"]], axis=1), t=hits["t"].copy(),
                        rays=rays, aux=aux, texture=0, camera_ray=True, camera=cam, tag=f"the camera's own rays: {cam}"))
    apply_camera(orc, host, "pinhole")
    return out


# ---- spawn
def _build_spawn(g):
    info = dict(zero=g.mesh(TRI, name="in z = 0 with a vertex at the origin")[0])
    info["negative"] = g.mesh(np.array([[-3, -2, -1], [-2.2, -2.5, -1.4], [-2.9, -1.1, -0.7]]), N=N_OK, name="negative coordinates")[0]
    info["huge"] = g.mesh(np.array([[1e6, 2e6, -1e6], [1.5e6, 2e6, -1e6], [1e6, 2.7e6, -0.8e6]]), name="huge coordinates")[0]
    info["tilted"] = add_flags_mesh(g, (3.0, 0.0, 0.0), (True, False, False, False, False), name="tilted")
    return info


def _cases_spawn(orc, host, g, info, templates, rng):
    tg = g.targets
    nr = 40
    idx = np.concatenate([np.repeat(np.arange(len(tg)), len(B_EDGES)), rng.integers(0, len(tg), nr)])
    prim = np.array([tg[i][0] for i in idx]); inst = np.zeros(len(idx), np.int64)
    b = np.concatenate([np.tile(B_EDGES, (len(tg), 1)), random_b(rng, nr)])
    base = batch(g, 3, prim, inst, b, np.array([0.3, -0.2, -1.0], F), rng, "base")
    o = oracle_op0(orc, host, templates, base)
    p, pe, nrm = o[:, 0:3], o[:, 3:6], o[:, 9:12]
    n = len(prim)
    # directions and targets per probe: wi with dot(wi, n) > 0, < 0, == 0 (an in-plane edge direction of the flat triangles; the zero vector everywhere) and wi = 0;
    # targets equal to p, one p_error away across the plane, 1e19 away, and with p_error 0 and 0.5
    kinds = []
    for wi_kind in range(5):
        for tgt_kind in range(5):
            kinds.append((wi_kind, tgt_kind))
    auxs = []
    for wk, tk in kinds:
        a = default_aux(n, rng)
        t1 = np.zeros((n, 3), F); t1[:, 0] = 1   # (1, 0, 0): in the plane of every triangle here whose normal is (0, 0, 1)
        wi = [nrm, -nrm, t1, np.zeros((n, 3), F), a[:, 4:7]][wk]
        a[:, 4:7] = wi
        step = (np.abs(nrm) * pe).sum(axis=1, keepdims=True) * nrm
        a[:, 7:10] = [p, p - step, p + step * F(3), p + nrm * F(1e19), a[:, 7:10] + p][tk]
        a[:, 10:13] = [np.zeros((n, 3), F), np.full((n, 3), 0.5, F), a[:, 10:13], a[:, 10:13], a[:, 10:13]][tk]
        auxs.append(a)
    big = dict(base)
    rep = len(kinds)
    big["prim"] = np.tile(prim, rep); big["inst"] = np.tile(inst, rep); big["b"] = np.tile(b, (rep, 1)); big["t"] = np.ones(n * rep, F)
    big["rays"] = np.tile(base["rays"], rep); big["aux"] = np.concatenate(auxs)
    big["tag"] = "wi on either side of n, in the plane and zero; targets at p, across the plane, 1e19 away; p_error 0 and 0.5"
    return [big]


# ---- bump
def _build_bump(g):
    build_flags32(g)
    info = dict(degenerate=build_degenerate(g, origin=(0.0, 20.0, 0.0)))
    info["inst"] = build_instances(g, origin=(0.0, 40.0, 0.0))
    return info


def _cases_bump(orc, host, g, info, templates, rng):
    out = []
    for name in ("zero", "one", "uv", "bilerp"):
        for cam_ray in (True, False):
            out.append(edge_then_random(g, 2, g.targets, rng, f"displacement {name}{' camera ray' if cam_ray else ''}", 300, b_edges=B_EDGES[[6]], texture=g.tex[name], camera_ray=cam_ray))
    return out


# ---- specular
def _build_specular(g):
    return dict(mesh=add_flags_mesh(g, (0.0, 0.0, 0.0), (True, True, True, False, False)), plain=g.mesh(TRI + [3.0, 0.0, 0.0], name="plain")[0])


def _cases_specular(orc, host, g, info, templates, rng):
    out = []
    tg = g.targets
    for transmit in (False, True):
        for eta in (1.0, 1.5, 1.0 / 1.5):
            n = 260
            pr = rng.integers(0, len(tg), n)
            prim = [tg[i][0] for i in pr]
            # directions from either side of the surface: dot(wo, ns) of both signs
            b = batch(g, 4, prim, 0, random_b(rng, n), random_d(rng, n), rng, f"{'transmit' if transmit else 'reflect'} eta {eta:.4g}")
            a = spec_aux(rng, n, transmit, eta)
            o = oracle_op0(orc, host, templates, b)
            ns = o[:, 12:15].astype(np.float64)
            # a fifth of the probes: wi nearly in the shading plane, |dot(wi, ns)| ~ 1e-6 (the large dmudx arm); a tenth each: zero dn/du, dn/dv; zero parent differentials
            k = n // 5
            tan = np.cross(ns[:k], rng.normal(size=(k, 3))); tan /= np.linalg.norm(tan, axis=1, keepdims=True)
            a[:k, 4:7] = (tan + 1e-6 * ns[:k]).astype(F)
            a[k:k + n // 10, 32:38] = 0
            a[k + n // 10:k + n // 5, 16:32] = 0
            a[k + n // 10:k + n // 5, 16:22] = -a[k + n // 10:k + n // 5][:, [4, 5, 6, 4, 5, 6]]
            b["aux"] = a
            out.append(b)
    return out


# ---- quadrics_and_curves (variant 2)
def _build_quadrics(g):
    host, s = g.host, g.s
    info = dict(mesh=add_flags_mesh(g, (0.0, 0.0, 0.0), (True, True, True, False, False)))
    info["mesh_rev"] = add_flags_mesh(g, (3.0, 0.0, 0.0), (True, False, True, True, False))
    rot = host.rotate(25.0, (0.3, 1.0, 0.2))
    at = lambda x, y: host.compose(host.translate((x, y, 0.5)), rot)
    info["centres"] = {}
    def put(name, x, y, add):
        add(at(x, y)); g.quadric_slot(name); info["centres"][name] = (x, y, 0.5)
    put("sphere", 0.0, 4.0, lambda t: s.add_sphere(t[0], t[1], 0.8, -0.6, 0.7, 300.0, g.mat))
    put("cylinder", 3.0, 4.0, lambda t: s.add_quadric("cylinder", t[0], t[1], 0.6, -0.5, 0.7, 270.0, g.mat))
    put("cone", 6.0, 4.0, lambda t: s.add_quadric("cone", t[0], t[1], 0.7, 1.2, 0.0, 360.0, g.mat))
    put("paraboloid", 9.0, 4.0, lambda t: s.add_quadric("paraboloid", t[0], t[1], 0.7, 0.1, 1.0, 360.0, g.mat))
    put("disk", 0.0, 8.0, lambda t: s.add_quadric("disk", t[0], t[1], 0.9, 0.2, 0.2, 330.0, g.mat, True))
    put("hyperboloid", 3.0, 8.0, lambda t: s.add_hyperboloid(t[0], t[1], (0.8, 0.0, -0.5), (0.5, 0.5, 0.6), 360.0, g.mat))
    # a flat cubic curve, last in the primitive list: the oracle holds no Curve shape, so only the product adds it and every earlier primitive keeps its number on both sides
    info["curve_first"] = len(g.tris)
    info["curve_cp"] = np.array([[6.0, 27.0, 0.5], [6.6, 28.2, 0.7], [7.4, 27.4, 0.3], [8.0, 28.6, 0.5]], F)   # far from the quadrics: no ray aimed at one of them meets it
    if s.b.prefix != "oracle_":
        I = (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY)
        s.add_curve(I[0], I[1], "flat", info["curve_cp"], (0.15, 0.1), split_depth=1, material=g.mat)
    return info


def quadric_rays(info, rng, per_shape=90):
    """rays from around each quadric towards points near its centre: most hit it somewhere"""
    rays = []
    for name, c in info["centres"].items():
        c = np.asarray(c, np.float64)
        v = rng.normal(size=(per_shape, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        o = c + 3.0 * v
        tgt = c + rng.normal(size=(per_shape, 3)) * 0.3
        r = np.zeros(per_shape, pbrt_hip.RAY_DTYPE)
        r["o"] = o.astype(F); r["d"] = (tgt - o).astype(F); r["t_max"] = np.inf; r["time"] = TIME
        rays.append(r)
    return np.concatenate(rays)


def _cases_quadrics(orc, host, g, info, templates, rng):
    out = []
    tri_targets = [t for t in g.targets if g.tris[t[0]]["P"] is not None]
    for op, kw in ((0, {}), (1, dict(camera_ray=True)), (2, dict(texture=g.tex["bilerp"], camera_ray=True)), (3, {})):
        out.append(edge_then_random(g, op, tri_targets, rng, "triangles through the quadric form", 500, b_edges=B_EDGES[[3, 6]], **kw))
    b4 = edge_then_random(g, 4, tri_targets, rng, "triangles through the quadric form", 500, b_edges=B_EDGES[[6]])
    b4["aux"] = spec_aux(rng, len(b4["prim"]), True)
    out.append(b4)
    # real hits on the quadrics: the oracle's answers choose the rays (those that hit a quadric); each backend then takes its own hit records for them
    rays = quadric_rays(info, rng)
    hits = orc.intersect_batch(rays)
    on_q = np.isin(hits["prim"], np.array(sorted(g.quadrics.values()), np.uint32))
    rays = rays[on_q]
    info["quadric_rays"] = rays
    n = len(rays)
    for op, kw in ((0, {}), (1, dict(camera_ray=True)), (1, dict(camera_ray=False)), (3, {})):
        out.append(dict(op=op, hits=slice(0, n), rays=rays, aux=default_aux(n, rng), texture=0, camera="pinhole", tag="real hits on the six quadric kinds", **dict(dict(camera_ray=False), **kw)))
    return out


def learn_real_hits(scene, templates, info):
    """the backend's own hit records of the set's real-hit rays (quadrics)"""
    templates["real"] = scene.intersect_batch(info["quadric_rays"]) if "quadric_rays" in info else np.zeros(0, pbrt_hip.HIT_DTYPE)


SETS = [
    SurfaceSet("flags32", _build_flags32, _cases_flags32, _mask(["FLIP_N", "REV_TS", "FACE_FORWARD", "OFFSET_NEG", "DIFF_SOLVED", "AXIS_Z"]), (0, 1, 3)),
    SurfaceSet("degenerate_frames", _build_degenerate, _cases_degenerate,
               _mask(["UV_DEGENERATE", "DPDU_CROSS_ZERO", "N_ZERO", "S_ZERO", "TS_ZERO", "DN_UV_DEGENERATE", "DN_ZERO", "DIFF_DET_SMALL", "REV_TS"]), (0, 1)),
    SurfaceSet("barycentric_edges", _build_barycentric, _cases_barycentric, _mask(["OFFSET_ZERO", "OFFSET_NEG"]), (0, 3)),
    SurfaceSet("instances", _build_instances, _cases_instances, _mask(["INST_IDENTITY", "INST_TRANSFORM", "INST_NS_FLIP", "REV_TS", "SPEC_REFLECT", "SPEC_TRANSMIT", "BUMP_DU_DEFAULT"]), (0, 1, 2, 3, 4)),
    SurfaceSet("rays", _build_rays, _cases_rays, _mask(["WO_ZERO", "TX_EARLY_OUT", "INST_TRANSFORM"]), (0, 1)),
    SurfaceSet("cameras", _build_cameras, _cases_cameras, _mask(["AXIS_X", "AXIS_Y", "AXIS_Z", "CAMERA_LENS", "DIFF_SOLVED"]), (1,)),
    SurfaceSet("spawn", _build_spawn, _cases_spawn, _mask(["OFFSET_ZERO", "OFFSET_NEG"]), (3,)),
    SurfaceSet("bump", _build_bump, _cases_bump, _mask(["BUMP_DU_DEFAULT", "INST_TRANSFORM", "UV_DEGENERATE", "DN_UV_DEGENERATE", "REV_TS"]), (2,)),
    SurfaceSet("quadrics_and_curves", _build_quadrics, _cases_quadrics, _mask(["QUADRIC"]), (0, 1, 2, 3, 4), variant=2),
    SurfaceSet("specular", _build_specular, _cases_specular, _mask(["SPEC_FLIP", "SPEC_TRANSMIT", "SPEC_REFLECT"]), (4,)),
]
SET_BY_NAME = {s.name: s for s in SETS}


def prepare(ss, scene, host, orc=None, orc_parts=None):
    """Captures set `ss` into `scene` and learns its hit templates.  For the oracle (orc is None) also makes the batches: returns (g, info, templates, batches).  For another
    backend pass the oracle's (info, batches): the set's real-hit rays are taken from there."""
    g, info = ss.capture(scene, host)
    templates = learn_templates(scene, g)
    if orc is None:
        batches = ss.cases(scene, host, g, info, templates)
        learn_real_hits(scene, templates, info)
        return g, info, templates, batches
    info_o, batches = orc_parts
    if "quadric_rays" in info_o:
        info["quadric_rays"] = info_o["quadric_rays"]
    learn_real_hits(scene, templates, info)
    return g, info, templates, batches
