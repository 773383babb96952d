"""LoopSubDiv::subdivide (shapes/src/loopsubdiv.rs:321-659) with TriangleMesh::new's move to world space (shapes/src/triangle.rs:93-96), restated in NumPy float32: sequential,
statement for statement, every product and sum rounded to f32 in the order the reference writes it.  cos / sin are the C library's cosf / sinf through ctypes (what Rust's
f32::cos / f32::sin call, and what the library's host table is made with), not NumPy's own.  The checker for pbrt_hip_loopsubdiv_mesh: never the thing under test.

subdivide(P, indices, n_levels, o2w=None, w2o=None) -> Result with P (V,3) f32, N (V,3) f32, indices (3 F 4^L,) u32, counts [(V, E, F) per level, 0..L], the control mesh's
arrays (fv, ff, start_face, boundary, regular, valence) and `branches`, the set of branches that ran: "even interior regular", "even interior valence n", "even boundary",
"edge interior", "edge boundary", "limit interior valence n", "limit boundary", "normal interior valence n", "normal boundary valence 2|3|4|n", "bow-tie".
Where the reference panics a ValueError carries its text."""
import ctypes
import ctypes.util
from types import SimpleNamespace

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]

PI = f32(np.pi)                 # std::f32::consts::PI (core/src/pbrt/common.rs:22)
TWO_PI = f32(PI * f32(2.0))     # PI * 2.0 (:34)


def cos32(x):
    return f32(_libm.cosf(ctypes.c_float(float(x))))


def sin32(x):
    return f32(_libm.sinf(ctypes.c_float(float(x))))


def _next(i):
    return (i + 1) % 3


def _prev(i):
    return (i + 2) % 3


def _pt(v):
    return np.array(v, dtype=np.float32)


class SDVertex:
    def __init__(self, p=None):
        self.p = _pt(p) if p is not None else np.zeros(3, np.float32)
        self.start_face = -1
        self.child = -1
        self.regular = False
        self.boundary = False

    def valence(self, vi, faces):   # :52-87
        f = self.start_face
        nf = 1
        if not self.boundary:
            while f != -1:
                f = faces[f].next_face(vi)
                if f == self.start_face:
                    break
                nf += 1
            return nf
        while f != -1:
            f = faces[f].next_face(vi)
            if f != -1:
                nf += 1
            else:
                break
        f = self.start_face
        while f != -1:
            f = faces[f].prev_face(vi)
            if f != -1:
                nf += 1
            else:
                break
        return nf + 1

    def one_ring(self, vi, verts, faces):   # :94-129
        p = []
        if not self.boundary:
            f = self.start_face
            while True:
                p.append(verts[faces[f].next_vert(vi)].p)
                f = faces[f].next_face(vi)
                if f == self.start_face:
                    break
        else:
            f = self.start_face
            while True:
                f2 = faces[f].next_face(vi)
                if f2 == -1:
                    break
                f = f2
            p.append(verts[faces[f].next_vert(vi)].p)
            while True:
                p.append(verts[faces[f].prev_vert(vi)].p)
                f = faces[f].prev_face(vi)
                if f == -1:
                    break
        return p


class SDFace:
    def __init__(self):
        self.v = [-1, -1, -1]
        self.f = [-1, -1, -1]
        self.children = [-1, -1, -1, -1]

    def vnum(self, vert):   # :232-239
        for i in range(3):
            if self.v[i] == vert:
                return i
        return -1

    def _at(self, vert, what):
        i = self.vnum(vert)
        if i == -1:
            raise ValueError(f"{what}({vert}) not found")
        return i

    def next_face(self, vert):
        return self.f[self._at(vert, "next_face")]

    def prev_face(self, vert):
        return self.f[_prev(self._at(vert, "prev_face"))]

    def next_vert(self, vert):
        return self.v[_next(self._at(vert, "next_vert"))]

    def prev_vert(self, vert):
        return self.v[_prev(self._at(vert, "prev_vert"))]

    def other_vert(self, v0, v1):   # :289-296
        for i in range(3):
            if self.v[i] != v0 and self.v[i] != v1:
                return self.v[i]
        raise ValueError(f"Basic logic error in SDVertex::other_vert({v0}, {v1})")


def _edge(v0, v1):   # SDEdge::new (:173-179): equality and hash are the ordered endpoint pair
    return (min(v0, v1), max(v0, v1))


def beta(valence):   # :695-701
    if valence == 3:
        return f32(3.0) / f32(16.0)
    return f32(3.0) / (f32(8.0) * f32(valence))


def loop_gamma(valence):   # :706-708
    return f32(1.0) / (f32(valence) + f32(3.0) / (f32(8.0) * beta(valence)))


def weight_one_ring(vert, b, vi, verts, faces):   # :717-731
    valence = vert.valence(vi, faces)
    p_ring = vert.one_ring(vi, verts, faces)
    p = vert.p * (f32(1.0) - f32(valence) * b)
    for i in range(valence):
        p = p + p_ring[i] * b
    return p


def weight_boundary(vert, b, vi, verts, faces):   # :740-754
    valence = vert.valence(vi, faces)
    p_ring = vert.one_ring(vi, verts, faces)
    p = vert.p * (f32(1.0) - f32(2.0) * b)
    p = p + p_ring[0] * b
    p = p + p_ring[valence - 1] * b
    return p


def normal_trig(valence, boundary):
    """the cos / sin the normal pass evaluates for a vertex of this valence: interior -> [(cos theta_j, sin theta_j)], theta_j = TWO_PI * j / valence (:605-607);
    boundary valence > 4 -> (sin theta, cos theta, [sin(k theta), k = 1 .. valence - 2]), theta = PI / (valence - 1) (:624-628)"""
    if not boundary:
        out = []
        for j in range(valence):
            theta = f32(f32(TWO_PI * f32(j)) / f32(valence))
            out.append((cos32(theta), sin32(theta)))
        return out
    theta = f32(PI / f32(valence - 1))
    return sin32(theta), cos32(theta), [sin32(f32(f32(k) * theta)) for k in range(1, valence - 1)]


def cross(a, b):   # Vector3::cross (core/src/geometry/vector3.rs:211-217): plain f32
    return np.array([(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])], np.float32)


def transform_point(m, p):   # Transform::transform_point (core/src/geometry/transform.rs:288-302)
    x, y, z = p
    xp = m[0] * x + m[1] * y + m[2] * z + m[3]
    yp = m[4] * x + m[5] * y + m[6] * z + m[7]
    zp = m[8] * x + m[9] * y + m[10] * z + m[11]
    wp = m[12] * x + m[13] * y + m[14] * z + m[15]
    if wp == f32(1.0):
        return np.array([xp, yp, zp], np.float32)
    inv = f32(1.0) / wp
    return np.array([inv * xp, inv * yp, inv * zp], np.float32)


def transform_normal(mi, n):   # Transform::transform_normal (:441-448): the transpose of the inverse
    x, y, z = n
    return np.array([mi[0] * x + mi[4] * y + mi[8] * z, mi[1] * x + mi[5] * y + mi[9] * z, mi[2] * x + mi[6] * y + mi[10] * z], np.float32)


def subdivide(P, indices, n_levels=3, o2w=None, w2o=None):
    P = np.asarray(P, np.float32).reshape(-1, 3)
    vertex_indices = [int(i) for i in np.asarray(indices).reshape(-1)]
    if len(vertex_indices) == 0:   # from_props (:674-679)
        raise ValueError("Vertex indices 'indices' not provided for LoopSubDiv shape.")
    if len(P) == 0:
        raise ValueError("Vertex positions 'P' not provided for LoopSubDiv shape.")
    branches = set()
    counts = []

    verts = [SDVertex(p) for p in P]
    n_faces = len(vertex_indices) // 3
    faces = [SDFace() for _ in range(n_faces)]

    # Set face to vertex pointers (:335-346)
    for i in range(n_faces):
        for j in range(3):
            vi = vertex_indices[i * 3 + j]
            faces[i].v[j] = vi
            verts[vi].start_face = i

    # Set neighbor pointers in faces (:348-370)
    edges = {}
    for i in range(n_faces):
        for edge_num in range(3):
            v0, v1 = edge_num, _next(edge_num)
            e = _edge(faces[i].v[v0], faces[i].v[v1])
            if e not in edges:
                edges[e] = (i, edge_num)
            else:
                f0, f0_edge_num = edges.pop(e)   # HashSet::take
                faces[f0].f[f0_edge_num] = i
                faces[i].f[edge_num] = f0

    # Finish vertex initialization (:372-400)
    named = [0] * len(verts)
    for v in vertex_indices[:3 * n_faces]:
        named[v] += 1
    for i, v in enumerate(verts):
        f = v.start_face
        if f == -1:
            raise ValueError(f"Start face for vertex {i} is not set. Check input mesh to ensure all vertices used.")
        while True:
            f = faces[f].next_face(i)
            if f == -1 or f == v.start_face:
                break
        valence = v.valence(i, faces)   # taken while `boundary` is still false, as the reference takes it: at a boundary vertex this counts only the faces from start_face on,
        v.boundary = f == -1            # plus one.  `regular` follows from it; nothing downstream reads a boundary vertex's `regular`, and 1/16 == beta(6) bit for bit
        if not v.boundary and valence == 6:
            v.regular = True
        elif v.boundary and valence == 4:
            v.regular = True
        else:
            v.regular = False
        valence = v.valence(i, faces)
        fan = valence if not v.boundary else valence - 1
        if named[i] > fan:
            branches.add("bow-tie")
    control = SimpleNamespace(
        fv=np.array([f.v for f in faces], np.int32), ff=np.array([f.f for f in faces], np.int32), start_face=np.array([v.start_face for v in verts], np.int32),
        boundary=np.array([v.boundary for v in verts], bool), regular=np.array([v.regular for v in verts], bool),
        valence=np.array([v.valence(i, faces) for i, v in enumerate(verts)], np.int32))

    def n_edges():
        return len({_edge(f.v[k], f.v[_next(k)]) for f in faces for k in range(3)})

    # Refine LoopSubDiv into triangles (:403-568)
    for _ in range(n_levels):
        counts.append((len(verts), n_edges(), len(faces)))
        new_faces, new_vertices = [], []
        for vert in verts:   # :409-417
            vert.child = len(new_vertices)
            child = SDVertex()
            child.regular = vert.regular
            child.boundary = vert.boundary
            new_vertices.append(child)
        for face in faces:   # :418-424
            for k in range(4):
                face.children[k] = len(new_faces)
                new_faces.append(SDFace())

        # Update vertex positions for even vertices (:429-450)
        for vi in range(len(verts)):
            child = new_vertices[verts[vi].child]
            if not verts[vi].boundary:
                if verts[vi].regular:
                    branches.add("even interior regular")
                    child.p = weight_one_ring(verts[vi], f32(1.0) / f32(16.0), vi, verts, faces)
                else:
                    val = verts[vi].valence(vi, faces)
                    branches.add(f"even interior valence {val}")
                    child.p = weight_one_ring(verts[vi], beta(val), vi, verts, faces)
            else:
                branches.add("even boundary")
                child.p = weight_boundary(verts[vi], f32(1.0) / f32(8.0), vi, verts, faces)

        # Compute new odd edge vertices (:453-483)
        edge_verts = {}
        for i in range(len(faces)):
            for k in range(3):
                edge = _edge(faces[i].v[k], faces[i].v[_next(k)])
                if edge not in edge_verts:
                    new_vi = len(new_vertices)
                    vert = SDVertex()
                    vert.regular = True
                    vert.boundary = faces[i].f[k] == -1
                    vert.start_face = faces[i].children[3]
                    v0, v1 = verts[edge[0]], verts[edge[1]]
                    if vert.boundary:
                        branches.add("edge boundary")
                        vert.p = f32(0.5) * v0.p + f32(0.5) * v1.p
                    else:
                        branches.add("edge interior")
                        ov = verts[faces[i].other_vert(edge[0], edge[1])]
                        fk = faces[faces[i].f[k]]
                        fk_ov = verts[fk.other_vert(edge[0], edge[1])]
                        vert.p = (f32(3.0) / f32(8.0)) * v0.p + (f32(3.0) / f32(8.0)) * v1.p + (f32(1.0) / f32(8.0)) * ov.p + (f32(1.0) / f32(8.0)) * fk_ov.p
                    edge_verts[edge] = new_vi
                    new_vertices.append(vert)

        # Update even vertex face pointers (:488-497)
        for vi, vert in enumerate(verts):
            if vert.child != -1:
                start_face = faces[vert.start_face]
                vert_num = start_face.vnum(vi)
                new_vertices[vert.child].start_face = start_face.children[vert_num]

        # Update face neighbor pointers (:500-534)
        for i in range(len(faces)):
            for j in range(3):
                new_faces[faces[i].children[3]].f[j] = faces[i].children[_next(j)]
                new_faces[faces[i].children[j]].f[_next(j)] = faces[i].children[3]
                f2 = faces[i].f[j]
                new_faces[faces[i].children[j]].f[j] = faces[f2].children[faces[f2].vnum(faces[i].v[j])] if f2 != -1 else -1
                f2 = faces[i].f[_prev(j)]
                new_faces[faces[i].children[j]].f[_prev(j)] = faces[f2].children[faces[f2].vnum(faces[i].v[j])] if f2 != -1 else -1

        # Update face vertex pointers (:537-563)
        for face in faces:
            for j in range(3):
                child = new_faces[face.children[j]]
                child.v[j] = verts[face.v[j]].child
                new_vi = edge_verts.get(_edge(face.v[j], face.v[_next(j)]), -1)
                if new_vi != -1:
                    child.v[_next(j)] = new_vi
                new_faces[face.children[_next(j)]].v[j] = new_vi
                new_faces[face.children[3]].v[j] = new_vi

        faces, verts = new_faces, new_vertices
    counts.append((len(verts), n_edges(), len(faces)))

    # Push vertices to limit surface (:571-593)
    p_limit = []
    for i in range(len(verts)):
        if verts[i].boundary:
            branches.add("limit boundary")
            p_limit.append(weight_boundary(verts[i], f32(1.0) / f32(5.0), i, verts, faces))
        else:
            val = verts[i].valence(i, faces)
            branches.add(f"limit interior valence {val}")
            p_limit.append(weight_one_ring(verts[i], loop_gamma(val), i, verts, faces))
    for i in range(len(verts)):
        verts[i].p = p_limit[i]

    # Compute vertex tangents on limit surface (:596-634)
    ns = []
    for i, vertex in enumerate(verts):
        s = np.zeros(3, np.float32)
        t = np.zeros(3, np.float32)
        valence = vertex.valence(i, faces)
        p_ring = vertex.one_ring(i, verts, faces)
        if not vertex.boundary:
            branches.add(f"normal interior valence {valence}")
            cs = normal_trig(valence, False)
            for j in range(valence):
                s = s + cs[j][0] * p_ring[j]
                t = t + cs[j][1] * p_ring[j]
        else:
            s = p_ring[valence - 1] - p_ring[0]
            if valence == 2:
                branches.add("normal boundary valence 2")
                t = p_ring[0] + p_ring[1] - f32(2.0) * vertex.p
            elif valence == 3:
                branches.add("normal boundary valence 3")
                t = p_ring[1] - vertex.p
            elif valence == 4:
                branches.add("normal boundary valence 4")
                t = f32(-1.0) * p_ring[0] + f32(2.0) * p_ring[1] + f32(2.0) * p_ring[2] - f32(1.0) * p_ring[3] - f32(2.0) * vertex.p
            else:
                branches.add("normal boundary valence n")
                sin_theta, cos_theta, sin_k = normal_trig(valence, True)
                t = sin_theta * (p_ring[0] + p_ring[valence - 1])
                for k in range(1, valence - 1):
                    wt = (f32(2.0) * cos_theta - f32(2.0)) * sin_k[k - 1]
                    t = t + wt * p_ring[k]
                t = -t
        ns.append(cross(s, t))

    # Create triangle mesh from subdivision mesh (:636-658), TriangleMesh::new (triangle.rs:93-96)
    out_idx = np.array([face.v[j] for face in faces for j in range(3)], np.uint32)
    out_p = np.array(p_limit, np.float32).reshape(-1, 3)
    out_n = np.array(ns, np.float32).reshape(-1, 3)
    if o2w is not None:
        m = np.asarray(o2w, np.float32).reshape(16)
        mi = np.asarray(w2o, np.float32).reshape(16)
        out_p = np.array([transform_point(m, p) for p in out_p], np.float32).reshape(-1, 3)
        out_n = np.array([transform_normal(mi, n) for n in out_n], np.float32).reshape(-1, 3)
    return SimpleNamespace(P=out_p, N=out_n, indices=out_idx, counts=counts, control=control, branches=branches)
