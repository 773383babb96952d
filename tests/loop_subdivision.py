"""Loop subdivision of a closed triangle mesh as the reference's LoopSubDiv::subdivide does it (shapes/src/loopsubdiv.rs:403-593), in NumPy float64: `levels` rounds of the
even-vertex rule (beta = 1/16 at valence 6, 3/16 at valence 3, else 3 / (8 valence); :428-444, :695-701) and the edge rule (3/8, 3/8, 1/8, 1/8; :470-477), then every vertex
pushed to the limit surface (loop_gamma, :570-593, :706-708).  No boundary rules: the meshes it is used for are closed.  Returns (P (n, 3), indices (3 m,)).

tests/test_curve_render_gpu.py gives the reference's shape showcase its subdivision surface back with this, as a plain triangle mesh: the device has no loopsubdiv shape."""
import numpy as np


def _beta(valence):
    return 3.0 / 16.0 if valence == 3 else 3.0 / (8.0 * valence)


def _rings(n, faces):
    nb = [set() for _ in range(n)]
    for a, b, c in faces:
        nb[a] |= {b, c}; nb[b] |= {a, c}; nb[c] |= {a, b}
    return nb


def loop_subdivide(P, faces, levels=3):
    P = np.asarray(P, np.float64)
    faces = [tuple(int(v) for v in f) for f in np.asarray(faces).reshape(-1, 3)]
    for _ in range(levels):
        nb = _rings(len(P), faces)
        new_p = []
        for i, ring in enumerate(nb):
            b = 1.0 / 16.0 if len(ring) == 6 else _beta(len(ring))
            new_p.append(P[i] * (1.0 - len(ring) * b) + sum(P[j] for j in ring) * b)
        opposite = {}
        for a, b, c in faces:
            for u, v, w in ((a, b, c), (b, c, a), (c, a, b)):
                opposite.setdefault((min(u, v), max(u, v)), []).append(w)
        edge_vertex = {}
        for (u, v), ws in opposite.items():
            assert len(ws) == 2, "a closed manifold mesh"
            edge_vertex[(u, v)] = len(new_p)
            new_p.append(3.0 / 8.0 * P[u] + 3.0 / 8.0 * P[v] + 1.0 / 8.0 * P[ws[0]] + 1.0 / 8.0 * P[ws[1]])
        e = lambda u, v: edge_vertex[(min(u, v), max(u, v))]
        faces = [t for a, b, c in faces for t in ((a, e(a, b), e(c, a)), (e(a, b), b, e(b, c)), (e(c, a), e(b, c), c), (e(a, b), e(b, c), e(c, a)))]
        P = np.array(new_p)
    nb = _rings(len(P), faces)
    limit = []
    for i, ring in enumerate(nb):
        g = 1.0 / (len(ring) + 3.0 / (8.0 * _beta(len(ring))))
        limit.append(P[i] * (1.0 - len(ring) * g) + sum(P[j] for j in ring) * g)
    return np.array(limit), np.array(faces, np.uint32).ravel()
