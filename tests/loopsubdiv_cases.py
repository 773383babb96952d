"""The control meshes the loopsubdiv tests share: the smallest at which each branch of LoopSubDiv::subdivide (shapes/src/loopsubdiv.rs) is reached.  Each case is
(name, P (n,3) float32, indices, levels to run).  Positions are deliberately uneven (a fixed perturbation) so that f32 rounding differs from term to term."""
import numpy as np


def _jitter(P, seed):
    rng = np.random.default_rng(seed)
    return (np.asarray(P, np.float64) + rng.uniform(-0.07, 0.07, np.shape(P))).astype(np.float32)


TETRA_P = np.array([[0.9428, 0.0, -0.3333], [-0.4714, 0.8165, -0.3333], [-0.4714, -0.8165, -0.3333], [0.0, 0.0, 1.0]], np.float32)   # scenes/shapes/all-shapes.pbrt
TETRA_IDX = [0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2]


def fan(n, closed, seed):
    """centre vertex 0 and a rim: closed -> n faces around an interior vertex of valence n; open -> n faces at a boundary vertex of valence n + 1"""
    rim = n if closed else n + 1
    span = 2.0 * np.pi if closed else np.pi
    P = [[0.0, 0.0, 0.35]] + [[np.cos(span * k / (rim if closed else rim - 1)), np.sin(span * k / (rim if closed else rim - 1)), 0.0] for k in range(rim)]
    idx = []
    for k in range(n):
        idx += [0, 1 + k, 1 + (k + 1) % rim]
    return _jitter(P, seed), idx


def grid(nq, seed, planar=False):
    """nq x nq quads, each split along the same diagonal: interior vertices are regular (valence 6), edge vertices have boundary valence 4, the corners 2 and 3"""
    n = nq + 1
    P = [[float(x), float(y), 0.0] for y in range(n) for x in range(n)]
    idx = []
    for y in range(nq):
        for x in range(nq):
            a, b, c, d = y * n + x, y * n + x + 1, (y + 1) * n + x + 1, (y + 1) * n + x
            idx += [a, b, c, a, c, d]
    return (np.array(P, np.float32) if planar else _jitter(P, seed)), idx


def octahedron():
    P = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    idx = [0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5]
    return _jitter(P, 11), idx


def bow_tie():
    """two fans of two faces that meet in vertex 0 only: its ring is the fan of its start_face (the last face that names it)"""
    P = [[0, 0, 0], [1, 0.2, 0.1], [1, 1, 0], [0.1, 1, 0.3], [-1, -0.2, 0.2], [-1, -1, 0], [-0.2, -1, 0.1]]
    idx = [0, 1, 2, 0, 2, 3, 0, 4, 5, 0, 5, 6]
    return _jitter(P, 13), idx


def cases():
    out = [("one triangle", _jitter([[0, 0, 0], [1, 0, 0.1], [0.2, 1, 0]], 1), [0, 1, 2], (0, 1, 2, 3)),
           ("two triangles", _jitter([[0, 0, 0], [1, 0, 0.2], [0, 1, 0.1], [1, 1, -0.3]], 2), [0, 1, 2, 2, 1, 3], (1, 2)),
           ("tetrahedron", TETRA_P, TETRA_IDX, (0, 1, 2, 3)),
           ("octahedron", *octahedron(), (2,)),
           ("fan of 5", *fan(5, True, 5), (2,)),
           ("fan of 7", *fan(7, True, 7), (2,)),
           ("boundary vertex with five faces", *fan(5, False, 9), (0, 2)),
           ("grid 3x3", *grid(3, 3), (0, 2)),
           ("bow-tie", *bow_tie(), (0, 2)),
           ("tetrahedron, 5 levels", TETRA_P, TETRA_IDX, (5,))]   # 1 024 faces = 3 072 face-edges enter the last level: two scan chunks, the second partial
    return out


# a non-uniform transform that swaps handedness (negative determinant), with its inverse, row-major
def swapping_transform(host):
    t = host.compose(host.translate([0.3, -1.2, 2.0]), host.compose(host.rotate(37.0, [0.3, 1.0, -0.2]), host.scale([1.7, -0.6, 2.3])))
    return t
