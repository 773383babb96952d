"""tests/loopsubdiv_restatement.py — the float32 checker of pbrt_hip_loopsubdiv_mesh — against what can be known without it: the closed form of the level counts, the float64
helper tests/loop_subdivision.py on closed meshes (indices face for face, positions to 1e-5 x the control mesh's largest |coordinate|: at most (levels + 1) (valence + 2)
f32 operations on values of that size stay under about 50 ulp = 3e-6, a threefold margin), the affine invariance of the rules on a planar regular grid, and a record of the
branches that ran.  No GPU is needed."""
import numpy as np
import pytest

import loopsubdiv_cases as cases
import loopsubdiv_restatement as R
from loop_subdivision import loop_subdivide

CASES = cases.cases()


@pytest.fixture(scope="module")
def results():
    return {(name, L): R.subdivide(P, idx, L) for name, P, idx, levels in CASES for L in levels}


def test_counts_match_the_closed_form(results):
    for (name, L), r in results.items():
        v, e, f = r.counts[0]
        assert len(r.counts) == L + 1
        for lv in range(1, L + 1):
            v, e, f = v + e, 2 * e + 3 * f, 4 * f          # V' = V + E, E' = 2E + 3F, F' = 4F
            assert r.counts[lv] == (v, e, f), (name, lv)
        assert len(r.P) == len(r.N) == v and len(r.indices) == 3 * f, name
        assert r.indices.max() < v
        assert set(r.indices.tolist()) == set(range(v)), name    # every vertex is used


@pytest.mark.parametrize("name", ["tetrahedron", "octahedron"])
def test_closed_meshes_equal_the_float64_helper(results, name):
    for (n, L), r in results.items():
        if n != name:
            continue
        _, P, idx, _ = next(c for c in CASES if c[0] == name)
        p64, i64 = loop_subdivide(P, np.array(idx).reshape(-1, 3), L)
        assert np.array_equal(r.indices, i64), (name, L)
        bound = 1e-5 * float(np.abs(P).max())
        err = float(np.abs(r.P.astype(np.float64) - p64).max())
        print(f"{name} at {L} levels: max |f32 - f64| = {err:.3g} (bound {bound:.3g})")
        assert err <= bound, (name, L, err)


def test_five_levels_of_the_tetrahedron_equal_the_float64_helper(results):
    r = results[("tetrahedron, 5 levels", 5)]
    p64, i64 = loop_subdivide(cases.TETRA_P, np.array(cases.TETRA_IDX).reshape(-1, 3), 5)
    assert np.array_equal(r.indices, i64)
    assert float(np.abs(r.P.astype(np.float64) - p64).max()) <= 1e-5 * float(np.abs(cases.TETRA_P).max())


def test_a_planar_regular_grid_stays_affine():
    """The rules are affine combinations with weights that sum to one: a grid in a plane stays in it; at the regular interior vertices, whose rings are symmetric about them,
    control points that are an affine image of the integer grid stay where they are, at every level and in the limit; every normal is parallel to the plane's."""
    P0, idx = cases.grid(4, 0, planar=True)
    A = np.array([[1.3, 0.4, 0.0], [-0.2, 0.9, 0.0], [0.5, -0.7, 0.0]])   # columns of the plane's frame: x -> A[:, 0], y -> A[:, 1]
    origin = np.array([0.25, -1.5, 2.0])
    P = (P0.astype(np.float64) @ A.T + origin).astype(np.float32)
    normal = np.cross(A[:, 0], A[:, 1]); normal /= np.linalg.norm(normal)
    bound = 1e-5 * float(np.abs(P).max())
    for L in (0, 1, 2):
        r = R.subdivide(P, idx, L)
        off_plane = np.abs((r.P.astype(np.float64) - origin) @ normal)
        assert off_plane.max() <= bound, (L, off_plane.max())
        n = r.N.astype(np.float64)
        ln = np.linalg.norm(n, axis=1)
        assert (ln > 0).all()
        assert np.abs(np.cross(n / ln[:, None], normal)).max() <= 1e-5, L
        # the 9 interior control vertices are children of themselves (vertex i's child is i) and regular
        for y in range(1, 4):
            for x in range(1, 4):
                i = y * 5 + x
                assert np.abs(r.P[i].astype(np.float64) - P[i].astype(np.float64)).max() <= bound, (L, i)


def test_every_branch_is_reached(results):
    ran = set()
    for r in results.values():
        ran |= r.branches
    for v in (3, 4, 5, 6, 7):
        assert f"normal interior valence {v}" in ran and f"limit interior valence {v}" in ran, v
    for v in (3, 4, 5, 7):
        assert f"even interior valence {v}" in ran, v
    for b in ("even interior regular", "even boundary", "edge interior", "edge boundary", "limit boundary", "normal boundary valence 2", "normal boundary valence 3",
              "normal boundary valence 4", "normal boundary valence n", "bow-tie"):
        assert b in ran, b
    assert "bow-tie" in results[("bow-tie", 2)].branches and "bow-tie" not in results[("grid 3x3", 2)].branches


def test_the_valence_for_regular_is_taken_before_the_boundary_flag():
    """loopsubdiv.rs:391-392: at a boundary vertex `regular` comes from the faces counted from start_face on; the restatement keeps the quirk (nothing downstream reads it)"""
    P, idx = cases.grid(3, 3)
    c = R.subdivide(P, idx, 0).control
    assert c.boundary.sum() == 12 and (c.valence[~c.boundary] == 6).all() and c.regular[~c.boundary].all()
    assert sorted(set(c.valence[c.boundary].tolist())) == [2, 3, 4]
    # start_face is the LAST face that names the vertex
    for v in range(len(P)):
        assert c.start_face[v] == max(f for f in range(len(idx) // 3) if v in idx[3 * f:3 * f + 3])


def test_the_panics_carry_the_reference_text():
    with pytest.raises(ValueError, match="Vertex indices 'indices' not provided for LoopSubDiv shape."):
        R.subdivide([[0, 0, 0]], [], 1)
    with pytest.raises(ValueError, match="Vertex positions 'P' not provided for LoopSubDiv shape."):
        R.subdivide(np.zeros((0, 3)), [0, 1, 2], 1)
    with pytest.raises(ValueError, match="Start face for vertex 3 is not set"):
        R.subdivide(np.zeros((4, 3)), [0, 1, 2], 1)
