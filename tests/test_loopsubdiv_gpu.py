"""Shape "loopsubdiv" on the device: pbrt_hip_loopsubdiv_mesh against the NumPy float32 restatement of LoopSubDiv::subdivide (tests/loopsubdiv_restatement.py) on EVERY word
of P, N and the indices, in object space and under a non-uniform, handedness-swapping transform, for the meshes of tests/loopsubdiv_cases.py; and pbrt_hip_add_loopsubdiv
against pbrt_hip_add_mesh of the restatement's mesh, on the film and the ray counters of a 32 x 32 @ 4 spp frame under every integrator, inside an instanced object and as an
area light."""
import numpy as np
import pytest

import loopsubdiv_cases as cases
import loopsubdiv_restatement as LR
import pbrt_hip
import reference_scenes as R

pytestmark = pytest.mark.gpu
CASES = cases.cases()


@pytest.fixture(scope="module")
def xf(host):
    m, mi = cases.swapping_transform(host)
    assert host.swaps_handedness(m)
    return m, mi


@pytest.fixture(scope="module")
def scene():
    with pbrt_hip.Scene() as s:
        yield s


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_mesh(got, want, label):
    gP, gN, gI = got
    assert gP.shape == want.P.shape and gN.shape == want.N.shape and gI.shape == want.indices.shape, label
    assert np.array_equal(gI, want.indices), (label, "indices")
    dp = (words(gP) != words(want.P)).any(-1); dn = (words(gN) != words(want.N)).any(-1)
    assert not dp.any(), (label, "P", int(dp.sum()), np.flatnonzero(dp)[:8].tolist())
    assert not dn.any(), (label, "N", int(dn.sum()), np.flatnonzero(dn)[:8].tolist())


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_mesh_equals_the_restatement_word_for_word(scene, xf, name):
    _, P, idx, levels = next(c for c in CASES if c[0] == name)
    for L in levels:
        want = LR.subdivide(P, idx, L)
        assert scene.loopsubdiv_mesh(P, idx, L, counts_only=True) == (len(want.P), len(want.indices) // 3)
        assert_same_mesh(scene.loopsubdiv_mesh(P, idx, L), want, (name, L, "object space"))
        assert np.isfinite(want.N).all() and (np.abs(want.N).max(axis=1) > 0).all(), (name, L)     # the comparison is not one of zeros
        if L == levels[-1]:
            want_w = LR.subdivide(P, idx, L, xf[0], xf[1])
            assert not np.array_equal(want_w.P, want.P)
            assert_same_mesh(scene.loopsubdiv_mesh(P, idx, L, xf[0], xf[1]), want_w, (name, L, "world space"))
        if name == "tetrahedron, 5 levels":     # 3 * 1 024 face-edges enter the last level: more than one 2 048-wide scan chunk, the second one partial
            assert want.counts[4][2] * 3 == 3072


def test_numbering_over_more_than_1024_scan_chunks(scene):
    """One level of a 600 x 600-quad grid: 720 000 faces, 2 160 000 face-edges = 1 055 scan chunks of 2 048, so the one-block scan of the chunk sums gives each of its
    1 024 threads more than one sum (the tetrahedron at 5 levels, above, has two chunks, the second partial).  The scan decides the new vertices' numbers and nothing else,
    so the indices pin it: they are held to the numbering worked out here with NumPy — an edge's vertex is V + the rank of the edge's first face-edge, in (face, edge) order,
    among all first face-edges (the order the reference's HashMap meets them, loopsubdiv.rs:454-483) — and the children's layout of :537-563."""
    P, idx = cases.grid(600, 0, planar=True)
    F = np.asarray(idx, np.int64).reshape(-1, 3)
    V, n_fe = len(P), 3 * len(F)
    assert (n_fe + 2047) // 2048 > 1024
    a, b = F.ravel(), np.roll(F, -1, axis=1).ravel()                     # face-edge (i, k) runs v[k] -> v[next(k)]
    key = np.minimum(a, b) * V + np.maximum(a, b)
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), np.int64); rank[np.argsort(first)] = np.arange(len(uniq))
    ev = (V + rank[inverse]).reshape(-1, 3)                              # ev[i, k]: the vertex on edge k of face i
    want = np.stack([F[:, 0], ev[:, 0], ev[:, 2], ev[:, 0], F[:, 1], ev[:, 1], ev[:, 2], ev[:, 1], F[:, 2], ev[:, 0], ev[:, 1], ev[:, 2]], 1).astype(np.uint32).ravel()
    assert scene.loopsubdiv_mesh(P, idx, 1, counts_only=True) == (V + len(uniq), 4 * len(F))
    gP, gN, gI = scene.loopsubdiv_mesh(P, idx, 1)
    assert np.array_equal(gI, want)
    assert np.isfinite(gP).all() and np.abs(gP[:, 2]).max() == 0.0 and (gN[:, 2] < 0).all() and np.abs(gN[:, :2]).max() == 0.0      # a grid in z = 0 stays there; the rings run clockwise round counter-clockwise faces, so s x t points along -z


def test_refusals_leave_the_scene_as_it_was(scene):
    m = scene.add_material_matte((0.5, 0.5, 0.5))
    for P, idx, L, text in ((np.zeros((4, 3), np.float32), [0, 1, 2, 0, 1, 3], 1, "in the same direction"), (np.zeros((4, 3), np.float32), [0, 1, 2], 1, "Start face for vertex 3 is not set"),
                            (cases.TETRA_P, cases.TETRA_IDX, -1, "nlevels -1 is negative.")):
        for call in (lambda: scene.loopsubdiv_mesh(P, idx, L), lambda: scene.add_loopsubdiv(P, idx, L, m)):
            with pytest.raises(pbrt_hip.PbrtHipError) as e:
                call()
            assert e.value.code == pbrt_hip.ERR_INVALID_ARG and text in str(e.value)
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        scene.add_loopsubdiv(cases.TETRA_P, cases.TETRA_IDX, 1, m + 7)
    assert e.value.code == pbrt_hip.ERR_INVALID_ARG and "unknown material" in str(e.value)
    first = scene.add_light_diffuse_area((1, 1, 1), 4)
    with pytest.raises(pbrt_hip.PbrtHipError) as e:      # one light per OUTPUT triangle: 4 lights do not serve 16 triangles
        scene.add_loopsubdiv(cases.TETRA_P, cases.TETRA_IDX, 1, m, first_area_light=first)
    assert e.value.code == pbrt_hip.ERR_INVALID_ARG and "area light ids out of range" in str(e.value)


# ---- frames -----------------------------------------------------------------------------------------------------------------------------------------------------------
LEVELS = 2
SURF_P, SURF_IDX = cases.TETRA_P, cases.TETRA_IDX


def frame(host, xf, how, variant, integrator):
    """the surface over a floor under a sky and a distant light, seen from the side.  how = "loopsubdiv": pbrt_hip_add_loopsubdiv; "mesh": the restatement's mesh through add_mesh"""
    with pbrt_hip.Scene() as s:
        s.add_light_infinite((0.6, 0.7, 0.9))
        s.add_light_distant((2.0, 1.8, 1.5), host.distant_direction(pbrt_hip.IDENTITY, (-3.0, 4.0, 10.0), (0.0, 0.0, 0.0)))
        matte = s.add_material_matte((0.6, 0.5, 0.4))
        mirror = s.add_material_mirror((0.9, 0.9, 0.9))
        n_out = len(SURF_IDX) // 3 * 4 ** LEVELS
        first = -1
        if variant == "area light":
            first = s.add_light_diffuse_area((3.0, 2.0, 1.0), n_out, two_sided=True)
        if variant == "instanced":
            obj = s.object_begin()
        if how == "loopsubdiv":
            s.add_loopsubdiv(SURF_P, SURF_IDX, LEVELS, mirror if variant == "mirror" else matte, xf[0], xf[1], first_area_light=first, swaps_handedness=True)
        else:
            w = LR.subdivide(SURF_P, SURF_IDX, LEVELS, xf[0], xf[1])
            s.add_mesh(w.P, w.indices, mirror if variant == "mirror" else matte, N=w.N, first_area_light=first, swaps_handedness=True)
        if variant == "instanced":
            s.object_end()
            for d in ((0.0, 0.0, 0.0), (1.5, 0.5, 0.8)):
                t = host.translate(d)
                s.add_instance(obj, t[0], t[1])
        s.add_mesh(host.transform_points(host.translate((0, 0, -1.5))[0], R.quad(10.0)), R.QUAD_IDX, matte, UV=R.QUAD_ST)
        R.camera_film(s, host, (0.3, 9.0, 3.0), (0.3, -1.2, 2.0), (0, 0, 1), 40.0, 32, 32, 4)
        s.build_accel_device_shapes(0, 4)
        xyz, wt, st = {"path": lambda: s.render_path(max_depth=5), "whitted": lambda: s.render_whitted(max_depth=5), "directlighting": lambda: s.render_direct("all", max_depth=5)}[integrator]()
        d = st.as_dict()
        return words(np.asarray(xyz, np.float32)).copy(), words(np.asarray(wt, np.float32)).copy(), {k: d[k] for k in ("camera_rays", "regular_rays", "shadow_rays")}, np.asarray(xyz).copy()


@pytest.mark.parametrize("variant,integrator", [("plain", "path"), ("mirror", "whitted"), ("plain", "directlighting"), ("instanced", "path"), ("area light", "path")])
def test_frame_equals_the_restatements_mesh_bit_for_bit(host, xf, variant, integrator):
    a = frame(host, xf, "loopsubdiv", variant, integrator)
    b = frame(host, xf, "mesh", variant, integrator)
    assert a[2] == b[2], (a[2], b[2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2]["camera_rays"] == 32 * 32 * 4 and a[2]["shadow_rays"] > 0
    assert np.isfinite(a[3]).all() and float(a[3].max()) > 0.05
