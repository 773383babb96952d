"""pbrt_hip_loopsubdiv_mesh and pbrt_hip_add_loopsubdiv as far as they can be checked without a GPU (tests/test_loopsubdiv_gpu.py holds what needs a handle): the symbols and
their declarations, the counts-only call (no device work, so a NULL handle serves), and the refusals with their sentences."""
import ctypes as C
import os
import re

import numpy as np

import loopsubdiv_cases as cases
import pbrt_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def _counts(product, P, idx, levels, n_verts=None):
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3); idx = np.ascontiguousarray(idx, np.uint32)
    nv, nt = C.c_uint32(12345), C.c_uint32(12345)
    rc = product.lib.pbrt_hip_loopsubdiv_mesh(None, None, None, P.ctypes.data_as(fp) if len(P) else None, len(P) if n_verts is None else n_verts,
                                              idx.ctypes.data_as(u32p) if len(idx) else None, len(idx), levels, C.byref(nv), C.byref(nt), None, None, None)
    return rc, nv.value, nt.value, (product.fn("last_error")(None) or b"").decode()


def test_the_calls_are_declared_and_exported(product):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    for name in ("pbrt_hip_loopsubdiv_mesh", "pbrt_hip_add_loopsubdiv"):
        assert re.search(r"\bint\s+%s\s*\(\s*PbrtHipScene\s*\*" % name, header), name
        assert hasattr(product.lib, name), name
    doc = header[header.index("LoopSubDiv::subdivide"):header.index("int pbrt_hip_loopsubdiv_mesh")]
    assert "loopsubdiv.rs:321-659" in doc and ":668-689" in doc and ":695-768" in doc and "triangle.rs:75-113" in doc     # cites the reference lines it replaces
    assert "uint32_t* out_n_verts, uint32_t* out_n_tris, float* out_P, float* out_N, uint32_t* out_indices" in header
    assert "int n_levels, uint32_t material_id, int32_t first_area_light_id, uint32_t flags, float alpha, float shadow_alpha" in header
    assert callable(pbrt_hip.Scene.loopsubdiv_mesh) and callable(pbrt_hip.Scene.add_loopsubdiv)


def test_counts_only_needs_no_device(product):
    for name, P, idx, levels in cases.cases():
        e = len({(min(idx[3 * t + k], idx[3 * t + (k + 1) % 3]), max(idx[3 * t + k], idx[3 * t + (k + 1) % 3])) for t in range(len(idx) // 3) for k in range(3)})
        for L in levels:
            v, ee, f = len(P), e, len(idx) // 3
            for _ in range(L):
                v, ee, f = v + ee, 2 * ee + 3 * f, 4 * f
            assert _counts(product, P, idx, L)[:3] == (pbrt_hip.OK, v, f), (name, L)
    # indices beyond the last multiple of 3 are ignored (n_faces = len / 3)
    assert _counts(product, cases.TETRA_P, cases.TETRA_IDX + [0, 1], 3)[:3] == (pbrt_hip.OK, 130, 256)
    assert _counts(product, cases.TETRA_P, cases.TETRA_IDX, 5)[:3] == (pbrt_hip.OK, 2050, 4096)


def test_the_largest_mesh_is_the_one_whose_indices_times_three_fit_an_int(product):
    """The kernels form 3 * vertex and 3 * face in signed 32-bit arithmetic, so no level may hold more than 0x7FFFFFFF / 3 = 715 827 882 of either.  The showcase's
    tetrahedron has 4 * 4^13 = 268 435 456 faces after 13 levels (accepted) and 1 073 741 824 after 14 (refused, though it would fit 32 unsigned bits)."""
    v, e, f = 4, 6, 4
    for _ in range(13):
        v, e, f = v + e, 2 * e + 3 * f, 4 * f
    assert f == 4 ** 14 and 3 * f < 2 ** 31 and 3 * v < 2 ** 31
    assert _counts(product, cases.TETRA_P, cases.TETRA_IDX, 13)[:3] == (pbrt_hip.OK, v, f)
    assert 3 * 4 * f >= 2 ** 31 and 4 * f < 2 ** 32 // 3
    rc, _, _, msg = _counts(product, cases.TETRA_P, cases.TETRA_IDX, 14)
    assert rc == pbrt_hip.ERR_INVALID_ARG and msg == "loopsubdiv_mesh: The mesh after 14 levels does not fit 32-bit indices."
    # every level count of the tetrahedron, against the closed form
    for L in range(0, 16):
        vv, ee, ff = 4, 6, 4
        ok = True
        for _ in range(L):
            vv, ee, ff = vv + ee, 2 * ee + 3 * ff, 4 * ff
            ok = ok and vv <= 0x7FFFFFFF // 3 and ff <= 0x7FFFFFFF // 3
        assert (_counts(product, cases.TETRA_P, cases.TETRA_IDX, L)[0] == pbrt_hip.OK) == ok, L


def test_refusals_come_back_as_invalid_arg_with_one_sentence(product):
    tri = np.zeros((3, 3), np.float32)
    for P, idx, L, nv, text in (
            (tri, [], 3, None, "Vertex indices 'indices' not provided for LoopSubDiv shape."),
            (np.zeros((0, 3), np.float32), [0, 1, 2], 3, None, "Vertex positions 'P' not provided for LoopSubDiv shape."),
            (tri, [0, 1, 3], 1, None, "Vertex index 3 is out of bounds (3 vertices)."),
            (tri, [0, 1, 1], 1, None, "Face 0 names a vertex twice."),
            (np.zeros((4, 3), np.float32), [0, 1, 2], 1, None, "Start face for vertex 3 is not set. Check input mesh to ensure all vertices used."),
            (np.zeros((5, 3), np.float32), [0, 1, 2, 1, 0, 3, 0, 1, 4], 1, None, "The edge between vertices 0 and 1 is in more than two faces."),
            (np.zeros((4, 3), np.float32), [0, 1, 2, 0, 1, 3], 1, None, "Faces 0 and 1 run through the edge between vertices 0 and 1 in the same direction."),
            (tri, [0, 1, 2], -1, None, "nlevels -1 is negative."),
            (tri, [0, 1, 2], 16, None, "The mesh after 16 levels does not fit 32-bit indices."),
            (cases.TETRA_P, cases.TETRA_IDX, 14, None, "The mesh after 14 levels does not fit 32-bit indices.")):
        rc, v, t, msg = _counts(product, P, idx, L, nv)
        assert rc == pbrt_hip.ERR_INVALID_ARG, text
        assert (v, t) == (12345, 12345), text                      # nothing written
        assert msg == "loopsubdiv_mesh: " + text


def test_argument_refusals(product):
    L = product.lib
    P = cases.TETRA_P; idx = np.array(cases.TETRA_IDX, np.uint32)
    nv, nt = C.c_uint32(0), C.c_uint32(0)
    ident = np.eye(4, dtype=np.float32).ravel()
    oP, oN, oI = np.zeros((130, 3), np.float32), np.zeros((130, 3), np.float32), np.zeros(768, np.uint32)
    head = (P.ctypes.data_as(fp), 4, idx.ctypes.data_as(u32p), 12, 3)
    assert product.fn("scene_create")(0) is None    # no device here: the handle is NULL
    # null count pointers; a matrix without its inverse; some but not all of the out arrays; the mesh itself without a handle
    assert L.pbrt_hip_loopsubdiv_mesh(None, None, None, *head, None, C.byref(nt), None, None, None) == pbrt_hip.ERR_INVALID_ARG
    assert L.pbrt_hip_loopsubdiv_mesh(None, ident.ctypes.data_as(fp), None, *head, C.byref(nv), C.byref(nt), None, None, None) == pbrt_hip.ERR_INVALID_ARG
    assert L.pbrt_hip_loopsubdiv_mesh(None, None, None, *head, C.byref(nv), C.byref(nt), oP.ctypes.data_as(fp), None, None) == pbrt_hip.ERR_INVALID_ARG
    assert L.pbrt_hip_loopsubdiv_mesh(None, None, None, *head, C.byref(nv), C.byref(nt), oP.ctypes.data_as(fp), oN.ctypes.data_as(fp), oI.ctypes.data_as(u32p)) == pbrt_hip.ERR_INVALID_ARG
    assert b"null handle" in product.fn("last_error")(None)
    assert L.pbrt_hip_add_loopsubdiv(None, None, None, *head, 0, -1, 0, C.c_float(1.0), C.c_float(1.0)) == pbrt_hip.ERR_INVALID_ARG
