"""The quadric shapes' capture calls (pbrt_hip_add_sphere / _add_quadric / _add_hyperboloid) as far as they can be checked without a GPU: the symbols, their behaviour on
null arguments, and the host BVH builders over triangles and all six kinds against the oracle's trees (bounds = Shape::world_bound, same topology, same leaf order)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pbrt_hip
from oracle_binding import OracleScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbrt_hip_add_sphere", "pbrt_hip_add_hyperboloid", "pbrt_hip_add_quadric")
KIND_NO = {"cylinder": 0, "cone": 1, "paraboloid": 2, "disk": 3, "sphere": 4, "hyperboloid": 5}


def test_the_three_calls_are_declared_and_exported(product):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*PbrtHipScene\s*\*" % name, header), name
        assert hasattr(product.lib, name), name
    assert "uint32_t material_id, uint32_t flags" in header[header.index("int pbrt_hip_add_sphere"):]
    for name in ("add_sphere", "add_hyperboloid", "add_quadric"):
        assert callable(getattr(pbrt_hip.Scene, name))


def test_null_arguments_are_errors_not_crashes(product):
    fp = C.POINTER(C.c_float)
    ident = np.eye(4, dtype=np.float32).ravel()
    m = ident.ctypes.data_as(fp)
    p = np.array([1, 0, 0], np.float32).ctypes.data_as(fp)
    L = product.lib
    assert product.fn("scene_create")(0) is None    # no device here: the handle is NULL
    assert L.pbrt_hip_add_sphere(None, m, m, C.c_float(1), C.c_float(-1), C.c_float(1), C.c_float(360), 0, 0) != pbrt_hip.OK
    assert L.pbrt_hip_add_sphere(None, None, None, C.c_float(1), C.c_float(-1), C.c_float(1), C.c_float(360), 0, 0) != pbrt_hip.OK
    assert L.pbrt_hip_add_hyperboloid(None, m, m, p, p, C.c_float(360), 0, 0) != pbrt_hip.OK
    assert L.pbrt_hip_add_hyperboloid(None, None, None, None, None, C.c_float(360), 0, 0) != pbrt_hip.OK
    assert L.pbrt_hip_add_quadric(None, 0, m, m, C.c_float(1), C.c_float(0), C.c_float(1), C.c_float(360), 0, 0) != pbrt_hip.OK
    assert L.pbrt_hip_add_quadric(None, 7, None, None, C.c_float(1), C.c_float(0), C.c_float(1), C.c_float(360), 0, 0) != pbrt_hip.OK


def _shapes(host, n, seed):
    """n random shapes of all six kinds: (kind, (o2w, w2o), parameters as the 7 floats of pbrt_hip_host_build_bvh_shapes)"""
    rng = np.random.default_rng(seed)
    kinds = list(KIND_NO)
    out = []
    for i in range(n):
        kind = kinds[i % 6]
        c = rng.uniform(-0.9, 0.9, 3); sc = float(rng.uniform(0.03, 0.2))
        t = host.compose(host.compose(host.translate(tuple(c)), host.rotate(float(rng.uniform(0, 360)), tuple(rng.normal(size=3)))),
                         host.scale((sc if i % 4 else -sc, sc * float(rng.uniform(0.5, 1.5)), sc)))
        phi = float(rng.choice([360.0, 250.0, 90.0]))
        if kind == "sphere": par = [1.0, float(rng.uniform(-1.2, 0)), float(rng.uniform(0, 1.2)), phi, 0, 0, 0]
        elif kind == "cylinder": par = [0.8, 0.6, -0.6, phi, 0, 0, 0]
        elif kind == "cone": par = [0.8, 1.3, 0.0, phi, 0, 0, 0]
        elif kind == "paraboloid": par = [0.8, 0.2, 1.0, phi, 0, 0, 0]
        elif kind == "disk": par = [0.9, float(rng.uniform(-0.5, 0.5)), 0.3, phi, 0, 0, 0]
        else: par = [0.6, 0.6, 0.8, 0.9, -0.6, -0.8, phi]
        out.append((kind, t, par))
    return out


def _add(scene, kind, t, par, material):
    if kind == "sphere": scene.add_sphere(t[0], t[1], par[0], par[1], par[2], par[3], material)
    elif kind == "hyperboloid": scene.add_hyperboloid(t[0], t[1], par[0:3], par[3:6], par[6], material)
    else: scene.add_quadric(kind, t[0], t[1], par[0], par[1], par[2], par[3], material)


@pytest.mark.parametrize("split_method,n_tris,n_shapes,max_prims", [(0, 3000, 60, 4), (0, 3000, 60, 1), (1, 3000, 60, 4), (0, 0, 6, 4), (0, 0, 1, 4), (3, 10, 6, 4), (3, 5, 6, 1)])
def test_host_bvh_over_triangles_and_quadrics_equals_the_oracles(host, product, split_method, n_tris, n_shapes, max_prims):
    """Same primitive bounds (Shape::world_bound of each quadric), same decisions, same partition order: leaf contents in depth-first order, leaf sizes, the root bound and
    every child box equal the oracle's.  (EqualCounts only on tie-free tiny scenes, as tests/test_capi_and_host.py explains.)"""
    P, idx = host.gen_random_tris(max(n_tris, 1), 9)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)[:n_tris]
    half = n_tris // 2
    shapes = _shapes(host, n_shapes, 4 + n_shapes)
    orc = OracleScene()
    m = orc.add_material_matte()
    if half: orc.add_mesh(P, idx[:half].ravel(), m)
    for kind, t, par in shapes:
        _add(orc, kind, t, par, m)
    if n_tris - half: orc.add_mesh(P, idx[half:].ravel(), m)
    orc.build_accel(split_method, max_prims)
    n = n_tris + n_shapes
    onodes = orc.bvh_nodes()
    oprims = np.zeros(n, np.uint32); orc.b.lib.oracle_bvh_ordered_prims(orc.h, oprims.ctypes.data)
    leaves = onodes[onodes["n_primitives"] > 0]
    oracle_leaves = [tuple(oprims[l["offset"]:l["offset"] + l["n_primitives"]]) for l in leaves]

    # the product's primitive list: the first mesh's triangles, the shapes, the second mesh's triangles
    pidx = np.zeros((n, 3), np.uint32); pidx[:half] = idx[:half]; pidx[half + n_shapes:] = idx[half:]
    prim_shape = np.zeros(n, np.uint32); prim_shape[half:half + n_shapes] = 1 + np.arange(n_shapes, dtype=np.uint32)
    rec = np.zeros((n_shapes, 40), np.float32)
    for k, (kind, t, par) in enumerate(shapes):
        rec[k, 0] = KIND_NO[kind]; rec[k, 1:17] = np.asarray(t[0], np.float32).ravel(); rec[k, 17:33] = np.asarray(t[1], np.float32).ravel(); rec[k, 33:40] = par
    order = np.zeros(n, np.uint32); last = np.zeros(n, np.uint32)
    nodes = np.zeros((max(n - 1, 1), 16), np.uint32); info = np.zeros(5, np.uint64); rb = np.zeros(6, np.float32)
    f = product.lib.pbrt_hip_host_build_bvh_shapes
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    Pc = np.ascontiguousarray(P, np.float32)
    for threads in (1, 4):
        rc = f(Pc.ctypes.data, pidx.ctypes.data, n, prim_shape.ctypes.data, rec.ctypes.data, n_shapes, split_method, max_prims, threads, order.ctypes.data, last.ctypes.data,
               nodes.ctypes.data, info.ctypes.data, rb.ctypes.data)
        assert rc == 0
        assert int(info[1]) == len(leaves) and int(info[0]) == len(onodes) - len(leaves)
        ends = np.flatnonzero(last); starts = np.concatenate([[0], ends[:-1] + 1])
        assert [tuple(order[a:b + 1]) for a, b in zip(starts, ends)] == oracle_leaves, "leaf contents / order differ"
        if split_method != 1:
            assert np.array_equal(order, oprims)
        assert np.array_equal(rb[:3], onodes[0]["pmin"]) and np.array_equal(rb[3:], onodes[0]["pmax"])
    if int(info[0]) > 0:
        fl = nodes.view(np.float32)
        boxes = set()
        for k in range(int(info[0])):
            for c in (0, 6):
                boxes.add((fl[k, c], fl[k, c + 2], fl[k, c + 4], fl[k, c + 1], fl[k, c + 3], fl[k, c + 5]))
        assert boxes == {tuple(nd["pmin"]) + tuple(nd["pmax"]) for nd in onodes[1:]}
    orc.close()
