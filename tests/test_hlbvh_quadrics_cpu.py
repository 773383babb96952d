"""No GPU: the yardstick behind tests/test_hlbvh_quadrics_device_gpu.py.  That file shows "device-built HLBVH == host-built HLBVH" on the edge scenes of
tests/hlbvh_quadric_scenes.py; this one shows "host-built HLBVH == the oracle's HLBVH" on the same flat scenes (pbrt_hip_host_build_bvh_shapes with split method 1 against
orc.build_accel(1, ..): leaf contents and order, node counts, the root bound, the set of child boxes — the relation of
test_quadrics_capi.py::test_host_bvh_over_triangles_and_quadrics_equals_the_oracles), so that device == host there also means device == reference.  A scene on which one of the
reference's HLBVH assertions fires (hlbvh.rs:338/356/418) must be refused by both sides; at most one of the edge scenes may be of that kind, and at most two of the twelve fuzz
seeds the GPU file draws — which the oracle alone decides, so it is checked here.  The host entry takes no object instances: for the instanced and masked scenes the host forest
builder is compared with the oracle on the GPU side (hits, occlusion, world bound), and here only the assertion class is counted."""
import ctypes as C

import numpy as np
import pytest

import pbrt_hip
import hlbvh_quadric_scenes as HQ
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1

FUZZ_INSTANCE_SEEDS = (201, 202, 203, 204, 205, 206)      # tests/test_fuzz_quadric_instances_gpu.py's generator (the reference asserts on 205)
FUZZ_ALPHA_SEEDS = (101, 102, 103, 104, 105, 106)         # tests/test_fuzz_quadric_alpha_gpu.py's generator (the reference asserts on 101)
FUZZ_MAX_PRIMS = (1, 4)                                   # seed % 2 picks one
FUZZ_REFUSED = {"instances 205", "alpha 101"}             # what the oracle decides, checked below: the GPU file expects both builders to refuse exactly these


def oracle_hlbvh(capture, max_prims):
    """-> (OracleScene built with HLBVH, 0), or (None, code) where the reference's build asserts"""
    orc = OracleScene()
    with libm1():          # (Sphere::new evaluates acos)
        capture(orc)
        try:
            orc.build_accel(1, max_prims)
        except pbrt_hip.PbrtHipError as e:
            orc.close()
            return None, e.code
    return orc, 0


@pytest.mark.parametrize("max_prims", [1, 4])
@pytest.mark.parametrize("name", list(HQ.FLAT))
def test_host_hlbvh_over_quadrics_equals_the_oracles(host, product, name, max_prims):
    parts = HQ.FLAT[name](host)
    orc, orc_code = oracle_hlbvh(HQ.capture_flat(parts), max_prims)
    P, pidx, prim_shape, rec = HQ.host_arrays(parts)
    n, n_shapes = len(pidx), len(rec)
    order = np.zeros(n, np.uint32); last = np.zeros(n, np.uint32)
    nodes = np.zeros((max(n - 1, 1), 16), np.uint32); info = np.zeros(5, np.uint64); rb = np.zeros(6, np.float32)
    f = product.lib.pbrt_hip_host_build_bvh_shapes
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    for threads in (1, 4):
        rc = f(P.ctypes.data, pidx.ctypes.data, n, prim_shape.ctypes.data, rec.ctypes.data, n_shapes, 1, max_prims, threads, order.ctypes.data, last.ctypes.data, nodes.ctypes.data,
               info.ctypes.data, rb.ctypes.data)
        if orc is None:      # the reference asserts: the host builder says so too (-2)
            assert (rc, orc_code) == (-2, pbrt_hip.ERR_INVALID_ARG)
            continue
        assert rc == 0
        onodes = orc.bvh_nodes()
        oprims = np.zeros(n, np.uint32); orc.b.lib.oracle_bvh_ordered_prims(orc.h, oprims.ctypes.data)
        leaves = onodes[onodes["n_primitives"] > 0]
        oracle_leaves = [tuple(oprims[l["offset"]:l["offset"] + l["n_primitives"]]) for l in leaves]
        assert int(info[1]) == len(leaves) and int(info[0]) == len(onodes) - len(leaves)
        ends = np.flatnonzero(last); starts = np.concatenate([[0], ends[:-1] + 1])
        assert [tuple(order[a:b + 1]) for a, b in zip(starts, ends)] == oracle_leaves, "leaf contents / order differ"
        assert np.array_equal(rb[:3], onodes[0]["pmin"]) and np.array_equal(rb[3:], onodes[0]["pmax"])
        fl = nodes.view(np.float32)
        boxes = set()
        for k in range(int(info[0])):
            for c in (0, 6):
                boxes.add((fl[k, c], fl[k, c + 2], fl[k, c + 4], fl[k, c + 1], fl[k, c + 3], fl[k, c + 5]))
        assert boxes == {tuple(nd["pmin"]) + tuple(nd["pmax"]) for nd in onodes[1:]}
    if orc is not None:
        orc.close()


def test_at_most_one_edge_scene_trips_the_references_assertions(host):
    refused = set()
    for name, make in HQ.all_scenes().items():
        for max_prims in (1, 4):
            orc, code = oracle_hlbvh(make(host), max_prims)
            if orc is None:
                assert code == pbrt_hip.ERR_INVALID_ARG, (name, code)
                refused.add(name)
            else:
                orc.close()
    assert len(refused) <= 1, refused


def fuzz_cases(host):
    """-> [(name, capture, max_prims)]: twelve seeds of the two quadric fuzz generators.  Their captures end with a host build of the generator's own choice; the HLBVH build
    under test follows on the same handle."""
    import test_fuzz_quadric_alpha_gpu as FA
    import test_fuzz_quadric_instances_gpu as FI
    return [(f"instances {seed}", FI.build_case(host, seed)[0], FUZZ_MAX_PRIMS[seed % 2]) for seed in FUZZ_INSTANCE_SEEDS] + \
           [(f"alpha {seed}", FA.build_case(host, seed)[0], FUZZ_MAX_PRIMS[seed % 2]) for seed in FUZZ_ALPHA_SEEDS]


def test_at_most_two_fuzz_seeds_trip_the_references_assertions(host):
    refused = []
    for name, capture, max_prims in fuzz_cases(host):
        orc, code = oracle_hlbvh(capture, max_prims)
        if orc is None:
            assert code == pbrt_hip.ERR_INVALID_ARG, (name, code)
            refused.append(name)
        else:
            orc.close()
    assert len(refused) <= 2 and set(refused) == FUZZ_REFUSED, refused
