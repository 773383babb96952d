"""Scenes for the HLBVH device build of scenes with quadric shapes (csrc/bvh_device.hip), for either binding: the smallest at which the new code can go wrong.

FLAT scenes are lists of parts — ("mesh", P, idx) or ("shape", kind, transform pair, parameters) in primitive order — so that one description feeds a scene handle (`capture`) and the
host builder's stand-alone entry pbrt_hip_host_build_bvh_shapes (`host_arrays`): tests/test_hlbvh_quadrics_cpu.py pins the host HLBVH builder to the oracle's on exactly the inputs
on which tests/test_hlbvh_quadrics_device_gpu.py pins the device builder to the host builder.  INSTANCED and MASKED scenes are capture functions (that entry takes no instances); the
CPU test checks on them what the oracle alone decides: whether the reference's HLBVH build asserts."""
import numpy as np

import quadric_alpha_scenes as QA
import quadric_instance_scenes as QI
from test_quadrics_capi import KIND_NO, _add, _shapes

I4 = QI.I4


# ---- flat scenes ------------------------------------------------------------------------------------------------------------------------------------------------------
def _mesh(host, n, seed, offset=(0, 0, 0)):
    P, idx = host.gen_random_tris(n, seed)
    return ("mesh", P + np.float32(offset), np.ascontiguousarray(idx, np.uint32))


def _shape_parts(host, n, seed):
    return [("shape",) + sh for sh in _shapes(host, n, seed)]


def same_centroid(host):
    """a full sphere and a disk at its centre: both bounds have the centroid (0.25, -0.5, 0.125), so equal Morton codes in one treelet"""
    t = QA.cf_ctm(host, host.translate((0.25, -0.5, 0.125)))
    return [("shape", "sphere", t, [1.0, -1.0, 1.0, 360.0, 0, 0, 0]), ("shape", "disk", t, [0.5, 0.0, 0.0, 360.0, 0, 0, 0])]


def interleaved(host, n=300):
    """n triangles and n quadrics in turn: every 256-thread block of the bounds and record kernels holds both kinds"""
    P, idx = host.gen_random_tris(n, 13)
    shapes = _shape_parts(host, n, 77)
    parts = []
    for k in range(n):
        parts += [("mesh", P[3 * k:3 * k + 3], np.arange(3, dtype=np.uint32)), shapes[k]]
    return parts


FLAT = {
    "one quadric": lambda h: _shape_parts(h, 5, 3)[4:],                     # a sphere; no interior node, no vertex at all
    "two quadrics": lambda h: _shape_parts(h, 2, 5),
    "six quadrics": lambda h: _shape_parts(h, 6, 10),                       # one of each kind
    "quadric first and last": lambda h: (lambda q: [q[0], _mesh(h, 20, 3), q[1], q[2], _mesh(h, 20, 4, (0.3, 0.1, -0.2)), q[3]])(_shape_parts(h, 4, 21)),
    "meshes around quadrics": lambda h: [_mesh(h, 30, 9)] + _shape_parts(h, 12, 16) + [_mesh(h, 31, 8)],   # test_quadrics_capi.py's layout
    "same centroid": same_centroid,
    "300 + 300 interleaved": interleaved,
}


def capture_flat(parts):
    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        for p in parts:
            if p[0] == "mesh": s.add_mesh(p[1], p[2], m)
            else: _add(s, p[1], p[2], p[3], m)
    return capture


def host_arrays(parts):
    """-> P, idx (n x 3), prim_shape (n), shape records (n_shapes x 40): the arguments of pbrt_hip_host_build_bvh_shapes"""
    Ps, rows, prim_shape, recs, base = [np.zeros((0, 3), np.float32)], [], [], [], 0
    for p in parts:
        if p[0] == "mesh":
            Ps.append(np.asarray(p[1], np.float32)); tri = np.asarray(p[2], np.uint32).reshape(-1, 3) + np.uint32(base)
            rows += list(tri); prim_shape += [0] * len(tri); base += len(p[1])
        else:
            rec = np.zeros(40, np.float32)
            rec[0] = KIND_NO[p[1]]; rec[1:17] = np.asarray(p[2][0], np.float32).ravel(); rec[17:33] = np.asarray(p[2][1], np.float32).ravel(); rec[33:40] = p[3]
            recs.append(rec); rows.append(np.zeros(3, np.uint32)); prim_shape.append(len(recs))
    P = np.ascontiguousarray(np.concatenate(Ps), np.float32)
    if not len(P): P = np.zeros((1, 3), np.float32)      # (a pointer to pass; no slot reads it)
    return P, np.ascontiguousarray(np.array(rows, np.uint32).reshape(-1, 3)), np.array(prim_shape, np.uint32), np.ascontiguousarray(np.array(recs, np.float32).reshape(-1, 40))


# ---- scenes with object instances, scenes with masks: capture(scene) builds nothing ------------------------------------------------------------------------------------
def interleaved_instanced(host):
    """300 + 300 interleaved at scene level and three instances among them: 603 scene-level items, so the block of threads 512 .. 767 straddles the scene's tree and the first
    object's; objects of 250, 1 and 7 triangles: tree boundaries inside blocks"""
    flat = capture_flat(interleaved(host))
    T = QI.transforms(host)
    objs = [host.gen_random_tris(k, 40 + k) for k in (250, 1, 7)]

    def capture(s):
        m = s.add_material_matte((0.2, 0.6, 0.8), 0.0)
        obs = []
        for P, idx in objs:
            ob = s.object_begin(); s.add_mesh(P * np.float32(0.8), idx, m); s.object_end(); obs.append(ob)
        s.add_instance(obs[0], *T[0])
        flat(s)
        s.add_instance(obs[1], *T[1]); s.add_instance(obs[2], *T[2])
    return capture


def quadrics_and_instances_only(host):
    """the scene's own tree holds quadrics and instances and no triangle; one of the objects has a single primitive"""
    shapes = _shapes(host, 7, 33)
    T = QI.transforms(host)
    P, idx = host.gen_random_tris(120, 31)

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        ob = s.object_begin(); s.add_mesh(P, idx, m); s.object_end()
        one = s.object_begin(); s.add_mesh(P[:3] * np.float32(2.0), [0, 1, 2], m); s.object_end()
        for k, (kind, t, par) in enumerate(shapes):
            _add(s, kind, t, par, m)
            if k < 4: s.add_instance(one if k == 2 else ob, *T[k])
    return capture


INSTANCED = {
    "stage": lambda h: (lambda s: QI.stage(s, h, split=1, build=False)),
    "one leaf, triangle first": lambda h: (lambda s: QI.one_leaf(s, h, instance_first=False, build=False)),
    "one leaf, instance first": lambda h: (lambda s: QI.one_leaf(s, h, instance_first=True, build=False)),
    "300 + 300 interleaved beside instances": interleaved_instanced,
    "quadrics and instances only": quadrics_and_instances_only,
}
# (mixed_scene ends with a SAH host build of its own; the tests build again on the same handle)
MASKED = {f"mixed scene, {mask}": (lambda h, mask=mask: (lambda s: QA.mixed_scene(s, h, mask=mask, shadow=True, res=(16, 16)))) for mask in QA.MASKS}


def all_scenes():
    """name -> host -> capture(scene)"""
    out = {name: (lambda h, f=f: capture_flat(f(h))) for name, f in FLAT.items()}
    out.update(INSTANCED); out.update(MASKED)
    return out


RAY_BOUND = {"stage": 3.5, "300 + 300 interleaved beside instances": 3.5, "quadrics and instances only": 3.5, "mixed scene, imagemap": 2.5, "mixed scene, checkerboard": 2.5}
