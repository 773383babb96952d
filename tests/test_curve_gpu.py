"""-m gpu: the reference's Curve shape on the device (csrc/curve.h) through pbrt_hip_add_curve.  The yardstick is tests/curve_restatement.py — NumPy float32 written from
shapes/src/curve.rs — and the comparisons are on bits (`view(np.uint32)`), never against the device's own output:
  - the probe: curve_test + curve_surface of single segments on every output word, closest-hit and shadow mode (tests/curve_cases.py: all three types, unequal and zero
    widths, a non-uniform mirror with ReverseOrientation, coincident and collinear control points, rays along the chord, from inside the width, with short t_max, stray
    ones, and the two hand-built quirk cases);
  - scene level, order pinned: scenes of <= 16 primitives — curve segments at split depths 0 .. 3 with a triangle and a sphere among them — where intersect_batch /
    occluded_batch must equal the restatement run over the primitives in the order the reference's BVHAccel::intersect meets them, with the shortening t_max (the oracle's
    entry points answer for the triangle and the sphere).  The reference's builders do NOT make one leaf of such a scene whatever max_prims_in_node is (sah.rs:350-351 splits
    wherever that is cheaper, hlbvh.rs sorts into treelets), so the order is not `add` order: it is read off the built tree — accel_copy's arrays — by walking it as
    bvh/mod.rs:173-226 does, boxes tested as bounds3.rs:292-325 tests them.  Host- and device-built trees, SAH and HLBVH; host and device builds give the same arrays;
  - the refusals of pbrt_hip_add_curve that need a handle."""
import numpy as np
import pytest

import curve_cases as CC
import curve_restatement as cr
import pbrt_hip
from oracle_binding import OracleScene, set_libm_mode

pytestmark = pytest.mark.gpu
MISS = 0xFFFFFFFF
RAYS_PER_CURVE = 4096


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def add_curve(scene, c, material):
    scene.add_curve(c["t"][0], c["t"][1], c["type"], c["cp"], c["width"], c["n"], c["split_depth"], material, c["reverse"])


@pytest.fixture(scope="module")
def probe_set(host):
    """(curves, first primitive of each, rays of each, the restatement's closest-hit rows and shadow flags): computed once"""
    curves = CC.probe_curves(host)
    rng = np.random.default_rng(5)
    rays = [CC.probe_rays(c, RAYS_PER_CURVE, rng) for c in curves]
    rays[-2][0] = CC.quirk_rays(CC.WRONG_HALF, CC.WRONG_HALF["t_short"])[0]; rays[-2][1] = CC.quirk_rays(CC.WRONG_HALF, CC.WRONG_HALF["t_long"])[0]
    rays[-1][0] = CC.quirk_rays(CC.OVERWRITE, CC.INF)[0]
    segs = cr.stack_segments([CC.restatement_segment(c)[1] for c in curves], [len(r) for r in rays])
    allr = np.concatenate(rays)
    want = cr.intersect(segs, allr["o"], allr["d"], allr["t_max"], shadow=False)
    want_p = cr.intersect(segs, allr["o"], allr["d"], allr["t_max"], shadow=True)[:, 0] != 0
    first, prim = [], 0
    for c in curves:
        first.append(prim); prim += 1 << c["split_depth"]
    return curves, first, rays, want, want_p


def test_probe_matches_the_restatement_bit_for_bit(probe_set):
    curves, first, rays, want, want_p = probe_set
    sc = pbrt_hip.Scene()
    m = sc.add_material_matte((0.5, 0.5, 0.5)); sc.add_light_infinite((1.0, 1.0, 1.0))
    for c in curves:
        add_curve(sc, c, m)
    sc.build_accel(0, 4)
    at = 0
    n_hit = n_hit_p = n_differ = 0
    for k, (c, r) in enumerate(zip(curves, rays)):
        w, wp = want[at:at + len(r)], want_p[at:at + len(r)]
        at += len(r)
        got = sc.curve_probe(first[k] + c["seg"], r, shadow=False)
        got_p = sc.curve_probe(first[k] + c["seg"], r, shadow=True)
        bad = np.nonzero((bits(got) != bits(w)).any(axis=1))[0]
        assert len(bad) == 0, f"curve {k} (type {c['type']}, split {c['split_depth']}): {len(bad)} rays differ, first {bad[0]}: got {got[bad[0]]} want {w[bad[0]]}"
        assert np.array_equal(got_p[:, 0] != 0, wp), f"curve {k}: shadow mode differs on {np.count_nonzero((got_p[:, 0] != 0) != wp)} rays"
        assert not got_p[:, 1:].any(), "shadow mode reports the accept decision alone"
        n_hit += int((w[:, 0] != 0).sum()); n_hit_p += int(wp.sum()); n_differ += int(((w[:, 0] != 0) != wp).sum())
    # the set does what it is for: plenty of hits in both modes, and rays on which the two modes disagree (the overwrite quirk)
    assert n_hit > 5000 and n_hit_p > 5000 and n_differ > 100, (n_hit, n_hit_p, n_differ)
    # the hand-built cases are in it, with the reference's odd answers
    wh = want[-2 * RAYS_PER_CURVE:-RAYS_PER_CURVE]
    assert wh[0, 0] == 0 and wh[1, 0] == 1 and wh[1, 1] < CC.WRONG_HALF["t_short"]
    assert want[-RAYS_PER_CURVE, 0] == 0 and want_p[-RAYS_PER_CURVE]
    sc.close()


# ---- scene level -----------------------------------------------------------------------------------------------------------------------------------------------
TRI_P = np.array([[-0.9, -0.8, 0.35], [0.9, -0.7, 0.3], [0.1, 0.9, 0.4]], np.float32)


def small_scene(host, scene, which):
    """<= 16 primitives in `add` order; returns the list of ("curve", restatement segment) / ("tri",) / ("sphere",) per primitive slot"""
    m = scene.add_material_matte((0.5, 0.5, 0.5)); scene.add_light_infinite((1.0, 1.0, 1.0))
    tfs = CC.transforms(host)
    rng = np.random.default_rng(100 + which)
    prims = []

    def curve(split, ctype, t, rev=False):
        c = dict(type=ctype, cp=rng.uniform(-1, 1, (4, 3)).astype(np.float32), width=rng.uniform(0.1, 0.5, 2).astype(np.float32),
                 n=rng.normal(size=(2, 3)).astype(np.float32) if ctype == cr.RIBBON else None, split_depth=split, seg=0, t=t, reverse=rev)
        if hasattr(scene, "add_curve"):
            add_curve(scene, c, m)
        cd = cr.curve_data(c["type"], c["cp"], c["width"], c["n"])
        for (a, b) in cr.create_segments(split):
            prims.append(("curve", cr.segment(cd, a, b, t[0], t[1], rev)))

    def tri():
        scene.add_mesh(TRI_P, np.array([0, 1, 2], np.uint32), m); prims.append(("tri",))

    def sphere():
        scene.add_sphere(tfs[1][0][0], tfs[1][0][1], 0.6, None, None, 360.0, m, False); prims.append(("sphere",))
    if which == 0:
        curve(0, cr.FLAT, tfs[0][0]); tri(); curve(1, cr.CYLINDER, tfs[1][0]); sphere(); curve(2, cr.RIBBON, tfs[2][0], True)      # 1 + 1 + 2 + 1 + 4 = 9
    else:
        curve(3, cr.CYLINDER, tfs[0][0]); sphere(); curve(2, cr.FLAT, tfs[3][0], True); tri(); curve(0, cr.RIBBON, tfs[1][0]); curve(0, cr.FLAT, tfs[2][0])   # 8 + 1 + 4 + 1 + 1 + 1 = 16
    return prims


def scene_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.2, 4.0, (n, 1))
    tgt = rng.uniform(-1.0, 1.0, (n, 3))
    r = CC.mk_rays(o, (tgt - o) * rng.uniform(0.4, 1.5, (n, 1)))
    short = rng.integers(0, 4, n) == 0
    r["t_max"][short] = rng.uniform(0.4, 1.5, short.sum()).astype(np.float32)
    return r


def _oracle_one(host, kind):
    o = OracleScene()
    m = o.add_material_matte((0.5, 0.5, 0.5)); o.add_light_infinite((1.0, 1.0, 1.0))
    if kind == "tri": o.add_mesh(TRI_P, np.array([0, 1, 2], np.uint32), m)
    else:
        t = CC.transforms(host)[1][0]; o.add_sphere(t[0], t[1], 0.6, None, None, 360.0, m, False)
    o.build_accel(0, 4)
    return o


class _Recorder:
    """small_scene's bookkeeping without a scene"""
    def add_material_matte(self, *a): return 0
    def add_light_infinite(self, *a): pass
    def add_mesh(self, *a): pass
    def add_sphere(self, *a): pass


_BOX_SCALE = np.float32(1) + np.float32(2) * cr._GAMMA3


def _box_pass(lo, hi, o, inv, neg, t_max):
    """Bounds3::intersect_p_inv (bounds3.rs:292-325) of one box against many rays"""
    F = np.float32
    near = [np.where(neg[:, k], hi[k], lo[k]).astype(np.float32) for k in range(3)]; far = [np.where(neg[:, k], lo[k], hi[k]).astype(np.float32) for k in range(3)]
    with np.errstate(all="ignore"):
        t_min = (near[0] - o[:, 0]) * inv[:, 0]; t_mx = (far[0] - o[:, 0]) * inv[:, 0]
        ty_min = (near[1] - o[:, 1]) * inv[:, 1]; ty_max = (far[1] - o[:, 1]) * inv[:, 1]
        t_mx = t_mx * _BOX_SCALE; ty_max = ty_max * _BOX_SCALE
        ok = ~((t_min > ty_max) | (ty_min > t_mx))
        t_min = np.where(ty_min > t_min, ty_min, t_min); t_mx = np.where(ty_max < t_mx, ty_max, t_mx)
        tz_min = (near[2] - o[:, 2]) * inv[:, 2]; tz_max = (far[2] - o[:, 2]) * inv[:, 2]
        ok &= ~((t_min > tz_max) | (tz_min > t_mx))
        t_min = np.where(tz_min > t_min, tz_min, t_min); t_mx = np.where(tz_max < t_mx, tz_max, t_mx)
        return ok & (t_min < t_max) & (t_mx > F(0))


def reference_answers(host, prims, nodes, recs, n_interior, rays):
    """BVHAccel::intersect (bvh/mod.rs:173-226) and ::intersect_p (:231-283) over the tree in `nodes` / `recs` (the device layout: an interior node holds its two children's
    boxes, references and its split axis; a leaf reference names its first record, the last record of a leaf carries bit 0 of its flags), one primitive test at a time"""
    LEAF = 0x80000000
    n = len(rays)
    nf = nodes.view(np.float32)
    box = {}
    for k in range(n_interior):
        for c in range(2):
            b = nf[k, 6 * c:6 * c + 6]
            box[int(nodes[k, 12 + c])] = (b[0::2].copy(), b[1::2].copy())
    if n_interior:
        (l0, h0), (l1, h1) = box[int(nodes[0, 12])], box[int(nodes[0, 13])]
        box[0] = (np.minimum(l0, l1), np.maximum(h0, h1))
        root = 0
    else:
        root = LEAF
    orcs = {k: _oracle_one(host, k) for k in ("tri", "sphere")}
    o, d = rays["o"], rays["d"]
    with np.errstate(all="ignore"):
        inv = (np.float32(1) / d).astype(np.float32)
    neg = inv < 0
    t_max = rays["t_max"].copy(); t0 = rays["t_max"].copy()
    hit_prim = np.full(n, MISS, np.uint32); b0 = np.zeros(n, np.float32); b1 = np.zeros(n, np.float32)
    cur = np.full(n, root, np.int64); stack = np.zeros((n, 64), np.int64); sp = np.zeros(n, np.int64)
    tested = 0

    def leaf_records(ref):
        k = ref & 0x7FFFFFFF
        while True:
            yield k
            if recs[k, 7] & 1: return
            k += 1

    def pop(idx):
        has = sp[idx] > 0
        sp[idx[has]] -= 1
        cur[idx[has]] = stack[idx[has], sp[idx[has]]]
        cur[idx[~has]] = -1
    set_libm_mode(1)
    try:
        while True:
            live = np.nonzero(cur >= 0)[0]
            if not len(live): break
            for ref in np.unique(cur[live]):
                ref = int(ref)
                idx = live[cur[live] == ref]
                if ref in box:
                    lo, hi = box[ref]
                    ok = _box_pass(lo, hi, o[idx], inv[idx], neg[idx], t_max[idx])
                    pop(idx[~ok]); idx = idx[ok]
                if not len(idx): continue
                if ref & LEAF:
                    for k in leaf_records(ref):
                        slot = int(recs[k, 3]); p = prims[slot]
                        r = rays[idx].copy(); r["t_max"] = t_max[idx]
                        if p[0] == "curve":
                            res = cr.intersect(cr.stack_segments([p[1]], [len(idx)]), r["o"], r["d"], r["t_max"], shadow=False)
                            h = res[:, 0] != 0; t, u, v = res[:, 1], res[:, 2], res[:, 3]
                        else:
                            hr = orcs[p[0]].intersect_batch(r)
                            h = hr["prim"] != MISS; t, u, v = hr["t"], hr["b0"], hr["b1"]
                        w = idx[h]
                        t_max[w] = t[h]; hit_prim[w] = slot; b0[w] = u[h]; b1[w] = v[h]
                        tested += len(idx)
                    pop(idx)
                else:
                    axis = int(nodes[ref, 14]); c0, c1 = int(nodes[ref, 12]), int(nodes[ref, 13])
                    far_first = neg[idx, axis]        # dir_is_neg[axis]: the first child waits, the second is visited
                    stack[idx, sp[idx]] = np.where(far_first, c0, c1); sp[idx] += 1
                    cur[idx] = np.where(far_first, c1, c0)
        # shadow rays keep their t_max: a primitive is tested if every box on the way to its leaf is met; the answer is whether any tested primitive is hit
        occ = np.zeros(n, bool)

        def walk(ref, reach):
            if ref in box:
                lo, hi = box[ref]
                reach = reach & _box_pass(lo, hi, o, inv, neg, t0)
            if not reach.any(): return
            if ref & LEAF:
                for k in leaf_records(ref):
                    p = prims[int(recs[k, 3])]
                    idx = np.nonzero(reach)[0]
                    if p[0] == "curve":
                        sh = cr.intersect(cr.stack_segments([p[1]], [len(idx)]), o[idx], d[idx], t0[idx], shadow=True)[:, 0] != 0
                    else:
                        sh = orcs[p[0]].occluded_batch(rays[idx]) != 0
                    occ[idx[sh]] = True
            else:
                walk(int(nodes[ref, 12]), reach); walk(int(nodes[ref, 13]), reach)
        walk(root, np.ones(n, bool))
    finally:
        set_libm_mode(0)
    for oc in orcs.values():
        oc.close()
    return t_max, hit_prim, b0, b1, occ, tested


@pytest.mark.parametrize("which", [0, 1])
def test_small_scene_in_the_trees_own_order(host, which):
    rays = scene_rays(6000, 40 + which)
    prims = small_scene(host, _Recorder(), which)
    assert len(prims) <= 16
    curve_slot = np.array([p[0] == "curve" for p in prims])
    copies = {}
    for build in ("host-sah", "device-sah", "host-hlbvh", "device-hlbvh"):
        sc = pbrt_hip.Scene()
        small_scene(host, sc, which)
        if build == "host-sah": sc.build_accel(0, 16)
        elif build == "host-hlbvh": sc.build_accel(1, 16)
        elif build == "device-sah": sc.build_accel_device_shapes(0, 16)
        else: sc.build_accel_device(1, 16)
        nodes, recs = sc.accel_copy()
        n_interior = sc.accel_stats()["interior_nodes"]
        copies[build] = (nodes[:max(n_interior, 1)].copy(), recs.copy())
        assert sorted(recs[:, 3].tolist()) == list(range(len(prims)))
        want_t, want_prim, want_b0, want_b1, want_occ, tested = reference_answers(host, prims, nodes, recs, n_interior, rays)
        hit = want_prim != MISS
        assert hit.sum() > 800 and len(np.unique(want_prim[hit])) >= 5, (hit.sum(), np.unique(want_prim[hit]))
        hits = sc.intersect_batch(rays); occ = sc.occluded_batch(rays)
        assert np.array_equal(hits["prim"], want_prim), f"{build}: {np.count_nonzero(hits['prim'] != want_prim)} rays report another primitive"
        assert np.array_equal(bits(hits["t"])[hit], bits(want_t)[hit]), build
        assert np.array_equal(bits(hits["b0"])[hit], bits(want_b0)[hit]) and np.array_equal(bits(hits["b1"])[hit], bits(want_b1)[hit]), build
        on_curve = hit & curve_slot[np.where(hit, want_prim, 0)]
        assert on_curve.sum() > 200 and not hits["b2"][on_curve].any() and hits["b0"][on_curve].any() and hits["b1"][on_curve].any()
        assert np.array_equal(occ != 0, want_occ), f"{build}: {np.count_nonzero((occ != 0) != want_occ)} shadow rays differ"
        assert want_occ.sum() > 800
        sc.close()
    for method in ("sah", "hlbvh"):
        assert np.array_equal(copies["host-" + method][0], copies["device-" + method][0]) and np.array_equal(copies["host-" + method][1], copies["device-" + method][1]), method


# ---- the refusals of pbrt_hip_add_curve that need a handle --------------------------------------------------------------------------------------------------------
def test_add_curve_refusals(host):
    ident = (pbrt_hip.IDENTITY.copy(), pbrt_hip.IDENTITY.copy())
    cp = np.array([[-1, 0, 0], [0, 1, 0], [1, -1, 0], [2, 0, 0]], np.float32); w = np.array([0.1, 0.2], np.float32); nn = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    sc = pbrt_hip.Scene()
    m = sc.add_material_matte((0.5, 0.5, 0.5)); sc.add_light_infinite((1.0, 1.0, 1.0))

    def refused(code, *a, **kw):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            sc.add_curve(*a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
    refused(pbrt_hip.ERR_INVALID_ARG, ident[0], ident[1], 3, cp, w)                          # an unknown type
    refused(pbrt_hip.ERR_INVALID_ARG, ident[0], ident[1], "ribbon", cp, w)                   # a ribbon without normals
    refused(pbrt_hip.ERR_INVALID_ARG, ident[0], ident[1], "flat", cp, w, None, 17)           # split_depth outside [0, 16]
    refused(pbrt_hip.ERR_INVALID_ARG, ident[0], ident[1], "flat", cp, w, None, -1)
    refused(pbrt_hip.ERR_INVALID_ARG, ident[0], ident[1], "flat", cp, w, None, 3, m + 5)     # an unknown material
    sc.object_begin()
    refused(pbrt_hip.ERR_UNSUPPORTED, ident[0], ident[1], "flat", cp, w, None, 3, m)         # inside an object definition
    sc.object_end()
    sc.add_light_diffuse_area((1.0, 1.0, 1.0), 1)
    refused(pbrt_hip.ERR_UNSUPPORTED, ident[0], ident[1], "flat", cp, w, None, 3, m)         # while an area light waits for its shape
    sc.close()
    sc = pbrt_hip.Scene()
    m = sc.add_material_matte((0.5, 0.5, 0.5)); sc.add_light_infinite((1.0, 1.0, 1.0))
    sc.add_curve(ident[0], ident[1], "ribbon", cp, w, nn, 2, m)
    sc.add_curve(ident[0], ident[1], "cylinder", cp, w, None, 0, m, True)
    tex = sc.add_texture_constant((0.5, 0.5, 0.5))
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        sc.set_last_mesh_alpha_textures(tex, None)
    assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
    sc.build_accel(0, 4)
    assert sc.accel_stats()["leaf_records"] == 5                                              # 2^2 + 2^0 primitive slots
    with pytest.raises(pbrt_hip.PbrtHipError):
        sc.curve_probe(7, CC.mk_rays([[0, 0, 3]], [[0, 0, -1]]))                              # not a curve segment
    sc.close()
