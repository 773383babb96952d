"""-m gpu: the device's hit-to-interaction code — tri_dpdu, make_surface_hit / _rec / _any / _q, offset_origin, spawn_ray, spawn_ray_to_hit (csrc/pt_device.h),
camera_ray_differentials, compute_differentials, hit_tex_ctx, hit_bump's own shading frame (csrc/texture.h), tri_shading_dn and specular_ray_differentials
(csrc/shading_diff.h) — against the oracle on explicit hits, through pbrt_hip_surface_probe_batch.  Per set of surface_probe_cases.SETS every output word of every probe must
equal the oracle's bits in libm mode 1 (sign of zero included; a NaN asks for a NaN in the same slot); word 39, the oracle's branch mask, is not compared.
test_surface_probe_cases_cpu.py shows, on the oracle alone, which branches the sets reach and that the oracle itself stands up to a float64 restatement.  No renders here."""
import numpy as np
import pytest

import pbrt_hip
import surface_probe_cases as sc
from oracle_binding import OracleScene, set_libm_mode
from probe_cases import first_difference, hexf

pytestmark = pytest.mark.gpu
F = np.float32
W = sc.MASK   # the words compared: 0 .. 38
_cache = {}


def surface_pair(name, host):
    """(set, product scene, its templates, batches, the oracle's outputs in libm mode 1, product Geo, info) of one set; computed once, shared by the tests below, left unchanged"""
    if name not in _cache:
        ss = sc.SET_BY_NAME[name]
        orc = OracleScene(); prod = pbrt_hip.Scene()
        g_o, info_o, tpl_o, batches = sc.prepare(ss, orc, host)   # the very batches test_surface_probe_cases_cpu.py measured
        g_p, info_p, tpl_p, _ = sc.prepare(ss, prod, host, orc=orc, orc_parts=(info_o, batches))
        set_libm_mode(1)
        try:
            want = sc.run_batches(orc, host, tpl_o, batches, ss.variant)
        finally:
            set_libm_mode(0)
        _cache[name] = (ss, prod, tpl_p, batches, want, g_p, info_p)
    return _cache[name]


def subset(b, keep):
    """the probes `keep` (a mask or an index array) of a batch of editable hits"""
    sub = dict(b)
    for key in ("prim", "inst", "b", "t", "rays", "aux"):
        sub[key] = np.ascontiguousarray(b[key][keep])
    return sub


def position(batches, b):
    return next(i for i, x in enumerate(batches) if x is b)


def assert_same(name, batches, got, want, what, cols=slice(0, W)):
    for b, g, w in zip(batches, got, want):
        g = np.ascontiguousarray(g[:, cols]); w = np.ascontiguousarray(w[:, cols])
        i = first_difference(g, w)
        assert i < 0, f"{what}: {sc.describe(name, b, i)}\n  device {hexf(g[i])}\n  oracle {hexf(w[i])}"


@pytest.mark.parametrize("name", [s.name for s in sc.SETS])
def test_surface_probe_bit_exact(host, name):
    ss, prod, tpl, batches, want, _, _ = surface_pair(name, host)
    assert_same(name, batches, sc.run_batches(prod, host, tpl, batches, ss.variant), want, f"variant {ss.variant}")


@pytest.mark.parametrize("name", [s.name for s in sc.SETS if s.variant == 1 and s.name != "instances"])
def test_prim_indexed_form_equals_the_leaf_record_form(host, name):
    """variant 0 (make_surface_hit, what Light::pdf_li's Triangle::intersect uses) on every hit outside an instance: equal to variant 1 and to the oracle"""
    ss, prod, tpl, batches, want, _, _ = surface_pair(name, host)
    bs, ws = [], []
    for b, w in zip(batches, want):
        keep = b["inst"] == 0
        if keep.any():
            bs.append(subset(b, keep)); ws.append(w[keep])
    assert sum(len(b["prim"]) for b in bs) >= 500
    v0 = sc.run_batches(prod, host, tpl, bs, 0)
    assert_same(name, bs, v0, ws, "variant 0 against the oracle")
    assert_same(name, bs, v0, sc.run_batches(prod, host, tpl, bs, 1), "variant 0 against variant 1")


def test_quadric_form_equals_the_leaf_record_form_on_triangles(host):
    """variant 2 (make_surface_hit_q<true>) on the triangle hits of the scene that also holds the six quadrics and a curve: equal to variant 1 (and, above, to the oracle)"""
    ss, prod, tpl, batches, want, _, _ = surface_pair("quadrics_and_curves", host)
    bs = [b for b in batches if "hits" not in b]
    assert sum(len(b["prim"]) for b in bs) >= 2500 and {b["op"] for b in bs} == {0, 1, 2, 3, 4}
    assert_same("quadrics_and_curves", bs, sc.run_batches(prod, host, tpl, bs, 2), sc.run_batches(prod, host, tpl, bs, 1), "variant 2 against variant 1")


@pytest.mark.parametrize("name", ["flags32", "degenerate_frames", "instances", "bump"])
def test_second_and_third_copy_of_the_shading_frame_match_the_oracle(host, name):
    """tri_shading_dn's dn/du, dn/dv (op 1, words 30 .. 35) against the oracle's shading dndu, dndv; hit_bump's result (op 2), which rests on its private dpdv_s, dn/du, dn/dv
    and their instance transform, against the oracle's bump on the oracle's own interaction"""
    ss, prod, tpl, batches, want, _, _ = surface_pair(name, host)
    for op, cols, what in ((1, slice(30, 36), "tri_shading_dn"), (2, slice(0, 6), "hit_bump")):
        sub = [(b, w) for b, w in zip(batches, want) if b["op"] == op]
        if not sub:
            assert op not in ss.ops
            continue
        bs, ws = [b for b, _ in sub], [w for _, w in sub]
        assert_same(name, bs, sc.run_batches(prod, host, tpl, bs, 1), ws, what, cols)
        if op == 1 and name != "bump":
            assert any(np.any(w[:, 30:36] != 0) for w in ws)   # the derivatives are there to be compared


def test_results_do_not_depend_on_a_probes_place_in_the_wave(host):
    ss, prod, tpl, batches, want, _, _ = surface_pair("flags32", host)
    b = next(b for b in batches if b["op"] == 0)
    n = len(b["prim"])
    base = sc.run_batches(prod, host, tpl, [b], 1)[0]
    for perm in (np.arange(n)[::-1], np.random.default_rng(5).permutation(n)):
        pb = subset(b, perm)
        got = sc.run_batches(prod, host, tpl, [pb], 1)[0]
        back = np.empty_like(got); back[perm] = got
        assert np.array_equal(back.view(np.uint32), base.view(np.uint32))


def test_curve_segments_through_the_quadric_form_equal_the_curve_probe(host):
    """The oracle holds no Curve shape (curve_restatement.py pins the device's curve code), so a curve hit's interaction is compared with pbrt_hip_curve_probe_batch — curve_test
    and curve_surface on the same ray — wherever that probe retires with the very t, u, v the traversal reported: op 0's p, p_error, n, shading n = n, shading dp/du = dp/du
    and op 1's uv, dp/du, dp/dv."""
    ss, prod, tpl, batches, want, g, info = surface_pair("quadrics_and_curves", host)
    rng = np.random.default_rng(11)
    cp = info["curve_cp"].astype(np.float64)
    ts = rng.random(120)[:, None]
    on_curve = ((1 - ts) ** 3) * cp[0] + 3 * ((1 - ts) ** 2) * ts * cp[1] + 3 * (1 - ts) * ts * ts * cp[2] + (ts ** 3) * cp[3]
    o = on_curve + np.array([0.0, 0.0, 2.0]) + rng.normal(size=on_curve.shape) * 0.3
    rays = np.zeros(len(o), pbrt_hip.RAY_DTYPE)
    rays["o"] = o.astype(F); rays["d"] = (on_curve + rng.normal(size=on_curve.shape) * 0.02 - o).astype(F); rays["t_max"] = np.inf; rays["time"] = sc.TIME
    hits = prod.intersect_batch(rays)
    compared = 0
    for prim in range(info["curve_first"], info["curve_first"] + 2):
        sel = hits["prim"] == prim
        if not sel.any():
            continue
        r, h = rays[sel], hits[sel]
        cpo = prod.curve_probe(prim, r)
        same = (cpo[:, 0] == 1) & (cpo[:, 1].view(np.uint32) == h["t"].view(np.uint32)) & (cpo[:, 2].view(np.uint32) == h["b0"].view(np.uint32)) & \
               (cpo[:, 3].view(np.uint32) == h["b1"].view(np.uint32))
        r, h, cpo = r[same], h[same], cpo[same]
        aux = sc.default_aux(len(r), rng)
        o0 = prod.surface_probe_batch(0, r, h, aux, variant=2)
        o1 = prod.surface_probe_batch(1, r, h, aux, variant=2)
        u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)
        assert np.array_equal(u32(o0[:, 0:3]), u32(cpo[:, 4:7])) and np.array_equal(u32(o0[:, 3:6]), u32(cpo[:, 7:10]))
        assert np.array_equal(u32(o0[:, 9:12]), u32(cpo[:, 16:19])) and np.array_equal(u32(o0[:, 12:15]), u32(cpo[:, 16:19])) and np.array_equal(u32(o0[:, 15:18]), u32(cpo[:, 10:13]))
        assert np.array_equal(u32(o1[:, 0:2]), u32(cpo[:, 2:4])) and np.array_equal(u32(o1[:, 2:5]), u32(cpo[:, 10:13])) and np.array_equal(u32(o1[:, 5:8]), u32(cpo[:, 13:16]))
        assert np.array_equal(o0[:, 19].view(np.uint32), h["prim"])
        compared += len(r)
    assert compared >= 8, compared


def test_refusals_leave_the_handle_usable(host):
    ss, prod, tpl, batches, want, g, info = surface_pair("instances", host)
    b = next(b for b in batches if b["op"] == 0)
    k = 64   # an 8 x 8 probe
    rays, hits, aux = b["rays"][:k], sc.hits_of(tpl, b)[:k], b["aux"][:k]

    def refused(scene, code, op, r, h, a, **kw):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            scene.surface_probe_batch(op, r, h, a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert scene.last_error() != ""

    def edited(**kw):
        h = hits.copy()
        for key, v in kw.items():
            if key.startswith("pad"):
                h["pad"][3, int(key[3])] = v
            else:
                h[key][3] = v
        return h

    n_recs = prod.accel_stats()["leaf_records"]
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 5, rays, hits, aux)                               # an unknown op
    refused(prod, pbrt_hip.ERR_INVALID_ARG, -1, rays, hits, aux)
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, rays, hits, aux, variant=3)                    # an unknown variant
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, rays, edited(prim=0xFFFFFFFF), aux)            # a miss
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, rays, edited(prim=len(g.tris)), aux)           # no primitive
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, rays, edited(pad0=n_recs), aux)                # no leaf record
    other = next(tpl[key]["pad"][0] for key in tpl if key != "real" and key[0] != int(hits["prim"][3]))
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, rays, edited(pad0=other), aux)                 # another primitive's leaf record
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, rays, edited(pad1=len(g.instances) + 1), aux)  # no instance
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 2, rays, hits, aux, texture=len(g.tex) + 50)      # an unknown texture
    refused(prod, pbrt_hip.ERR_UNSUPPORTED, 0, rays, hits, aux, variant=0)                    # hits inside instances have no prim-indexed form
    refused(prod, pbrt_hip.ERR_UNSUPPORTED, 0, rays, hits, aux, variant=2)                    # no quadric in this scene: no such instantiation
    fn = prod.b.fn("surface_probe_batch")
    out = np.zeros((k, sc.STRIDE), F)
    fp = lambda a: a.ctypes.data_as(pbrt_hip.C.POINTER(pbrt_hip.C.c_float))
    r2, h2, a2 = rays.copy(), hits.copy(), aux.copy()
    assert fn(prod.h, 0, 1, 0, 0, k, None, h2.ctypes.data, fp(a2), fp(out)) == pbrt_hip.ERR_INVALID_ARG        # null arrays with n > 0
    assert fn(prod.h, 0, 1, 0, 0, k, r2.ctypes.data, None, fp(a2), fp(out)) == pbrt_hip.ERR_INVALID_ARG
    assert fn(prod.h, 0, 1, 0, 0, k, r2.ctypes.data, h2.ctypes.data, None, fp(out)) == pbrt_hip.ERR_INVALID_ARG
    assert fn(prod.h, 0, 1, 0, 0, k, r2.ctypes.data, h2.ctypes.data, fp(a2), None) == pbrt_hip.ERR_INVALID_ARG
    assert fn(prod.h, 0, 1, 0, 0, 2 ** 32, r2.ctypes.data, h2.ctypes.data, fp(a2), fp(out)) == pbrt_hip.ERR_INVALID_ARG   # more than 2^32 - 1 probes
    assert prod.last_error() != ""
    assert fn(None, 0, 1, 0, 0, k, r2.ctypes.data, h2.ctypes.data, fp(a2), fp(out)) == pbrt_hip.ERR_INVALID_ARG          # no handle
    assert fn(prod.h, 0, 1, 0, 0, 0, None, None, None, None) == pbrt_hip.OK                                               # nothing to do
    # quadric slots and curve segments
    qs, qprod, qtpl, qb, qwant, qg, qinfo = surface_pair("quadrics_and_curves", host)
    real = next(b for b in qb if "hits" in b and b["op"] == 0)
    qh = sc.hits_of(qtpl, real)[:4]; qr = real["rays"][:4]; qa = real["aux"][:4]
    refused(qprod, pbrt_hip.ERR_UNSUPPORTED, 0, qr, qh, qa, variant=1)                        # a quadric's interaction comes from variant 2 alone
    refused(qprod, pbrt_hip.ERR_UNSUPPORTED, 0, qr, qh, qa, variant=0)
    cp = qinfo["curve_cp"].astype(np.float64)
    mid = 0.125 * cp[0] + 0.375 * cp[1] + 0.375 * cp[2] + 0.125 * cp[3]
    cr = np.zeros(1, pbrt_hip.RAY_DTYPE); cr["o"] = (mid + [0, 0, 2.0]).astype(F); cr["d"] = np.array([0, 0, -2.0], F); cr["t_max"] = np.inf
    ch = qprod.intersect_batch(cr)
    assert ch["prim"][0] >= qinfo["curve_first"]
    refused(qprod, pbrt_hip.ERR_UNSUPPORTED, 2, cr, ch, qa[:1], variant=2, texture=qg.tex["one"])   # Material::bump on a curve segment
    # no accelerator; a camera ray without a camera, a film or a sampler
    bare = pbrt_hip.Scene()
    gb = sc.Geo(bare, host)
    gb.mesh(sc.TRI)
    refused(bare, pbrt_hip.ERR_STATE, 0, rays[:1], hits[:1], aux[:1])
    bare.build_accel(0, 4)
    bt = sc.learn_templates(bare, gb)
    bb = sc.batch(gb, 1, [0] * 4, 0, sc.CENTROID, np.array([0.1, 0.2, -1.0], F), np.random.default_rng(3), "bare")
    refused(bare, pbrt_hip.ERR_STATE, 1, bb["rays"], sc.hits_of(bt, bb), bb["aux"], camera_ray=True)
    refused(bare, pbrt_hip.ERR_STATE, 2, bb["rays"], sc.hits_of(bt, bb), bb["aux"], camera_ray=True, texture=gb.tex["one"])
    assert bare.surface_probe_batch(1, bb["rays"], sc.hits_of(bt, bb), bb["aux"]).shape == (4, sc.STRIDE)   # without camera_ray nothing is missing
    # the handles still answer, and as before
    sub = subset(b, np.arange(k))
    assert_same("instances", [sub], sc.run_batches(prod, host, tpl, [sub], 1), [want[position(batches, b)][:k]], "after the refusals")
    assert_same("quadrics_and_curves", [real], sc.run_batches(qprod, host, qtpl, [real], 2), [qwant[position(qb, real)]], "after the refusals")
