"""The surface probe case sets (surface_probe_cases.py) on the oracle alone: every set's batches run; the oracle's branch masks show that the sets reach the branches they were
built for, so that the GPU comparison (test_surface_probe_gpu.py) is known to cover them; and the oracle's outputs satisfy properties worked out from a float64 restatement of
the reference (surface_restatement.py) — exact ones (the hit point lies within its error box, spawned rays start on the right side of the exact plane, the normals' signs) and
approximate ones, whose residuals are measured here and quoted in surface_restatement.RESIDUALS."""
import numpy as np
import pytest

import surface_probe_cases as sc
import surface_restatement as sr
from oracle_binding import OracleScene
from surface_probe_cases import F

_cache = {}
NAMES = [s.name for s in sc.SETS]


def surface_set(name, host):
    """(oracle scene, Geo, info, templates, batches, outputs) of one set, computed once and left unchanged"""
    if name not in _cache:
        ss = sc.SET_BY_NAME[name]
        orc = OracleScene()
        g, info, tpl, batches = sc.prepare(ss, orc, host)
        _cache[name] = (orc, g, info, tpl, batches, sc.run_batches(orc, host, tpl, batches, ss.variant))
    return _cache[name]


def tri_probes(g, b):
    """indices of a batch's probes that lie on triangles (every probe of a batch without real hits), or an empty list"""
    return [] if "hits" in b else list(range(len(b["prim"])))


def matrix_of(g, inst):
    return None if inst == 0 else g.instances[inst - 1][1]


@pytest.mark.parametrize("name", NAMES)
def test_every_set_runs_with_500_probes_per_op(host, name):
    _, g, _, _, batches, outs = surface_set(name, host)
    per_op = {}
    nan = total = 0
    for b, o in zip(batches, outs):
        assert o.shape == (len(b["rays"]), sc.STRIDE), b["tag"]
        per_op[b["op"]] = per_op.get(b["op"], 0) + len(o)
        nan += int(np.isnan(o[:, :sc.MASK]).any(axis=1).sum()); total += len(o)
    print(f"\nsurface[{name}]: primitives {len(g.tris)}, probes per op {per_op}, with a NaN {nan}, branch bits {sc.bit_names(sc.bits_of(outs))}")
    assert set(per_op) == set(sc.SET_BY_NAME[name].ops)
    assert all(v >= 500 for v in per_op.values()), per_op
    assert len(g.tris) < 200 and max(len(o) for o in outs) <= 5000
    assert nan <= 0.05 * total   # a set must not pass on NaNs: only `rays` holds any, by construction


@pytest.mark.parametrize("name", NAMES)
def test_each_set_reaches_the_branches_it_exists_for(host, name):
    outs = surface_set(name, host)[5]
    got = sc.bits_of(outs)
    missing = sc.SET_BY_NAME[name].expect & ~got
    assert not missing, f"set {name} does not reach {sc.bit_names(missing)}"


def test_the_sets_together_reach_every_listed_branch(host):
    union = 0
    for name in NAMES:
        union |= sc.bits_of(surface_set(name, host)[5])
    assert union & sc.ALL_BITS == sc.ALL_BITS, f"no set reaches {sc.bit_names(sc.ALL_BITS & ~union)}"
    assert union & ~sc.ALL_BITS == 0, "the oracle reports a branch bit that surface_probe_cases.BITS does not list"


def test_every_flag_combination_and_both_sides_are_in_flags32(host):
    _, g, _, _, batches, outs = surface_set("flags32", host)
    combos = {(t["N"] is not None, t["S"] is not None, t["UV"] is not None, t["rev"], t["swp"]) for t in g.tris}
    assert len(combos) == 32
    o = np.concatenate([o for b, o in zip(batches, outs) if b["op"] == 0])
    ff = (o[:, sc.MASK].view(np.uint32) & sc.BITS["FACE_FORWARD"]) != 0
    assert 0.2 < ff.mean() < 0.8   # half the triangles carry N on the far side
    n, ns = o[:, 9:12].astype(np.float64), o[:, 12:15].astype(np.float64)
    has_n = np.array([g.tris[p]["N"] is not None for b in batches if b["op"] == 0 for p in b["prim"]])
    cosine = (n * ns).sum(axis=1)[has_n]
    assert (cosine < np.cos(np.radians(15.0))).mean() > 0.9   # N is tilted: ns != n


# ---------------------------------------------------------------- exact conditions --------------------------------------------------------------------------------------
def f32_dot(a, b):
    """dot in float32, in the order of the vector type (x * x + y * y + z * z)"""
    a = np.asarray(a, F); b = np.asarray(b, F)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def no_underflow(P, b):
    prod = np.abs(np.asarray(b, np.float64)[:, None] * np.asarray(P, np.float64))
    return bool(np.all((prod == 0) | (prod > 1e-30)))


def share_ok(name, what, passed, total):
    print(f"\nsurface[{name}] {what}: predicate holds for {passed} of {total} probes")
    assert total == 0 or passed >= 0.9 * total, (name, what, passed, total)


@pytest.mark.parametrize("name", NAMES)
def test_hit_point_lies_within_its_error_box_and_normals_agree_in_sign(host, name):
    """op 0 on triangles.  Exact: |p - sum b_i p_i| <= p_error per component, the exact point carried through the instance's matrix; dot(n, ns) >= 0; n lies on the side the
    restatement gives it (reverse_orientation ^ swaps_handedness, then face_forward towards the shading normal).
    Predicates: finite inputs and no product b_i * p_i that underflows (the error bound's model is relative rounding); for the side of n, a margin of 1e-3 on every cosine
    the decision rests on."""
    orc, g, _, tpl, batches, outs = surface_set(name, host)
    total = ok_box = ok_side = 0
    for b, o in zip(batches, outs):
        if b["op"] != 0:
            continue
        for i in tri_probes(g, b):
            total += 1
            tri = g.tris[int(b["prim"][i])]; m = matrix_of(g, int(b["inst"][i]))
            if not (np.isfinite(b["rays"]["d"][i]).all() and np.isfinite(o[i, :18]).all()):
                continue
            n, ns = o[i, 9:12].astype(np.float64), o[i, 12:15].astype(np.float64)
            assert np.dot(n, ns) >= 0.0, sc.describe(name, b, i)
            if no_underflow(tri["P"], b["b"][i]):
                ok_box += 1
                exact = sr.exact_point(tri["P"], b["b"][i], m)
                err = np.abs(o[i, 0:3].astype(np.float64) - exact)
                assert (err <= o[i, 3:6].astype(np.float64)).all(), f"{sc.describe(name, b, i)}\n  |p - exact| {err} p_error {o[i, 3:6]}"
            fr = sr.shading_frame(tri, b["b"][i], m)
            if fr["margin"] > 1e-3 and np.isfinite(fr["n"]).all():
                ok_side += 1
                assert np.dot(n, fr["n"]) > 0.0, f"{sc.describe(name, b, i)}\n  n {n} restated {fr['n']}"
                assert np.dot(ns, fr["ns"]) > 0.0, f"{sc.describe(name, b, i)}\n  ns {ns} restated {fr['ns']}"
    if 0 in sc.SET_BY_NAME[name].ops:
        assert total >= 500
        share_ok(name, "error box", ok_box, total); share_ok(name, "side of n", ok_side, total)


@pytest.mark.parametrize("name", [s.name for s in sc.SETS if 3 in s.ops])
def test_spawned_rays_start_on_the_right_side_of_the_exact_plane(host, name):
    """op 3 on triangles.  Exact: spawn_ray's origin lies strictly on wi's side of the triangle's exact plane (the side offset_origin chose from dot(wi, n) in float32; +n for a
    zero dot), spawn_ray_to_hit's origin on its target's side.  Where the offset is zero (dot(|n|, p_error) == 0: a triangle in a coordinate plane through the origin)
    both origins are p itself, bit for bit.  Predicate: finite values below 1e30."""
    orc, g, _, tpl, batches, outs = surface_set(name, host)
    total = passed = 0
    for b, o in zip(batches, outs):
        if b["op"] != 3 or "hits" in b:
            continue
        si = sc.oracle_op0(orc, host, tpl, b)
        p, pe, n = si[:, 0:3], si[:, 3:6], si[:, 9:12]
        off = f32_dot(np.abs(n), pe)
        for i in range(len(o)):
            total += 1
            a = b["aux"][i]
            vals = np.concatenate([o[i, 0:3], o[i, 8:11], a[4:10], p[i]])
            if not (np.isfinite(vals).all() and np.abs(vals).max() < 1e30):
                continue
            passed += 1
            if not off[i] > 0:   # the `offset == 0` arms: every coordinate stays untouched
                assert np.array_equal(o[i, 0:3].view(np.uint32), p[i].view(np.uint32)) and np.array_equal(o[i, 8:11].view(np.uint32), p[i].view(np.uint32)), sc.describe(name, b, i)
                continue
            ng, Pw = sr.plane_normal(g.tris[int(b["prim"][i])]["P"], matrix_of(g, int(b["inst"][i])))
            side_n = 1.0 if np.dot(n[i].astype(np.float64), ng) > 0 else -1.0
            for origin, w, what in ((o[i, 0:3], a[4:7], "spawn_ray"), (o[i, 8:11], a[7:10] - p[i], "spawn_ray_to_hit")):
                want = -1.0 if f32_dot(w, n[i]) < 0 else 1.0
                dist = np.dot(origin.astype(np.float64) - Pw[0], ng) * side_n * want
                assert dist > 0.0, f"{what}: {sc.describe(name, b, i)}\n  origin {origin} signed distance {dist}"
    assert total >= 500
    share_ok(name, "spawn side", passed, total)


# ---------------------------------------------------------------- approximate conditions -------------------------------------------------------------------------------------
def measure(name, host):
    """{condition: largest residual relative to the operands' norms} of one set, and per condition how many probes its predicate admitted"""
    orc, g, _, tpl, batches, outs = surface_set(name, host)
    worst = {k: 0.0 for k in sr.RESIDUALS}
    count = {k: 0 for k in sr.RESIDUALS}

    def note(k, v):
        count[k] += 1
        if v > worst[k]:
            worst[k] = v

    for b, o in zip(batches, outs):
        if "hits" in b:
            continue
        if b["op"] == 0:
            for i in range(len(o)):
                if not np.isfinite(o[i, :18]).all():
                    continue
                tri = g.tris[int(b["prim"][i])]; m = matrix_of(g, int(b["inst"][i]))
                n, ns, ss = (o[i, k:k + 3].astype(np.float64) for k in (9, 12, 15))
                note("unit_ns", abs(sr.norm(ns) - 1.0))
                if m is None and (tri["N"] is not None or tri["S"] is not None):
                    note("unit_ss", abs(sr.norm(ss) - 1.0))
                if sr.norm(ss) > 0:
                    note("ss_dot_ns", abs(np.dot(ss, ns)) / (sr.norm(ss) * sr.norm(ns)))
                fr = sr.shading_frame(tri, b["b"][i], m)
                if fr["margin"] > 1e-3 and np.isfinite(fr["n"]).all():
                    note("n_matches_plane", sr.rel(n - fr["n"], n))
        elif b["op"] == 1:
            si = sc.oracle_op0(orc, host, tpl, b) if b["camera_ray"] else None
            for i in range(len(o)):
                if not np.isfinite(o[i, :36]).all():
                    continue
                tri = g.tris[int(b["prim"][i])]; m = matrix_of(g, int(b["inst"][i]))
                dpdu, dpdv, dpdx, dpdy, dndu, dndv = (o[i, k:k + 3].astype(np.float64) for k in (2, 5, 12, 15, 30, 33))
                bits = int(o[i, sc.MASK].view(np.uint32))
                if abs(sr.uv_determinant(tri)) >= 1e-2 and not bits & sc.BITS["DPDU_CROSS_ZERO"]:   # (a uv scale of 1e12 keeps the determinant but underflows dpdu x dpdv: the fallback frame)
                    uv = sr.uvs_of(tri)
                    _, Pw = sr.plane_normal(tri["P"], m)
                    for k in (0, 1):
                        du, dv = uv[k] - uv[2]
                        note("dpdu_dpdv_span", sr.rel(Pw[k] - Pw[2] - (dpdu * du + dpdv * dv), Pw[k] - Pw[2], dpdu * du, dpdv * dv))
                        if tri["N"] is not None:
                            N = sr.f64(tri["N"]) if m is None else sr.apply_normal(m, sr.f64(tri["N"]))
                            note("dndu_dndv_span", sr.rel(N[k] - N[2] - (dndu * du + dndv * dv), N[k] - N[2], dndu * du, dndv * dv))
                if si is not None and (np.abs(dpdx).max() > 0 or np.abs(dpdy).max() > 0):
                    n = si[i, 9:12].astype(np.float64); p = si[i, 0:3].astype(np.float64)
                    for dp in (dpdx, dpdy):
                        note("n_dot_dpdx", abs(np.dot(n, dp)) / max(sr.norm(p), sr.norm(dp), float(np.abs(o[i, 18:24]).max())))   # operands: p, the offset rays' origins, px - p
                    if bits & sc.BITS["DIFF_SOLVED"]:
                        an = np.abs(si[i, 9:12])
                        dims = (1, 2) if an[0] > an[1] and an[0] > an[2] else ((0, 2) if an[1] > an[2] else (0, 1))
                        for dp, du, dv in ((dpdx, o[i, 8], o[i, 9]), (dpdy, o[i, 10], o[i, 11])):
                            lhs = np.array([dp[d] for d in dims]); a_u = np.array([dpdu[d] for d in dims]) * float(du); a_v = np.array([dpdv[d] for d in dims]) * float(dv)
                            note("dpdx_solved", sr.rel(lhs - (a_u + a_v), lhs, a_u, a_v))
    return worst, count


def test_approximate_conditions_hold_within_8x_the_measured_residuals(host):
    """Orthonormality of the shading frame; p_i - p_2 = dpdu (u_i - u_2) + dpdv (v_i - v_2) and the same for N with dn/du, dn/dv on triangles with |uv determinant| >= 1e-2;
    n . dpdx = n . dpdy = 0; dpdx = dudx dpdu + dvdx dpdv in the two coordinates compute_differentials solves; n against the restated plane normal.  Each residual is taken
    relative to the norms of its operands; the largest over all sets is printed and must stay within FACTOR x the value recorded in surface_restatement.RESIDUALS."""
    worst = {k: (0.0, "") for k in sr.RESIDUALS}
    counts = {k: 0 for k in sr.RESIDUALS}
    for name in NAMES:
        w, c = measure(name, host)
        for k in w:
            counts[k] += c[k]
            if w[k] > worst[k][0]:
                worst[k] = (w[k], name)
    for k, (v, where) in worst.items():
        print(f"\nsurface residual {k}: {v:.3e} (set {where}, {counts[k]} probes); recorded {sr.RESIDUALS[k][0]:.3e} ({sr.RESIDUALS[k][1]})")
    for k, (v, where) in worst.items():
        assert counts[k] >= 500, (k, counts[k])
        assert v <= sr.FACTOR * sr.RESIDUALS[k][0], f"{k}: {v:.3e} in set {where} exceeds {sr.FACTOR} x {sr.RESIDUALS[k][0]:.3e}"
