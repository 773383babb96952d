"""The light probe case sets (light_probe_cases.py) measured on the oracle alone: the cases reach the branches they were built for — counted from the oracle's own
outputs, so that the GPU comparison (test_light_probe_gpu.py) is known to cover them — and the oracle's light code agrees with a plain float64 restatement of the
reference's formulas on well-conditioned probes.  The counts and the two measured float64 tolerances are quoted in DESIGN 0c."""
import math

import numpy as np
import pytest

import pbrt_hip
import light_probe_cases as lc
from light_probe_cases import F, PDF, VAL, VALID, VN, VP, WI
from oracle_binding import OracleScene

_cache = {}
FLT_MAX = float(np.finfo(F).max)


def light_set(name, host):
    """(oracle scene, batches, oracle outputs) of one light set, computed once and left unchanged."""
    if name not in _cache:
        ls = lc.LIGHT_SET_BY_NAME[name]
        orc = OracleScene()
        ls.capture(orc, host)
        batches = ls.cases(orc, host)
        _cache[name] = (orc, batches, lc.run_batches(orc, batches, ls.variant))
    return _cache[name]


def sample_batches(batches, outs, light=None):
    return [(b, o) for b, o in zip(batches, outs) if b["op"] == 0 and (light is None or b["light"] == light)]


def show(name, c):
    print(f"\nreach[{name}]: " + ", ".join(f"{k} {v}" for k, v in c.items()))


@pytest.mark.parametrize("name", [s.name for s in lc.LIGHT_SETS])
def test_nan_share_and_size(host, name):
    _, batches, outs = light_set(name, host)
    total = sum(len(o) for o in outs)
    nan = sum(int(np.isnan(o).any(axis=1).sum()) for o in outs)
    show(name, dict(batches=len(batches), probes=total, nan=nan))
    assert 1000 <= total <= lc.MAX_PROBES
    assert nan <= 0.01 * total
    for op in ((0,) if lc.LIGHT_SET_BY_NAME[name].variant == 2 else (0, 1, 2)):
        assert sum(len(o) for b, o in zip(batches, outs) if b["op"] == op) >= 10, op


def test_the_thinning_keeps_a_set_that_is_mostly_nan_under_the_cap(host):
    orc, _, _ = light_set("point_distant", host)
    at = lc.mk_ref(np.tile(np.array(lc.POINT_POS, F), (50, 1)))   # normalize of a zero vector: every probe a NaN
    fine = lc.random_refs(np.random.default_rng(1), lc.POINT_POS, 2.0, 1000)
    thinned = lc.thin_nans(orc, [lc.batch(0, 0, at, tag="at the light"), lc.batch(0, 0, fine, tag="fine")], 0)
    outs = lc.run_batches(orc, thinned)
    nan = sum(int(np.isnan(o).any(axis=1).sum()) for o in outs); total = sum(len(o) for o in outs)
    assert 1 <= nan <= 0.01 * total and len(thinned[1]["ref"]) == 1000


# ---------------------------------------------------------------- what each set reaches ----------------------------------------------------------------------------------
INFINITE_MIN = {
    "infinite_constant": dict(valid=2000, valid_pdf_zero=120, pdf_li_zero=60, pdf_li_negative=48, clamped_dw=90, clamped_dh=48, on_cdf_entry=700, le_nan=30),
    "infinite_map": dict(valid=12000, valid_pdf_zero=900, invalid=700, flat_cdf_rows=4, pdf_li_zero=400, pdf_li_negative=85, clamped_dw=130, clamped_dh=95, on_cdf_entry=8500, le_nan=25),
}


def test_infinite_sets_reach_their_branches(host):
    for name in ("infinite_constant", "infinite_map"):
        orc, batches, outs = light_set(name, host)
        c = dict(valid=0, valid_pdf_zero=0, invalid=0, pdf_li_zero=0, pdf_li_negative=0, clamped_dw=0, clamped_dh=0, on_cdf_entry=0, flat_cdf_rows=0, le_nan=0)
        for b, o in zip(batches, outs):
            if b["op"] == 0:
                c["valid"] += int((o[:, VALID] == 1).sum()); c["invalid"] += int((o[:, VALID] == 0).sum())
                c["valid_pdf_zero"] += int(((o[:, VALID] == 1) & (o[:, PDF] == 0)).sum())
            elif b["op"] == 1:
                c["pdf_li_zero"] += int((o[:, 0] == 0).sum()); c["pdf_li_negative"] += int((o[:, 0] < 0).sum())
            else:
                c["le_nan"] += int(np.isnan(o[:, 0]).sum())
        lights = sorted({b["light"] for b in batches})
        ts = lc._const_transforms(host) if name == "infinite_constant" else [host.rotate(lc.ROT["theta"], lc.ROT["axis"]) if k % 2 else (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY) for k in lights]
        for li in lights:
            dw, dh, marg, cond = lc.light_distribution(orc, li)
            c["flat_cdf_rows"] += int((np.diff(marg) == 0).sum())
            for b, o in zip(batches, outs):
                if b["light"] != li:
                    continue
                if b["op"] == 0:
                    c["on_cdf_entry"] += int(np.isin(b["u"][:, 1], marg).sum()) + int(np.isin(b["u"][:, 0], cond.reshape(-1)).sum())
                if b["op"] == 1:   # Distribution2D::pdf's two clamps, restated in float32 on the light-space direction
                    w = host.transform_vectors(ts[li][1], b["wi"]).astype(np.float64)
                    with np.errstate(invalid="ignore"):
                        phi = np.arctan2(w[:, 1], w[:, 0]); phi = np.where(phi < 0, phi + 2 * math.pi, phi).astype(F)
                        theta = np.arccos(np.clip(w[:, 2], -1, 1)).astype(F)
                        live = o[:, 0] != 0
                        c["clamped_dw"] += int((live & (phi * F(1 / (2 * math.pi)) * F(dw) >= dw)).sum())
                        c["clamped_dh"] += int((live & (theta * F(1 / math.pi) * F(dh) >= dh)).sum())
        show(name, c)
        need = INFINITE_MIN[name]   # about four fifths of what the sets deliver: a set that loses cases is noticed
        for k, v in need.items():
            assert c[k] >= v, (name, k, c[k], v)
        if name == "infinite_constant":
            assert c["invalid"] == 0


def test_spot_set_reaches_both_cut_offs(host):
    orc, batches, outs = light_set("spot", host)
    c = {}
    for li in range(5):
        k = dict(zero=0, one=0, between=0, nan=0)
        for b, o in sample_batches(batches, outs, li):
            pt = orc.light_probe_batch(5, 0, b["ref"])[:, VAL]   # the point light at the same position: I / d^2, what a spot gives where fall == 1
            v = o[:, VAL]
            lit = np.isfinite(pt[:, 0]) & (pt[:, 0] > 0)
            k["zero"] += int((lit & (v[:, 0] == 0)).sum()); k["one"] += int((lit & (v.view(np.uint32) == pt.view(np.uint32)).all(axis=1)).sum())
            k["between"] += int((lit & (v[:, 0] > 0) & (v[:, 0] < pt[:, 0])).sum()); k["nan"] += int(np.isnan(v[:, 0]).sum())
        for key, val in k.items():
            c[f"light{li}_{key}"] = val
    eq = {b["tag"]: len(b["ref"]) for b in batches if b["light"] == 0 and "==" in b["tag"]}
    c["equal_total"], c["equal_start"] = eq["cos_theta == SPOT_TOTAL"], eq["cos_theta == SPOT_START"]
    for li, tag, want_lit in ((1, "cos_theta == SPOT_TOTAL", True), (2, "cos_theta == SPOT_TOTAL", False), (3, "cos_theta == SPOT_START", True), (4, "cos_theta == SPOT_START", False)):
        for b, o in sample_batches(batches, outs, li):
            if b["tag"] == tag:   # by construction: lit by the cone whose cut-off equals the cosine, dark one float32 above
                assert ((o[:, VAL][:, 0] > 0) == want_lit).all()
    # distance_squared a nonzero float32 denormal (the lights 0 .. 5 sit at the origin: d^2 = p . p as the vector type forms it), with a value that is finite and not 0
    c["denormal_d2_finite"] = c["denormal_d2_overflow"] = 0
    for li in range(6):
        for b, o in sample_batches(batches, outs, li):
            p = b["ref"][:, 0:3]
            with np.errstate(all="ignore"):
                d2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]).astype(F)
            den = (d2 > 0) & (d2 < np.finfo(F).tiny)
            v = o[:, VAL][:, 0]
            c["denormal_d2_finite"] += int((den & np.isfinite(v) & (v != 0)).sum()); c["denormal_d2_overflow"] += int((den & np.isinf(v)).sum())
    for li in (6, 7):
        o = np.concatenate([o for _, o in sample_batches(batches, outs, li)])
        c[f"light{li}_zero"], c[f"light{li}_lit"] = int((o[:, VAL][:, 0] == 0).sum()), int((o[:, VAL][:, 0] > 0).sum())
    show("spot", c)
    assert c["equal_total"] >= 55 and c["equal_start"] >= 75
    assert c["light0_zero"] >= 950 and c["light0_one"] >= 850 and c["light0_between"] >= 800
    for li in (1, 2, 3, 4):
        assert c[f"light{li}_zero"] >= 850 and c[f"light{li}_one"] >= 750 and c[f"light{li}_between"] == 0
    assert c["light6_zero"] >= 220 and c["light6_lit"] >= 480 and c["light7_zero"] >= 240 and c["light7_lit"] >= 240
    assert c["denormal_d2_finite"] >= 15 and c["denormal_d2_overflow"] >= 8


def test_projection_set_reaches_the_window_and_the_near_plane(host):
    orc, batches, outs = light_set("projection", host)
    c = dict(inside=0, left=0, right=0, bottom=0, top=0, near_plane_dark=0, near_plane_lit=0, behind=0, on_axis=0)
    for b, o in sample_batches(batches, outs):
        fov, shape, rotated = lc.PROJECTIONS[b["light"]]
        t = lc._proj_transform(host, rotated)
        aspect = 1.0 if shape is None else shape[1] / shape[0]
        sx, sy = (aspect, 1.0) if aspect > 1 else (1.0, 1.0 / aspect)
        q = host.transform_points(t[1], b["ref"][:, 0:3]).astype(np.float64)
        with np.errstate(all="ignore"):
            wlz = q[:, 2] / np.linalg.norm(q, axis=1)
            cot = 1.0 / math.tan(math.radians(fov) / 2.0)
            px, py = cot * q[:, 0] / q[:, 2], cot * q[:, 1] / q[:, 2]
        dark = o[:, VAL][:, 0] == 0
        front = wlz > 2e-3
        c["inside"] += int((~dark & np.isfinite(o[:, VAL][:, 0])).sum())
        inx, iny = np.abs(px) < sx * 0.99, np.abs(py) < sy * 0.99
        c["left"] += int((dark & front & iny & (px < -sx) & (px > -sx * 1.001)).sum()); c["right"] += int((dark & front & iny & (px > sx) & (px < sx * 1.001)).sum())
        c["bottom"] += int((dark & front & inx & (py < -sy) & (py > -sy * 1.001)).sum()); c["top"] += int((dark & front & inx & (py > sy) & (py < sy * 1.001)).sum())
        near = (np.abs(wlz - 1e-3) < 2e-9) & inx & iny   # the wide frustums: the window test would pass, only `wl.z < 1e-3` decides
        c["near_plane_dark"] += int((near & dark).sum()); c["near_plane_lit"] += int((near & ~dark).sum())
        c["behind"] += int((dark & (wlz < 0)).sum())
        c["on_axis"] += int(((q[:, 0] == 0) & (q[:, 1] == 0) & (q[:, 2] > 0) & ~dark).sum())
    show("projection", c)
    for k, v in dict(inside=1500, left=25, right=25, bottom=24, top=24, near_plane_dark=28, near_plane_lit=30, behind=200, on_axis=12).items():
        assert c[k] >= v, (k, c[k], v)


def test_triangle_set_reaches_its_exits(host):
    orc, batches, outs = light_set("triangle", host)
    c = dict(valid=0, zero_length_exit=0, isinf_exit=0, other_invalid=0, value_zero_from_behind=0, flipped_normal=0, kept_normal=0, pdf_li_hit=0, pdf_li_miss=0)
    for b, o in zip(batches, outs):
        k = b["light"]
        P = lc.tri_points(k).astype(np.float64)
        ng = np.cross(P[1] - P[0], P[2] - P[0])
        if b["op"] == 0:
            ok = o[:, VALID] == 1
            c["valid"] += int(ok.sum())
            if "on the sampled point" in b["tag"]:
                c["zero_length_exit"] += int((~ok).sum())
            elif lc.TRIANGLES[k][0] != "zero_area":   # the isinf exit proper: the float64 restatement of the pdf is infinite or beyond float32 (|n . wi| == 0, d^2 overflowing)
                u = b["u"].astype(np.float64); su = np.sqrt(u[:, 0]); b0, b1 = 1 - su, u[:, 1] * su
                q = b0[:, None] * P[0] + b1[:, None] * P[1] + (1 - b0 - b1)[:, None] * P[2]
                w = q - b["ref"][:, 0:3].astype(np.float64); d2 = (w ** 2).sum(axis=1)
                with np.errstate(all="ignore"):
                    pdf64 = d2 / (np.abs((w / np.sqrt(d2)[:, None]) @ (ng / np.linalg.norm(ng))) * 0.5 * np.linalg.norm(ng))
                c["isinf_exit"] += int((~ok & (pdf64 > FLT_MAX)).sum()); c["other_invalid"] += int((~ok & ~(pdf64 > FLT_MAX)).sum())
            c["value_zero_from_behind"] += int((ok & (o[:, VAL] == 0).all(axis=1)).sum())
            d = o[:, VN].astype(np.float64) @ ng
            c["flipped_normal"] += int((ok & (d < 0)).sum()); c["kept_normal"] += int((ok & (d > 0)).sum())
        elif b["op"] == 1:
            c["pdf_li_hit"] += int((o[:, 0] > 0).sum()); c["pdf_li_miss"] += int((o[:, 0] == 0).sum())
    show("triangle", c)
    for k, v in dict(valid=12500, zero_length_exit=250, isinf_exit=850, value_zero_from_behind=5000, flipped_normal=4100, kept_normal=8300, pdf_li_hit=580, pdf_li_miss=5100).items():
        assert c[k] >= v, (k, c[k], v)
    # the face_forward tie: normals perpendicular to the geometric normal keep it
    k = [t[0] for t in lc.TRIANGLES].index("normals_perpendicular")
    o = np.concatenate([o for _, o in sample_batches(batches, outs, k)]); ok = o[:, VALID] == 1
    assert ok.sum() > 50 and (o[ok][:, VN] == np.array([0, 0, 1], F)).all()
    # the four combinations of reverse_orientation and a handedness swap: the normal flips where exactly one holds
    for name, flipped in (("one_sided", False), ("reversed", True), ("swapped", True), ("reversed_swapped", False)):
        k = [t[0] for t in lc.TRIANGLES].index(name)
        o = np.concatenate([o for _, o in sample_batches(batches, outs, k)]); ok = o[:, VALID] == 1
        assert ok.sum() > 50 and (o[ok][:, VN][:, 2] == (-1 if flipped else 1)).all(), name


def test_sphere_set_reaches_both_samplers_and_both_cones(host):
    orc, batches, outs = light_set("sphere", host)
    c = dict(inside=0, outside=0, taylor_cone=0, exact_cone=0, invalid=0, value_zero=0, moved_inside_by_offset=0, moved_outside_by_offset=0, steps_below_switch=0, steps_above_switch=0)
    for b, o in zip(batches, outs):
        name, centre, r, _, _, _, _, _, scale = lc.SPHERES[b["light"]]
        if scale is not None:
            c["invalid"] += int((o[:, VALID] == 0).sum())
            continue
        ok = o[:, VALID] == 1
        p = b["ref"][:, 0:3].astype(np.float64); d = np.linalg.norm(p - np.array(centre), axis=1)
        # the cone's pdf does not depend on u, the area sampler's does: a sample is from the cone where its pdf equals uniform_cone_pdf of its distance
        with np.errstate(all="ignore"):
            s2 = (r / d) ** 2
            cone_pdf = 1.0 / (2 * math.pi * (1.0 - np.sqrt(np.maximum(0.0, 1.0 - s2))))
            is_cone = ok & (d > r) & (np.abs(o[:, PDF] / cone_pdf - 1.0) < 1e-2)
        c["outside"] += int(is_cone.sum()); c["inside"] += int((ok & ~is_cone).sum())
        c["taylor_cone"] += int((is_cone & (s2 < float(lc.TAYLOR) * 0.999)).sum()); c["exact_cone"] += int((is_cone & (s2 > float(lc.TAYLOR) * 1.001)).sum())
        c["moved_inside_by_offset"] += int((ok & ~is_cone & (d > r * 1.0005)).sum()); 
        with np.errstate(all="ignore"):   # inside, yet sampled by the cone (sin_theta_max = r / d > 1: cos_theta_max = 0, pdf = 1 / 2 pi): the offset origin overshot the far side
            c["moved_outside_by_offset"] += int((ok & (d < r) & (np.abs(b["ref"][:, 3:6]).max(axis=1) > 2 * r) & (np.abs(o[:, PDF] * 2 * math.pi - 1.0) < 1e-5)).sum())
            # sin_theta_max2 as the sampler forms it in float32, within 3e-6 (a dozen float32 steps) of the Taylor switch on either side
            q32 = b["ref"][:, 0:3] - np.array(centre, F)
            dc = np.sqrt(q32[:, 0] * q32[:, 0] + q32[:, 1] * q32[:, 1] + q32[:, 2] * q32[:, 2], dtype=F)
            st = F(r) * (F(1) / dc); s2f = (st * st).astype(np.float64); T = float(lc.TAYLOR)
            c["steps_below_switch"] += int((is_cone & (s2f < T) & (s2f > T * (1 - 3e-6))).sum()); c["steps_above_switch"] += int((is_cone & (s2f >= T) & (s2f < T * (1 + 3e-6))).sum())
        c["invalid"] += int((~ok).sum()); c["value_zero"] += int((ok & (o[:, VAL] == 0).all(axis=1)).sum())
    show("sphere", c)
    for k, v in dict(inside=4800, outside=7600, taylor_cone=128, exact_cone=5700, value_zero=4200, moved_inside_by_offset=730, moved_outside_by_offset=128, steps_below_switch=760,
                     steps_above_switch=1000).items():
        assert c[k] >= v, (k, c[k], v)


def test_delta_sets_reach_their_edges(host):
    for name in ("goniometric", "point_distant"):
        orc, batches, outs = light_set(name, host)
        o = np.concatenate([o for _, o in sample_batches(batches, outs)])
        c = dict(lit=int((o[:, VAL][:, 0] > 0).sum()), overflow_dark=int(((o[:, VAL] == 0).all(axis=1) & (o[:, VALID] == 1)).sum()), nan=int(np.isnan(o).any(axis=1).sum()),
                 pdf_li_zero=sum(int((o[:, 0] == 0).sum()) for b, o in zip(batches, outs) if b["op"] == 1))
        show(name, c)
        need = dict(lit=1450, overflow_dark=4, nan=10, pdf_li_zero=38) if name == "goniometric" else dict(lit=1450, overflow_dark=6, nan=5, pdf_li_zero=28)
        for k, v in need.items():
            assert c[k] >= v, (name, k, c[k], v)


# ---------------------------------------------------------------- the oracle against float64 ------------------------------------------------------------------------------
# Largest relative errors measured on the oracle (float32, libm mode 0) against the float64 restatements below, asserted with a margin of 4: float32 round-off along two
# routes differs by small factors from case to case.
FORMULA_REL = {"point": 2.14e-7, "point_wi": 1.47e-7, "spot": 8.21e-5, "triangle_pdf": 1.86e-5, "cone_pdf": 5.36e-6}   # I / d^2 and wi of the point light, spot falloff, triangle and cone pdfs
CONSISTENCY_REL = {"triangle": 2.11e-4, "infinite_constant": 5.71e-5, "infinite_map": 5.05e-4}                          # sample_li.pdf against pdf_li(sample_li.wi)


def rel(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want))) if len(want) else 0.0


def test_oracle_formulas_against_float64(host):
    worst = {}
    # I / d^2 of the point light
    orc, batches, outs = light_set("point_distant", host)
    b, o = sample_batches(batches, outs, 0)[0]
    p = b["ref"][:, 0:3].astype(np.float64); pl = np.array(lc.POINT_POS, F).astype(np.float64)
    d2 = ((pl - p) ** 2).sum(axis=1)
    sel = (d2 > 1e-3) & (d2 < 1e6)
    assert sel.sum() >= 500
    worst["point"] = max(rel(o[sel][:, VAL][:, c], np.float64(F((5.0, 4.0, 3.0)[c])) / d2[sel]) for c in range(3))
    worst["point_wi"] = rel(o[sel][:, WI] + 2.0, (pl - p[sel]) / np.sqrt(d2[sel])[:, None] + 2.0)
    # spot falloff: light 0, at the origin along +z with the identity transform
    orc, batches, outs = light_set("spot", host)
    got, want = [], []
    ct, cs = float(lc.SPOT_TOTAL), float(lc.SPOT_START)
    for b, o in sample_batches(batches, outs, 0):
        p = b["ref"][:, 0:3].astype(np.float64); d2 = (p ** 2).sum(axis=1)
        with np.errstate(all="ignore"):
            cos = p[:, 2] / np.sqrt(d2)
            delta = (cos - ct) / (cs - ct)
            fall = np.where(cos >= cs, 1.0, np.clip(delta, 0, 1) ** 4)
            sel = (d2 > 1e-3) & (d2 < 1e6) & (np.abs(cos - cs) > 1e-4) & (delta > 0.1)
        got.append(o[sel][:, VAL][:, 0]); want.append(float(F(lc.SPOT_I[0])) * fall[sel] / d2[sel])
    got, want = np.concatenate(got), np.concatenate(want)
    assert len(want) >= 300
    worst["spot"] = rel(got, want)
    # Triangle::sample's solid-angle pdf
    orc, batches, outs = light_set("triangle", host)
    got, want = [], []
    for b, o in sample_batches(batches, outs):
        k = b["light"]
        if lc.TRIANGLES[k][0] in ("zero_area",):
            continue
        P = lc.tri_points(k).astype(np.float64); size = np.linalg.norm(P[1] - P[0])
        u = b["u"].astype(np.float64); su = np.sqrt(u[:, 0]); b0, b1 = 1 - su, u[:, 1] * su
        q = b0[:, None] * P[0] + b1[:, None] * P[1] + (1 - b0 - b1)[:, None] * P[2]
        n = np.cross(P[1] - P[0], P[2] - P[0]); area = 0.5 * np.linalg.norm(n); n /= 2 * area
        w = q - b["ref"][:, 0:3].astype(np.float64); d2 = (w ** 2).sum(axis=1)
        with np.errstate(all="ignore"):
            ad = np.abs((w / np.sqrt(d2)[:, None]) @ n)
            sel = (o[:, VALID] == 1) & (ad > 0.1) & (np.sqrt(d2) < 100 * size) & (np.sqrt(d2) > 0.01 * size)
            got.append(o[sel][:, PDF]); want.append((d2 / (ad * area))[sel])
    got, want = np.concatenate(got), np.concatenate(want)
    assert len(want) >= 3000
    worst["triangle_pdf"] = rel(got, want)
    # uniform_cone_pdf of the spheres with a rigid transform
    orc, batches, outs = light_set("sphere", host)
    got, want = [], []
    for b, o in zip(batches, outs):
        name, centre, r, _, _, _, _, _, scale = lc.SPHERES[b["light"]]
        if scale is not None:
            continue
        p = b["ref"][:, 0:3].astype(np.float64); d = np.linalg.norm(p - np.array(centre), axis=1)
        with np.errstate(all="ignore"):
            s2 = (r / d) ** 2
            sel = (o[:, VALID] == 1) & (d > 1.3 * r) & (s2 > 0.01) & (np.abs(b["ref"][:, 3:6]).max(axis=1) < 1e-3)   # well outside, a cone wide enough that 1 - cos keeps its digits
            got.append(o[sel][:, PDF]); want.append((1.0 / (2 * math.pi * (1.0 - np.sqrt(1.0 - s2))))[sel])
    got, want = np.concatenate(got), np.concatenate(want)
    assert len(want) >= 1000
    worst["cone_pdf"] = rel(got, want)
    print("\nfloat64 formulas, largest relative error: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 4 * FORMULA_REL[k], (k, v)


def test_oracle_sample_pdf_is_consistent_with_pdf_li(host):
    worst = {}
    orc, batches, outs = light_set("triangle", host)
    got, want, interior = [], [], []
    for b, o in sample_batches(batches, outs):
        k = b["light"]
        if lc.TRIANGLES[k][0] == "zero_area":
            continue
        P = lc.tri_points(k).astype(np.float64); size = np.linalg.norm(P[1] - P[0])
        wi = o[:, WI].astype(np.float64); n = b["ref"][:, 6:9].astype(np.float64)
        dist = np.linalg.norm(o[:, VP].astype(np.float64) - b["ref"][:, 0:3].astype(np.float64), axis=1)
        # ... and an error bound that is small against the distance: pdf_li measures to where the ray from the offset origin meets the triangle, a different point under a large p_error
        sel = (o[:, VALID] == 1) & (np.abs((n * wi).sum(axis=1)) > 0.1) & (dist < 100 * size) & (np.abs(b["ref"][:, 3:6]).max(axis=1) < 1e-5 * dist)
        if sel.any():
            back = orc.light_probe_batch(k, 1, b["ref"][sel], wi=o[sel][:, WI])[:, 0]
            got.append(back); want.append(o[sel][:, PDF].astype(np.float64))
            su = np.sqrt(b["u"][sel][:, 0].astype(np.float64)); b0, b1 = 1 - su, b["u"][sel][:, 1] * su
            ngl = np.cross(P[1] - P[0], P[2] - P[0]); ngl /= np.linalg.norm(ngl)
            interior.append((np.minimum(np.minimum(b0, b1), 1 - b0 - b1) > 0.02) & (np.abs(wi[sel] @ ngl) > 1e-3))
    got, want, interior = np.concatenate(got), np.concatenate(want), np.concatenate(interior)
    hit = got > 0   # a sample on the triangle's rim can miss the triangle on the way back: Triangle::intersect decides, as for every ray, and so can a ray
    # within float32 of the triangle's plane (the reference point of the tilted triangle that lies in its plane); a sample well inside, met at more than 1e-3 of cosine, cannot
    print(f"\ntriangle consistency: {len(got)} probes, {int(interior.sum())} interior, {int((~hit).sum())} misses (on the rim or grazing)")
    assert interior.sum() >= 2000 and hit[interior].all() and (~hit).sum() <= 0.25 * len(hit)
    worst["triangle"] = rel(got[hit], want[hit])
    for name in ("infinite_constant", "infinite_map"):
        orc, batches, outs = light_set(name, host)
        lights = sorted({b["light"] for b in batches})
        ts = lc._const_transforms(host) if name == "infinite_constant" else [host.rotate(lc.ROT["theta"], lc.ROT["axis"]) if k % 2 else (pbrt_hip.IDENTITY, pbrt_hip.IDENTITY) for k in lights]
        got, want = [], []
        for b, o in sample_batches(batches, outs):
            li = b["light"]
            dw, dh, _, _ = lc.light_distribution(orc, li)
            w = host.transform_vectors(ts[li][1], o[:, WI]).astype(np.float64)
            with np.errstate(all="ignore"):
                w /= np.linalg.norm(w, axis=1)[:, None]
                phi = np.arctan2(w[:, 1], w[:, 0]); phi = np.where(phi < 0, phi + 2 * math.pi, phi)
                cu, cv = phi / (2 * math.pi) * dw, np.arccos(np.clip(w[:, 2], -1, 1)) / math.pi * dh
                away = (np.abs(cu - np.round(cu)) >= 1e-3) & (np.abs(cv - np.round(cv)) >= 1e-3)
                n = b["ref"][:, 6:9].astype(np.float64)
                sel = (o[:, VALID] == 1) & (o[:, PDF] > 0) & away & (np.abs((n * o[:, WI]).sum(axis=1)) > 0.1)
            if sel.any():
                got.append(orc.light_probe_batch(li, 1, b["ref"][sel], wi=o[sel][:, WI])[:, 0]); want.append(o[sel][:, PDF].astype(np.float64))
        got, want = np.concatenate(got), np.concatenate(want)
        assert len(want) >= 500, (name, len(want))
        worst[name] = rel(got, want)
    print("\nsample_li.pdf against pdf_li, largest relative error: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 4 * CONSISTENCY_REL[k], (k, v)
