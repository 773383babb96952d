"""The texture probe case sets (texture_probe_cases.py) measured on the oracle alone: the work caps and the NaN cap hold, the variants agree as the device is held to, the cases
reach the branches they were built for — counted from the inputs restated in float32 and from the oracle's own outputs, so that the GPU comparison (test_texture_probe_gpu.py)
is known to cover them — and the oracle's texture code agrees with a plain float64 restatement of the reference's formulas on well-conditioned probes.  The counts and the
measured float64 errors are quoted in DESIGN 0d.  No GPU is needed."""
import math

import numpy as np
import pytest

import pbrt_hip
import texture_probe_cases as tc
from texture_probe_cases import F
from oracle_binding import set_libm_mode

MARGIN = 4.0   # the project's margin over a measured error


def show(name, c):
    print(f"\nreach[{name}]: " + ", ".join(f"{k} {v}" for k, v in c.items()))


def key_of(ps):
    return "inp" if ps.kind == "bump" else "ctx"


def same_bits(a, b):
    """bit for bit, a NaN asking for a NaN in the same slot"""
    return bool(np.where(np.isnan(a), np.isnan(b), a.view(np.uint32) == b.view(np.uint32)).all())


# ---------------------------------------------------------------- c. caps and consistency -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in tc.SETS])
def test_caps_hold(host, name):
    ps, orc, batches, work, want = tc.prepared(name, host)
    total = sum(len(b[key_of(ps)]) for b in batches)
    nan = sum(int(np.isnan(o).any(axis=1).sum()) for o in want[0])
    texels = max(int(w[:, 0].max()) for w in work); noise = max(int(w[:, 1].max()) for w in work)
    show(name, dict(batches=len(batches), probes=total, nan=nan, most_texels=texels, most_noise_calls=noise))
    assert 500 <= total <= tc.MAX_PROBES
    assert nan <= tc.NAN_SHARE * total
    assert texels <= tc.WORK_TEXELS and noise <= tc.WORK_NOISE


def test_a_probe_above_a_work_cap_is_refused_before_any_device_sees_it(host, monkeypatch):
    monkeypatch.setattr(tc, "WORK_NOISE", 2)
    monkeypatch.setattr(tc, "_prepared", {})
    with pytest.raises(AssertionError, match="above the caps"):
        tc.prepared("procedural_3d", host)


@pytest.mark.parametrize("name", [s.name for s in tc.SETS])
def test_variants_agree_on_the_oracle(host, name):
    """variant 1 = variant 0 on zero derivatives, 2 and 3 = 0 and 1, 4 = the red channel of 1: trivially so on the oracle; this is the contract the device is held to"""
    ps, orc, batches, work, want = tc.prepared(name, host)
    k = key_of(ps)
    n_zero = 0
    for i, b in enumerate(batches):
        vs = tc.batch_variants(ps, b)
        if 1 in vs:
            c = b[k][:, :15]
            zero = (c[:, 2:6] == 0).all(axis=1) & (c[:, 9:15] == 0).all(axis=1)
            n_zero += int(zero.sum())
            assert same_bits(want[1][i][zero], want[0][i][zero]), b["tag"]
            z = b[k].copy(); z[:, 2:6] = 0; z[:, 9:15] = 0
            set_libm_mode(1)   # as the set was run
            try:
                again = orc.bump_probe_batch(b["tex"], z, 0) if ps.kind == "bump" else orc.texture_probe_batch(b["tex"], z, 0)
            finally:
                set_libm_mode(0)
            assert same_bits(want[1][i], again), b["tag"]
        if 2 in vs:
            assert same_bits(want[2][i], want[0][i]), b["tag"]
        if 3 in vs:
            assert same_bits(want[3][i], want[1][i]), b["tag"]
        if 4 in vs:
            assert same_bits(want[4][i][:, 0], want[1][i][:, 0]) and (want[4][i][:, 1:] == 0).all(), b["tag"]
    if 1 in ps.variants:
        assert n_zero >= 20, n_zero


def test_refusals(host):
    ps, orc, batches, work, want = tc.prepared("procedural_2d", host)
    b = batches[0]; c4 = np.ascontiguousarray(b["ctx"][:4]); i33 = np.zeros((4, 33), F)

    def refused(fn, code, word, *a):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            fn(*a)
        assert e.value.code == code and word in str(e.value), (e.value.code, str(e.value))

    for fn, arg in ((orc.texture_probe_batch, c4), (orc.bump_probe_batch, i33)):
        refused(fn, pbrt_hip.ERR_INVALID_ARG, "unknown texture", 64, arg, 0)
        refused(fn, pbrt_hip.ERR_INVALID_ARG, "unknown variant", b["tex"], arg, -1)
        refused(fn, pbrt_hip.ERR_UNSUPPORTED, "variants 2 and above", b["tex"], arg, 2)
        refused(fn, pbrt_hip.ERR_UNSUPPORTED, "variants 2 and above", b["tex"], arg, 3)
    refused(orc.texture_probe_batch, pbrt_hip.ERR_INVALID_ARG, "unknown variant", b["tex"], c4, 5)
    refused(orc.texture_probe_batch, pbrt_hip.ERR_UNSUPPORTED, "variants 2 and above", b["tex"], c4, 4)
    refused(orc.bump_probe_batch, pbrt_hip.ERR_INVALID_ARG, "unknown variant", b["tex"], i33, 4)
    fp = lambda a: a.ctypes.data_as(pbrt_hip.C.POINTER(pbrt_hip.C.c_float))
    out = np.zeros((4, 6), F)
    for name, arr in (("texture_probe_batch", c4), ("bump_probe_batch", i33)):
        fn = orc.b.fn(name)
        assert fn(orc.h, b["tex"], 0, 4, None, fp(out)) == pbrt_hip.ERR_INVALID_ARG
        assert fn(orc.h, b["tex"], 0, 2 ** 32, fp(arr), fp(out)) == pbrt_hip.ERR_INVALID_ARG
        assert fn(orc.h, b["tex"], 0, 0, None, None) == pbrt_hip.OK
    assert pbrt_hip.default_binding().has("texture_probe_batch") and pbrt_hip.default_binding().has("bump_probe_batch")


# ---------------------------------------------------------------- float32 restatements of the branch conditions ------------------------------------------------------------
def log2_f32(x):
    with np.errstate(all="ignore"):
        return np.log2(x.astype(np.float64)).astype(F)


def st_of(b):
    su, sv, du, dv = b.get("xf", (1.0, 1.0, 0.0, 0.0))
    c = b["ctx"]
    with np.errstate(all="ignore"):
        return (F(su) * c[:, 0] + F(du)).astype(F), (F(sv) * c[:, 1] + F(dv)).astype(F)


def trilinear_level(b):
    c = b["ctx"]; L = b["map"]["levels"]
    with np.errstate(all="ignore"):
        a = np.abs(c[:, 2:6])
        # pmax written with `>`: a NaN operand loses unless it comes first (common.rs:66-107); fmax ignores NaNs, which is the same for the slots the set fills
        width = np.fmax(np.fmax(a[:, 0], a[:, 1]), np.fmax(a[:, 2], a[:, 3]))
        return (F(L) - F(1) + log2_f32(np.fmax(width, F(1e-8)))).astype(F)


def ewa_state(b):
    """per probe of an EWA batch, in float32 as MIPMap::lookup forms them: (clamped, minor_length after the clamp, lod, il)"""
    c = b["ctx"]; m = b["map"]; L = m["levels"]
    with np.errstate(all="ignore"):
        d0 = c[:, [2, 3]].copy(); d1 = c[:, [4, 5]].copy()
        l0 = (d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]).astype(F); l1 = (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(F)
        swap = l0 < l1
        d0[swap], d1[swap] = c[:, [4, 5]][swap], c[:, [2, 3]][swap]
        major = np.sqrt(np.where(swap, l1, l0)).astype(F); minor = np.sqrt(np.where(swap, l0, l1)).astype(F)
        adjusted = (minor * F(m["aniso"])).astype(F)
        clamped = (adjusted < major) & (minor > 0)
        sc = (major / adjusted).astype(F)
        minor2 = np.where(clamped, (minor * sc).astype(F), minor)
        d1 = np.where(clamped[:, None], (d1 * sc[:, None]).astype(F), d1)
        lod = (F(L) - F(1) + log2_f32(minor2)).astype(F)
        lod = np.where(lod > 0, lod, F(0)).astype(F)   # pmax(0, lod): NaN -> 0
        il = np.floor(lod)
    return dict(swap=swap, clamped=clamped, minor=minor2, lod=lod, il=il, d0=d0, d1=d1, tie=(l0 == l1) & (l0 > 0))


def ewa_box(s32, t32, d0, d1, lw, lh):
    """(s0, s1, t0, t1) of MIPMap::ewa's footprint loops (mipmap/mod.rs:320-357) on a level of lw x lh texels, every operation in float32 and in the reference's order"""
    with np.errstate(all="ignore"):
        us, vs, one, two = F(lw), F(lh), F(1), F(2)
        s = s32 * us - F(0.5); t = t32 * vs - F(0.5)
        d0x, d0y, d1x, d1y = d0[:, 0] * us, d0[:, 1] * vs, d1[:, 0] * us, d1[:, 1] * vs
        a = d0y * d0y + d1y * d1y + one
        b = F(-2) * (d0x * d0y + d1x * d1y)
        c = d0x * d0x + d1x * d1x + one
        inv_f = one / (a * c - b * b * F(0.25))
        a, b, c = a * inv_f, b * inv_f, c * inv_f
        det = -b * b + F(4) * a * c
        inv_det = one / det
        u_sqrt, v_sqrt = np.sqrt(det * c), np.sqrt(a * det)
        assert all(x.dtype == F for x in (s, t, a, b, c, det, u_sqrt, v_sqrt))
        return np.ceil(s - two * inv_det * u_sqrt), np.floor(s + two * inv_det * u_sqrt), np.ceil(t - two * inv_det * v_sqrt), np.floor(t + two * inv_det * v_sqrt)


# ---------------------------------------------------------------- a. what each set reaches ----------------------------------------------------------------------------------
REACH_MIN = {}   # per set: four fifths of the counts measured on the oracle (DESIGN 0d quotes the measured ones)


def check_reach(name, c):
    show(name, c)
    need = REACH_MIN[name]   # about four fifths of what the sets deliver: a set that loses cases is noticed
    assert set(need) == set(c), sorted(set(need) ^ set(c))
    for k, v in need.items():
        assert c[k] >= v, (name, k, c[k], v)


REACH_MIN["texel_grid"] = dict(ds_zero=2748, dt_zero=2556, black_all_outside=832, index_2_30=833, on_u_exact=598, programs=1822)


def test_texel_grid_reach(host):
    ps, orc, batches, work, want = tc.prepared("texel_grid", host)
    c = dict(ds_zero=0, dt_zero=0, black_all_outside=0, index_2_30=0, on_u_exact=0, programs=0)
    for b, o in zip(batches, want[0]):
        if "map" not in b:
            c["programs"] += len(o)
            continue
        m = b["map"]
        s, t = st_of(b)
        with np.errstate(all="ignore"):
            ts = (s * F(m["lw"]) - F(0.5)).astype(F); tt = (t * F(m["lh"]) - F(0.5)).astype(F)
            fin = np.isfinite(ts) & np.isfinite(tt)
            c["ds_zero"] += int((fin & (ts == np.floor(ts))).sum()); c["dt_zero"] += int((fin & (tt == np.floor(tt))).sum())
            c["index_2_30"] += int(((np.abs(ts) >= 2.0 ** 30) | (np.abs(tt) >= 2.0 ** 30)).sum())
            if m["wrap"] == "black":
                out = (ts < -1) | (ts >= m["lw"]) | (tt < -1) | (tt >= m["lh"])
                assert (o[fin & out & (np.abs(ts) < 2.0 ** 60) & (np.abs(tt) < 2.0 ** 60)] == 0).all()
                c["black_all_outside"] += int((fin & out).sum())
            if b["xf"][0] != 1.0:   # the scaled and shifted imagemap still lands on the grid
                c["on_u_exact"] += int((fin & (ts == np.floor(ts)) & (tt == np.floor(tt))).sum())
    check_reach("texel_grid", c)


REACH_MIN["trilinear_levels"] = dict(level_negative=4761, top_level=5222, between=10982, delta_zero=3993)


def test_trilinear_reach(host):
    ps, orc, batches, work, want = tc.prepared("trilinear_levels", host)
    c = dict(level_negative=0, top_level=0, between=0, delta_zero=0)
    for b in batches:
        L = b["map"]["levels"]; lv = trilinear_level(b)
        with np.errstate(all="ignore"):
            neg = lv < 0; top = ~neg & (lv >= L - 1); mid = ~neg & ~top & ~np.isnan(lv)
            c["level_negative"] += int(neg.sum()); c["top_level"] += int(top.sum()); c["between"] += int(mid.sum())
            c["delta_zero"] += int((mid & (lv == np.floor(lv))).sum())
    check_reach("trilinear_levels", c)


REACH_MIN["ewa_ellipse"] = dict(clamped=6412, unclamped=10184, ratio_on_the_clamp=1429, tie=1732, to_triangle=4468, next_level_outside=5232, lod_on_integer=1112, crosses_wrap=10310, index_2_30=1436, il_0=9254, il_1=2093, il_2=972, il_3=470, il_4=355, il_5=92, il_6=92)


def test_ewa_reach(host):
    ps, orc, batches, work, want = tc.prepared("ewa_ellipse", host)
    c = {k: 0 for k in REACH_MIN["ewa_ellipse"]}
    n_checked = 0
    for b, w in zip(batches, work):
        m = b["map"]; L = m["levels"]; e = ewa_state(b)
        s, t = st_of(b)
        with np.errstate(all="ignore"):
            tri = e["minor"] == 0
            live = ~tri & ~np.isnan(e["minor"])
            c["clamped"] += int(e["clamped"].sum()); c["unclamped"] += int((live & ~e["clamped"]).sum()); c["tie"] += int(e["tie"].sum()); c["to_triangle"] += int(tri.sum())
            l0 = np.sqrt((e["d0"] ** 2).sum(axis=1).astype(F)).astype(F)
            c["ratio_on_the_clamp"] += int((live & ~e["clamped"] & ((e["minor"] * F(m["aniso"])).astype(F) == l0)).sum())
            c["next_level_outside"] += int((live & (e["il"] + 1 >= L)).sum())
            c["lod_on_integer"] += int((live & (e["lod"] > 0) & (e["lod"] == e["il"]) & (e["il"] < L)).sum())
            for k in range(7):
                c[f"il_{k}"] += int((live & (e["il"] == k) & (k < L)).sum())
            ts = (s * F(m["lw"]) - F(0.5)).astype(F); tt = (t * F(m["lh"]) - F(0.5)).astype(F)
            c["index_2_30"] += int((live & ((np.abs(ts) >= 2.0 ** 30) | (np.abs(tt) >= 2.0 ** 30))).sum())
            # the box of MIPMap::ewa at level il, restated in float32: it holds texels inside the level and texels beyond one of its edges.  The restatement is held to the oracle:
            # over both levels of a look-up its boxes hold exactly the texels the oracle counted
            texels = np.zeros(len(s))
            for lv in range(L):
                lw, lh = max(m["lw"] >> lv, 1), max(m["lh"] >> lv, 1)
                s0, s1, t0, t1 = ewa_box(s, t, e["d0"], e["d1"], lw, lh)
                box = np.where((s0 <= s1) & (t0 <= t1), (s1 - s0 + 1) * (t1 - t0 + 1), 0)
                texels += np.where((e["il"] == lv) | (e["il"] + 1 == lv), box, 0)
                at = live & (e["il"] == lv) & (s0 <= s1) & (t0 <= t1)
                c["crosses_wrap"] += int((at & (((s0 < 0) & (s1 >= 0)) | ((s0 <= lw - 1) & (s1 > lw - 1)) | ((t0 < 0) & (t1 >= 0)) | ((t0 <= lh - 1) & (t1 > lh - 1)))).sum())
            sel = live & (e["il"] + 1 < L) & np.isfinite(e["d0"]).all(axis=1) & np.isfinite(e["d1"]).all(axis=1) & (np.abs(s) < 1e6) & (np.abs(t) < 1e6)
            assert (texels[sel] == w[sel, 0]).all(), b["tag"]
            n_checked += int(sel.sum())
    assert n_checked >= 10000, n_checked
    check_reach("ewa_ellipse", c)


REACH_MIN["ewa_saturated"] = dict(at_2_62=1041, at_2_63_or_beyond=3575, both_coordinates=1419, ewa=1820, trilinear=2796)


def test_ewa_saturated_reach(host):
    """texel coordinates of level 0 from 2^62 on; from 2^63 on `as isize` saturates and both bounds of a footprint loop are isize::MAX"""
    ps, orc, batches, work, want = tc.prepared("ewa_saturated", host)
    c = {k: 0 for k in REACH_MIN["ewa_saturated"]}
    for b, w in zip(batches, work):
        m = b["map"]; s, t = st_of(b)
        with np.errstate(all="ignore"):
            ts = np.abs((s * F(m["lw"]) - F(0.5)).astype(F)); tt = np.abs((t * F(m["lh"]) - F(0.5)).astype(F))
            big = np.fmax(ts, tt)
            c["at_2_62"] += int(((big >= 2.0 ** 62) & (big < 2.0 ** 63)).sum()); c["at_2_63_or_beyond"] += int((big >= 2.0 ** 63).sum())
            c["both_coordinates"] += int(((ts >= 2.0 ** 62) & (tt >= 2.0 ** 62)).sum())
            c["trilinear" if m["trilinear"] else "ewa"] += int((big >= 2.0 ** 62).sum())
        assert int(w[:, 0].max()) <= 64   # a footprint at such a coordinate is one column or one texel: the float32 spacing there exceeds every ellipse
    check_reach("ewa_saturated", c)


REACH_MIN["procedural_2d"] = dict(checker_point=591, checker_filtered=852, checker_wide=1056, ds_zero_dt_positive=809, ds_exactly_one=105, cell_sum_wraps=216, dots_inside_rim=1526, dots_outside_rim=1696, uv_one_exactly=40, bilerp_corners=8)


def test_procedural_2d_reach(host):
    ps, orc, batches, work, want = tc.prepared("procedural_2d", host)
    c = {k: 0 for k in REACH_MIN["procedural_2d"]}
    CA = np.array(tc.CA, F)
    for b, o in zip(batches, want[0]):
        x = b["ctx"]
        with np.errstate(all="ignore"):
            if b["tag"] in ("checker", "checker_none"):
                s, t = x[:, 0], x[:, 1]
                ds = np.fmax(np.abs(x[:, 2]), np.abs(x[:, 4])); dt = np.fmax(np.abs(x[:, 3]), np.abs(x[:, 5]))
                point = (np.floor(s - ds) == np.floor(s + ds)) & (np.floor(t - dt) == np.floor(t + dt))
                wide = ~point & ((ds > 1) | (dt > 1))
                if b["tag"] == "checker":
                    c["checker_point"] += int(point.sum()); c["checker_wide"] += int(wide.sum()); c["checker_filtered"] += int((~point & ~wide).sum())
                    c["ds_zero_dt_positive"] += int(((ds == 0) & (dt > 0)).sum()); c["ds_exactly_one"] += int((~point & (ds == 1)).sum())
                fs, ft = np.floor(s), np.floor(t)
                c["cell_sum_wraps"] += int((np.abs(np.clip(fs, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.float64) + np.clip(ft, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.float64)) >= 2.0 ** 31).sum())
            elif b["tag"] == "dots":
                s, t = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
                ok = np.isfinite(s) & np.isfinite(t) & (np.abs(s) < 100) & (np.abs(t) < 100)
                cells = np.stack([np.floor(x[:, 0] + F(0.5)), np.floor(x[:, 1] + F(0.5))], axis=1)[ok]
                has, cs, ct = tc.dot_centres(cells)
                dist = np.hypot(s[ok] - cs, t[ok] - ct)
                rim = has & (np.abs(dist - 0.35) < 1e-6)
                inside = (o[ok] == CA).all(axis=1)
                c["dots_inside_rim"] += int((rim & inside).sum()); c["dots_outside_rim"] += int((rim & ~inside).sum())
                assert (inside[has & (dist < 0.35 - 1e-5)]).all() and (~inside[~has | (dist > 0.35 + 1e-5)]).all()
            elif b["tag"] == "uv":
                c["uv_one_exactly"] += int(((o[:, 0] == 1) | (o[:, 1] == 1)).sum())
            elif b["tag"] == "bilerp":
                c["bilerp_corners"] += int((np.isin(x[:, 0], [0, 1]) & np.isin(x[:, 1], [0, 1])).sum())
    check_reach("procedural_2d", c)


def map64(rec, p):
    """(s, t) of SphericalMapping2D / CylindricalMapping2D / PlanarMapping2D in float64"""
    p = np.asarray(p, np.float64)
    if rec["kind"] == "planar":
        prm = np.asarray(rec["prm"], np.float64)
        return prm[6] + p @ prm[0:3], prm[7] + p @ prm[3:6]
    M = rec["w2t"]
    q = p @ M[:3, :3].T + M[:3, 3]
    with np.errstate(all="ignore"):
        v = q / np.linalg.norm(q, axis=1)[:, None]
        if rec["kind"] == "spherical":
            phi = np.arctan2(v[:, 1], v[:, 0]); phi = np.where(phi < 0, phi + 2 * math.pi, phi)
            return np.arccos(np.clip(v[:, 2], -1, 1)) / math.pi, phi / (2 * math.pi)
        return (math.pi + np.arctan2(v[:, 1], v[:, 0])) / (2 * math.pi), v[:, 2]


REACH_MIN["mappings"] = dict(flipped_down=1466, flipped_up=1276, beside_the_switch=2618, at_the_origin=67, on_the_seam=1142, at_a_pole=470)


def test_mappings_reach(host):
    ps, orc, batches, work, want = tc.prepared("mappings", host)
    c = {k: 0 for k in REACH_MIN["mappings"]}
    for b, o in zip(batches, want[0]):
        rec = b["rec"]
        if rec["kind"] == "planar":
            continue
        x = b["ctx"].astype(np.float64); delta = 0.1 if rec["kind"] == "spherical" else 0.01
        with np.errstate(all="ignore"):
            st = map64(rec, x[:, 6:9])
            for dcol in (slice(9, 12), slice(12, 15)):
                sx = map64(rec, x[:, 6:9] + delta * x[:, dcol])
                d = (sx[1] - st[1]) / delta
                c["flipped_down"] += int((d > 0.5).sum()); c["flipped_up"] += int((d < -0.5).sum())
                c["beside_the_switch"] += int((np.abs(np.abs(d) - 0.5) < 1e-5).sum())
            q = x[:, 6:9] @ rec["w2t"][:3, :3].T + rec["w2t"][:3, 3]
            r = np.linalg.norm(q, axis=1)
            c["at_the_origin"] += int((r < 1e-6).sum())
            c["on_the_seam"] += int(((np.abs(q[:, 1]) <= 1e-6 * r) & (np.abs(q[:, 0]) > 0.1 * r) & (r > 1e-3)).sum())
            c["at_a_pole"] += int(((np.hypot(q[:, 0], q[:, 1]) <= 1e-6 * r) & (r > 1e-3)).sum())
    check_reach("mappings", c)


def fbm_n(b):
    """(n, n_int, n_partial) in float32 as fbm forms them (common.rs:119-160); the probes' 3D mapping is the identity"""
    x = b["ctx"]; oc = int(b["tag"].split()[1])
    with np.errstate(all="ignore"):
        dx, dy = x[:, 9:12], x[:, 12:15]
        lx = ((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]).astype(F) + dx[:, 2] * dx[:, 2]).astype(F); ly = ((dy[:, 0] * dy[:, 0] + dy[:, 1] * dy[:, 1]).astype(F) + dy[:, 2] * dy[:, 2]).astype(F)
        len2 = np.where(lx > ly, lx, ly)
        n = (F(-1) - F(0.5) * log2_f32(len2)).astype(F)
        n = np.where(n < 0, F(0), np.where(n > oc, F(oc), n)).astype(F)   # pclamp: a NaN passes through
        n_int = np.floor(n)
    return n, n_int, (n - n_int).astype(F), oc


REACH_MIN["procedural_3d"] = dict(n_int_0=1161, n_int_1=688, n_int_2=212, n_int_3=201, n_int_4=212, n_int_5=255, n_int_6=212, n_int_7=201, n_int_8=468, partial_below=2335, partial_between=776, partial_above=545, n_on_integer=327, n_nan=24, lattice_points=32, marble_first_0=30, marble_first_1=61, checker3d_wraps=47)


def test_procedural_3d_reach(host):
    ps, orc, batches, work, want = tc.prepared("procedural_3d", host)
    c = {k: 0 for k in REACH_MIN["procedural_3d"]}
    for b, o in zip(batches, want[0]):
        x = b["ctx"]
        with np.errstate(all="ignore"):
            if b["tag"].startswith(("fbm", "wrinkled")):
                n, n_int, part, oc = fbm_n(b)
                for k in range(9):
                    c[f"n_int_{k}"] += int((n_int == k).sum())
                c["partial_below"] += int((part < F(0.3)).sum()); c["partial_above"] += int((part > F(0.7)).sum()); c["partial_between"] += int(((part >= F(0.3)) & (part <= F(0.7))).sum())
                c["n_on_integer"] += int(((part == 0) & (n > 0) & (n < oc)).sum()); c["n_nan"] += int(np.isnan(o[:, 0]).sum())
            elif b["tag"].startswith("noise"):
                p = x[:, 6:9]
                c["lattice_points"] += int(((p == np.floor(p)).all(axis=1) & np.isfinite(p).all(axis=1)).sum())
            elif b["tag"] == "marble, variation 0":
                tt = 0.5 + 0.5 * np.sin(x[:, 7].astype(np.float64))
                c["marble_first_0"] += int((tt * 6 < 1).sum()); c["marble_first_1"] += int((tt * 6 >= 1).sum())
            elif b["tag"] == "checkerboard3d":
                f = np.clip(np.floor(x[:, 6:9]), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.float64)
                c["checker3d_wraps"] += int((np.abs(f.sum(axis=1)) >= 2.0 ** 31).sum())
    check_reach("procedural_3d", c)


def bump64(inp, displace, du_disp=None, dv_disp=None):
    """Material::bump's normal before face_forward, in float64, for a displacement that is `displace` at the hit and du_disp / dv_disp at the shifted points (default: the same)"""
    x = inp.astype(np.float64)
    du = 0.5 * (np.abs(x[:, 2]) + np.abs(x[:, 4])); du = np.where(du == 0, 0.0005, du)
    dv = 0.5 * (np.abs(x[:, 3]) + np.abs(x[:, 5])); dv = np.where(dv == 0, 0.0005, dv)
    ud = displace if du_disp is None else du_disp; vd = displace if dv_disp is None else dv_disp
    ns, dpdu, dpdv, dndu, dndv = x[:, 18:21], x[:, 21:24], x[:, 24:27], x[:, 27:30], x[:, 30:33]
    a = dpdu + ((ud - displace) / du)[:, None] * ns + displace * dndu
    bb = dpdv + ((vd - displace) / dv)[:, None] * ns + displace * dndv
    return np.cross(a, bb), a, bb


REACH_MIN["bump"] = dict(substitute_du=2312, substitute_dv=2314, denormal_du=1391, flipped=422, kept=636, tie=844, nan_normal=67, zero_cross=10)


def test_bump_reach(host):
    ps, orc, batches, work, want = tc.prepared("bump", host)
    c = {k: 0 for k in REACH_MIN["bump"]}
    for b, o in zip(batches, want[0]):
        x = b["inp"]
        with np.errstate(all="ignore"):
            du = (F(0.5) * (np.abs(x[:, 2]) + np.abs(x[:, 4]))).astype(F); dv = (F(0.5) * (np.abs(x[:, 3]) + np.abs(x[:, 5]))).astype(F)
            c["substitute_du"] += int((du == 0).sum()); c["substitute_dv"] += int((dv == 0).sum()); c["denormal_du"] += int(((du > 0) & (du < np.finfo(F).tiny)).sum())
            c["nan_normal"] += int(np.isnan(o[:, 0:3]).any(axis=1).sum())
            if b["tag"] == "constant":
                cr, _, _ = bump64(x, 0.25)
                dots = (cr * x[:, 15:18].astype(np.float64)).sum(axis=1)
                ln = np.linalg.norm(cr, axis=1)
                c["zero_cross"] += int((ln == 0).sum())
                c["flipped"] += int((dots < -1e-6 * ln).sum()); c["kept"] += int((dots > 1e-6 * ln).sum()); c["tie"] += int(((dots == 0) & (ln > 0)).sum())
    check_reach("bump", c)


# ---------------------------------------------------------------- b. the oracle against float64 ----------------------------------------------------------------------------
# Each restatement takes the float32 inputs as they are, forms the texel coordinates and branch decisions in float32 as the reference does (they select what is computed) and
# everything after them in float64.  The conditioning masks keep probes whose result is a sum of terms of one sign or stays away from a cancellation; `rel` is
# |oracle - float64| / max(|float64|, floor) with the floor stated per operation.
MEASURED = {}


def rel_err(got, ref, floor):
    return float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), floor))) if len(ref) else 0.0


def check_err(what, got, ref, floor, n_min):
    assert len(ref) >= n_min, (what, len(ref))
    e = rel_err(got, ref, floor)
    print(f"\nfloat64[{what}]: {len(ref)} probes, largest relative error {e:.3e} (asserted {MARGIN * MEASURED[what]:.3e})")
    assert e <= MARGIN * MEASURED[what], (what, e)


def level_texels(orc, m, level=0):
    return orc.mipmap_pyramid(m["id"])[level].astype(np.float64)   # (h, w, 3), row 0 = t 0


def texel64(tex, wrap, s, t):
    h, w = tex.shape[:2]
    if wrap == "repeat":
        return tex[np.mod(t, h), np.mod(s, w)]
    if wrap == "clamp":
        return tex[np.clip(t, 0, h - 1), np.clip(s, 0, w - 1)]
    inside = (s >= 0) & (s < w) & (t >= 0) & (t < h)
    return np.where(inside[:, None], tex[np.clip(t, 0, h - 1), np.clip(s, 0, w - 1)], 0.0)


def triangle64(tex, wrap, s32, t32):
    """MIPMap::triangle (mipmap/mod.rs:293-312) on one level: s32, t32 the float32 st; the texel coordinates in float32, the blend in float64"""
    h, w = tex.shape[:2]
    s = (s32 * F(w) - F(0.5)).astype(F); t = (t32 * F(h) - F(0.5)).astype(F)
    s0 = np.floor(s).astype(np.int64); t0 = np.floor(t).astype(np.int64)
    ds = (s.astype(np.float64) - s0)[:, None]; dt = (t.astype(np.float64) - t0)[:, None]
    return (texel64(tex, wrap, s0, t0) * (1 - ds) * (1 - dt) + texel64(tex, wrap, s0, t0 + 1) * (1 - ds) * dt + texel64(tex, wrap, s0 + 1, t0) * ds * (1 - dt) + texel64(tex, wrap, s0 + 1, t0 + 1) * ds * dt)


MEASURED["bilinear triangle"] = 1.849e-05   # measured on the oracle, 10170 probes


def test_triangle_against_float64(host):
    """mask: finite st with |st| < 1000 (float32 texel coordinates hold their fraction); floor 1e-3 of a texel value in [0, 1] (black wrap mixes in zeros)"""
    ps, orc, batches, work, want = tc.prepared("texel_grid", host)
    got, ref = [], []
    for b, o in zip(batches, want[0]):
        if "map" not in b:
            continue
        s, t = st_of(b)
        ok = np.isfinite(s) & np.isfinite(t) & (np.abs(s) < 1000) & (np.abs(t) < 1000)
        got.append(o[ok]); ref.append(triangle64(level_texels(orc, b["map"]), b["map"]["wrap"], s[ok], t[ok]))
    check_err("bilinear triangle", np.concatenate(got), np.concatenate(ref), 1e-3, 5000)


MEASURED["trilinear blend"] = 1.732e-07   # measured on the oracle, 13728 probes


def test_trilinear_against_float64(host):
    """mask: the blended branch (0 <= level < levels - 1); floor 1e-3"""
    ps, orc, batches, work, want = tc.prepared("trilinear_levels", host)
    got, ref = [], []
    for b, o in zip(batches, want[0]):
        m = b["map"]; L = m["levels"]; lv = trilinear_level(b)
        with np.errstate(all="ignore"):
            ok = (lv >= 0) & (lv < L - 1)
        if not ok.any():
            continue
        pyr = [p.astype(np.float64) for p in orc.mipmap_pyramid(m["id"])]
        s, t = st_of(b)
        il = np.floor(lv[ok]).astype(int); delta = (lv[ok].astype(np.float64) - il)[:, None]
        r = np.zeros((int(ok.sum()), 3))
        for k in np.unique(il):
            sel = il == k
            r[sel] = triangle64(pyr[k], m["wrap"], s[ok][sel], t[ok][sel]) * (1 - delta[sel]) + triangle64(pyr[k + 1], m["wrap"], s[ok][sel], t[ok][sel]) * delta[sel]
        got.append(o[ok]); ref.append(r)
    check_err("trilinear blend", np.concatenate(got), np.concatenate(ref), 1e-3, 3000)


LUT64 = np.array([math.exp(-2.0 * (i / 127.0)) - math.exp(-2.0) for i in range(128)])


def ewa64(tex, wrap, s32, t32, d0, d1):
    """MIPMap::ewa (mipmap/mod.rs:320-371) for one probe in float64, the weight table restated.  Returns (value, conditioned): not conditioned where a texel's r2 is within
    1e-4 of 1 or within 1e-4 * 128 of a table step, where float32 may decide otherwise."""
    h, w = tex.shape[:2]
    s = float(F(s32 * F(w) - F(0.5))); t = float(F(t32 * F(h) - F(0.5)))
    d0x, d0y, d1x, d1y = float(d0[0]) * w, float(d0[1]) * h, float(d1[0]) * w, float(d1[1]) * h
    a = d0y * d0y + d1y * d1y + 1; bq = -2 * (d0x * d0y + d1x * d1y); cq = d0x * d0x + d1x * d1x + 1
    inv_f = 1 / (a * cq - bq * bq * 0.25)
    a *= inv_f; bq *= inv_f; cq *= inv_f
    det = -bq * bq + 4 * a * cq
    us, vs = math.sqrt(det * cq), math.sqrt(a * det)
    lo_s, hi_s, lo_t, hi_t = s - 2 / det * us, s + 2 / det * us, t - 2 / det * vs, t + 2 / det * vs
    edge = min(abs(v - round(v)) for v in (lo_s, hi_s, lo_t, hi_t)) < 1e-3
    iss, itt = np.meshgrid(np.arange(math.ceil(lo_s), math.floor(hi_s) + 1), np.arange(math.ceil(lo_t), math.floor(hi_t) + 1))
    iss, itt = iss.reshape(-1), itt.reshape(-1)
    ss, tt = iss - s, itt - t
    r2 = a * ss * ss + bq * ss * tt + cq * tt * tt
    near = (np.abs(r2 - 1) < 1e-4) | (np.abs(r2 * 128 - np.round(r2 * 128)) < 1e-2)
    inside = r2 < 1
    wts = LUT64[np.minimum((r2[inside] * 128).astype(int), 127)]
    val = (texel64(tex, wrap, iss[inside], itt[inside]) * wts[:, None]).sum(axis=0) / wts.sum() if inside.any() else np.full(3, np.nan)
    return val, not (edge or (near & (r2 < 1.01)).any()) and inside.any()


MEASURED["ewa weighted mean"] = 5.239e-07   # measured on the oracle, 1228 probes


def test_ewa_against_float64(host):
    """every 7th probe with minor_length > 0, both levels il and il + 1 inside the pyramid, finite derivatives and |st| < 100; mask: no texel of either level within 1e-4 of the ellipse's rim or 1e-2 of a weight-table step; floor 1e-3"""
    ps, orc, batches, work, want = tc.prepared("ewa_ellipse", host)
    got, ref = [], []
    for b, o in zip(batches, want[0]):
        m = b["map"]; L = m["levels"]; e = ewa_state(b)
        s, t = st_of(b)
        with np.errstate(all="ignore"):
            ok = (e["minor"] > 0) & (e["lod"] >= 0) & (e["il"] + 1 < L) & np.isfinite(e["d0"]).all(axis=1) & np.isfinite(e["d1"]).all(axis=1) & (np.abs(s) < 100) & (np.abs(t) < 100)
        idx = np.flatnonzero(ok)[::7]
        if not len(idx):
            continue
        pyr = [p.astype(np.float64) for p in orc.mipmap_pyramid(m["id"])]
        for i in idx:
            il = int(e["il"][i]); tl = float(e["lod"][i]) - il
            v0, c0 = ewa64(pyr[il], m["wrap"], s[i], t[i], e["d0"][i], e["d1"][i]); v1, c1 = ewa64(pyr[il + 1], m["wrap"], s[i], t[i], e["d0"][i], e["d1"][i])
            if c0 and c1:
                r = v0 * (1 - tl) + v1 * tl
                got.append(o[i]); ref.append(r)
    check_err("ewa weighted mean", np.array(got), np.array(ref), 1e-3, 300)


MEASURED["checkerboard area"] = 8.821e-06   # measured on the oracle, 599 probes


def test_checker_area_against_float64(host):
    """mask: the filtered branch with 1e-3 <= ds, dt <= 1, |st| < 100, st -+ ds at least 1e-4 from a cell boundary (floor decides the integral's terms); floor 1e-3"""
    ps, orc, batches, work, want = tc.prepared("procedural_2d", host)
    b, o = next((b, o) for b, o in zip(batches, want[0]) if b["tag"] == "checker")
    x = b["ctx"].astype(np.float64)
    with np.errstate(all="ignore"):
        s, t = x[:, 0], x[:, 1]
        ds = np.fmax(np.abs(x[:, 2]), np.abs(x[:, 4])); dt = np.fmax(np.abs(x[:, 3]), np.abs(x[:, 5]))
        s0, s1, t0, t1 = s - ds, s + ds, t - dt, t + dt
        point = (np.floor(s0) == np.floor(s1)) & (np.floor(t0) == np.floor(t1))
        away = lambda v: np.abs(v / 2 - np.round(v / 2)) > 1e-4
        half = lambda v: np.abs(v / 2 - np.floor(v / 2) - 0.5) > 1e-4
        ok = ~point & (ds >= 1e-3) & (dt >= 1e-3) & (ds <= 1) & (dt <= 1) & (np.abs(s) < 100) & (np.abs(t) < 100)
        for v in (s0, s1, t0, t1):
            ok &= away(v) & half(v)
        bump = lambda v: np.floor(v / 2) + 2 * np.maximum(v / 2 - np.floor(v / 2) - 0.5, 0)
        sint = (bump(s1) - bump(s0)) / (2 * ds); tint = (bump(t1) - bump(t0)) / (2 * dt)
        area = sint + tint - 2 * sint * tint
        ref = np.array(tc.CA)[None, :] * (1 - area)[:, None] + np.array(tc.CB)[None, :] * area[:, None]
    check_err("checkerboard area", o[ok], ref[ok], 1e-3, 300)


MEASURED["uv"] = 6.046e-10   # measured on the oracle, 230 probes
MEASURED["bilerp"] = 9.154e-08   # measured on the oracle, 54 probes


def test_uv_and_bilerp_against_float64(host):
    """uv — mask: finite st, |st| < 2^20; the float32 st as input; floor 1e-6 (st - floor(st) is exact in float32 for these: the error is the mapping's).  bilerp — mask: st in
    [0, 1]^2 (every weight non-negative); floor 1e-3"""
    ps, orc, batches, work, want = tc.prepared("procedural_2d", host)
    for b, o in zip(batches, want[0]):
        x = b["ctx"]
        if b["tag"] == "uv":
            ok = np.isfinite(x[:, 0]) & np.isfinite(x[:, 1]) & (np.abs(x[:, 0]) < 2 ** 20) & (np.abs(x[:, 1]) < 2 ** 20)
            st = x[ok, 0:2].astype(np.float64)
            ref = np.concatenate([st - np.floor(st), np.zeros((len(st), 1))], axis=1)
            check_err("uv", o[ok], ref, 1e-6, 200)
        if b["tag"] == "bilerp":
            ok = (x[:, 0] >= 0) & (x[:, 0] <= 1) & (x[:, 1] >= 0) & (x[:, 1] <= 1)
            s, t = x[ok, 0].astype(np.float64)[:, None], x[ok, 1].astype(np.float64)[:, None]
            v = [np.array(c, F).astype(np.float64)[None, :] for c in ((0.1, 0.2, 0.3), (0.9, 0.1, 0.5), (0.2, 0.8, 0.1), (0.7, 0.7, 0.9))]
            ref = v[0] * (1 - s) * (1 - t) + v[1] * (1 - s) * t + v[2] * s * (1 - t) + v[3] * s * t
            check_err("bilerp", o[ok], ref, 1e-3, 30)


MEASURED["mapping (s, t)"] = 1.884e-07   # measured on the oracle, 2252 probes


def test_mappings_against_float64(host):
    """through the uv texture, which returns st - floor(st).  mask: finite points with 1e-3 < |q| < 1e3 in texture space, the float64 fraction within [0.01, 0.99] (away from
    the seam, the poles' phi and an integer of a planar st), planar vectors of moderate size; floor 1e-2"""
    ps, orc, batches, work, want = tc.prepared("mappings", host)
    got, ref = [], []
    for b, o in zip(batches, want[0]):
        rec = b["rec"]
        if rec["tex"] != "uv" or rec.get("xform") in ("huge", "zero"):
            continue
        p = b["ctx"][:, 6:9].astype(np.float64)
        with np.errstate(all="ignore"):
            s, t = map64(rec, p)
            fs, ft = s - np.floor(s), t - np.floor(t)
            r = np.linalg.norm(p, axis=1)
            ok = np.isfinite(p).all(axis=1) & (r > 1e-3) & (r < 1e3) & (fs > 0.01) & (fs < 0.99) & (ft > 0.01) & (ft < 0.99)
            if rec["kind"] != "planar":
                q = p @ rec["w2t"][:3, :3].T + rec["w2t"][:3, 3]
                ok &= (np.linalg.norm(q, axis=1) > 1e-3) & (np.hypot(q[:, 0], q[:, 1]) > 1e-3)
        got.append(o[ok][:, 0:2]); ref.append(np.stack([fs[ok], ft[ok]], axis=1))
    check_err("mapping (s, t)", np.concatenate(got), np.concatenate(ref), 1e-2, 1000)


MEASURED["noise_3d"] = 2.501e-06   # measured on the oracle, 289 probes
MEASURED["fbm, up to 3 octaves"] = 2.598e-05   # measured on the oracle, 822 probes


def test_noise_and_fbm_against_float64(host):
    """noise — mask: finite |p| < 300; floor 0.05 (a noise value is a signed sum of gradient terms of size ~1: the error is absolute at that scale).  fbm — mask: n <= 3,
    n_partial at least 1e-3 from 0, 0.3, 0.7 and 1, finite |p| < 300; floor 0.05"""
    ps, orc, batches, work, want = tc.prepared("procedural_3d", host)
    got, ref = [], []
    for b, o in zip(batches, want[0]):
        x = b["ctx"]; p = x[:, 6:9].astype(np.float64)
        fin = np.isfinite(p).all(axis=1) & (np.abs(p) < 300).all(axis=1)
        if b["tag"].startswith("noise"):
            check_err("noise_3d", o[fin][:, 0], noise64(p[fin]), 0.05, 200)
        elif b["tag"].startswith("fbm"):
            n, n_int, part, oc = fbm_n(b); omega = float(b["tag"].split()[2])
            with np.errstate(all="ignore"):
                fin = fin & np.isfinite(x[:, 9:15]).all(axis=1)   # (the identity mapping's matrix product turns an infinite component into NaNs)
                ok = fin & (n <= 3) & ~np.isnan(n)
                for edge in (0.0, 0.3, 0.7, 1.0):
                    ok &= np.abs(part - edge) > 1e-3
                ok |= fin & (n <= 3) & (part == 0)   # exactly on an integer: smooth_step(0) = 0 on both sides
            if not ok.any():
                continue
            r = np.zeros(int(ok.sum())); lam, w = 1.0, 1.0
            ni = n_int[ok].astype(int); pp = p[ok]
            for k in range(3):
                r += np.where(ni > k, w * noise64(lam * pp), 0.0)
                lam, w = lam * 1.99, w * omega
            # the partial octave: o = omega^n_int, lambda = 1.99^n_int
            v = np.clip((part[ok].astype(np.float64) - 0.3) / 0.4, 0, 1); ss = v * v * (-2 * v + 3)
            r += omega ** ni * ss * noise64((1.99 ** ni)[:, None] * pp)
            got.append(o[ok][:, 0]); ref.append(r)
    check_err("fbm, up to 3 octaves", np.concatenate(got), np.concatenate(ref), 0.05, 200)


def noise64(p):
    return tc.noise64(p[:, 0], p[:, 1], p[:, 2])


MEASURED["bumped normal"] = 1.638e-07   # measured on the oracle, 960 probes


def test_bumped_normal_against_float64(host):
    """the constant displacement (u_displace = v_displace = displace: the normal is that of dpdu + d dndu and dpdv + d dndv).  mask: finite inputs, |cross| at least 1e-3 of the
    product of the two lengths, |normal . n| at least 1e-3 (away from face_forward's tie); floor 1e-3 per component of a unit vector"""
    ps, orc, batches, work, want = tc.prepared("bump", host)
    b, o = next((b, o) for b, o in zip(batches, want[0]) if b["tag"] == "constant")
    x = b["inp"]
    with np.errstate(all="ignore"):
        cr, a, bb = bump64(x, float(F(0.25)))
        ln = np.linalg.norm(cr, axis=1)
        nrm = cr / ln[:, None]
        dots = (nrm * x[:, 15:18].astype(np.float64)).sum(axis=1)
        ok = np.isfinite(x).all(axis=1) & (ln > 1e-3 * np.linalg.norm(a, axis=1) * np.linalg.norm(bb, axis=1)) & (np.abs(dots) > 1e-3) & (ln < 1e30) & (ln > 1e-30)
        ref = np.where((dots < 0)[:, None], -nrm, nrm)
    check_err("bumped normal", o[ok][:, 0:3], ref[ok], 1e-3, 500)
    assert same_bits(o[ok][:, 3:6], a[ok].astype(F)) or rel_err(o[ok][:, 3:6], a[ok], 1e-30) < 1e-6
