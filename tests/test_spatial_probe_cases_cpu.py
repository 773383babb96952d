"""not gpu: what the sets of spatial_probe_cases reach on the oracle, and the oracle's answers against an independent float64 NumPy restatement of
core/src/light_distrib/spatial.rs (the voxel of a point, the resolution rule) and distribution_1d.rs (cdf, func_int, the floor), in the manner of test_oracle_spatial.py.
Every distribution of every set must be finite: the comparison on the device then needs no rule for NaN."""
import os
import re

import numpy as np
import pytest

import pbrt_hip
import spatial_probe_cases as sc
from oracle_binding import OracleScene
from probe_cases import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(case, host):
    """(oracle scene, p, u, pi, light, pdf, nv, {voxel: (func, cdf, func_int)}) of one case"""
    orc = OracleScene()
    case.capture(orc, host)
    p, u = case.points(orc)
    pi, light, pdf, nv = orc.spatial_lookup_batch(p, u, case.strategy)
    tables = {}
    if len(case.voxels):
        vpi = orc.spatial_lookup_batch(case.voxels, np.full(len(case.voxels), 0.5, F))[0]
        tables = {tuple(int(x) for x in q): orc.spatial_voxel(q, case.n_lights) for q in vpi}
    return orc, p, u, pi, light, pdf, nv, tables


def voxel_f64(case, p, nv):
    """lookup's voxel in float64: offset = (p - lo) / (hi - lo) where hi > lo, else p - lo; index = clamp(trunc(offset * nv), 0, nv - 1), NaN -> 0.  Also the products."""
    lo, hi = case.lo.astype(np.float64), case.hi.astype(np.float64)
    o = p.astype(np.float64) - lo
    ext = hi - lo
    o = np.where(ext > 0, o / np.where(ext > 0, ext, 1.0), o)
    prod = o * np.asarray(nv, np.float64)
    with np.errstate(invalid="ignore"):
        idx = np.where(np.isnan(prod), 0.0, np.clip(np.trunc(np.nan_to_num(prod, nan=0.0, posinf=1e18, neginf=-1e18)), 0, np.asarray(nv, np.float64) - 1))
    return idx.astype(np.int64), prod


@pytest.mark.parametrize("name", ["grid", "flat"])
def test_lookup_sets_reach_their_flags_and_match_float64(host, name, capsys):
    """The float32 oracle and the float64 restatement may name different voxels only at boundary points whose float64 product (p - lo) / (hi - lo) * nv lies within
    BOUNDARY_SLACK of an integer: an absolute 1e-6 where the product is at most 1; above that what float32's three roundings (p - lo, the division, the product) can move
    it by, 2^-24 of the product each and once more for lo, hi and the extent being float32 themselves: 4 * 2^-24 * |product| (1.5e-5 at the top of a 64-voxel axis).  The
    farthest disagreement is asserted against that bound.  Measured: grid 135 of 552 boundary points differ, the farthest 5.3e-6 from its integer at a product of 63
    (1.4 * 2^-24 of it); flat 0 of 726 (there p - lo, the division and the product are exact in float32)."""
    reached, n_boundary, n_close, farthest = 0, 0, 0, 0.0
    for case in sc.SETS[name]:
        orc, p, u, pi, light, pdf, nv, _ = run_case(case, host)
        assert nv == sc.resolution_rule(case.hi - case.lo)[0], (case.name, nv)
        assert ((pi >= 0) & (pi < np.asarray(nv))).all(), "every voxel is a valid clamped index, NaN and inf included"
        assert np.isfinite(pdf).all() and (light < case.n_lights).all()
        reached |= sc.flags_of(case, p, u, pi, light, nv)
        want, prod = voxel_f64(case, p, nv)
        differ = want != pi
        with np.errstate(invalid="ignore"):
            dist = np.abs(prod - np.round(prod))
            slack = np.where(np.abs(prod) <= 1.0, 1e-6, 4.0 * 2.0 ** -24 * np.abs(prod))
            near = dist <= slack
        bad = (differ & ~near).any(axis=1)
        assert not bad.any(), sc.describe(name, case, p, u, int(np.flatnonzero(bad)[0])) + f" oracle {pi[bad][0]} float64 {want[bad][0]}"
        bp = sc.boundary_points(case, orc, nv, every=7 if case.name == "far_from_origin" else 1)
        n_boundary += len(bp); n_close += int(differ.any(axis=1).sum())
        if differ.any():
            farthest = max(farthest, float(dist[differ].max()))
            assert (dist[differ] <= slack[differ]).all() and farthest <= 4.0 * 2.0 ** -24 * 64.0
    with capsys.disabled():
        print(f"\n[spatial probe] set {name}: flags {sc.flag_names(reached)}; {n_close} of {n_boundary} boundary points differ from float64, the farthest {farthest:.3g} from an integer")
    assert n_close * 2 < n_boundary, "the disagreements must be a minority of the boundary points"
    missing = sc.MUST_REACH[name] & ~reached
    assert not missing, sc.flag_names(missing)


def test_resolution_rule(host):
    """round-half-away of diag / max * 64 in float32; the chosen extents put exact halves in front of the rounding"""
    halves = 0
    for case, extent in zip(sc.SETS["resolution"], sc.RESOLUTION_EXTENTS):
        want, ratio = sc.resolution_rule(extent)
        halves += int(np.sum(ratio - np.floor(ratio) == F(0.5)))
        orc, p, u, pi, light, pdf, nv, _ = run_case(case, host)
        assert nv == want, (extent, nv, want)
        assert ((pi >= 0) & (pi < np.asarray(nv))).all()
    assert sc.resolution_rule((64.0, 2.5, 4.5))[0] == (64, 3, 5) and sc.resolution_rule((64.0, 0.5, 1.5))[0] == (64, 1, 2)   # banker's rounding would give (64, 2, 4) and (64, 0 -> 1, 2)
    assert sc.resolution_rule((4.0, 2.0, 0.01))[0] == (64, 32, 1) and sc.resolution_rule((1.0, 1.0, 1.0))[0] == (64, 64, 64)
    assert halves == 4, "2.5, 4.5, 0.5 and 1.5 of 64 are exact halves in float32"


def test_many_voxels_are_distinct(host):
    case = sc.SETS["many_voxels"][0]
    orc = OracleScene(); case.capture(orc, host)
    first, second, third = sc.many_voxel_batches()
    seen = set()
    counts = []
    for b in (first, second, third):
        pi, light, pdf, nv = orc.spatial_lookup_batch(b, np.full(len(b), 0.5, F))
        assert nv == (64, 64, 64) and np.isfinite(pdf).all()
        seen |= {tuple(q) for q in pi}
        counts.append(len(seen))
    assert counts == [sc.MANY_LATTICE ** 3, sc.MANY_LATTICE ** 3 + 1, sc.MANY_LATTICE ** 3 + 2] and counts[0] >= 3000
    p, u = case.points(orc)
    pi = orc.spatial_lookup_batch(p, u)[0]
    assert sc.flags_of(case, p, u, pi, np.zeros(len(p), np.uint32), (64, 64, 64)) & sc.SECOND_STRIDE


def check_tables(case, tables):
    """cdf[k] = sum func / n normalised, func_int = mean(func), the floor: float64 against the oracle's float32, at test_oracle_spatial.py's tolerance"""
    for q, (func, cdf, func_int) in tables.items():
        assert np.isfinite(func).all() and np.isfinite(cdf).all() and np.isfinite(func_int), (case.name, q)
        n = len(func)
        f64 = func.astype(np.float64)
        tol = 1e-6 * max(1.0, n / 64.0)   # the float32 running sum of n terms
        assert func_int == pytest.approx(f64.mean(), rel=tol), (case.name, q)
        assert cdf[0] == 0 and cdf[-1] == 1
        np.testing.assert_allclose(cdf[1:], np.cumsum(f64) / f64.sum(), rtol=tol, atol=tol, err_msg=f"{case.name} {q}")
        floor = f64.min()
        if func_int == 1 and (func == 1).all():
            continue   # every light contributed nothing: min_contrib = 1
        assert (f64 > 0).all()
        floored = f64 == floor
        if floored.sum() > 1 or case.name.startswith("lights_"):   # a floored entry: 0.001 * the average of the contributions, which the unfloored entries alone made up
            avg = f64[~floored].sum() / (128.0 * n)
            if np.isclose(floor, 0.001 * avg, rtol=1e-3):
                assert floor == pytest.approx(0.001 * avg, rel=2e-5), (case.name, q)


@pytest.mark.parametrize("name", ["light_counts", "kinds", "pick"])
def test_table_sets_reach_their_flags_and_match_float64(host, name, capsys):
    reached, n_u = 0, 0
    for case in sc.SETS[name]:
        orc, p, u, pi, light, pdf, nv, tables = run_case(case, host)
        assert np.isfinite(pdf).all() and (light < case.n_lights).all(), case.name
        check_tables(case, tables)
        reached |= sc.flags_of(case, p, u, pi, light, nv, tables)
        n_u += len(u)
        if case.strategy == 2:   # the pick against the table: light k for cdf[k] <= u < cdf[k + 1], pdf = func[k] / (func_int * n)
            for v in case.voxels:
                q = tuple(int(x) for x in orc.spatial_lookup_batch(v.reshape(1, 3), [0.5])[0][0])
                func, cdf, func_int = tables[q]
                sel = (p == v).all(axis=1) & (u >= 0) & (u < 1)
                k = light[sel].astype(np.int64)
                assert ((cdf[k] <= u[sel]) & (u[sel] < cdf[k + 1])).all(), (case.name, q)
                np.testing.assert_allclose(pdf[sel], func[k].astype(np.float64) / (np.float64(func_int) * len(func)), rtol=1e-6)
    if name == "kinds":   # the disk and cylinder lights, which the oracle does not have (test_disk_and_cylinder_voxels)
        from oracle_binding import oracle_binding
        reached |= sc.restated_points(sc.DISK_CYLINDER, host, oracle_binding().lib.oracle_radical_inverse)[6]
    if name == "light_counts":
        assert [c.n_lights for c in sc.SETS[name]] == sc.LIGHT_COUNTS
    with capsys.disabled():
        print(f"\n[spatial probe] set {name}: flags {sc.flag_names(reached)}; {n_u} samples over {sum(len(c.voxels) for c in sc.SETS[name])} voxels")
    missing = sc.MUST_REACH[name] & ~reached
    assert not missing, sc.flag_names(missing)


def test_kind_voxels_lie_where_they_were_aimed(host):
    """the spot's three regions, the emitters' sides, the sphere's inside, the floor of 1: read off the oracle's tables"""
    by_name = {c.name: c for c in sc.KINDS}

    def funcs(name):
        case = by_name[name]
        orc, p, u, pi, light, pdf, nv, tables = run_case(case, host)
        vpi = orc.spatial_lookup_batch(case.voxels, np.full(len(case.voxels), 0.5, F))[0]
        return [tables[tuple(int(x) for x in q)][0] for q in vpi]
    inside, across, outside, _ = funcs("spot")   # lights 0 .. 4 about +z: falloff cone; no falloff at the total width (1, 2) and at the start of the falloff (3, 4); 5 a point light
    assert inside[0] == inside[1] == inside[3] == inside[5] > 1.0                      # fall = 1: the spots are the point light
    assert across[3] == across[4] == across.min() < across[0] < across[1] == across[5]   # outside the narrow cones (floored), partly lit by the falloff, fully by the wide cone
    assert (outside[:5] == outside.min()).all() and outside[5] > 1.0                   # every cone about +z floored at 0.001 x average, which the point light alone makes up
    assert outside.min() == pytest.approx(0.001 * outside[5] / (128.0 * 8), rel=2e-5)
    below, holds, far, beside = funcs("triangles")   # emitters: towards, away, two_sided, inside
    assert below[1] == below.min() == below[3] and below[0] > below[2] > 1.0          # under the inner emitter, which faces up, and behind the one facing away
    assert holds[3] > 1.0 and holds[1] == holds.min()                                 # the voxel that contains the emitter
    sph = funcs("quadrics")
    assert sph[0][0] == sph[0].min() and sph[2][0] > sph[1][0] > 1.0                   # inside the one-sided sphere nothing arrives; straddling it less than outside
    assert sph[4][1] > 1000.0                                                          # inside the reversed two-sided sphere
    for f in funcs("facing_away"):
        assert (f == 1).all()
    for f in funcs("infinite_map"):
        assert f[6] == f.min() and (f[:6] > 100).all()                                 # the black map


def test_disk_and_cylinder_voxels(host, capsys):
    """the part of `kinds` the oracle cannot run: the float32 restatement's tables are finite, its voxels reach the four positions against a light, and it agrees with float64"""
    from oracle_binding import oracle_binding
    case = sc.DISK_CYLINDER
    p, u, tables, pi, light, pdf, reached = sc.restated_points(case, host, oracle_binding().lib.oracle_radical_inverse)
    case.n_lights = len(sc.QUADRIC_LIGHTS)
    check_tables(case, tables)
    assert np.isfinite(pdf).all() and len(tables) == len(case.voxels)
    want, _ = voxel_f64(case, p, (64, 64, 64))
    assert (want == pi).all()
    # the same contributions from the restatement run in float64: sample_li's own arithmetic, not only the sums
    halton = sc.halton_128(oracle_binding().lib.oracle_radical_inverse)
    shapes = sc.quadric_shapes(host)
    worst = 0.0
    for q, (func, cdf, func_int) in tables.items():
        lo, hi = sc.voxel_bounds_f32(case, q, (64, 64, 64))
        ref = np.zeros((128, 10)); ref[:, :3] = (1.0 - halton[:, :3].astype(np.float64)) * lo + halton[:, :3].astype(np.float64) * hi
        for j, (shape, L, two) in enumerate(shapes):
            o = sc.QR.sample_li(shape, L, two, ref, halton[:, 3:5].astype(np.float64), T=np.float64)
            ok = (o[:, 7] == 1) & (o[:, 3] > 0)
            acc = float(np.sum((0.212671 * o[ok, 4] + 0.715160 * o[ok, 5] + 0.072169 * o[ok, 6]) / o[ok, 3]))
            if func[j] > func.min():   # not floored
                worst = max(worst, abs(func[j] - acc) / acc)
    with capsys.disabled():
        print(f"\n[spatial probe] disk and cylinder lights: flags {sc.flag_names(reached)}; {len(u)} samples over {len(tables)} voxels; func against float64: {worst:.3g} relative at most")
    assert worst <= 2e-5   # test_oracle_spatial.py's tolerance for the 128-point quadrature
    assert reached == sc.Q_OUTSIDE | sc.Q_STRADDLES | sc.Q_CONTAINS | sc.Q_INSIDE


def test_point_light_quadrature_float64(host):
    """func of the 2-light case against the 128-point Halton quadrature in float64 (test_oracle_spatial.py's check, at the probe's voxels)"""
    from test_oracle_spatial import radical_inverse
    case = sc.SETS["light_counts"][0]
    orc, p, u, pi, light, pdf, nv, tables = run_case(case, host)
    pos, inten = sc.count_light_arrays(2)
    pos = pos.astype(np.float64)
    y = lambda c: 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2]
    ext = (case.hi - case.lo).astype(np.float64)
    for q, (func, cdf, func_int) in tables.items():
        lo = case.lo + np.array(q) / np.array(nv) * ext; hi = case.lo + (np.array(q) + 1) / np.array(nv) * ext
        acc = 0.0
        for i in range(128):
            t = np.array([radical_inverse(2, i), radical_inverse(3, i), radical_inverse(5, i)])
            acc += y(inten[0].astype(np.float64)) / np.sum((pos[0] - ((1 - t) * lo + t * hi)) ** 2)
        assert func[0] == pytest.approx(acc, rel=2e-5)
        assert func[1] == pytest.approx(0.001 * acc / 256.0, rel=2e-5)   # the zero-intensity light: the floor


def test_the_probe_is_declared_and_bound():
    text = open(ROOT + "/include/pbrt_hip.h").read()
    for name in ("spatial_probe_begin", "spatial_probe_batch", "spatial_probe_voxel"):
        assert re.search(r"\bint\s+pbrt_hip_%s\s*\(" % name, text)
        assert pbrt_hip.default_binding().has(name)
    b = pbrt_hip.default_binding()
    assert b.fn("spatial_probe_begin")(None, None, None) == pbrt_hip.ERR_INVALID_ARG   # a null handle is an error, not a crash
    assert b.fn("spatial_probe_voxel")(None, None, None, None, None) == pbrt_hip.ERR_INVALID_ARG
