"""tests/curve_restatement.py alone, against closed forms and the reference's source text (no GPU, no library): a straight flat curve seen at right angles, the two quirks of
recursive_intersect as it runs (each with the reference's odd answer, and Curve::intersect_p differing from Curve::intersect where curve.rs says it must), log2int at its
edges, CurveData::new, object_bound, create_segments and from_props."""
import numpy as np
import pytest

import curve_cases as CC
import curve_restatement as cr

F = np.float32
INF = np.float32(np.inf)


def straight(width, ctype="flat", n=None):
    # collinear, evenly spaced in exact binary fractions along x: the Bezier is the line itself, u = (x + 1) / 2
    return cr.curve_data(ctype, [[-1, 0, 0], [-0.5, 0, 0], [0, 0, 0], [0.5, 0, 0]], [width, width], n)


def test_straight_flat_curve_seen_at_right_angles():
    """A hit exactly when the ray passes within w / 2 of the axis and between the end tangent planes; v = 0.5 +- dist / w; t = the distance to the axis plane"""
    w = 0.25
    cd = straight(w)
    seg = cr.segment(cd, 0, 1)
    rng = np.random.default_rng(3)
    n = 20000
    # x, y on a 1/1024 grid (exact in f32, and so is everything the test derives from them); rays run down -z from z = 3
    x = rng.integers(-1280, 768, n) / 1024.0; y = rng.integers(-256, 257, n) / 1024.0
    y[:64] = np.array([w / 2, -w / 2] * 32); x[64:128] = np.array([-1.0, 0.5] * 32)          # on the rim and on the end planes: inclusive
    o = np.stack([x, y, np.full(n, 3.0)], 1).astype(np.float32); d = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
    r = cr.intersect(seg, o, d, np.full(n, INF))
    want = (np.abs(y) <= w / 2) & (x >= -1.0) & (x <= 0.5)
    assert np.array_equal(r[:, 0] != 0, want)
    assert want.sum() > 3000 and (~want).sum() > 3000
    h = want
    assert np.all(np.abs(r[h, 1] - 3.0) < 2e-6)      # t: z = 3 down to the plane z = 0, less the push of transform_ray_with_error (gamma(3) * |o|, transform.rs:485-490)
    assert np.allclose(r[h, 2], (x[h] + 1.0) / 1.5, atol=2e-7)                                  # u along the line
    dist = np.abs(y[h]) / w
    assert np.all((np.abs(r[h, 3] - (0.5 + dist)) < 1e-6) | (np.abs(r[h, 3] - (0.5 - dist)) < 1e-6))   # v = 0.5 +- dist / w
    side = np.sign(r[h, 3] - 0.5)
    assert np.all(side[y[h] != 0] == side[y[h] != 0][0] * np.sign(y[h][y[h] != 0]) * np.sign(y[h][y[h] != 0][0]))   # one side of the axis, one sign
    assert np.allclose(r[h, 4:7], np.stack([x[h], y[h], np.zeros(h.sum())], 1), atol=1e-6)      # p = ray.at(t)
    assert np.all(np.abs(r[h, 7:10] - 2 * w) < 1e-5)      # p_error = 2 * hit_width, plus the gamma(3) terms of transform_point_with_abs_error
    # a flat curve faces the ray: n is +-z; dpdu runs along the line, |dpdv| = the width
    assert np.allclose(np.abs(r[h, 16:19]), [0, 0, 1], atol=1e-6)
    assert np.allclose(r[h, 10:13], [1.5, 0, 0], atol=1e-6) and np.allclose(np.linalg.norm(r[h, 13:16], axis=1), w, atol=1e-6)
    # intersect_p agrees here (refinement depth 0: no halves to overwrite), and a t_max short of the plane misses
    assert np.array_equal(cr.intersect_p(seg, o, d, np.full(n, INF)), want)
    assert not cr.intersect(seg, o, d, np.full(n, 2.5, np.float32))[:, 0].any()


def test_ribbon_edge_on_has_no_width():
    """Ribbon normals perpendicular to the view: |n_hit . d| = 0 scales hit_width to zero, so no ray that misses the axis itself survives the width test"""
    # (two EQUAL normals would make normal_angle 0 and inv_sin_normal_angle infinite: sin0 = 0 * inf = NaN, and a NaN hit_width passes the width test — the reference's answer too)
    cd = straight(0.25, "ribbon", [[0, 1, 0], [0.1, 1, 0]])
    seg = cr.segment(cd, 0, 1)
    y = np.array([1e-4, 1e-3, -1e-3, 0.05, -0.1], np.float32)
    o = np.stack([np.zeros(5), y, np.full(5, 3.0)], 1).astype(np.float32); d = np.tile(np.array([0, 0, -1], np.float32), (5, 1))
    r = cr.intersect(seg, o, d, np.full(5, INF))
    assert not r[:, 0].any()
    face_on = cr.segment(straight(0.25, "ribbon", [[0, 0, 1], [0.1, 0, 1]]), 0, 1)
    assert list(cr.intersect(face_on, o, d, np.full(5, INF))[:, 0] != 0) == [True, True, True, True, True]


def test_overwrite_quirk():
    """curve.rs:413: `hit = self.recursive_intersect(..)` is unconditional, so a miss in the second half erases the first half's hit — for Curve::intersect only;
    Curve::intersect_p returned at the first hit (:429-431)"""
    q = CC.OVERWRITE
    seg = cr.segment(cr.curve_data(q["type"], q["cp"], q["width"]), 0, 1)
    o, d = np.array([q["o"]], np.float32), np.array([q["d"]], np.float32)
    assert cr.intersect_p(seg, o, d, [INF])[0]
    assert cr.intersect(seg, o, d, [INF])[0, 0] == 0
    # the ray does pass through the ribbon, in its first half, and nowhere near the second: in float64, the curve's distance to the ray in the plane it is seen in
    u = np.linspace(0, 1, 4001)[:, None]
    c = np.asarray(q["cp"], np.float64)
    pts = (1 - u) ** 3 * c[0] + 3 * (1 - u) ** 2 * u * c[1] + 3 * (1 - u) * u * u * c[2] + u ** 3 * c[3]
    dist = np.hypot(pts[:, 0] - q["o"][0], pts[:, 1] - q["o"][1])
    assert dist[:2000].min() < 0.25 * q["width"][0] and dist[2000:].min() > 5 * q["width"][0]


def test_wrong_half_quirk():
    """curve.rs:381 / :395 / :410 / :433: `continue` skips `cps += 3`, so after a culled first half the second is tested on the FIRST half's control points.  Here the first half
    is culled by z_max = ray_length * t_max, so a shorter t_max loses a hit that lies well inside it"""
    q = CC.WRONG_HALF
    seg = cr.segment(cr.curve_data(q["type"], q["cp"], q["width"]), 0, 1)
    o, d = np.array([q["o"]], np.float32), np.array([q["d"]], np.float32)
    long_ = cr.intersect(seg, o, d, [q["t_long"]])
    assert long_[0, 0] == 1 and abs(long_[0, 1] - 1.6) < 1e-5 and long_[0, 2] > 0.5          # in the second half, at t = 1.6
    assert long_[0, 1] < q["t_short"]
    short = cr.intersect(seg, o, d, [q["t_short"]])
    assert short[0, 0] == 0                                                                     # the reference's answer: missed
    assert cr.intersect_p(seg, o, d, [q["t_long"]])[0] and not cr.intersect_p(seg, o, d, [q["t_short"]])[0]   # intersect_p walks the same boxes: it differs with t_max the same way
    # the second half as a Curve of its own has no first half to be confused with: it reports the hit under the short t_max
    own = cr.intersect(cr.segment(cr.curve_data(q["type"], q["cp"], q["width"]), 0.5, 1.0), o, d, [q["t_short"]])
    assert own[0, 0] == 1 and abs(own[0, 1] - 1.6) < 1e-4


def test_log2int_edges_and_refinement_depth():
    x = np.array([0.0, -3.0, 0.99999994, 1.0, 1.0000001, 2.0, 3.0, 4.0, 1e30, np.inf, np.nan, -np.inf], np.float32)
    # exponent + the mantissa's lowest bit (log2int.rs:19-23: `a` is 1, not 1 << 22)
    assert list(cr.log2int(x)[:9]) == [0, 0, 0, 0, 1, 1, 1, 2, 99 + int(np.float32(1e30).view(np.uint32) & 1)]
    assert cr.log2int(x[9:10])[0] == 128 and cr.log2int(x[10:11])[0] >= 128 and cr.log2int(x[11:12])[0] == 0
    assert int(cr.max_depth_of(F(0), F(0))) == 10      # 0 / 0 = NaN fails `< 1.0`: depth 10 (collinear control points AND zero width)
    assert int(cr.max_depth_of(F(1), F(0))) == 10      # x / 0 = +inf
    assert int(cr.max_depth_of(F(0), F(0.1))) == 0     # l0 == 0: depth 0
    assert int(cr.max_depth_of(F(0.01), F(1.0))) == 0
    assert int(cr.max_depth_of(F(1.0), F(0.01))) == (int(cr.log2int(F(1.41421356237) * F(6.0) * F(1.0) / (F(8.0) * F(0.01)))) // 2)
    assert int(cr.max_depth_of(F(1e30), F(1e-30))) == 10


def test_curve_data_and_bounds():
    cd = cr.curve_data("flat", [[0, 0, 0], [1, 2, 0], [2, -1, 1], [3, 0, 0]], [0.2, 0.6])
    assert not cd["n"].any() and abs(float(cd["normal_angle"]) - np.pi / 2) < 1e-6 and float(cd["inv_sin_normal_angle"]) == 1.0   # acos(0), 1 / sin of it
    rb = cr.curve_data("ribbon", [[0, 0, 0], [1, 2, 0], [2, -1, 1], [3, 0, 0]], [0.2, 0.6], [[0, 0, 2], [0, 3, 3]])
    assert np.allclose(np.linalg.norm(rb["n"], axis=1), 1, atol=1e-6) and abs(float(rb["normal_angle"]) - np.pi / 4) < 1e-6
    lo, hi = cr.object_bound(cd, 0, 1)
    assert np.allclose(lo, [-0.3, -1.3, -0.3], atol=1e-6) and np.allclose(hi, [3.3, 2.3, 1.3], atol=1e-6)      # the hull of the four points, + half the larger width
    segs = cr.create_segments(3)
    assert len(segs) == 8 and segs[0][0] == 0 and segs[-1][1] == 1 and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
    # a segment's bound holds its piece of the curve and shrinks with it
    u = np.linspace(0.25, 0.5, 50)[:, None]
    c = cd["cp_obj"].astype(np.float64)
    pts = (1 - u) ** 3 * c[0] + 3 * (1 - u) ** 2 * u * c[1] + 3 * (1 - u) * u * u * c[2] + u ** 3 * c[3]
    lo, hi = cr.object_bound(cd, 0.25, 0.5)
    assert np.all(pts >= lo - 1e-6) and np.all(pts <= hi + 1e-6) and np.all(hi - lo < np.array([3.6, 3.6, 1.6]))


def test_from_props():
    P4 = [[0, 0, 0], [1, 1, 0], [2, -1, 0], [3, 0, 0]]
    segs, warn = cr.from_props(P4)
    assert len(segs) == 1 and not warn and segs[0]["type"] == cr.FLAT and segs[0]["split_depth"] == 3 and np.array_equal(segs[0]["cp"], np.asarray(P4, np.float32))
    assert np.array_equal(segs[0]["width"], [1, 1])
    P7 = P4 + [[4, 1, 0], [5, -1, 0], [6, 0, 0]]
    segs, _ = cr.from_props(P7, width0=0.0, width1=1.0, splitdepth=1)
    assert len(segs) == 2 and np.allclose(segs[0]["width"], [0, 0.5]) and np.allclose(segs[1]["width"], [0.5, 1.0]) and segs[1]["split_depth"] == 1
    assert np.array_equal(segs[1]["cp"][0], segs[0]["cp"][3])
    # degree 2: elevated to a cubic that is the same parabola
    q, _ = cr.from_props([[0, 0, 0], [1, 2, 0], [2, 0, 0]], degree=2)
    u = 0.3
    quad = (1 - u) ** 2 * np.array([0, 0, 0]) + 2 * (1 - u) * u * np.array([1, 2, 0]) + u * u * np.array([2, 0, 0])
    c = q[0]["cp"].astype(np.float64)
    assert np.allclose((1 - u) ** 3 * c[0] + 3 * (1 - u) ** 2 * u * c[1] + 3 * (1 - u) * u * u * c[2] + u ** 3 * c[3], quad, atol=1e-6)
    # b-splines: n_cp - degree segments that join
    b3, _ = cr.from_props(P7, basis="bspline")
    assert len(b3) == 4 and all(np.allclose(a["cp"][3], b["cp"][0], atol=1e-6) for a, b in zip(b3, b3[1:]))
    b2, _ = cr.from_props(P7, basis="bspline", degree=2)
    assert len(b2) == 5 and np.allclose(b2[0]["cp"][0], [0.5, 0.5, 0])
    # the type: an unknown name is a cylinder with a warning; normals on a non-ribbon are dropped with a warning
    s, warn = cr.from_props(P4, curve_type="tube")
    assert s[0]["type"] == cr.CYLINDER and "Unknown curve type" in warn[0]
    s, warn = cr.from_props(P4, curve_type="cylinder", N=[[0, 0, 1], [0, 0, 1]])
    assert s[0]["n"] is None and "only used with 'ribbon'" in warn[0]
    s, _ = cr.from_props(P7, curve_type="ribbon", N=[[0, 0, 1], [0, 1, 1], [0, 1, 0]])
    assert np.array_equal(s[1]["n"], np.array([[0, 1, 1], [0, 1, 0]], np.float32))
    for bad in (dict(degree=4), dict(basis="catmull"), dict(P=P4 + [[4, 0, 0]]), dict(P=P4[:3], basis="bspline"), dict(curve_type="ribbon"),
                dict(curve_type="ribbon", N=[[0, 0, 1]])):
        kw = dict(P=P4); kw.update(bad)
        with pytest.raises(cr.CurvePanic):
            cr.from_props(**kw)


def test_loop_subdivision_of_the_showcases_tetrahedron():
    """tests/loop_subdivision.py (the stand-in for the showcase's loopsubdiv block in tests/test_curve_render_gpu.py): counts of a closed mesh, symmetry, the limit surface inside
    the control hull, and the four original vertices still of valence 3"""
    from loop_subdivision import loop_subdivide
    tet = np.array([[0.9428, 0.0, -0.3333], [-0.4714, 0.8165, -0.3333], [-0.4714, -0.8165, -0.3333], [0.0, 0.0, 1.0]])
    faces = [0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2]
    for levels in range(4):
        P, idx = loop_subdivide(tet, faces, levels)
        f = 4 * 4 ** levels
        assert len(idx) == 3 * f and len(P) == f // 2 + 2            # V - E + F = 2 with E = 3 F / 2
        valence = np.bincount(idx)
        assert sorted(valence)[:4] == [3, 3, 3, 3] and (np.sort(valence)[4:] == 6).all()
        assert np.abs(P).max() < np.abs(tet).max() and np.allclose(P.mean(0), tet.mean(0), atol=0.05)
    # one level by hand: an original vertex keeps 1 - 3 * 3/16 of itself; an edge vertex is 3/8, 3/8, 1/8, 1/8
    P, idx = loop_subdivide(tet, faces, 0)
    g = 1.0 / (3 + 3.0 / (8.0 * 3.0 / 16.0))
    assert np.allclose(P[3], tet[3] * (1 - 3 * g) + (tet[0] + tet[1] + tet[2]) * g)
