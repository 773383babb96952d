"""The curves and rays the curve tests share: the two hand-built quirk cases (tests/test_curve_restatement_cpu.py explains them), the probe set of tests/test_curve_gpu.py
(about 64 single segments x 4096 rays), and the small scenes of its scene-level test.  Everything is seeded; nothing here needs a GPU."""
import numpy as np

import curve_restatement as cr
import pbrt_hip

INF = np.float32(np.inf)

# The wrong-half quirk.  The curve runs from z = 4 to z = 1 almost along the ray (origin (0.03, 0, 0), direction +z), so both halves' boxes hold the ray in x and y; refinement depth 1.
# With a long t_max both halves are evaluated and the second — on its own control points — is hit at t = 1.6.  With t_max = 2.2 the FIRST half (z in [2.5, 4]) is culled in z, `cps`
# stays 0, and the second half is tested on the first half's control points: culled as well.  The reference misses a hit at t = 1.6 < 2.2.
WRONG_HALF = dict(type="flat", cp=[[-0.05, 0, 4], [-0.02, 0.05, 3], [0.02, -0.05, 2], [0.05, 0, 1]], width=[0.4, 0.4], o=[0.03, 0, 0], d=[0, 0, 1], t_long=3.0, t_short=2.2)
# The overwrite quirk.  An arch seen from above; the ray comes down on its left leg (first half).  The second half's box — the hull of its control points — holds the ray too, its
# leaf evaluation misses, and `hit = ...` overwrites the first half's hit: Curve::intersect misses what Curve::intersect_p (which returned at the first hit) reports.
OVERWRITE = dict(type="flat", cp=[[-1, -1, 0], [-1, 1, 0], [1, 1, 0], [1, -1, 0]], width=[0.2, 0.2], o=[-1.0, -0.7, -3.0], d=[0, 0, 1])


def mk_rays(o, d, t_max=INF):
    r = np.zeros(len(o), pbrt_hip.RAY_DTYPE)
    r["o"] = np.asarray(o, np.float32); r["d"] = np.asarray(d, np.float32); r["t_max"] = t_max
    return r


def transforms(host):
    ident = (pbrt_hip.IDENTITY.copy(), pbrt_hip.IDENTITY.copy())
    rst = host.compose(host.compose(host.translate((0.1, -0.05, 0.2)), host.rotate(35.0, (1.0, 2.0, 0.5))), host.scale((1.1, 0.7, 1.3)))
    mirror = host.compose(host.rotate(20.0, (0, 1, 0)), host.scale((-1.0, 1.6, 0.6)))   # non-uniform, swaps handedness
    return [(ident, False), (rst, False), (mirror, False), (mirror, True)]


def probe_curves(host, n_random=64, seed=11):
    """[dict(type, cp (4,3), width (2,), n (2,3) or None, split_depth, seg, t (o2w, w2o), reverse)]: n_random generated curves, then the two quirk cases"""
    rng = np.random.default_rng(seed)
    tfs = transforms(host)
    out = []
    for k in range(n_random):
        ctype = k % 3
        cat = k % 8
        t, rev = tfs[(k // 3) % 4]
        cp = rng.uniform(-1.0, 1.0, (4, 3)).astype(np.float32)
        width = rng.uniform(0.05, 0.4, 2).astype(np.float32)
        split, seg = 0, 0
        if cat == 1: width[1] = width[0]
        elif cat == 2: width[:] = 0.0                                   # eps == 0: refinement depth 10
        elif cat == 3: width[0] = 0.0
        elif cat == 4: cp[1] = cp[0]; cp[2] = cp[0]                     # eval_bezier's zero derivative at u = 0
        elif cat == 5:                                                  # collinear, evenly spaced in exact binary fractions: l0 == 0, depth 0
            a = np.round(rng.uniform(-1, 1, 3) * 4) / 4; b = np.round(rng.uniform(0.25, 1, 3) * 4) / 4 * 0.75
            cp = np.stack([a + b * i for i in range(4)]).astype(np.float32)
        elif cat == 6: split, seg = 2, int(rng.integers(0, 4))
        elif cat == 7: split, seg = 3, int(rng.integers(0, 8))
        n = rng.normal(size=(2, 3)).astype(np.float32) if ctype == cr.RIBBON else None
        out.append(dict(type=ctype, cp=cp, width=width, n=n, split_depth=split, seg=seg, t=t, reverse=rev))
    for q in (WRONG_HALF, OVERWRITE):
        out.append(dict(type=cr.TYPES[q["type"]], cp=np.asarray(q["cp"], np.float32), width=np.asarray(q["width"], np.float32), n=None, split_depth=0, seg=0, t=tfs[0][0], reverse=False))
    return out


def restatement_segment(c):
    cd = cr.curve_data(c["type"], c["cp"], c["width"], c["n"])
    u_min, u_max = cr.create_segments(c["split_depth"])[c["seg"]]
    return cd, cr.segment(cd, u_min, u_max, c["t"][0], c["t"][1], c["reverse"])


def probe_rays(c, n, rng):
    """n world-space rays for one curve: aimed at the curve (long and short t_max), along its chord, from inside its width, and stray ones"""
    cd, seg = restatement_segment(c)
    M = np.asarray(c["t"][0], np.float64).reshape(4, 4)
    cp = cr.segment_cp(cd["cp_obj"], seg["u_min"], seg["u_max"]).astype(np.float64)
    u = rng.uniform(0, 1, n)[:, None]
    on = ((1 - u) ** 3) * cp[0] + 3 * ((1 - u) ** 2) * u * cp[1] + 3 * (1 - u) * u * u * cp[2] + (u ** 3) * cp[3]
    wmax = float(max(c["width"].max(), 0.02))
    tgt = on + rng.uniform(-0.7, 0.7, (n, 3)) * wmax
    o = rng.normal(size=(n, 3)); o = tgt + o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.5, 4.0, (n, 1))
    d = (tgt - o) * rng.uniform(0.3, 2.0, (n, 1))                      # |d| != 1: ray_length matters
    t_max = np.full(n, np.inf)
    kind = rng.integers(0, 20, n)
    short = kind < 4                                                    # a t_max around the target's: culls halves, and the leaf's z test
    t_max[short] = rng.uniform(0.3, 1.3, short.sum())
    inside = (kind >= 4) & (kind < 6)                                   # origins inside the width
    o[inside] = on[inside] + rng.uniform(-0.3, 0.3, (inside.sum(), 3)) * wmax; d[inside] = rng.normal(size=(inside.sum(), 3))
    stray = (kind >= 6) & (kind < 8)
    d[stray] = rng.normal(size=(stray.sum(), 3))
    chord = (kind >= 8) & (kind < 10)                                   # along the chord: dx == 0 where the transform keeps the bits (identity)
    ch32 = (cp[3].astype(np.float32) - cp[0].astype(np.float32)).astype(np.float64)
    d[chord] = ch32 * np.where(rng.integers(0, 2, (chord.sum(), 1)) == 0, 1.0, -1.0)
    o[chord] = on[chord] - d[chord] * rng.uniform(0.0, 2.0, (chord.sum(), 1)) + rng.uniform(-0.3, 0.3, (chord.sum(), 3)) * wmax * (rng.integers(0, 2, (chord.sum(), 1)))
    ow = o @ M[:3, :3].T + M[:3, 3]; dw = d @ M[:3, :3].T
    return mk_rays(ow, dw, t_max.astype(np.float32))


def quirk_rays(q, t_max):
    return mk_rays([q["o"]], [q["d"]], np.float32(t_max))
