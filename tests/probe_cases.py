"""Case generators for the BSDF and sampler probes (bsdf_probe_batch / sampler_value_batch), shared by the CPU tests that measure what the
cases reach on the oracle and the GPU tests that compare the device with the oracle bit for bit.

BSDF cases are per material and in the material's local frame: a deterministic edge set (grazing and denormal cos theta, the poles, wi = -wo, the
mirror direction, wo + eta * wi = 0, directions either side of the 0.9999 switch of the visible-normal sampler and of the critical angle, sample
values at every branch threshold) crossed with a seeded random fill and seven flag sets, plus two frames whose geometric and shading normals disagree.
Everything is float32 from the start, so that both sides receive the same bits."""
import math

import numpy as np

F = np.float32
REFL, TRANS, DIFF, GLOSSY, SPEC, ALL = 1, 2, 4, 8, 16, 31
FLAG_SETS = [ALL, ALL & ~SPEC, ALL & ~TRANS, ALL & ~REFL, SPEC | REFL, SPEC | TRANS, 0]
ONE_MINUS_EPS = np.nextafter(F(1), F(0))
MAX_PROBES = 65536
SWITCH = F(0.9999)   # tr_sample_11's `cos_theta > 0.9999`


def up(x):
    return np.nextafter(F(x), F(np.inf))


def dn(x):
    return np.nextafter(F(x), F(-np.inf))


def roughness_to_alpha(r):
    x = math.log(max(r, 1e-3))
    return 1.62142 + 0.819955 * x + 0.1734 * x * x + 0.0171201 * x ** 3 + 0.000640711 * x ** 4


class Mat:
    """One probe material: make(scene) adds it and returns its id.  eta: the dielectric's index (None: no refraction); alpha: the (x, y) Trowbridge-Reitz
    widths of its microfacet lobes (None: none), exact_alpha when they are the float32 values the lobes hold; lobe kinds as flags for the coverage checks."""

    def __init__(self, name, make, eta=None, alpha=None, exact_alpha=False, matte=False, fresnel_specular=False, fresnel_blend=False, transmission=False):
        self.name, self.make, self.eta, self.alpha, self.exact_alpha = name, make, eta, alpha, exact_alpha
        self.matte, self.fresnel_specular, self.fresnel_blend, self.transmission = matte, fresnel_specular, fresnel_blend, transmission


def _alpha(u, v, remap):
    return (max(1e-3, roughness_to_alpha(u)), max(1e-3, roughness_to_alpha(v))) if remap else (max(1e-3, u), max(1e-3, v))


def _glass(name, ur, vr, eta, remap=True):
    smooth = ur == 0.0 and vr == 0.0
    return Mat(name, lambda s: s.add_material_glass((0.9, 0.8, 0.7), (0.7, 0.8, 0.9), ur, vr, eta, remap), eta=eta, alpha=None if smooth else _alpha(ur, vr, remap),
               exact_alpha=not remap, fresnel_specular=smooth, transmission=True)


def _mix2(s):
    a = s.add_material_plastic((0.3, 0.4, 0.5), (0.2, 0.25, 0.3), 0.15, True)
    b = s.add_material_glass((0.9, 0.8, 0.7), (0.7, 0.8, 0.9), 0.0, 0.0, 1.5, True)
    c = s.add_material_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.05, 0.2, True)
    return s.add_material_mix(s.add_material_mix(a, b, (0.3, 0.5, 0.7)), c, (0.6, 0.4, 0.2))


KD, KS = (0.5, 0.4, 0.3), (0.25, 0.3, 0.35)
MATERIALS = [
    Mat("matte_lambert", lambda s: s.add_material_matte(KD, 0.0), matte=True),
    Mat("matte_oren", lambda s: s.add_material_matte(KD, 25.0), matte=True),
    Mat("matte_black", lambda s: s.add_material_matte((0, 0, 0), 0.0), matte=True),
    Mat("mirror", lambda s: s.add_material_mirror((0.9, 0.8, 0.7))),
    Mat("plastic", lambda s: s.add_material_plastic(KD, KS, 0.1, True), alpha=_alpha(0.1, 0.1, True)),
    Mat("plastic_rough_1", lambda s: s.add_material_plastic(KD, KS, 1.0, True), alpha=_alpha(1.0, 1.0, True)),
    _glass("glass_smooth_eta_1.5", 0.0, 0.0, 1.5),
    _glass("glass_smooth_eta_1.0", 0.0, 0.0, 1.0),
    _glass("glass_smooth_eta_0.75", 0.0, 0.0, 0.75),
    _glass("glass_rough_eta_1.5", 0.1, 0.1, 1.5),
    _glass("glass_rough_eta_1.0", 0.1, 0.2, 1.0),
    _glass("glass_rough_eta_0.75", 0.2, 0.1, 0.75),
    _glass("glass_anisotropic", 0.02, 0.5, 1.5, remap=False),
    _glass("glass_rough_1e-3_raw", 1e-3, 1e-3, 1.5, remap=False),
    Mat("metal", lambda s: s.add_material_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.05, 0.2, True), alpha=_alpha(0.05, 0.2, True)),
    Mat("metal_rough_1_raw", lambda s: s.add_material_metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 1.0, 1.0, False), alpha=(1.0, 1.0), exact_alpha=True),
    # eta = 2: the one index here at which g_refract's `sin2_t >= 1` is met with equality in float32 (4 * 0.25; critical_exact_z finds no such cos theta for 1.5 or 0.75)
    Mat("uber_opaque_eta_2", lambda s: s.add_material_uber(KD, KS, (0.2, 0.2, 0.3), (0.3, 0.2, 0.2), (1, 1, 1), 0.1, 0.2, 2.0, True), eta=2.0, alpha=_alpha(0.1, 0.2, True),
        transmission=True),
    Mat("uber_opacity_0.6", lambda s: s.add_material_uber(KD, KS, (0.2, 0.2, 0.3), (0.3, 0.2, 0.2), (0.6, 0.6, 0.6), 0.1, 0.2, 1.5, True), eta=1.5,
        alpha=_alpha(0.1, 0.2, True), transmission=True),
    Mat("substrate", lambda s: s.add_material_substrate(KD, KS, 0.1, 0.3, True), alpha=_alpha(0.1, 0.3, True), fresnel_blend=True),
    Mat("translucent", lambda s: s.add_material_translucent(KD, KS, (0.5, 0.6, 0.7), (0.4, 0.3, 0.2), 0.1, True), eta=1.5, alpha=_alpha(0.1, 0.1, True), transmission=True),
    Mat("translucent_black_reflect", lambda s: s.add_material_translucent(KD, KS, (0, 0, 0), (0.4, 0.3, 0.2), 0.1, True), eta=1.5, alpha=_alpha(0.1, 0.1, True),
        transmission=True),
    Mat("translucent_black_transmit", lambda s: s.add_material_translucent(KD, KS, (0.5, 0.6, 0.7), (0, 0, 0), 0.1, True), alpha=_alpha(0.1, 0.1, True)),
    Mat("mix_two_levels", _mix2, eta=1.5, alpha=_alpha(0.15, 0.15, True), fresnel_specular=True, transmission=True),
]
MATERIAL_BY_NAME = {m.name: m for m in MATERIALS}

# two frames whose normals disagree (ns, ng, dpdu): a tilted geometric normal under an axis-aligned shading frame with a dpdu that is not unit length,
# and a rotated shading frame whose geometric normal points far from it
FRAMES = [
    np.array([0, 0, 1, 0.6, 0, 0.8, 2, 0, 0], F),
    np.array([1 / 3, 2 / 3, 2 / 3, 0.2, 0.9, math.sqrt(0.15), 2 / 3, -2 / 3, 1 / 3], F),
]

Z_EDGES = [0.0, 1e-40, -1e-40, 1e-7, -1e-7, 1e-4, -1e-4, 1e-3, -1e-3, 0.5, -0.5, 1.0, -1.0]
AZIMUTHS = [0.0, 0.7, 2.5, 4.0]


def unit_dir(z, phi):
    """(sin theta cos phi, sin theta sin phi, z) rounded to float32; z is kept as given (denormals included), the poles are exact."""
    z32 = F(z)
    s = math.sqrt(max(0.0, 1.0 - float(z32) * float(z32)))
    if s == 0.0:
        return np.array([0, 0, z32], F)
    return np.array([s * math.cos(phi), s * math.sin(phi), z32], F)


def stretched_z(alpha, w):
    """ws.z of tr_sample_wh in float32: normalize((ax * x, ay * y, |z|)).z with the vector type's operations (length_squared, sqrt, 1 / length, product)."""
    w = np.asarray(w, F).reshape(-1, 3)
    ax, ay = F(alpha[0]), F(alpha[1])
    x = ax * w[:, 0]; y = ay * w[:, 1]; z = np.abs(w[:, 2])
    ln = np.sqrt(x * x + y * y + z * z, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (F(1) / ln) * z


def edge_wo(mat):
    """The outgoing directions of a material's edge set, (n, 3) float32."""
    out = []
    for z in Z_EDGES:
        for phi in (AZIMUTHS if abs(z) != 1.0 else AZIMUTHS[:1]):
            out.append(unit_dir(z, phi))
    if mat.alpha is not None:   # either side of ws.z = 0.9999: tan(theta) * alpha = sqrt(1 / 0.9999^2 - 1) along each axis
        t = math.sqrt(1.0 / 0.9999 ** 2 - 1.0)
        for axis, phi in ((0, 0.0), (1, math.pi / 2)):
            tc = math.atan(t / mat.alpha[axis])
            for d in (-1e-3, -1e-5, -1e-6, -3e-7, -1e-7, 0.0, 1e-7, 3e-7, 1e-6, 1e-5, 1e-3):
                th = tc * (1.0 + d)
                for sgn in (1.0, -1.0):
                    v = np.array([math.sin(th) * math.cos(phi), math.sin(th) * math.sin(phi), sgn * math.cos(th)], F)
                    if axis == 1:
                        v[0] = F(0)
                    out.append(v)
    if mat.eta is not None and mat.eta != 1.0:   # inside the denser medium at, just under and just over the critical angle
        e = mat.eta if mat.eta > 1.0 else 1.0 / mat.eta
        sgn = -1.0 if mat.eta > 1.0 else 1.0
        zc = math.sqrt(1.0 - 1.0 / (e * e))
        for phi in AZIMUTHS[:2]:
            for d in (-1e-2, -1e-4, -1e-6, -2e-7, -1e-7, 0.0, 1e-7, 2e-7, 1e-6, 1e-4, 1e-2):
                out.append(unit_dir(sgn * zc * (1.0 + d), phi))
        for z in critical_exact_z(mat.eta):   # sin2_t == 1 exactly, and one ulp of cos theta either side
            for zz in (z, up(z), dn(z)):
                out.append(unit_dir(zz, 0.3))
    return np.array(out, F)


def refract_sin2_t(eta, z):
    """g_refract's sin2_t for wo = (., ., z) against the pole it faces, in float32: eta * eta * max(0, 1 - cos_i * cos_i) with eta = eta_i / eta_t of the side wo is on."""
    z = np.asarray(z, F)
    ratio = np.where(z > 0, F(1) / F(eta), F(eta) / F(1)).astype(F)
    c = np.abs(z)
    return (ratio * ratio) * np.maximum(F(0), F(1) - c * c)


def critical_exact_z(eta, limit=4):
    """cos theta values, within a few thousand ulps of the critical angle on the dense side, at which g_refract's `sin2_t >= 1` holds with equality in float32."""
    e = eta if eta > 1.0 else 1.0 / eta
    zc = F((-1.0 if eta > 1.0 else 1.0) * math.sqrt(1.0 - 1.0 / (e * e)))
    bits = zc.view(np.uint32).astype(np.int64) + np.arange(-6000, 6001)
    z = bits.astype(np.uint32).view(F)
    hit = z[refract_sin2_t(eta, z) == F(1)]
    return hit[:: max(1, len(hit) // limit)][:limit]


def random_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def zero_sum_pairs(mat):
    """(wo, wi) with wo + eta * wi == 0 exactly in float32, for the eta MicrofacetTransmission takes on either side: wi has a short mantissa and wo = -(wi * eta)
    is the very product the lobe forms."""
    if mat.eta is None:
        return np.zeros((0, 3), F), np.zeros((0, 3), F)
    wo, wi = [], []
    for w in ([-0.375, -0.25, -0.5], [0.5, -0.25, 0.625], [0.0, 0.0, -0.75], [0.0, 0.0, 0.75]):
        w = np.array(w, F)
        e = F(mat.eta) / F(1) if w[2] < 0 else F(1) / F(mat.eta)   # wo.z > 0: eta_b / eta_a, else eta_a / eta_b
        wo.append(-(w * e)); wi.append(w)
    return np.array(wo, F), np.array(wi, F)


def _ux_values(matching):
    v = [F(0), F(0.5), dn(0.5), up(0.5), ONE_MINUS_EPS, F(0.25), dn(0.25), up(0.25), F(0.75), dn(0.75), up(0.75), F(0.3137), F(0.6871)]
    for k in range(matching + 1):   # floor(u.x * matching) at the exact multiples of 1 / matching
        x = F(k) / F(matching)
        v += [x, dn(x), up(x)]
    return [min(max(x, F(0)), ONE_MINUS_EPS) for x in v]


UY_VALUES = [F(0), F(0.5), dn(0.5), up(0.5), ONE_MINUS_EPS, F(0.123), F(0.77)]


def u_pairs(matching):
    """Sample values for a flag set that matches `matching` lobes, (n, 2) float32."""
    if matching == 0:
        return np.array([[0.5, 0.5]], F)
    ux = _ux_values(matching)
    p = []
    for j, x in enumerate(ux):
        p += [(x, UY_VALUES[j % len(UY_VALUES)]), (x, UY_VALUES[(j + 3) % len(UY_VALUES)])]
    for y in UY_VALUES:
        p += [(F(0.3), y), (F(0.8), y)]
    return np.unique(np.array(p, F), axis=0)


def _batch(op, frame, wo, wi, u, flags):
    wo = np.ascontiguousarray(wo, F).reshape(-1, 3); n = len(wo)
    wi = np.ascontiguousarray(wi, F).reshape(-1, 3) if wi is not None else np.tile(np.array([0, 0, 1], F), (n, 1))
    u = np.ascontiguousarray(u, F).reshape(-1, 2) if u is not None else np.full((n, 2), 0.5, F)
    flags = np.ascontiguousarray(flags, np.uint32).reshape(-1)
    assert len(wi) == n and len(u) == n and len(flags) == n
    return dict(op=op, frame=frame, wo=wo, wi=wi, u=u, flags=flags)


def _cross(a, b):
    """every row of a with every row of b"""
    return np.repeat(a, len(b), axis=0), np.tile(b, (len(a), 1))


def bsdf_cases(mat, orc, mid, seed=0):
    """The probe batches of material `mat` (id `mid` in the oracle scene `orc`, which answers the lobe counts and the Fresnel reflectances the sample values are
    placed around).  A list of dicts {op, frame (None = canonical), wo, wi, u, flags}; at most MAX_PROBES probes in all."""
    rng = np.random.default_rng(1000 + seed)
    flag_arr = np.array(FLAG_SETS, np.uint32)
    z3 = np.zeros((len(FLAG_SETS), 3), F); z3[:, 2] = 1
    counts = orc.bsdf_probe_batch(mid, 2, z3, z3, np.zeros((len(FLAG_SETS), 2), F), flag_arr)
    matching = {f: int(c) for f, c in zip(FLAG_SETS, counts[:, 0])}
    batches = [_batch(2, None, z3, None, None, flag_arr)]
    wo = np.concatenate([edge_wo(mat), random_dirs(rng, 30)])
    # ---- op 0, canonical frame: every wo against -wo, its mirror image, edge and random directions
    wi_common = np.concatenate([random_dirs(rng, 6), [unit_dir(0.0, 1.0), unit_dir(1e-40, 2.0), unit_dir(-1e-7, 3.0), unit_dir(1.0, 0.0), unit_dir(-1.0, 0.0), unit_dir(-0.5, 5.0)]]).astype(F)
    a, b = _cross(wo, wi_common)
    pw = [a, wo, wo]; pi = [b, -wo, wo * np.array([-1, -1, 1], F)]
    zo, zi = zero_sum_pairs(mat)
    pw += [zo, zi]; pi += [zi, zo]
    pw = np.concatenate(pw); pi = np.concatenate(pi)
    a, f = _cross(pw, flag_arr.reshape(-1, 1)); b, _ = _cross(pi, flag_arr.reshape(-1, 1))
    batches.append(_batch(0, None, a, b, None, f))
    # ---- op 1, canonical frame: per flag set, the sample values of its lobe count
    for fl in FLAG_SETS:
        up_ = u_pairs(matching[fl])
        w = wo[::7] if not matching[fl] else (wo if fl in (ALL, ALL & ~SPEC) else wo[::2])
        a, b = _cross(w, up_)
        batches.append(_batch(1, None, a, None, b, np.full(len(a), fl, np.uint32)))
    if mat.fresnel_specular and matching[ALL]:   # u.x either side of the Fresnel reflectance the oracle reports for each wo (FresnelSpecular: pdf of the reflection = fr)
        m = matching[ALL]
        for k in range(m):   # u.x = k / matching picks the k-th matching lobe with a remapped sample of 0: where that is the Fresnel lobe it reflects with pdf = fr / matching
            r = orc.bsdf_probe_batch(mid, 1, wo, wo, np.tile(np.array([F(k) / F(m), 0.4], F), (len(wo), 1)), np.full(len(wo), ALL, np.uint32))
            sel = (r[:, 7] == SPEC | REFL) & (r[:, 3] > 0)
            fr = r[sel, 3] * F(m)
            x = ((F(k) + fr) / F(m)).astype(F)
            xs = np.clip(np.concatenate([x, np.nextafter(x, F(-1)), np.nextafter(x, F(2))]), F(0), ONE_MINUS_EPS)
            w = np.tile(wo[sel], (3, 1))
            batches.append(_batch(1, None, w, None, np.stack([xs, np.full(len(xs), 0.4, F)], axis=1), np.full(len(w), ALL, np.uint32)))
    # ---- the frames whose normals disagree: random world directions, so that pairs fall on the same side of one normal and opposite sides of the other
    for fr in FRAMES:
        wo_w = random_dirs(rng, 40)
        wi_w = np.concatenate([random_dirs(rng, 10), [fr[0:3], -fr[3:6]]]).astype(F)
        a, b = _cross(wo_w, wi_w)
        a2, f = _cross(a, flag_arr.reshape(-1, 1)); b2, _ = _cross(b, flag_arr.reshape(-1, 1))
        batches.append(_batch(0, fr, a2, b2, None, f))
        for fl in FLAG_SETS:
            if matching[fl]:
                a, b = _cross(wo_w, u_pairs(matching[fl])[::4])
                batches.append(_batch(1, fr, a, None, b, np.full(len(a), fl, np.uint32)))
    batches = thin_nans(orc, mid, batches)
    total = sum(len(b["wo"]) for b in batches)
    assert total <= MAX_PROBES, (mat.name, total)
    return batches


NAN_SHARE = 0.009


def thin_nans(orc, mid, batches):
    """Some inputs make the reference itself produce a NaN (a grazing wo whose stretched tangent overflows, normalize(wo + eta * wi) of a zero vector — every transmitted sample
    of a rough dielectric with eta = 1).  They stay in the set, where both sides must put their NaNs in the same slots, but thinned at a fixed stride until they are at most
    NAN_SHARE of the material's probes, so that a set cannot pass on NaNs alone.  Decided on the oracle's output only."""
    outs = run_batches(orc, mid, batches)
    total = sum(len(b["wo"]) for b in batches)
    n_nan = sum(int(np.isnan(o).any(axis=1).sum()) for o in outs)
    if n_nan <= NAN_SHARE * total:
        return batches
    keep_every = int(math.ceil(n_nan / (NAN_SHARE * (total - n_nan) / (1.0 - NAN_SHARE))))
    thinned = []
    seen = 0
    for b, o in zip(batches, outs):
        nan = np.isnan(o).any(axis=1)
        order = seen + np.cumsum(nan) - 1
        keep = ~nan | (order % keep_every == 0)
        seen += int(nan.sum())
        thinned.append(dict(op=b["op"], frame=b["frame"], wo=b["wo"][keep], wi=b["wi"][keep], u=b["u"][keep], flags=b["flags"][keep]))
    return thinned


def run_batches(scene, mid, batches, path=0):
    """The outputs of `batches` on `scene` (oracle or device), one (n, 8) array per batch."""
    return [scene.bsdf_probe_batch(mid, b["op"], b["wo"], b["wi"], b["u"], b["flags"], frame=b["frame"], path=path) for b in batches]


def hexf(a):
    return "(" + ", ".join(float(x).hex() for x in np.asarray(a).reshape(-1)) + ")"


def describe(mat_name, batch, i):
    """One probe's inputs as hex floats, for a failure message."""
    fr = "canonical" if batch["frame"] is None else hexf(batch["frame"])
    return f"material {mat_name} op {batch['op']} flags {int(batch['flags'][i])} frame {fr} wo {hexf(batch['wo'][i])} wi {hexf(batch['wi'][i])} u {hexf(batch['u'][i])}"


def first_difference(got, want):
    """Index of the first row where `got` departs from `want` bit for bit — a NaN in `want` asks only for a NaN in the same slot — or -1."""
    g = got.view(np.uint32); w = want.view(np.uint32)
    nan_w = np.isnan(want)
    bad = np.where(nan_w, ~np.isnan(got), g != w).any(axis=1)
    idx = np.flatnonzero(bad)
    return int(idx[0]) if len(idx) else -1


# ---------------------------------------------------------------- samplers ----------------------------------------------------------------------------------------
HALTON_STRIDE_MAX = 128 * 243
HALTON_SPP_MAX = (2 ** 32 - 1) // HALTON_STRIDE_MAX - 1   # the largest spp with (spp + 1) * stride < 2^32
# (name, sample bounds x0 y0 x1 y1, spp)
HALTON_SETUPS = [
    ("1x1", (0, 0, 1, 1), 4),
    ("16x16", (0, 0, 16, 16), 8),
    ("200x150", (0, 0, 200, 150), 16),
    ("300x260_from_-2", (-2, -2, 298, 258), 5),
    ("200x150_max_spp", (0, 0, 200, 150), HALTON_SPP_MAX),
]
HALTON_DIMS = list(range(0, 71)) + [100, 167, 255, 256, 500, 997, 998, 999]   # 54 = the first dimension read from the global tables with the LDS copy; 999 = the last the table holds


def halton_cases(bounds, spp):
    """(xy, sample, dim) for one Halton set-up: corner pixels, pixels either side of 128 and 243 (the CRT's moduli) and negative ones (a filter's margin), first and last samples."""
    x0, y0, x1, y1 = bounds
    xs = sorted({x0, x1 - 1, 127, 128, 129, 242, 243, 244, -1, -2, -129})
    ys = sorted({y0, y1 - 1, 127, 128, 129, 242, 243, 244, -1, -3, -130})
    px = np.array([(x, y) for y in ys for x in xs], np.int32)
    samples = np.array(sorted({0, 1, spp - 1}), np.uint32)
    dims = np.array(HALTON_DIMS, np.uint32)
    P, S, D = np.meshgrid(np.arange(len(px)), samples, dims, indexing="ij")
    # around the last dimension the LDS copy serves (53: prime 251, the last whose digits fit a byte; 54: prime 257): many indices, so that every digit of the permutations occurs
    px2 = np.array([(x0, y0), (x1 - 1, y1 - 1), (129, 244), (-2, -3)], np.int32)
    P2, S2, D2 = np.meshgrid(np.arange(len(px2)), np.arange(256, dtype=np.uint32), np.arange(48, 60, dtype=np.uint32), indexing="ij")
    return (np.concatenate([px[P.reshape(-1)], px2[P2.reshape(-1)]]), np.concatenate([S.reshape(-1), S2.reshape(-1)]).astype(np.uint32),
            np.concatenate([D.reshape(-1), D2.reshape(-1)]).astype(np.uint32))


SOBOL_RESOLUTIONS = [(1, 1), (100, 60), (512, 512)]
SOBOL_MINIMA = [(0, 0), (-2, -3)]
SOBOL_SAMPLES = [0, 1, 15] + [2 ** k for k in range(1, 32)]   # at 512 x 512 (m = 9) sample 2^31 has index < 2^50: every u32 sample number stays below the 52 columns


def sobol_cases(res, minimum, n_dims):
    x0, y0 = minimum; x1, y1 = x0 + res[0], y0 + res[1]
    px = sorted({(x0, y0), (x1 - 1, y0), (x0, y1 - 1), (x1 - 1, y1 - 1), ((x0 + x1) // 2, (y0 + y1) // 2), (min(x0 + 37, x1 - 1), min(y0 + 21, y1 - 1))})
    px = np.array(px, np.int32)
    P, S, D = np.meshgrid(np.arange(len(px)), np.array(sorted(set(SOBOL_SAMPLES)), np.uint32), np.arange(n_dims, dtype=np.uint32), indexing="ij")
    return (x0, y0, x1, y1), px[P.reshape(-1)], S.reshape(-1).astype(np.uint32), D.reshape(-1).astype(np.uint32)
