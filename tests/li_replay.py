"""A float64 replay of PathIntegrator::li (integrators/src/path.rs:103-284) on chains of specular events, sample by sample.

On a path of specular vertices nothing is random beyond the sampler's values, so each sample's fate can be predicted exactly: which
lobe BSDF::sample_f takes (core/src/reflection/bsdf.rs:160-292: component floor(u[0] * matching), u[0] remapped, pdf 1 / matching),
what SpecularReflection, SpecularTransmission and FresnelSpecular return, where Russian roulette stops it and what it carries when it
reaches the sky.  The replay is written from path.rs, core/src/reflection and materials/src/{uber,glass,mirror}.rs with numpy alone.
It takes two things from the side under test: the camera rays (generate_camera_rays) and the sampler's value per (pixel, sample,
dimension) (sampler_value_batch, pinned by its own known-answer and Sobol-fixture tests).  It never renders.

Geometry: a stack of parallel interfaces (plane_stack) wider than the view, under a constant sky, seen by an orthographic camera; or
the mirror corridor of closed_form.py, where a sample meets a known number of identical mirrors (`chain`).

`wrong` names one deliberate misreading of li (WRONGS); the tests use the replay's own prediction under each to prove that a case
could tell the misreading from the truth."""
import math

import numpy as np

import closed_form as cf

BAND = 1e-5            # a sample with a decision |u - threshold| < BAND is not predicted: f32 decides it
EXCLUSION_CAP = 0.005  # at most this share of a frame's samples may lie in such a band; measured on the oracle: 0 to 1 sample per frame, 0.098 % at most (1 of 1024)
# The largest relative deviation, per colour component, of the oracle's film from the replay over all CASES is 8.13e-5 (stack_eta1.5_k6, the blue component
# of samples that crossed 12 interfaces; 4.0e-6 at 8 interfaces, 2.4e-5 at 10 with eta 1.1).  It is rounding, but not of the 12-term product: measured
# against the pixel's LARGEST component the deviation is 1.2e-6 or less in every case.  The film stores XYZ, and the way from RGB to XYZ and back mixes
# the channels, so each component carries an absolute f32 error of the size of the largest one.  A survivor of 12 interfaces carries (1.0, 0.144,
# 0.00125): blue lies 800 times below red, and 1e-7 of red is 8e-5 of blue.  Rounding the replay's own float64 values to f32 and taking them through
# the two 3 x 3 matrices in f32 gives 8.1267e-5 in blue (6.0e-7 in red, 1.1e-6 in green), the oracle's figure to every digit: the path's product adds
# nothing visible.  The tolerance is 4 x the measured value, far below the smallest shift a misreading causes (a factor 1 / 0.95).
MEASURED_MAX_REL_DEVIATION = 8.13e-5
TOL = 4.0 * MEASURED_MAX_REL_DEVIATION
assert TOL <= 1e-3
ESCAPED, DEPTH, RR_KILLED, ABSORBED = 0, 1, 2, 3
ONE_MINUS_EPSILON = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
LUM = np.array([0.212671, 0.715160, 0.072169])   # RGBSpectrum::y

WRONGS = ("no_eta_scale", "inverted_eta_scale", "eta_scale_on_reflection", "bsdf_eta_is_the_index", "rr_from_bounces_gt_2", "rr_from_bounces_gt_4",
          "no_floor", "min_component", "luminance", "le_threshold", "rr_dimension_always", "no_rr_weight")


def _f32(v):
    return np.asarray(np.asarray(v, np.float32), np.float64)


# ---- materials: the lobe list and BSDF::eta each material file builds ---------------------------------------------------------

def uber(kr=(0, 0, 0), kt=(0, 0, 0), opacity=1.0, eta=1.5):
    return ("uber", dict(kr=tuple(kr), kt=tuple(kt), opacity=(float(opacity),) * 3, eta=float(eta)))


def glass(kr, kt, eta=1.5):
    return ("glass", dict(kr=tuple(kr), kt=tuple(kt), eta=float(eta)))


def mirror(kr):
    return ("mirror", dict(kr=tuple(kr)))


def add_material(s, spec):
    kind, p = spec
    if kind == "uber":
        return s.add_material_uber(kd=(0, 0, 0), ks=(0, 0, 0), kr=p["kr"], kt=p["kt"], opacity=p["opacity"], eta=p["eta"])
    if kind == "glass":
        return s.add_material_glass(p["kr"], p["kt"], 0.0, 0.0, p["eta"])
    return s.add_material_mirror(p["kr"])


def lobes_of(spec):
    """(lobes in the order the material adds them, BSDF::eta, the index).  Lobes: ("R", k, eta or None for FresnelNoOp), ("T", k, eta_b),
    ("FS", r, t, eta_b); eta_a is 1 in all of them."""
    kind, p = spec
    if kind == "uber":      # uber.rs:128-180 with Kd = Ks = 0
        op = _f32(p["opacity"]); e = float(_f32(p["eta"]))
        t = np.clip(1.0 - op, 0.0, None)
        lobes = []
        bsdf_eta = e
        if t.any():
            bsdf_eta = 1.0                       # BSDF::new(.., Some(1.0)) (:133)
            lobes.append(("T", t, 1.0))          # the pass-through SpecularTransmission::new(t, 1.0, 1.0, mode)
        kr = op * _f32(p["kr"]); kt = op * _f32(p["kt"])
        if kr.any():
            lobes.append(("R", kr, e))
        if kt.any():
            lobes.append(("T", kt, e))
        return lobes, bsdf_eta, e
    if kind == "glass":     # glass.rs:102-129: one FresnelSpecular lobe, BSDF::new(.., None): BSDF::eta = 1
        r = _f32(p["kr"]); t = _f32(p["kt"]); e = float(_f32(p["eta"]))
        return ([("FS", r, t, e)] if (r.any() or t.any()) else []), 1.0, e
    return [("R", _f32(p["kr"]), None)], 1.0, 1.0   # mirror.rs: SpecularReflection with FresnelNoOp


class Interface:
    """One plane of the stack: its material and whether its geometric normal points towards the camera side (up)."""

    def __init__(self, spec, normal_up):
        self.spec = spec
        self.s = 1 if normal_up else -1
        self.lobes, self.bsdf_eta, self.index = lobes_of(spec)


def slabs(specs):
    """Each spec a slab of its own: a face whose normal points up, then one whose normal points down; air between slabs."""
    out = []
    for sp in specs:
        out += [Interface(sp, True), Interface(sp, False)]
    return out


def fr_dielectric(cos_i, eta_i, eta_t):
    """Unpolarised Fresnel reflectance (core/src/reflection/fresnel.rs), cos_i >= 0 on the eta_i side; 1 under total internal reflection."""
    cos_i = np.clip(cos_i, 0.0, 1.0)
    sin_t = eta_i / eta_t * np.sqrt(np.maximum(0.0, 1.0 - cos_i * cos_i))
    tir = sin_t >= 1.0
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    r_parl = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t)
    r_perp = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t)
    return np.where(tir, 1.0, 0.5 * (r_parl * r_parl + r_perp * r_perp))


# ---- the replay ------------------------------------------------------------------------------------------------------------

def replay(ifaces, u, cos0, Le, max_depth, rr_threshold=1.0, chain=None, wrong=None, exact_threshold=False):
    """li for n samples.  ifaces: the stack top to bottom (chain: one interface, met chain[i] times by sample i).  u (n, >= 5 + 3 max_depth):
    the sampler's values by dimension; the camera took 0-4.  cos0 (n,): the camera ray's |cosine| with the stack's axis.
    exact_threshold: max(beta * eta_scale) == rr_threshold is a prediction (both are exact in f32 as in f64: products of 1.0), not a decision to exclude.
    Returns dict(L (n,3), fate (n,), vertices (n,), excluded (n,))."""
    assert wrong is None or wrong in WRONGS, wrong
    u = np.asarray(u, np.float64); n = len(u)
    assert u.shape[1] >= 5 + 3 * max_depth
    Le = np.asarray(Le, np.float64)
    idx = np.zeros(n, np.int64); d = np.ones(n, np.int64); cosv = np.asarray(cos0, np.float64).copy()
    beta = np.ones((n, 3)); eta_scale = np.ones(n); bounces = np.zeros(n, np.int64); dim = np.full(n, 5, np.int64)
    L = np.zeros((n, 3)); fate = np.full(n, -1, np.int64); verts = np.zeros(n, np.int64); excl = np.zeros(n, bool); alive = np.ones(n, bool)
    n_if = np.full(n, len(ifaces), np.int64) if chain is None else np.asarray(chain, np.int64)
    rr_start = {"rr_from_bounces_gt_2": 2, "rr_from_bounces_gt_4": 4}.get(wrong, 3)
    floor = 0.0 if wrong == "no_floor" else 0.05

    while alive.any():
        # the emission rule: every vertex before was specular (or this is the camera ray), so a ray that leaves the stack adds beta * sky
        out = alive & ((idx < 0) | (idx >= n_if))
        L[out] = beta[out] * Le; fate[out] = ESCAPED; alive &= ~out
        cut = alive & (bounces >= max_depth)      # the depth cut-off, after the emission rule; no interface here emits
        fate[cut] = DEPTH; alive &= ~cut
        at = np.zeros(n, np.int64) if chain is not None else idx
        for k in np.unique(at[alive]):
            I = np.flatnonzero(alive & (at == k))
            face = ifaces[k]; m = len(face.lobes)
            verts[I] += 1
            u0 = u[I, dim[I]]; dim[I] += 2        # get_2d; the specular lobes read u[0] only
            if m == 0:                            # BSDF::sample_f returns the default sample: f is black
                fate[I] = ABSORBED; alive[I] = False
                continue
            comp = np.minimum(np.floor(u0 * m), m - 1).astype(np.int64)
            ur = np.minimum(u0 * m - comp, ONE_MINUS_EPSILON)
            for j in range(1, m):
                excl[I] |= np.abs(u0 - j / m) < BAND
            front = d[I] * face.s > 0             # wo . n > 0: the ray arrives on the normal's side, where eta_a = 1 is
            c = cosv[I]
            w = np.zeros((len(I), 3)); flip = np.zeros(len(I), bool); trans = np.zeros(len(I), bool); c_out = c.copy(); dead = np.zeros(len(I), bool)
            for j, lobe in enumerate(face.lobes):
                J = comp == j
                if not J.any():
                    continue
                if lobe[0] == "R":                # SpecularReflection: f = Fr(cos wi) R / |cos wi|, pdf 1
                    _, kr, e = lobe
                    F = 1.0 if e is None else fr_dielectric(c[J], np.where(front[J], 1.0, e), np.where(front[J], e, 1.0))
                    w[J] = np.reshape(F, (-1, 1)) * kr * m
                    flip[J] = True
                    continue
                e = lobe[-1]
                ei = np.where(front[J], 1.0, e); et = np.where(front[J], e, 1.0)
                sin2_t = (ei / et) ** 2 * np.maximum(0.0, 1.0 - c[J] ** 2)
                tir = sin2_t >= 1.0               # refract() fails: pdf 0, the path ends
                ct = np.sqrt(np.maximum(0.0, 1.0 - sin2_t))
                radiance = (ei * ei) / (et * et)  # TransportMode::Radiance
                if lobe[0] == "T":                # SpecularTransmission: f = T (1 - Fr(cos wi)) (eta_i/eta_t)^2 / |cos wi|, pdf 1
                    F = fr_dielectric(ct, et, ei)                 # evaluated for wi, which lies on the eta_t side
                    w[J] = lobe[1] * ((1.0 - F) * radiance * m)[:, None]
                    trans[J] = True; c_out[J] = ct; dead[J] = tir
                else:                             # FresnelSpecular: u[0] < F reflects (f = F R / |cos|, pdf F), else transmits (pdf 1 - F)
                    _, r, t, _ = lobe
                    F = fr_dielectric(c[J], ei, et)
                    refl = ur[J] < F
                    excl[I[J]] |= np.abs(ur[J] - F) < BAND * m
                    w[J] = np.where(refl[:, None], r * float(m), t * (radiance * m)[:, None])
                    flip[J] = refl; trans[J] = ~refl; c_out[J] = np.where(refl, c[J], ct); dead[J] = ~refl & tir
            dead |= ~w.any(axis=1)                # f.is_black() || pdf == 0
            fate[I[dead]] = ABSORBED; alive[I[dead]] = False
            I, w, flip, trans, c_out, front = I[~dead], w[~dead], flip[~dead], trans[~dead], c_out[~dead], front[~dead]
            beta[I] *= w
            # eta_scale (path.rs:192-203): specular transmission only, with the BSDF's eta, by the side wo is on
            e = face.index if wrong == "bsdf_eta_is_the_index" else face.bsdf_eta
            fac = np.where(front, e * e, 1.0 / (e * e))
            if wrong == "inverted_eta_scale":
                fac = 1.0 / fac
            upd = trans | (wrong == "eta_scale_on_reflection")
            if wrong != "no_eta_scale":
                eta_scale[I[upd]] *= fac[upd]
            d[I] = np.where(flip, -d[I], d[I]); cosv[I] = c_out
            idx[I] += 1 if chain is not None else d[I]
            # Russian roulette (path.rs:266-276): its dimension is consumed only when the condition holds
            rr_beta = beta[I] * eta_scale[I][:, None]
            stat = rr_beta.min(axis=1) if wrong == "min_component" else (rr_beta @ LUM if wrong == "luminance" else rr_beta.max(axis=1))
            late = bounces[I] > rr_start
            cond = ((stat <= rr_threshold) if wrong == "le_threshold" else (stat < rr_threshold)) & late
            excl[I] |= late & ~(exact_threshold & (stat == rr_threshold)) & (np.abs(stat - rr_threshold) < BAND * rr_threshold)
            q = np.maximum(floor, 1.0 - stat)
            ur_ = u[I, dim[I]]
            dim[I] += 1 if wrong == "rr_dimension_always" else cond.astype(np.int64)
            kill = cond & (ur_ < q)
            excl[I] |= cond & (np.abs(ur_ - q) < BAND)
            keep = cond & ~kill
            if wrong != "no_rr_weight":
                beta[I[keep]] /= (1.0 - q[keep])[:, None]
            fate[I[kill]] = RR_KILLED; alive[I[kill]] = False
            bounces[I] += 1
    return dict(L=L, fate=fate, vertices=verts, excluded=excl)


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def plane_stack(host, Le, ifaces, tilt_deg=0.0, res=32, spp=1, sampler=cf.HALTON, sobol_tables=None, gap=0.25, W=60.0):
    """The interfaces as parallel quads `gap` apart, the first through the origin, tilted by tilt_deg about x, each wider than the view
    and centred off it (no triangle edge under a pixel), under a constant sky Le; an orthographic camera looks down -z, every sample at
    its pixel's centre, box filter of radius 0.5.  One material per distinct spec."""
    t = math.radians(tilt_deg)
    n = np.array([0.0, -math.sin(t), math.cos(t)])
    a = np.array([1.0, 0.0, 0.0]); b = np.cross(n, a)       # a x b = n
    off = 33.0 * a - 25.0 * b

    def quad(c, e1, e2):
        P = np.array([c - W * e1 - W * e2, c + W * e1 - W * e2, c + W * e1 + W * e2, c - W * e1 + W * e2], np.float32)
        return P, np.array([0, 1, 2, 0, 2, 3], np.uint32)

    def capture(s):
        ids = {}
        for k, f in enumerate(ifaces):
            key = repr(f.spec)
            if key not in ids:
                ids[key] = add_material(s, f.spec)
            c = off - k * gap * n
            s.add_mesh(*(quad(c, a, b) if f.s > 0 else quad(c, b, a)), ids[key])
        s.add_light_infinite(Le)
        cf._setup_view(s, host, res, spp, sampler, cf.ortho_down(host, res), at_center=True, sobol_tables=sobol_tables)
        s.build_accel(0, 4)
    return capture, n


def sobol_tables_for(max_depth):
    """The fixture's 48 Sobol dimensions, repeated until the render's dimension check (5 + 8 (max_depth + 1), which allows for light
    sampling at every vertex) is met.  A specular path reads 5 + 3 max_depth dimensions at most, all inside the fixture's own 48 as
    long as max_depth <= 14: the repeats are never read."""
    assert 5 + 3 * max_depth <= 48
    m32, vdc, vdci = cf.sobol_fixture()
    reps = -(-(5 + 8 * (max_depth + 1)) // (len(m32) // 52))
    return np.tile(m32, reps), vdc, vdci


# ---- a case: the scene, the sampler's values, the replay's verdicts ----------------------------------------------------------

class Case:
    def __init__(self, name, catches, ifaces=None, max_depth=8, rr_threshold=1.0, res=32, spp=1, tilt_deg=0.0, sampler=cf.HALTON,
                 corridor=None, rr_kills=True, exact_threshold=False):
        self.name, self.catches, self.ifaces, self.max_depth, self.rr_threshold = name, tuple(catches), ifaces, max_depth, rr_threshold
        self.res, self.spp, self.tilt_deg, self.sampler, self.corridor, self.rr_kills = res, spp, tilt_deg, sampler, corridor, rr_kills
        self.exact_threshold = exact_threshold
        assert set(self.catches) <= set(WRONGS)

    def __repr__(self):
        return self.name

    def capture(self, host):
        if self.corridor is not None:
            return cf.mirror_corridor(host, cf.LE, self.corridor["kr"], res=self.res, spp=self.spp, angle_deg=self.corridor["angle_deg"])
        tables = sobol_tables_for(self.max_depth) if self.sampler == cf.SOBOL else None
        return plane_stack(host, cf.LE, self.ifaces, self.tilt_deg, self.res, self.spp, self.sampler, tables)[0]

    def scene(self, host, Scene):
        s = Scene()
        self.capture(host)(s)
        return s

    def inputs(self, host, s):
        """From the side under test: the sampler's values u (res^2 spp, dims), and from its camera rays the cosine (stack) or the
        reflection count and the usable mask (corridor).  Samples are ordered pixel-major (y, x, sample)."""
        res, spp = self.res, self.spp
        ys, xs = np.mgrid[0:res, 0:res]
        xy = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
        ndim = 5 + 3 * self.max_depth
        n = res * res * spp
        XY = np.repeat(np.repeat(xy, spp, axis=0), ndim, axis=0)
        S = np.repeat(np.tile(np.arange(spp), res * res), ndim)
        Dm = np.tile(np.arange(ndim), n)
        u = s.sampler_value_batch(XY, S, Dm).astype(np.float64).reshape(n, ndim)
        # one ray per pixel: Halton puts every sample at its pixel's centre; under Sobol the rays are parallel and the stack is uniform
        rays, _ = s.generate_camera_rays([0, 0, res, res], 0)
        if self.corridor is not None:
            N, ok = cf.mirror_bounces(rays)
            return u, np.ones(n), np.repeat(N, spp), np.repeat(ok, spp)
        t = math.radians(self.tilt_deg)
        axis = np.array([0.0, -math.sin(t), math.cos(t)])
        cos0 = np.abs(rays["d"].astype(np.float64) @ axis)
        return u, np.repeat(cos0, spp), None, np.ones(n, bool)

    def predict(self, inputs, wrong=None):
        """The replay's verdict per sample and per pixel (box_film)."""
        u, cos0, chain, ok = inputs
        ifaces = [Interface(mirror(self.corridor["kr"]), True)] if self.corridor is not None else self.ifaces
        r = replay(ifaces, u, cos0, cf.LE, self.max_depth, self.rr_threshold, chain=chain, wrong=wrong, exact_threshold=self.exact_threshold)
        r["excluded"] = r["excluded"] | ~ok
        r["pixel"], r["pixel_excluded"] = box_film(self.res, self.spp, u, r["L"], r["excluded"])
        return r


def box_film(res, spp, u, L, excluded):
    """Film::add_sample with a box filter of radius 0.5 (core/src/film.rs): the sample at p = pixel + (u[0], u[1]) goes, with weight
    1, to the pixels ceil(p - 0.5 - 0.5) .. floor(p - 0.5 + 0.5) inside the film; a pixel is its samples' mean.  At a pixel's centre
    (Halton with sample_at_pixel_center) that is the sample's own pixel; the Sobol sampler has no such switch, and a sample whose
    offset is exactly 0 (sample index 0 has many) also lands in the pixel before.  Positions are formed in f32 as the film forms them."""
    ys, xs = np.mgrid[0:res, 0:res]
    sum_l = np.zeros((res, res, 3)); sum_w = np.zeros((res, res)); bad = np.zeros((res, res), bool)
    lo, hi = [], []
    for pix, k in ((xs, 0), (ys, 1)):
        p = (np.repeat(pix.reshape(-1), spp).astype(np.float32) + u[:, k].astype(np.float32)) - np.float32(0.5)
        lo.append(np.maximum(np.ceil(p - np.float32(0.5)).astype(np.int64), 0))
        hi.append(np.minimum(np.floor(p + np.float32(0.5)).astype(np.int64), res - 1))
    for dy in (0, 1):
        for dx in (0, 1):
            x = lo[0] + dx; y = lo[1] + dy
            on = (x <= hi[0]) & (y <= hi[1])
            np.add.at(sum_l, (y[on], x[on]), L[on]); np.add.at(sum_w, (y[on], x[on]), 1.0)
            np.logical_or.at(bad, (y[on], x[on]), excluded[on])
    assert (sum_w >= spp).all() and ((hi[0] - lo[0]) <= 1).all() and ((hi[1] - lo[1]) <= 1).all()
    return sum_l / sum_w[..., None], bad


def differs(a, b, tol):
    """Per pixel: the two predictions are further apart than a film within `tol` of one of them could hide."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return (np.abs(a - b) > 4.0 * tol * np.maximum(np.abs(a), np.abs(b))).any(axis=-1)


def assert_case_sound(case, inputs, tol, exclusion_cap=EXCLUSION_CAP):
    """With no renderer involved: few samples are excluded, the case is not empty, and each misreading it claims to catch moves the
    replay's own prediction on at least 10 % of its pixels.  Returns the figures."""
    right = case.predict(inputs)
    n = len(right["fate"])
    # the corridor's rim band (mirror_bounces) is geometry, not a sampler decision: it has its own bound in the tests
    share = float((right["excluded"] & inputs[3]).mean())
    assert share <= exclusion_cap, f"{case}: {share:.4%} of samples lie within {BAND} of a decision"
    fates = {f: float((right["fate"] == f).mean()) for f in (ESCAPED, DEPTH, RR_KILLED, ABSORBED)}
    assert (right["fate"] >= 0).all()
    assert fates[ESCAPED] >= 0.10, f"{case}: only {fates[ESCAPED]:.1%} of samples survive"
    if case.rr_kills:
        assert fates[RR_KILLED] >= 0.10, f"{case}: only {fates[RR_KILLED]:.1%} of samples die by Russian roulette"
    else:
        assert fates[RR_KILLED] == 0.0, f"{case}: Russian roulette must not run here"
    long_share = float((right["vertices"] > 4).mean())
    assert long_share >= 0.10, f"{case}: only {long_share:.1%} of paths are longer than 4 vertices"
    power = {}
    for wname in WRONGS:
        wr = case.predict(inputs, wrong=wname)
        both = ~(right["pixel_excluded"] | wr["pixel_excluded"])
        power[wname] = float(differs(right["pixel"], wr["pixel"], tol)[both].mean())
    for wname in case.catches:
        assert power[wname] >= 0.10, f"{case}: '{wname}' moves only {power[wname]:.1%} of the pixels"
    return dict(excluded=share, fates=fates, long=long_share, power=power)


def deviation(rgb, pred):
    """(largest relative deviation of the film from the replay over the predicted non-zero components, pixels predicted zero but not zero)."""
    keep = ~pred["pixel_excluded"]
    want = pred["pixel"][keep]; got = np.asarray(rgb, np.float64)[keep]
    nz = want != 0.0
    rel = float((np.abs(got - want)[nz] / want[nz]).max()) if nz.any() else 0.0
    return rel, int(((got != 0.0) & ~nz).any(axis=-1).sum())


def assert_film_matches(rgb, pred, tol, label=""):
    """Every pixel the replay predicts: zeros exactly, the rest within tol (relative, per component)."""
    rel, wrong_zeros = deviation(rgb, pred)
    keep = ~pred["pixel_excluded"]
    want = pred["pixel"][keep]; got = np.asarray(rgb, np.float64)[keep]
    bad = (np.abs(got - want) > tol * np.abs(want)).any(axis=-1)
    assert wrong_zeros == 0 and not bad.any(), (f"{label}: {int(bad.sum())} of {int(keep.sum())} predicted pixels differ from the replay "
                                               f"({wrong_zeros} of them where it predicts 0); largest relative deviation {rel:.3g}")
    return rel


# ---- the cases, shared by the oracle's tests and the device's ---------------------------------------------------------------------

KT = (0.97, 0.85, 0.6)                       # per channel; max 0.97: RR bites from the fifth vertex on
_RR = ("rr_from_bounces_gt_2", "rr_from_bounces_gt_4", "min_component", "luminance", "rr_dimension_always", "no_rr_weight")
_STACK = ("no_eta_scale", "inverted_eta_scale") + _RR
_WALK = ("eta_scale_on_reflection", "rr_from_bounces_gt_2", "rr_from_bounces_gt_4", "rr_dimension_always")
_ETA1 = ("bsdf_eta_is_the_index",) + _RR    # BSDF::eta is 1: no_eta_scale / inverted_eta_scale predict the same as the truth there
_T15, _T11 = uber(kt=KT, eta=1.5), uber(kt=KT, eta=1.1)
_MULTI = [uber(kt=KT, eta=1.5), uber(kt=(0.9, 0.95, 0.7), eta=1.2), uber(kt=(0.8, 0.9, 0.99), eta=1.33), uber(kt=(0.95, 0.95, 0.9), eta=1.1)]
_WALKER = uber(kr=(0.95, 0.9, 0.8), kt=(0.55, 0.5, 0.45), eta=3.0)   # F = 0.25 at normal incidence: both lobes keep a path alive for a while

CASES = [
    # transmission stacks: uber with Kt only, one SpecularTransmission lobe, max depth = the number of interfaces
    Case("stack_eta1.5_k4", _STACK, slabs([_T15] * 4), max_depth=8, res=32),
    Case("stack_eta1.5_k6", _STACK, slabs([_T15] * 6), max_depth=12, res=48),
    Case("stack_eta1.1_k5", _STACK + ("no_floor",), slabs([_T11] * 5), max_depth=10, res=48),       # 1 - max(rr_beta) < 0.05 here: the floor binds
    Case("stack_four_materials", _STACK, slabs(_MULTI), max_depth=8, res=32),                        # four shade-queue keys live in one round
    Case("stack_four_materials_spp4", _STACK, slabs(_MULTI), max_depth=8, res=32, spp=4),            # the device's tests also chunk and tile this one
    Case("stack_eta1.5_k4_rr0.8", _STACK, slabs([_T15] * 4), max_depth=8, res=32, rr_threshold=0.8),
    Case("stack_eta1.1_k5_rr0.8", ("no_eta_scale", "inverted_eta_scale", "min_component", "luminance", "rr_dimension_always", "no_rr_weight"),
         slabs([_T11] * 5), max_depth=10, res=48, rr_threshold=0.8),
    Case("stack_eta1.5_k4_rr0", (), slabs([_T15] * 4), max_depth=8, res=32, rr_threshold=0.0, rr_kills=False),   # RR off: every sample arrives
    Case("stack_eta1.5_k4_sobol_spp4", _STACK, slabs([_T15] * 4), max_depth=8, res=32, spp=4, sampler=cf.SOBOL),
    Case("stack_eta1.1_k5_spp4", _STACK + ("no_floor",), slabs([_T11] * 5), max_depth=10, res=32, spp=4),
    Case("stack_eta1.5_k4_tilt40", _STACK, slabs([_T15] * 4), max_depth=8, res=32, tilt_deg=40.0),
    # layer walks: Kr and Kt, two specular lobes chosen by u[0]; the sample wanders between the interfaces and leaves up or down
    Case("walk_k3_spp4", _WALK, slabs([_WALKER] * 3), max_depth=14, res=32, spp=4),
    Case("walk_k3_sobol_spp4", _WALK, slabs([_WALKER] * 3), max_depth=14, res=32, spp=4, sampler=cf.SOBOL),
    Case("walk_k3_tilt40_spp4", _WALK, slabs([_WALKER] * 3), max_depth=14, res=32, spp=4, tilt_deg=40.0),
    # glass: BSDF::new(.., None) (glass.rs:109), so eta_scale stays 1 and rr_beta keeps the 1/eta^2 of a path inside the glass
    Case("glass_kr0", _ETA1, slabs([glass((0, 0, 0), KT, 1.5)] * 4), max_depth=8, res=48),          # the reflect choice ends the path: f = 0
    Case("glass_tinted", _ETA1, slabs([glass((0.97, 0.9, 0.75), (0.97, 0.9, 0.75), 1.5)] * 3), max_depth=14, res=48),
    # uber with opacity < 1: a pass-through lobe comes first and BSDF::new(.., Some(1.0)) (uber.rs:133), though the Kt lobe still scales beta by 1/eta^2
    # At opacity 0.5 the pass-through lobe's weight is exactly 1 (2 lobes x 0.5), and a path that has just survived RR has max(rr_beta) = 1 within
    # rounding: under rr_threshold 1 the next `<` is decided by f32 rounding for 24 % of the samples.  So opacity 0.5 runs at rr_threshold 0.8, 0.6 at 1.
    Case("sheet_opacity0.5_rr0.8", _ETA1, slabs([uber(kt=KT, opacity=0.5, eta=1.5)] * 3), max_depth=12, res=48, rr_threshold=0.8),
    Case("sheet_opacity0.6", _ETA1, slabs([uber(kt=KT, opacity=0.6, eta=1.5)] * 3), max_depth=12, res=48),
    # the mirror corridor of closed_form.py at 65 degrees (5 to 9 reflections); after a survival max(beta) is back at 1, so the next q is 0.03: the floor binds
    Case("corridor", ("no_floor",) + _RR, corridor=dict(kr=KT, angle_deg=65.0), max_depth=20, res=32),
    # kr = 1 in one channel: max(beta) == rr_threshold == 1 exactly at every vertex, and `<` never starts RR
    Case("corridor_kr1", ("le_threshold", "min_component", "luminance"), corridor=dict(kr=(1.0, 0.85, 0.6), angle_deg=65.0), max_depth=20, res=32,
         rr_kills=False, exact_threshold=True),
]
