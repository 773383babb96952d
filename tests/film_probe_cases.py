"""Case sets of the film probe (pbrt_hip_film_probe / oracle_film_probe): explicit camera samples — radiance and film position per sample — put through FilmTile::add_sample per
tile and Film::merge_film_tile, at the positions, radii, windows and radiance values chosen to break a gather that restates them.  tests/test_film_probe_cases_cpu.py proves
the sets on the CPU (the oracle against `twin`, and that each family a case names is in it); tests/test_film_probe_gpu.py runs them on the device against the oracle, bit for bit.

`twin` is the float64 twin of the oracle's film probe: it makes the reference's float32 decisions (which pixels a sample reaches, which table entry, whether the luminance clamp
applies) and computes each term `l * 1 * weight` in float32 as the reference does, but sums in float64.  A pixel that receives n terms is within gamma(n + 2) * sum|terms| of
it: n - 1 additions across the tile sums and the merge, one product and two additions of the rgb -> xyz row."""
import functools
import zlib

import numpy as np

F = np.float32
INF = float("inf")
REC = 20   # bytes of a sample record (band_plan.h)
LUM = np.array([0.212671, 0.715160, 0.072169], F)
XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], F)


def below(v):
    return np.nextafter(F(v), F(-INF))


def above(v):
    return np.nextafter(F(v), F(INF))


def lum(L):
    L = np.asarray(L, F)
    return LUM[0] * L[..., 0] + LUM[1] * L[..., 1] + LUM[2] * L[..., 2]


def clamped(c, max_lum):
    """film_tile.rs:66-69 once the test has said yes: l * max_lum / y, a spectrum dividing by multiplying with 1 / y (rgb_spectrum.rs:255-263)"""
    return (np.asarray(c, F) * F(max_lum) * (F(1) / lum(c))).astype(F)


# the colour whose luminance is a finite case's max_lum, exactly: the clamp must leave it alone, and clamping it would show (not every colour's bits move under * y * (1 / y))
C_EQ = next(c for c in (np.array([0.8, 1.1, 0.6], F) * F(1 + k * 2.0 ** -20) for k in range(64)) if (clamped(c, lum(c)) != c).all())
MAX_LUM = float(lum(C_EQ))
C_OVER = next(c for c in (C_EQ * F(1 + k * 2.0 ** -22) for k in range(1, 64)) if lum(c) > F(MAX_LUM))   # ... and one a few ulps brighter
C_LUM0 = np.array([LUM[1], -LUM[0], 0.0], F) * F(4)   # mixed signs: .212671 * .715160 - .715160 * .212671 + 0 is exactly 0


class Case:
    def __init__(self, name, crop, radius, tile=16, spp=3, res=None, max_lum=INF, parts=(1,), bands=(None,), missing="some", expect=()):
        self.name, self.crop, self.tile, self.spp, self.max_lum, self.parts, self.bands, self.missing = name, tuple(crop), tile, spp, max_lum, tuple(parts), tuple(bands), missing
        self.radius = (F(radius[0]), F(radius[1]))
        self.res = res if res is not None else (crop[2] + 8, crop[3] + 8)
        self.expect = tuple(expect)
        self.seed = zlib.crc32(name.encode())
        self.table = np.random.default_rng(self.seed ^ 0x5EED).uniform(-0.25, 1.0, 256).astype(F)   # random, not symmetric: a swapped or mirrored index shows

    def __repr__(self):
        return self.name

    def sample_bounds(self):
        c, (rx, ry) = self.crop, self.radius
        return (int(np.floor(F(c[0]) + F(0.5) - rx)), int(np.floor(F(c[1]) + F(0.5) - ry)), int(np.ceil(F(c[2]) - F(0.5) + rx)), int(np.ceil(F(c[3]) - F(0.5) + ry)))

    def setup(self, scene):
        scene.set_film(self.res[0], self.res[1], self.crop, self.radius, self.table, 1.0, self.max_lum)
        scene.set_sampler(0, self.spp, self.sample_bounds())

    def tile_records(self):
        """bytes of one whole tile's sample records"""
        return self.tile * self.tile * self.spp * REC


HAIR = [below(0.5), below(1.5), below(2.5)]
ALWAYS = ("offset0_x", "offset0_y", "rounded_x", "rounded_y", "rounded_corner", "ulp_inside", "shared_position", "pixel_without_sample")
CASES = [
    # radii and placements
    Case("box .5 .5 at the origin", (0, 0, 37, 22), (0.5, 0.5), expect=("idx15_exact", "rounded_reaches_x", "rounded_reaches_y")),
    Case("1.5 1.25 crop not on tiles", (5, 3, 44, 26), (1.5, 1.25), expect=("idx15_exact",)),
    Case("2 2", (0, 0, 33, 21), (2.0, 2.0), expect=("idx15_exact", "negative_sample_bounds")),
    Case(".3 .7: pixels that receive nothing", (3, 2, 40, 24), (0.3, 0.7), spp=2, expect=("weightless_pixel",)),
    Case("1.5 1.5 across 512", (500, 506, 524, 522), (1.5, 1.5), res=(600, 600), spp=4, expect=("tie_reach_x", "tie_reach_y")),
    Case("1.5 1.5 across 1024", (1010, 1016, 1040, 1034), (1.5, 1.5), res=(1100, 1100), spp=4, expect=("tie_reach_x", "tie_reach_y")),
    Case("1.5 1.5 across 4096", (4085, 4090, 4110, 4104), (1.5, 1.5), res=(4200, 4200), spp=4, expect=("tie_reach_x", "tie_reach_y")),
    Case("4 4 tile 2", (2, 1, 25, 15), (4.0, 4.0), tile=2, spp=2, expect=("far_tile",)),
    Case("4 4 tile 3", (0, 0, 22, 14), (4.0, 4.0), tile=3, spp=2, expect=("far_tile", "negative_sample_bounds")),
    Case("17 .5: wider than a tile", (3, 2, 43, 20), (17.0, 0.5), spp=2, expect=("far_tile",)),
    Case("one third", (1, 1, 30, 20), (1.0 / 3.0, 1.0 / 3.0), expect=("weightless_pixel",)),
    Case("1.4998 from 4096", (4090, 4094, 4120, 4110), (1.4998, 1.4998), res=(4200, 4200), expect=("hair_reach",)),
    # the hair radii: a sample ON a pixel coordinate two columns away is added, and tiles are two pixels wider than floor(.5 + r) + floor(r - .5) + 1
    Case("hair under .5", (0, 0, 30, 20), (HAIR[0], HAIR[0]), expect=("hair_reach", "wide_tile")),
    Case("hair under 1.5", (0, 0, 30, 20), (HAIR[1], HAIR[1]), tile=8, expect=("hair_reach", "wide_tile")),
    Case("hair under 2.5", (7, 5, 36, 24), (HAIR[2], HAIR[1]), tile=8, expect=("hair_reach", "wide_tile")),
    # windows
    Case("crop one pixel wide", (9, 2, 10, 25), (1.5, 1.25), expect=()),
    Case("crop one pixel high", (2, 9, 40, 10), (2.0, 2.0), expect=()),
    Case("tile larger than the crop", (3, 3, 20, 12), (1.5, 1.5), tile=64, expect=("single_tile",)),
    Case("tile size 1", (0, 0, 12, 9), (1.5, 1.25), tile=1, spp=2, expect=("far_tile", "negative_sample_bounds")),
    # missing samples
    Case("whole tiles without samples", (0, 0, 40, 24), (2.0, 2.0), tile=8, missing="tiles", expect=("tile_without_sample",)),
    # radiance
    Case("finite clamp", (0, 0, 36, 20), (1.5, 1.25), max_lum=MAX_LUM, expect=("lum_equal_max", "lum_over_max", "huge_clamped", "negative_lum", "denormal", "lum0_mixed", "zero_radiance")),
    Case("no clamp", (0, 0, 36, 20), (1.5, 1.25), max_lum=INF, expect=("huge_unclamped", "negative_lum", "denormal", "lum0_mixed", "zero_radiance")),
    Case("clamp to zero", (0, 0, 36, 20), (1.5, 1.25), max_lum=0.0, expect=("clamped_to_zero", "negative_lum", "lum0_mixed", "zero_radiance")),
    # partition: tile parts merged from separate buffers, and bands of tiles (one tile per band, two per band, one band) whose edges carry rounded-up samples
    Case("parts 2 and 3", (2, 3, 40, 25), (2.0, 2.0), tile=8, parts=(1, 2, 3), expect=("rounded_on_tile_edge_x", "rounded_on_tile_edge_y")),
    Case("64 parts, fewer tiles", (0, 0, 38, 22), (1.5, 1.25), parts=(1, 64), expect=("part_without_tiles",)),
    Case("bands box", (0, 0, 40, 24), (0.5, 0.5), tile=8, bands=(None, "tile", "two"), expect=("rounded_on_tile_edge_x", "rounded_on_tile_edge_y", "rounded_reaches_x", "rounded_reaches_y")),
    Case("bands 1.5 across 1024", (1012, 1014, 1044, 1036), (1.5, 1.5), res=(1100, 1100), tile=8, bands=(None, "tile", "two"), parts=(1, 3),
         expect=("rounded_on_tile_edge_x", "rounded_on_tile_edge_y", "tie_reach_x")),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- geometry, restated from the reference in float32 (film/mod.rs:150-198, sampler_integrator.rs:252-259, 331-336) ---------------------------------------------------
def tile_grid(case):
    sb = case.sample_bounds()
    ntx, nty = max((sb[2] - sb[0] + case.tile - 1) // case.tile, 0), max((sb[3] - sb[1] + case.tile - 1) // case.tile, 0)
    return sb, ntx, nty


def pixel_list(case, part=0, parts=1):
    """(pixels (n, 2) of the part's list: tile by tile in increasing index, row-major inside a tile; tile index of each pixel)"""
    sb, ntx, nty = tile_grid(case)
    px, tl = [], []
    for t in range(part, ntx * nty, parts):
        x0, y0 = sb[0] + (t % ntx) * case.tile, sb[1] + (t // ntx) * case.tile
        x1, y1 = min(x0 + case.tile, sb[2]), min(y0 + case.tile, sb[3])
        ys, xs = np.mgrid[y0:y1, x0:x1]
        px.append(np.stack([xs.ravel(), ys.ravel()], 1)); tl.append(np.full(xs.size, t))
    if not px:
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int64)
    return np.concatenate(px).astype(np.int32), np.concatenate(tl)


def _tile_pixels_axis(s, sb0, sb1, c0, c1, r, tile):
    """FilmTile pixel range [p0, p1) of the tile that holds sample coordinate s, and that tile's number, along one axis"""
    t = (s - sb0) // tile
    a = sb0 + t * tile; b = np.minimum(a + tile, sb1)
    p0 = np.maximum(np.ceil(a.astype(F) - F(0.5) - r).astype(np.int64), c0)
    p1 = np.minimum(np.floor(b.astype(F) - F(0.5) + r).astype(np.int64) + 1, c1)
    return p0, p1, t


# ---- samples ----------------------------------------------------------------------------------------------------------------------------------------------------------
N_FAM = 11   # 0 random, 1 offset 0, 2 ON the next coordinate, 3 / 4 one ulp inside either end, 5-7 and 8-10 the float32 neighbours of frac(.5 + r) and frac(.5 - r)


def _axis_positions(s, fam, r, u):
    base = s.astype(F)
    top = (s + 1).astype(F)
    out = np.minimum(base + u, top)
    out = np.where(fam == 1, base, out)
    out = np.where(fam == 2, top, out)
    out = np.where(fam == 3, np.nextafter(base, F(INF)), out)
    out = np.where(fam == 4, np.nextafter(top, F(-INF)), out)
    for k, sign in ((5, 1.0), (8, -1.0)):
        edge = 0.5 + sign * float(r)
        cand = base + F(edge - np.floor(edge))
        out = np.where(fam == k, np.nextafter(cand, F(-INF)), out)
        out = np.where(fam == k + 1, cand, out)
        out = np.where(fam == k + 2, np.nextafter(cand, F(INF)), out)
    return np.clip(out, base, top).astype(F)


def samples(case):
    """(pixels (n, 2), L (spp, n, 3), p_film (spp, n, 2)) for the whole frame's pixel list (one part); the samples of a pixel do not depend on the partition"""
    px, tl = pixel_list(case)
    n, spp = len(px), case.spp
    rng = np.random.default_rng(case.seed)
    prob = np.array([0.34] + [0.066] * (N_FAM - 1)); prob /= prob.sum()
    fx = rng.choice(N_FAM, (spp, n), p=prob); fy = rng.choice(N_FAM, (spp, n), p=prob)
    corner = rng.random((spp, n)) < 0.08      # both coordinates of the same family: a corner
    fy = np.where(corner, fx, fy)
    pf = np.stack([_axis_positions(np.broadcast_to(px[:, 0], (spp, n)), fx, case.radius[0], rng.random((spp, n)).astype(F)),
                   _axis_positions(np.broadcast_to(px[:, 1], (spp, n)), fy, case.radius[1], rng.random((spp, n)).astype(F))], -1)
    shared = np.arange(n) % 7 == 3             # every sample of these pixels at the first one's position
    pf[:, shared] = pf[0, shared]
    # radiance
    kind = rng.choice(8, (spp, n), p=[0.44] + [0.08] * 7)
    L = rng.uniform(0.0, 2.0, (spp, n, 3)).astype(F)
    L[kind == 1] = 0.0
    if case.max_lum != 0.0:   # (under a clamp to 0 a denormal luminance gives 0 * (1 / y) = 0 * inf, a NaN whose sign bit is the processor's choice: not a case)
        L[kind == 2] = np.array([1e-40, 2e-41, 0.0], F)
    L[kind == 3] = np.array([-0.5, -0.25, -0.1], F)
    L[kind == 4] = C_EQ
    L[kind == 5] = C_OVER
    L[kind == 6] = F(1e30)
    L[kind == 7] = C_LUM0
    # missing samples: whole pixels, single samples, and (missing == "tiles") every third tile
    none = np.zeros((spp, n), bool)
    none[:, rng.random(n) < 0.08] = True
    none |= rng.random((spp, n)) < 0.04
    if case.missing == "tiles":
        none[:, tl % 3 == 1] = True
    pf[none, 0] = np.nan
    return px, L, pf


def for_part(case, part, parts):
    """the frame's samples in the order of one part's pixel list"""
    px, L, pf = samples(case)
    mine, _ = pixel_list(case, part, parts)
    index = {(int(x), int(y)): i for i, (x, y) in enumerate(px)}
    sel = np.array([index[(int(x), int(y))] for x, y in mine], np.int64)
    return mine, np.ascontiguousarray(L[:, sel]), np.ascontiguousarray(pf[:, sel])


# ---- the float64 twin -------------------------------------------------------------------------------------------------------------------------------------------------
def twin(case):
    """(xyz (h, w, 3) float64, weight (h, w) float64, bound_xyz, bound_weight, stats) of the whole frame (one part)"""
    px, L, pf = samples(case)
    spp, n = pf.shape[:2]
    c = case.crop; cw, ch = c[2] - c[0], c[3] - c[1]
    (rx, ry), ts = case.radius, case.tile
    sb, ntx, nty = tile_grid(case)
    sx = np.broadcast_to(px[:, 0].astype(np.int64), (spp, n)); sy = np.broadcast_to(px[:, 1].astype(np.int64), (spp, n))
    valid = ~np.isnan(pf[..., 0])
    pbx0, pbx1, tx = _tile_pixels_axis(sx, sb[0], sb[2], c[0], c[2], rx, ts)
    pby0, pby1, ty = _tile_pixels_axis(sy, sb[1], sb[3], c[1], c[3], ry, ts)
    with np.errstate(all="ignore"):
        pdx = np.where(valid, pf[..., 0], F(0)) - F(0.5); pdy = pf[..., 1] - F(0.5)
        p0x = np.maximum(np.ceil(pdx - rx).astype(np.int64), pbx0); p1x = np.minimum(np.floor(pdx + rx).astype(np.int64) + 1, pbx1)
        p0y = np.maximum(np.ceil(pdy - ry).astype(np.int64), pby0); p1y = np.minimum(np.floor(pdy + ry).astype(np.int64) + 1, pby1)
        ly = lum(L)
        clamp = ly > F(case.max_lum)
        l = np.where(clamp[..., None], L * F(case.max_lum) * (F(1) / ly)[..., None], L).astype(F)    # film_tile.rs:66-69; a spectrum divides by multiplying with 1 / y (rgb_spectrum.rs:255-263)
    inv_rx, inv_ry = F(1) / rx, F(1) / ry
    rgb = np.zeros((ch, cw, 3)); absrgb = np.zeros((ch, cw, 3)); wsum = np.zeros((ch, cw)); absw = np.zeros((ch, cw)); terms = np.zeros((ch, cw), np.int64)
    up_x = pf[..., 0] == (sx + 1).astype(F); up_y = pf[..., 1] == (sy + 1).astype(F)
    st = dict.fromkeys(("rounded_reaches_x", "rounded_reaches_y", "idx15_exact", "far_tile", "tie_reach_x", "tie_reach_y", "hair_reach"), 0)
    kx, ky = int(np.ceil(rx)) + 2, int(np.ceil(ry)) + 2
    for oy in range(-ky, ky + 1):
        y = sy + oy
        oky = valid & (y >= p0y) & (y < p1y)
        if not oky.any():
            continue
        fy = np.abs((y.astype(F) - pdy) * inv_ry * F(16))
        iy = np.minimum(np.floor(fy), F(15)).astype(np.int64)
        for ox in range(-kx, kx + 1):
            x = sx + ox
            ok = oky & (x >= p0x) & (x < p1x)
            if not ok.any():
                continue
            fx = np.abs((x.astype(F) - pdx) * inv_rx * F(16))
            ix = np.minimum(np.floor(fx), F(15)).astype(np.int64)
            fw = case.table[np.where(ok, iy * 16 + ix, 0)]
            with np.errstate(all="ignore"):
                term = (l * F(1) * fw[..., None]).astype(F)                                     # film_tile.rs:100-104
            at = (y[ok] - c[1], x[ok] - c[0])
            np.add.at(rgb, at, term[ok].astype(np.float64)); np.add.at(absrgb, at, np.abs(term[ok]).astype(np.float64))
            np.add.at(wsum, at, fw[ok].astype(np.float64)); np.add.at(absw, at, np.abs(fw[ok]).astype(np.float64)); np.add.at(terms, at, 1)
            # which families this (sample, pixel) pair belongs to.  In exact arithmetic a sample reaches x iff |x + .5 - p| <= r.
            st["rounded_reaches_x"] += int((ok & up_x).sum()); st["rounded_reaches_y"] += int((ok & up_y).sum())
            st["idx15_exact"] += int((ok & ((fx >= F(16)) | (fy >= F(16)))).sum())
            st["far_tile"] += int((ok & ((np.abs((x - sb[0]) // ts - tx) >= 2) | (np.abs((y - sb[1]) // ts - ty) >= 2))).sum())
            ex = np.abs(x + 0.5 - pf[..., 0].astype(np.float64)) > float(rx); ey = np.abs(y + 0.5 - pf[..., 1].astype(np.float64)) > float(ry)
            st["tie_reach_x"] += int((ok & ex & ~up_x).sum()); st["tie_reach_y"] += int((ok & ey & ~up_y).sum())      # reached only because a float32 sum rounded
            st["hair_reach"] += int((ok & (ex | ey)).sum())   # ... samples ON a coordinate included: at a radius a hair under a half-integer those reach a column further
    m = XYZ.astype(np.float64)
    xyz = rgb @ m.T
    u = 2.0 ** -24
    gamma = (terms + 2) * u / (1 - (terms + 2) * u)
    tiny = (terms + 2) * 2.0 ** -149   # a product that underflows is off by an absolute half denormal, which no relative bound covers (the denormal radiance family)
    bound_xyz = gamma[..., None] * (absrgb @ np.abs(m).T) + tiny[..., None]
    bound_w = gamma * absw
    # the families that do not depend on a (sample, pixel) pair
    off0x = valid & (pf[..., 0] == sx.astype(F)); off0y = valid & (pf[..., 1] == sy.astype(F))
    last_col = (sx + 1 - sb[0]) % ts == 0; last_row = (sy + 1 - sb[1]) % ts == 0
    same_pos = valid.all(0) & (pf == pf[0]).all((0, 2)) if spp > 1 else np.zeros(n, bool)
    tile_of = ty * ntx + tx
    tiles_with = set(np.unique(tile_of[valid]).tolist())
    e_x = int(np.floor(0.5 + float(rx)) + np.floor(float(rx) - 0.5) + 1); e_y = int(np.floor(0.5 + float(ry)) + np.floor(float(ry) - 0.5) + 1)
    lyv = ly[valid]; Lv = L[valid]
    st.update({
        "offset0_x": int(off0x.sum()), "offset0_y": int(off0y.sum()), "rounded_x": int((valid & up_x).sum()), "rounded_y": int((valid & up_y).sum()),
        "rounded_corner": int((valid & up_x & up_y).sum()),
        "ulp_inside": int((valid & ((pf[..., 0] == np.nextafter(sx.astype(F), F(INF))) | (pf[..., 0] == np.nextafter((sx + 1).astype(F), F(-INF))))).sum()),
        "shared_position": int(same_pos.sum()), "pixel_without_sample": int((~valid).all(0).sum()),
        "weightless_pixel": int((terms == 0).sum()), "negative_sample_bounds": int(sb[0] < 0 and sb[1] < 0),
        "rounded_on_tile_edge_x": int((valid & up_x & last_col & (sx + 1 < sb[2])).sum()), "rounded_on_tile_edge_y": int((valid & up_y & last_row & (sy + 1 < sb[3])).sum()),
        "tile_without_sample": ntx * nty - len(tiles_with), "single_tile": int(ntx * nty == 1),
        "wide_tile": int(((pbx1 - pbx0).max() > ts + e_x) or ((pby1 - pby0).max() > ts + e_y)),
        "part_without_tiles": int(ntx * nty < 64),
        "lum_equal_max": int((lyv == F(case.max_lum)).sum()), "lum_over_max": int(((Lv == C_OVER).all(-1) & (lyv > F(case.max_lum))).sum()),
        "huge_clamped": int(((lyv > F(1e29)) & (lyv > F(case.max_lum))).sum()), "huge_unclamped": int(((lyv > F(1e29)) & ~(lyv > F(case.max_lum))).sum()),
        "clamped_to_zero": int(((lyv > 0) & (case.max_lum == 0.0)).sum()), "negative_lum": int((lyv < 0).sum()),
        "denormal": int(((np.abs(Lv) > 0) & (np.abs(Lv) < F(1.17549435e-38))).any(-1).sum()),
        "lum0_mixed": int(((lyv == 0) & (Lv[..., 0] > 0) & (Lv[..., 1] < 0)).sum()), "zero_radiance": int((Lv == 0).all(-1).sum()),
    })
    return xyz, wsum, bound_xyz, bound_w, st


@functools.lru_cache(maxsize=None)
def twin_of(name):
    return twin(BY_NAME[name])


# ---- comparing a device tile buffer with the oracle's tiles -----------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def tile_buffer_mismatches(buf, slot, pbs, oracle_tiles):
    """number of floats of a part's device tile buffer (slots of slot_h x slot_w x 4) that differ from the oracle's tiles; outside a tile's pixels a slot holds +0"""
    sw, sh = slot
    slots = bits(buf).reshape(-1, sh, sw, 4)
    assert len(slots) == max(len(oracle_tiles), 1) and len(pbs) == len(oracle_tiles)
    want = np.zeros_like(slots)
    for k, (pb, sums) in enumerate(oracle_tiles):
        assert tuple(pbs[k]) == tuple(pb), (k, pbs[k], pb)
        h, w = sums.shape[:2]
        assert h <= sh and w <= sw, ("a tile's pixels do not fit its slot", pb, slot)
        want[k, :h, :w] = bits(sums)
    return int((slots != want).sum())
