"""Case generators for the texture probes (texture_probe_batch, bump_probe_batch), shared by the CPU test that measures what the cases reach on the oracle and the GPU
test that compares the device with the oracle bit for bit.

One small scene of textures per set (no geometry: the probes need an uploaded scene only), captured into both sides by `ProbeSet.capture`; a set's cases are batches
{tex, ctx (n, 15) = u v du/dx dv/dx du/dy dv/dy p dp/dx dp/dy, tag} — for the bump set {tex, inp (n, 33), tag} — built from deterministic edge lists, float32 from the
start so that both sides receive the same bits.  `prepared(name, host)` runs a set through the oracle first (libm mode 1, as test_textures_gpu.py): the work of every probe
(footprint texels, noise calls) is counted there and held to WORK_TEXELS / WORK_NOISE before anything is handed to a device, probes whose oracle output holds a NaN are
thinned to NAN_SHARE of the set, and the oracle's outputs per variant are kept for both test files."""
import math

import numpy as np

import pbrt_hip
from oracle_binding import OracleScene, set_libm_mode
from probe_cases import F, NAN_SHARE, ONE_MINUS_EPS, hexf
from texture_scenes import make_image

MAX_PROBES = 60000
WORK_TEXELS = 8192   # twice the ~65^2 box of a 16 : 1 ellipse at one level: both levels of a look-up
WORK_NOISE = 64
INF = F(np.inf)
DENORMAL = F(1e-40)
# wherever a coordinate or a derivative is free
EDGE = np.array([0.0, -0.0, ONE_MINUS_EPS, 1e-45, -1e-45, DENORMAL, -DENORMAL, 1e-30, -1e-30, 2 ** 24 + 1, -(2 ** 24 + 1), 2.0 ** 31, -2.0 ** 31, 1e19, -1e19, 3e38, -3e38,
                 np.inf, -np.inf, np.nan], F)
SIZES = [(1, 1), (2, 2), (4, 4), (5, 3), (16, 1), (1, 16), (37, 24)]   # (w, h); 5 x 3 and 37 x 24 are resampled to 8 x 4 and 64 x 32
WRAPS = ["repeat", "black", "clamp"]
ANISO = [1.0, 2.0, 8.0, 16.0]
XFORMS = [(1.0, 1.0, 0.0, 0.0), (1.5, 0.75, 0.1, -0.2)]   # imagemap scale / offset


def pow2_up(v):
    p = 1
    while p < v:
        p *= 2
    return p


def levels_of(w, h):
    return 1 + int(math.log2(max(pow2_up(w), pow2_up(h))))


def step(x, k):
    """x moved by k float32 steps (through zero and the denormals as nextafter goes)"""
    x = F(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, INF if k > 0 else -INF)
    return x


def beside(x, k=1):
    """x with its k float32 neighbours on either side, in increasing order"""
    return np.array([step(x, j) for j in range(-k, k + 1)], F)


def ctx(uv, d=None, p=None, dpdx=None, dpdy=None):
    """(n, 15) contexts; every argument broadcasts over the rows"""
    parts = [np.asarray(uv, F).reshape(-1, 2)]
    n = max([len(parts[0])] + [len(np.asarray(a, F).reshape(-1, k)) for a, k in ((d, 4), (p, 3), (dpdx, 3), (dpdy, 3)) if a is not None])
    out = np.zeros((n, 15), F)
    out[:, 0:2] = parts[0]
    for a, sl in ((d, slice(2, 6)), (p, slice(6, 9)), (dpdx, slice(9, 12)), (dpdy, slice(12, 15))):
        if a is not None:
            out[:, sl] = np.asarray(a, F).reshape(-1, sl.stop - sl.start)
    return out


def cross2(a, b):
    """every (a_i, b_j) as an (n, 2) float32 array"""
    a = np.asarray(a, F).reshape(-1); b = np.asarray(b, F).reshape(-1)
    return np.stack([np.repeat(a, len(b)), np.tile(b, len(a))], axis=1)


def batch(tex, c, tag, **meta):
    """meta: what the CPU test needs to restate the batch (the map's record, the imagemap's scale / offset)"""
    return dict(tex=tex, ctx=np.ascontiguousarray(c, dtype=F).reshape(-1, 15), tag=tag, **meta)


def uv_for_st(st, su, du):
    """u such that the float32 `su * u + du` (UVMapping2D::map) is `st`, where one exists within two steps of the float64 solution; else the nearest"""
    st = np.asarray(st, F)
    if su == 1.0 and du == 0.0:
        return st.copy()
    with np.errstate(all="ignore"):
        u0 = ((st.astype(np.float64) - du) / su).astype(F)
        best = u0.copy(); err = np.abs((F(su) * best + F(du)).astype(np.float64) - st)
        for k in (-2, -1, 1, 2):
            u = u0.copy()
            for _ in range(abs(k)):
                u = np.nextafter(u, INF if k > 0 else -INF)
            e = np.abs((F(su) * u + F(du)).astype(np.float64) - st)
            take = e < err
            best[take] = u[take]; err[take] = e[take]
    return best


class Maps:
    """the mipmaps of a scene, in creation order: (id, w, h, as_float, wrap, trilinear, max_anisotropy)"""

    def __init__(self, scene):
        self.scene = scene; self.rec = []

    def add(self, w, h, as_float, wrap, trilinear=False, aniso=8.0):
        img = make_image(w, h, seed=1000 + 37 * w + h)
        mid = self.scene.add_mipmap(img, as_float=as_float, trilinear=trilinear, wrap=wrap, max_anisotropy=aniso)
        r = dict(id=mid, w=w, h=h, lw=pow2_up(w), lh=pow2_up(h), levels=levels_of(w, h), as_float=as_float, wrap=wrap, trilinear=trilinear, aniso=aniso)
        self.rec.append(r)
        return r


def grid_ints(w):
    """the texel indices around which the coordinates are placed: every integer from -2 to w + 1"""
    return list(range(-2, w + 2))


def grid_coords(w):
    """st for which the float32 `st * w - 0.5` is on, and one float32 either side of, each integer of grid_ints(w) (w a power of two: (k + 0.5) / w is exact)"""
    return np.concatenate([beside(F((k + 0.5) / w)) for k in grid_ints(w)])


# ---------------------------------------------------------------- texel_grid ------------------------------------------------------------------------------------------------
class ProbeSet:
    name = ""; variants = (0,); kind = "texture"

    def capture(self, scene, host):
        raise NotImplementedError

    def cases(self, info):
        raise NotImplementedError


class TexelGrid(ProbeSet):
    """MIPMap::triangle(0, st) under zero derivatives: texel centres, the wrap modes' edges, saturating coordinates; the same inside scale and mix and in a six-deep program"""
    name = "texel_grid"; variants = (0, 1, 2, 3, 4)

    def capture(self, scene, host):
        maps = Maps(scene); tex = []
        k = 0
        for (w, h) in SIZES:
            for as_float in (False, True):
                for wrap in WRAPS:
                    m = maps.add(w, h, as_float, wrap, trilinear=(k % 2 == 1), aniso=ANISO[k % 4]); k += 1
                    for xf in XFORMS:
                        tex.append(dict(id=scene.add_texture_imagemap(m["id"], *xf), map=m, xf=xf, kind="image"))
        by = {(m["w"], m["h"], m["as_float"], m["wrap"]): m for m in maps.rec}
        a = scene.add_texture_imagemap(by[(4, 4, False, "repeat")]["id"]); b = scene.add_texture_imagemap(by[(5, 3, False, "clamp")]["id"], 1.5, 0.75, 0.1, -0.2)
        c = scene.add_texture_imagemap(by[(16, 1, True, "black")]["id"]); d = scene.add_texture_imagemap(by[(2, 2, True, "repeat")]["id"], 3.0, 2.0, 0.0, 0.0)
        k3 = scene.add_texture_constant((0.5, 2.0, 1.5)); k03 = scene.add_texture_constant(0.3); k0 = scene.add_texture_constant(0.0); k1 = scene.add_texture_constant(1.0)
        progs = [("scale(image, constant)", scene.add_texture_scale(a, k3)), ("scale(image, image)", scene.add_texture_scale(a, b)),
                 ("mix(image, image, 0.3)", scene.add_texture_mix(a, b, k03)), ("mix(image, image, float image)", scene.add_texture_mix(a, b, c)),
                 ("mix(image, image, 0)", scene.add_texture_mix(a, b, k0)), ("mix(image, image, 1)", scene.add_texture_mix(a, b, k1)),
                 ("mix(black-wrapped image, constant, float image)", scene.add_texture_mix(c, k3, d))]
        deep = scene.add_texture_scale(a, scene.add_texture_mix(b, c, scene.add_texture_mix(d, a, b)))   # needs six live values: the evaluators' stack limit
        progs.append(("six-deep program", deep))
        for tag, t in progs:
            tex.append(dict(id=t, kind="program", tag=tag))
        return dict(maps=maps.rec, tex=tex)

    def cases(self, info):
        out = []
        for t in info["tex"]:
            if t["kind"] == "program":
                s = grid_coords(16)   # the widest level 0 among the programs' images (16 x 1); the narrower ones see the same st as their own grid and, beside it, coordinates between texels
                pts = np.concatenate([cross2(s, [0.3]), cross2([0.3], s), np.stack([s, s], axis=1), np.stack([s, s[::-1]], axis=1), cross2(EDGE, [0.3]), cross2([0.3], EDGE), np.stack([EDGE, EDGE], axis=1)])
                out.append(batch(t["id"], ctx(pts), t["tag"]))
                continue
            m, (su, sv, du, dv) = t["map"], t["xf"]
            first = su == 1.0
            s, tt = grid_coords(m["lw"]), grid_coords(m["lh"])
            mid_t, mid_s = F(0.3), F(0.3)
            st = [np.stack([s, np.resize(tt, len(s))], axis=1)]   # both on the grid
            if first:
                st += [cross2(s, [mid_t]), cross2([mid_s], tt), cross2([0.0, 1.0, -0.0], [0.0, 1.0, -0.0, 0.3]), cross2(EDGE, [0.3]), cross2([0.3], EDGE), np.stack([EDGE, EDGE[::-1]], axis=1)]
            else:
                st += [cross2([0.0, 1.0, -0.0], [0.0, 1.0]), np.stack([EDGE, EDGE], axis=1)]
            st = np.concatenate(st)
            uv = np.stack([uv_for_st(st[:, 0], su, du), uv_for_st(st[:, 1], sv, dv)], axis=1)
            out.append(batch(t["id"], ctx(uv), f"{m['w']}x{m['h']} {'float' if m['as_float'] else 'rgb'} {m['wrap']} scale/offset {t['xf']}", map=m, xf=t["xf"]))
        return out


# ---------------------------------------------------------------- trilinear_levels -------------------------------------------------------------------------------------------
def uv_maps(scene, trilinear, aniso_of=None):
    """every size as RGB and as float under every wrap mode, one uv-mapped (1, 1, 0, 0) image texture each"""
    maps = Maps(scene); tex = []
    k = 0
    for (w, h) in SIZES:
        for as_float in (False, True):
            for wrap in WRAPS:
                m = maps.add(w, h, as_float, wrap, trilinear=trilinear, aniso=(aniso_of(k) if aniso_of else 8.0)); k += 1
                tex.append(dict(id=scene.add_texture_imagemap(m["id"]), map=m))
    return maps, tex


def map_tag(m):
    return f"{m['w']}x{m['h']} {'float' if m['as_float'] else 'rgb'} {m['wrap']}" + ("" if m["trilinear"] else f" aniso {m['aniso']}")


class TrilinearLevels(ProbeSet):
    """MIPMap::lookup's trilinear branch: `levels - 1 + log2(width)` on and beside every level boundary, the width in each derivative slot with either sign"""
    name = "trilinear_levels"; variants = (0, 2)

    def capture(self, scene, host):
        maps, tex = uv_maps(scene, True)
        return dict(maps=maps.rec, tex=tex)

    def cases(self, info):
        out = []
        sts = np.array([[0.37, 0.61], [-0.26, 1.07]], F)
        for t in info["tex"]:
            m = t["map"]; L = m["levels"]
            widths = [beside(F(2.0 ** (lv - (L - 1))), 3) for lv in range(L)]                       # level = lv exactly at the middle one (log2 of a power of two is exact)
            widths += [beside(F(1e-8), 1), np.array([0.0, 1.0, 1.5, 2.0, 1e19, np.inf, np.nan, 1e-45, DENORMAL], F)]
            widths = np.concatenate(widths)
            rows = []
            for slot in range(4):
                for sign in (1.0, -1.0):
                    d = np.zeros((len(widths), 4), F)
                    with np.errstate(all="ignore"):
                        d[:, (slot + 1) % 4] = F(0.5) * widths; d[:, (slot + 2) % 4] = F(-0.25) * widths   # the other three stay below the largest
                        d[:, slot] = F(sign) * widths
                    rows.append(d)
            d = np.concatenate(rows)
            for st in sts:
                out.append(batch(t["id"], ctx(np.tile(st, (len(d), 1)), d), map_tag(m), map=m))
        return out


# ---------------------------------------------------------------- ewa_ellipse ------------------------------------------------------------------------------------------------
def pair(kind, major, minor):
    """(dst0, dst1) of an ellipse with the given axis lengths: 0 major along s, 1 major along t, 2 diagonal, 3 rotated by 30 degrees; float32, (.., 4) = du/dx dv/dx du/dy dv/dy"""
    major = np.asarray(major, F); minor = np.asarray(minor, F)
    z = np.zeros_like(major)
    with np.errstate(all="ignore"):
        if kind == 0:
            return np.stack([major, z, z, minor], axis=-1)
        if kind == 1:
            return np.stack([z, minor, major, z], axis=-1)   # the major axis arrives in dst1: the swap
        c, s = (F(math.sqrt(0.5)), F(math.sqrt(0.5))) if kind == 2 else (F(math.cos(math.radians(30))), F(math.sin(math.radians(30))))
        return np.stack([major * c, major * s, -minor * s, minor * c], axis=-1).astype(F)


class EwaEllipse(ProbeSet):
    """MIPMap::lookup's EWA branch and MIPMap::ewa: the swap, the anisotropy clamp, lod against the pyramid, footprints across the wrap, the device's 64-bit loop"""
    name = "ewa_ellipse"; variants = (0, 2)

    def capture(self, scene, host):
        maps, tex = uv_maps(scene, False, aniso_of=lambda k: ANISO[k % 4])
        for a in ANISO:
            for (w, h) in ((4, 4), (16, 1)):
                m = maps.add(w, h, False, "repeat", aniso=a)
                tex.append(dict(id=scene.add_texture_imagemap(m["id"]), map=m))
        return dict(maps=maps.rec, tex=tex)

    def cases(self, info):
        out = []
        st3 = np.array([[0.37, 0.61], [-0.26, 1.07], [0.02, 0.98]], F)
        near = np.array([[0.0, 0.0], [1.0, 1.0], [0.01, 0.5], [-0.01, 0.5], [0.99, 0.5], [1.01, 0.5], [0.5, 0.01], [0.5, -0.01], [0.5, 0.99], [0.5, 1.01], [-0.0, 1.0], [1.0, -0.0]], F)
        for t in info["tex"]:
            m = t["map"]; L = m["levels"]; A = F(m["aniso"]); w = m["lw"]
            rows = []

            def add(st, d):
                d = np.asarray(d, F).reshape(-1, 4); st = np.asarray(st, F).reshape(-1, 2)
                rows.append(ctx(np.repeat(st, len(d), axis=0), np.tile(d, (len(st), 1))))
            # lod = levels - 1 + log2(minor) on and beside every integer, below 0, at levels - 1 and above it; ratio 1.5: not clamped (1.5 > 1 = the smallest max_anisotropy: clamped there)
            minors = np.concatenate([beside(F(2.0 ** (lv - (L - 1)))) for lv in range(-2, L + 2)])
            add(st3, pair(0, F(1.5) * minors, minors))
            for kind in (1, 2, 3):
                add(st3[:1], pair(kind, F(1.5) * minors, minors))
            # the anisotropy clamp `minor * max_anisotropy < major`: the ratio on and beside max_anisotropy; equal lengths (the swap's tie); far beyond and inside
            mn = F(1.5 * 2.0 ** -(L - 1))
            majors = np.concatenate([beside(mn * A), beside(mn), np.array([mn * A * F(2), mn * A * F(0.5), mn * A * F(100)], F)])
            for kind in range(4):
                add(st3, pair(kind, majors, np.full(len(majors), mn, F)))
            # minor 0 with major > 0, both 0, a denormal minor
            for kind in range(4):
                add(st3, pair(kind, [0.01, 0.3, 0.0, 0.01, 0.2, 1e-45], [0.0, 0.0, 0.0, DENORMAL, 1e-45, 1e-45]))
            # st within a footprint of 0 and of 1
            for kind in (0, 2):
                add(near, pair(kind, [mn * F(3), F(0.3)], [mn, F(0.1)]))
            # texel coordinates from 2^30 on: the device's 64-bit counters; just below: its 32-bit ones
            big = np.array([2.0 ** 30 / w, -(2.0 ** 30) / w, (2.0 ** 30 - 64) / w, 3 * 2.0 ** 30 / w, 2.0 ** 40, -(2.0 ** 33), 2.0 ** 24 + 1, 1e19], F)
            add(np.concatenate([cross2(big, [0.3]), cross2([0.3], big), np.stack([big, big], axis=1)]), pair(0, [mn * F(3), F(0.05), F(0.0)], [mn, F(0.05), F(0.0)]))
            # the general edge values in every derivative slot, and in st under a small ellipse
            for slot in range(4):
                d = np.tile(pair(0, [mn * F(2)], [mn])[0], (len(EDGE), 1)); d[:, slot] = EDGE
                add(st3[:1], d)
            add(np.concatenate([cross2(EDGE, [0.3]), cross2([0.3], EDGE)]), pair(0, [mn * F(2)], [mn]))
            out.append(batch(t["id"], np.concatenate(rows), map_tag(m), map=m))
        return out


class EwaSaturated(ProbeSet):
    """texel coordinates at +-2^62, +-2^63, one float32 either side of each, and +-3e38 (scripts/ewa_loop_check.cpp's): the EWA loops' bounds and triangle's neighbour index saturate"""
    name = "ewa_saturated"; variants = (0, 1, 2, 3)

    def capture(self, scene, host):
        maps = Maps(scene); tex = []
        for (w, h) in ((4, 4), (2, 16)):
            for wrap in WRAPS:
                for tri in (False, True):
                    m = maps.add(w, h, False, wrap, trilinear=tri, aniso=8.0)
                    tex.append(dict(id=scene.add_texture_imagemap(m["id"]), map=m))
        return dict(maps=maps.rec, tex=tex)

    def cases(self, info):
        out = []
        coord = np.concatenate([np.concatenate([beside(F(sg * b)) for sg in (1, -1)]) for b in (2.0 ** 63, 2.0 ** 62)] + [np.array([3e38, -3e38], F)])
        for t in info["tex"]:
            m = t["map"]; L = m["levels"]
            rows = [ctx([[2.0 ** 61, 0.3]], [[0.1, 0.0, 0.0, 0.1]])]
            for lv in range(L):   # the coordinate lands on the saturating value at level lv too (trilinear: triangle(lv) and triangle(lv + 1); EWA: ewa(lv), ewa(lv + 1))
                lw, lh = max(m["lw"] >> lv, 1), max(m["lh"] >> lv, 1)
                wd = F(2.0 ** (lv - (L - 1)) * 1.25)
                d = np.array([[0.1, 0.0, 0.0, 0.1], [0.0, 0.0, 0.0, 0.0], [0.4, 0.1, -0.05, 0.3], [wd, 0.0, 0.0, wd]], F)
                with np.errstate(all="ignore"):
                    st = np.concatenate([cross2(coord / F(lw), [0.3]), cross2([0.3], coord / F(lh)), np.stack([coord / F(lw), coord / F(lh)], axis=1)])
                rows.append(ctx(np.repeat(st, len(d), axis=0), np.tile(d, (len(st), 1))))
            out.append(batch(t["id"], np.concatenate(rows), map_tag(m), map=m))
        return out


# ---------------------------------------------------------------- procedural textures ----------------------------------------------------------------------------------------
PERM = np.array([
    151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240, 21, 10, 23, 190, 6, 148, 247, 120, 234, 75, 0, 26,
    197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88, 237, 149, 56, 87, 174, 20, 125, 136, 171, 168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146,
    158, 231, 83, 111, 229, 122, 60, 211, 133, 230, 220, 105, 92, 41, 55, 46, 245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1, 216, 80, 73, 209, 76, 132, 187, 208, 89,
    18, 169, 200, 196, 135, 130, 116, 188, 159, 86, 164, 100, 109, 198, 173, 186, 3, 64, 52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118, 126, 255, 82, 85, 212, 207,
    206, 59, 227, 47, 16, 58, 17, 182, 189, 28, 42, 223, 183, 170, 213, 119, 248, 152, 2, 44, 154, 163, 70, 221, 153, 101, 155, 167, 43, 172, 9, 129, 22, 39, 253, 19, 98,
    108, 110, 79, 113, 224, 232, 178, 185, 112, 104, 218, 246, 97, 228, 251, 34, 242, 193, 238, 210, 144, 12, 191, 179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107,
    49, 192, 214, 31, 181, 199, 106, 157, 184, 84, 204, 176, 115, 121, 50, 45, 127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243, 141, 128, 195, 78, 66,
    215, 61, 156, 180], np.int64)   # Ken Perlin's published permutation
PERM2 = np.concatenate([PERM, PERM])


def noise64(x, y, z):
    """Perlin noise (core/src/texture/common.rs:9-117) in float64 on finite coordinates of moderate size"""
    x, y, z = (np.asarray(a, np.float64) for a in np.broadcast_arrays(x, y, z))
    ix, iy, iz = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64), np.floor(z).astype(np.int64)
    dx, dy, dz = x - ix, y - iy, z - iz
    ix &= 255; iy &= 255; iz &= 255

    def grad(gx, gy, gz, ddx, ddy, ddz):
        h = PERM2[PERM2[PERM2[gx] + gy] + gz] & 15
        u = np.where((h < 8) | (h == 12) | (h == 13), ddx, ddy)
        v = np.where((h < 4) | (h == 12) | (h == 13), ddy, ddz)
        return np.where(h & 1, -u, u) + np.where(h & 2, -v, v)

    def wt(t):
        return 6 * t ** 5 - 15 * t ** 4 + 10 * t ** 3

    def lerp(t, a, b):
        return (1 - t) * a + t * b
    w = [[[grad(ix + i, iy + j, iz + k, dx - i, dy - j, dz - k) for k in (0, 1)] for j in (0, 1)] for i in (0, 1)]
    wx, wy, wz = wt(dx), wt(dy), wt(dz)
    x00, x10, x01, x11 = lerp(wx, w[0][0][0], w[1][0][0]), lerp(wx, w[0][1][0], w[1][1][0]), lerp(wx, w[0][0][1], w[1][0][1]), lerp(wx, w[0][1][1], w[1][1][1])
    return lerp(wz, lerp(wy, x00, x10), lerp(wy, x01, x11))


def dot_centres(cells):
    """per (s_cell, t_cell): (has a dot, centre s, centre t) of DotsTexture (textures/src/dots.rs:48-69) in float64"""
    sc, tc = np.asarray(cells, np.float64).T
    has = noise64(sc + 0.5, tc + 0.5, 0.5) > 0
    return has, sc + 0.15 * noise64(sc + 1.5, tc + 2.8, 0.5), tc + 0.15 * noise64(sc + 4.5, tc + 9.8, 0.5)


CA, CB = (0.9, 0.1, 0.2), (0.1, 0.2, 0.8)


class Procedural2D(ProbeSet):
    """checkerboard (closed form and none), dots, uv and bilerp under the uv mapping"""
    name = "procedural_2d"; variants = (0, 1)

    def capture(self, scene, host):
        a, b = scene.add_texture_constant(CA), scene.add_texture_constant(CB)
        return dict(tex=dict(checker=scene.add_texture_checkerboard(a, b), checker_none=scene.add_texture_checkerboard(a, b, aa="none"),
                             checker_scaled=scene.add_texture_checkerboard(a, b, 2.0, 3.0, 0.25, -0.5), dots=scene.add_texture_dots(a, b), uv=scene.add_texture_uv(),
                             uv_scaled=scene.add_texture_uv(1.5, 0.75, 0.1, -0.2), bilerp=scene.add_texture_bilerp((0.1, 0.2, 0.3), (0.9, 0.1, 0.5), (0.2, 0.8, 0.1), (0.7, 0.7, 0.9))))

    def cases(self, info):
        T = info["tex"]; out = []
        ints = np.concatenate([beside(F(k)) for k in (-3, -2, -1, 0, 1, 2, 3)] + [np.array([-0.0], F)])
        widths = np.concatenate([beside(F(1.0)), np.array([0.0, 0.01, 0.25, 0.5, 0.75, 1.5, 2.0, 1e-45, 1e19, np.inf, np.nan], F)])
        # st on and beside integers x ds / dt on and beside 1 (the `> 1` branch), 0 and between
        st = np.concatenate([cross2(ints, [0.4]), cross2([0.4], ints), np.stack([ints, ints[::-1]], axis=1)])
        zw, w3 = np.zeros_like(widths), np.full_like(widths, 0.3)
        d = np.concatenate([np.stack([widths, zw, zw, w3], axis=1), np.stack([zw, w3, zw, -widths], axis=1), np.stack([zw, widths, zw, zw], axis=1), np.stack([-widths, widths, widths, -widths], axis=1)])
        c1 = ctx(np.repeat(st, len(d), axis=0), np.tile(d, (len(st), 1)))
        # s +- ds on a cell boundary: ds = the distance to the next integer, on and beside
        s = np.array([0.25, 0.75, -0.25, 1.5, -2.125, 3.625], F)
        rows = []
        for sv in s:
            for edge in (np.floor(sv), np.floor(sv) + 1):
                for w in beside(F(abs(float(edge) - float(sv)))):
                    rows += [[sv, 0.4, w, 0, 0, 0], [0.4, sv, 0, w, 0, 0], [sv, sv, w, w, 0, 0], [sv, 0.4, 0, 0.1, 0, 0]]   # the last: ds 0 with dt > 0
        c2 = np.zeros((len(rows), 15), F); c2[:, 0:6] = np.array(rows, F)
        # cell sums at +-2^31: floor(s) + floor(t) as wrapping i32
        bigs = np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, -2.0 ** 31 - 256, 3e9, -3e9, 2.0 ** 30, -2.0 ** 30, 1e19, -1e19, 3e38, 2 ** 24 + 1], F)
        c3 = ctx(np.concatenate([cross2(bigs, [0.0, 1.0, -1.0, 0.5]), cross2([0.0, 1.0, -1.0], bigs), cross2(bigs, bigs)]), [[0.01, 0, 0, 0.01]])
        c4 = ctx(np.concatenate([cross2(EDGE, [0.4]), cross2([0.4], EDGE), np.stack([EDGE, EDGE], axis=1)]), [[0.2, 0.0, 0.0, 0.3]])
        chk = np.concatenate([c1, c2, c3, c4])
        for k in ("checker", "checker_none", "checker_scaled"):
            out.append(batch(T[k], chk, k))
        # dots: st + 0.5 on and beside integers; points on and beside the rim of every dot of the cells around the origin
        half = np.concatenate([beside(F(k + 0.5)) for k in (-3, -2, -1, 0, 1, 2)])
        pts = [cross2(half, [0.1, 0.5]), cross2([0.1, -0.5], half), np.stack([half, half], axis=1)]
        cells = np.array([[i, j] for i in range(-4, 5) for j in range(-4, 5)], np.float64)
        has, cs, ct = dot_centres(cells)
        ang = np.linspace(0.0, 2 * math.pi, 24, endpoint=False)
        for (i, j), h, x0, y0 in zip(cells, has, cs, ct):
            if not h:
                pts.append(np.array([[i, j], [i + 0.3, j - 0.3]], F))
                continue
            rim = np.stack([x0 + 0.35 * np.cos(ang), y0 + 0.35 * np.sin(ang)], axis=1).astype(F)
            pts.append(rim)
            for k in (-2, -1, 1, 2):   # step the coordinate that moves across the rim fastest
                q = rim.copy()
                ax = (np.abs(np.sin(ang)) > np.abs(np.cos(ang))).astype(int)
                for r in range(len(q)):
                    q[r, ax[r]] = step(q[r, ax[r]], k)
                pts.append(q)
            pts.append(np.array([[x0, y0]], F))
        pts += [cross2(EDGE, [0.4]), cross2([0.4], EDGE), np.stack([EDGE, EDGE], axis=1), cross2([2.0 ** 24, -2.0 ** 24, 2.0 ** 31, 254.5, 255.5, 256.5], [0.5, 2.0 ** 31])]
        # odd integers from 2^23 on: `st + 0.5` is a tie that rounds to the even neighbour, so floor(st + 0.5) is the NEXT cell, one away from the cell the point sits in the middle of
        odd = (2.0 ** 23 + 1 + 2 * np.arange(24)).astype(F)
        pts += [cross2(odd, [0.0, 1.0, 2.0, 3.0]), cross2([0.0, 1.0, 2.0, 3.0], -odd)]
        out.append(batch(T["dots"], ctx(np.concatenate(pts)), "dots"))
        # uv: negative denormals (st - floor(st) == 1.0 exactly), integers, the edge values
        neg = np.array([-1e-45, -DENORMAL, -1e-38, -1e-30, -1e-10, -5.9e-8, -6e-8, -1.0, -0.0, 0.0, 1.0, ONE_MINUS_EPS, 2 ** 24 + 1, -(2 ** 24 + 1)], F)
        uvp = np.concatenate([cross2(neg, [0.25]), cross2([0.25], neg), np.stack([neg, neg], axis=1), cross2(EDGE, [0.4]), cross2([0.4], EDGE), cross2(ints, ints[::3])])
        out.append(batch(T["uv"], ctx(uvp), "uv")); out.append(batch(T["uv_scaled"], ctx(uvp), "uv scaled"))
        # bilerp: the corners, outside [0, 1], the edge values
        corners = np.array([0.0, 1.0, -0.0, ONE_MINUS_EPS, 0.5, -1.0, 2.0, 1e-45, -1e-45, 100.0, -1e19], F)
        out.append(batch(T["bilerp"], ctx(np.concatenate([cross2(corners, corners), cross2(EDGE, [0.4]), cross2([0.4], EDGE), np.stack([EDGE, EDGE], axis=1)])), "bilerp"))
        return out


ROT_T = dict(theta=35.0, axis=(0.3, 1.0, -0.5), t=(0.25, -0.5, 0.75))


def rotated(host):
    """a rotated and translated world_to_texture and its inverse (texture space's origin is world point `t` moved back)"""
    return host.compose(host.rotate(ROT_T["theta"], ROT_T["axis"]), host.translate(ROT_T["t"]))


class Mappings(ProbeSet):
    """SphericalMapping2D, CylindricalMapping2D and PlanarMapping2D under a uv texture (st itself), a checkerboard (the differentials) and an image map"""
    name = "mappings"; variants = (0, 1)

    def capture(self, scene, host):
        a, b = scene.add_texture_constant(CA), scene.add_texture_constant(CB)
        mip = scene.add_mipmap(make_image(8, 8, seed=5), wrap="repeat", max_anisotropy=8.0)
        tex = []
        rot = rotated(host)
        for kind in ("spherical", "cylindrical"):
            for xname, m in (("identity", pbrt_hip.IDENTITY), ("rotated", rot[0])):
                for tname, make in (("uv", lambda: scene.add_texture_uv()), ("checker", lambda: scene.add_texture_checkerboard(a, b, 4.0, 4.0, 0.0, 0.0)), ("image", lambda: scene.add_texture_imagemap(mip))):
                    t = make(); scene.set_texture_mapping(t, kind, m)
                    tex.append(dict(id=t, kind=kind, xform=xname, tex=tname, w2t=np.asarray(m, np.float64).reshape(4, 4)))
        planes = [("unit", [1, 0, 0, 0, 1, 0, 0.0, 0.0]), ("zero", [0, 0, 0, 0, 0, 0, 0.25, 0.5]), ("huge", [1e19, -3e38, 1e30, 2e19, 1e19, -1e38, 0.0, 0.0]), ("skew", [0.5, 0.25, -1.0, 0.0, 2.0, 0.125, -0.5, 0.75])]
        for pname, prm in planes:
            for tname, make in (("uv", lambda: scene.add_texture_uv()), ("checker", lambda: scene.add_texture_checkerboard(a, b))):
                t = make(); scene.set_texture_mapping(t, "planar", prm)
                tex.append(dict(id=t, kind="planar", xform=pname, tex=tname, prm=prm))
        return dict(tex=tex, rot=rot)

    def cases(self, info):
        out = []
        host = pbrt_hip.Host()
        rot = info["rot"]
        tiny = np.array([0.0, -0.0, 1e-45, -1e-45], F)
        for t in info["tex"]:
            if t["kind"] == "planar":
                p = np.concatenate([np.array([[0, 0, 0], [1, 2, 3], [-0.5, 0.25, 1e-45], [1e19, -1e19, 1.0], [3e38, 3e38, 3e38]], F), np.stack([EDGE, EDGE[::-1], np.resize(EDGE[3:], len(EDGE))], axis=1)])
                dp = np.array([[0, 0, 0], [0.01, 0.02, -0.01], [1e19, 0, 0], [1e-45, -1e-45, 0]], F)
                c = ctx(np.zeros((1, 2), F), None, np.repeat(p, len(dp), axis=0), np.tile(dp, (len(p), 1)), np.tile(dp[::-1], (len(p), 1)))
                out.append(batch(t["id"], c, f"planar {t['xform']} {t['tex']}", rec=t))
                continue
            # texture-space points: the poles, the origin, the seam with y = +-0, +-1e-45 on both sides of x, generic points; carried to world space for the rotated mapping
            q = [[0, 0, 1], [0, 0, -1], [0, 0, 2.5], [0, 0, 0], [0, 0, 1e-45], [1e-45, 0, 0], [1e-20, 1e-20, 1e-20]]
            for y in tiny:
                q += [[1, y, 0], [-1, y, 0], [0.5, y, 0.5], [-0.5, y, -0.25], [1e-45, y, 0], [y, y, 1]]
            q += [[0.3, 0.4, 0.5], [-0.7, 0.2, 0.1], [0.2, -0.9, -0.3], [1e19, 1e19, 1e19], [3e38, 0, 0], [np.inf, 0, 0], [np.nan, 0, 0], [0, 1, 0], [0, -1, 0]]
            q = np.array(q, F)
            dq = np.array([[0, 0, 0], [0.01, 0.02, -0.01], [0, -0.05, 0], [0, 0.05, 0], [-0.2, 0.1, 0.3], [1e-45, 0, 0]], F)
            Q = np.repeat(q, len(dq), axis=0); DX = np.tile(dq, (len(q), 1)); DY = np.tile(dq[::-1], (len(q), 1))
            # fix_wrap's switch: `inv * (sx.y - st.y)` on and beside +-0.5.  On the unit circle at angle phi the t coordinate is phi / 2 pi (spherical, from +x; cylindrical from -x):
            # a step of +-0.05 (spherical, delta 0.1) or +-0.005 (cylindrical, delta 0.01) in t is the switch.  The chord's end point is swept over a window around it.
            sph = t["kind"] == "spherical"
            delta, jump = (0.1, 0.05) if sph else (0.01, 0.005)
            fw_p, fw_d = [], []
            for phi0 in (0.7, 2.9, 4.4, 6.0, 0.1):
                for sgn in (1, -1):
                    for k in range(-24, 25):
                        dphi = sgn * 2 * math.pi * jump * (1 + k * 2.5e-7)
                        p0 = np.array([math.cos(phi0), math.sin(phi0), 0.0]); p1 = np.array([math.cos(phi0 + dphi), math.sin(phi0 + dphi), 0.0])
                        fw_p.append(p0); fw_d.append((p1 - p0) / delta)
            fw_p = np.array(fw_p, F); fw_d = np.array(fw_d, F)
            Q = np.concatenate([Q, fw_p, fw_p, q]); DX = np.concatenate([DX, fw_d, np.zeros_like(fw_d), np.zeros_like(q)]); DY = np.concatenate([DY, np.zeros_like(fw_d), fw_d, np.zeros_like(q)])   # (the last: no differentials at all)
            if t["xform"] == "rotated":   # world = texture_to_world(point); the probe's origin case must land on the mapping's origin as exactly as float32 allows
                with np.errstate(all="ignore"):
                    Q = host.transform_points(rot[1], Q).astype(F); DX = host.transform_vectors(rot[1], DX).astype(F); DY = host.transform_vectors(rot[1], DY).astype(F)
            out.append(batch(t["id"], ctx(np.zeros((1, 2), F), None, Q, DX, DY), f"{t['kind']} {t['xform']} {t['tex']}", rec=t))
        return out


class Procedural3D(ProbeSet):
    """Perlin noise through a one-octave fbm, fbm and wrinkled around every octave count, marble's spline segments, windy, the 3D checkerboard"""
    name = "procedural_3d"; variants = (0, 1)

    def capture(self, scene, host):
        a, b = scene.add_texture_constant(CA), scene.add_texture_constant(CB)
        tex = dict(noise=scene.add_texture_fbm(omega=1.0, octaves=1))
        for wr in (False, True):
            for oc in (0, 1, 8):
                for om in (0.0, 0.5, 1.0):
                    tex[f"{'wrinkled' if wr else 'fbm'} {oc} {om}"] = scene.add_texture_fbm(omega=om, octaves=oc, wrinkled=wr)
        tex["fbm 16 0.5"] = scene.add_texture_fbm(omega=0.5, octaves=16)
        tex["marble flat"] = scene.add_texture_marble(scale=1.0, variation=0.0)
        tex["marble"] = scene.add_texture_marble(scale=1.5, variation=0.2)
        tex["windy"] = scene.add_texture_windy()
        tex["checker3d"] = scene.add_texture_checkerboard3d(a, b)
        tex["checker3d scaled"] = scene.add_texture_checkerboard3d(a, b, m=host.scale([2.0, 0.5, 4.0])[0])
        return dict(tex=tex)

    def cases(self, info):
        T = info["tex"]; out = []
        small = np.array([[2.0 ** -6, 0, 0]], F)   # len2 = 2^-12: n = 5, every octave of a texture of up to 5 runs in full
        lat = np.concatenate([np.arange(-3, 4).astype(F), np.array([255, 256, 257, -1, -256, -257, 254.5], F)])
        below = np.array([step(k, -1) for k in (-2, -1, 0, 1, 2, 255, 256, -255)] + [-1e-45, -DENORMAL, 1e-45], F)
        far = np.array([2.0 ** 24, -2.0 ** 24, 2.0 ** 31, -2.0 ** 31, 2.0 ** 63, -2.0 ** 63, 2.0 ** 24 + 2, 1e30, 3e38], F)
        line = np.concatenate([np.linspace(254.5, 256.5, 17).astype(F), np.linspace(-1.5, 0.5, 17).astype(F)])
        vals = np.concatenate([lat, below, far, line, EDGE])
        v3, v7 = np.full_like(vals, 0.3), np.full_like(vals, 0.7)
        p = np.concatenate([np.stack([vals, v3, v7], axis=1), np.stack([v3, vals, v7], axis=1), np.stack([v3, v7, vals], axis=1), np.stack([vals, vals, vals], axis=1),
                            np.stack([lat, lat[::-1], np.roll(lat, 3)], axis=1)])
        generic = np.array([[0.37, 1.61, -2.43], [10.25, -3.5, 7.125], [-100.3, 55.7, 0.01]], F)
        out.append(batch(T["noise"], ctx(np.zeros((1, 2), F), None, np.concatenate([p, generic]), small, [[0, 2.0 ** -7, 0]]), "noise through fbm(octaves 1, omega 1)"))
        for name, tid in T.items():
            if not (name.startswith("fbm") or name.startswith("wrinkled")):
                continue
            oc = int(name.split()[1])
            lens = []
            for k in range(0, min(oc, 8) + 2):   # n = -1 - log2(len2) / 2 = k for dpdx = (2^-(k + 1), 0, 0)
                lens.append(beside(F(2.0 ** -(k + 1)), 2))
                for part in (0.3, 0.7):
                    lens.append(beside(F(2.0 ** -(k + 1 + part)), 3))
            lens.append(np.array([0.0, 1.0, 2.0, 1e-45, DENORMAL, 1e-30, 1e19, 3e38, np.inf, np.nan, -0.25], F))
            lens = np.concatenate(lens)
            dpdx = np.stack([lens, np.zeros_like(lens), np.zeros_like(lens)], axis=1)
            rows = [ctx(np.zeros((1, 2), F), None, np.repeat(generic[:2], len(dpdx), axis=0), np.tile(dpdx, (2, 1)), np.tile(dpdx[:, ::-1] * F(0.5), (2, 1)))]
            pe = np.concatenate([generic, np.array([[1e30, 1e30, 1e30], [0, 0, 0], [-0.0, 255.0, 256.0], [1e-45, -1e-45, 0.5], [3e38, 0, 0], [np.inf, 0, 0], [np.nan, 1, 1], [2.0 ** 24, 0.5, -2.0 ** 31]], F)])
            rows.append(ctx(np.zeros((1, 2), F), None, np.repeat(pe, 3, axis=0), np.tile(np.array([[2.0 ** -6, 0, 0], [0.3, 0.01, 0], [0, 0, 0]], F), (len(pe), 1)), np.tile(np.array([[0, 2.0 ** -7, 0], [0, 0.01, 0.2], [0, 0, 0]], F), (len(pe), 1))))
            out.append(batch(tid, np.concatenate(rows), name))
        # marble with variation 0: marble = p.y, tt = 0.5 + 0.5 sin(p.y); tt * 6 on and beside 6 (p.y = pi / 2) and 1 (sin = -2 / 3), and around the whole period
        ys = np.concatenate([beside(F(math.pi / 2), 8), beside(F(math.asin(-2.0 / 3.0)), 8), beside(F(math.pi - math.asin(-2.0 / 3.0)), 8), beside(F(-math.pi / 2), 4), np.linspace(-4, 4, 41).astype(F), EDGE])
        pm = np.stack([np.full_like(ys, 0.3), ys, np.full_like(ys, 0.7)], axis=1)
        out.append(batch(T["marble flat"], ctx(np.zeros((1, 2), F), None, pm, small, [[0, 2.0 ** -7, 0]]), "marble, variation 0"))
        gp = np.concatenate([pm[::3], generic, p[::5]])
        out.append(batch(T["marble"], ctx(np.zeros((1, 2), F), None, gp, [[0.01, 0.002, 0]], [[0, 0.004, 0.01]]), "marble"))
        wd = np.array([[2.0 ** -6, 0, 0], [0.3, 0.01, 0], [0, 0, 0], [1e-3, 1e-3, 1e-3], [np.inf, 0, 0], [2.0 ** -3, 0, 0], [2.0 ** -4, 0, 0]], F)
        wp = np.concatenate([generic, p[::4]])
        out.append(batch(T["windy"], ctx(np.zeros((1, 2), F), None, np.repeat(wp, len(wd), axis=0), np.tile(wd, (len(wp), 1)), np.tile(wd[::-1], (len(wp), 1))), "windy"))
        # checkerboard3d: integer planes, -0.0, sums that saturate and wrap
        cv = np.concatenate([np.concatenate([beside(F(k)) for k in (-2, -1, 0, 1, 2)]), np.array([-0.0, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, 3e9, -3e9, 2.0 ** 30, -2.0 ** 30, 1e19, -1e19], F), EDGE])
        cp = np.concatenate([np.stack([cv, np.full_like(cv, 0.5), np.full_like(cv, 1.5)], axis=1), np.stack([cv, cv, cv], axis=1), np.stack([cv, cv[::-1], np.roll(cv, 5)], axis=1),
                             np.stack([np.roll(cv, 2), np.full_like(cv, 0.5), cv], axis=1)])
        out.append(batch(T["checker3d"], ctx(np.zeros((1, 2), F), None, cp), "checkerboard3d")); out.append(batch(T["checker3d scaled"], ctx(np.zeros((1, 2), F), None, cp), "checkerboard3d scaled"))
        return out


# ---------------------------------------------------------------- bump --------------------------------------------------------------------------------------------------------
class Bump(ProbeSet):
    """Material::bump on explicit shading frames: the 0.0005 substitute, a zero cross product, the face_forward tie, dn/du and dn/dv"""
    name = "bump"; kind = "bump"; variants = (0, 1, 2, 3)

    def capture(self, scene, host):
        mip = scene.add_mipmap(make_image(16, 16, seed=9), as_float=True, wrap="repeat", max_anisotropy=8.0)
        img = scene.add_texture_imagemap(mip, 2.0, 2.0, 0.0, 0.0)
        a, b = scene.add_texture_constant(0.05), scene.add_texture_constant(-0.02)
        wr = scene.add_texture_scale(scene.add_texture_fbm(omega=0.5, octaves=6, wrinkled=True), scene.add_texture_constant(0.1))
        return dict(tex=[dict(id=scene.add_texture_constant(0.25), tag="constant", simple=True), dict(id=img, tag="float image", simple=True),
                         dict(id=scene.add_texture_dots(a, b, 4.0, 4.0, 0.0, 0.0), tag="dots", simple=False), dict(id=wr, tag="wrinkled times a constant", simple=False)])

    def cases(self, info):
        uvs = np.array([[0.37, 0.61], [0.5, 0.5], [-0.26, 1.07], [0.124, 0.126]], F)
        ps = np.array([[0.3, -0.2, 0.1], [2.5, 1.5, -0.5]], F)
        derivs = np.array([[0, 0, 0, 0], [0.01, 0.0, 0.0, 0.02], [-0.01, 0.003, 0.004, -0.02], [0, 0.01, 0, 0], [0.01, 0, 0, 0], [DENORMAL, 0, 0, -DENORMAL], [1e-45, 1e-45, 1e-45, 1e-45],
                           [-0.0, 0.0, -0.0, 0.0], [0.2, 0.1, -0.1, 0.2], [np.inf, 0, 0, 0.01], [np.nan, 0, 0, 0.01], [1e19, 0, 0, 1e19]], F)
        dp = np.array([[0, 0, 0, 0, 0, 0], [0.01, 0, 0, 0, 0.02, 0], [0.002, 0.001, 0, -0.001, 0.003, 0]], F)
        # frames: (n, ns, dpdu_s, dpdv_s, dndu, dndv)
        z = [0, 0, 0]
        frames = [
            ([0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 1, 0], z, z),                    # n with the new normal
            ([0, 0, -1], [0, 0, 1], [1, 0, 0], [0, 1, 0], z, z),                   # n against it
            ([1, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], z, z),                    # n perpendicular (for a flat displacement): face_forward's tie
            ([0, 1, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], z, z),
            ([0, 0, 1], [0, 0, 1], [1, 0, 0], [2, 0, 0], z, z),                    # dpdu_s parallel to dpdv_s: a zero cross product under a constant displacement
            ([0, 0, 1], [0, 0, 1], [1, 0, 0], [-1, 0, 0], z, z),
            ([0, 0, 1], [0, 0, 1], z, z, z, z),
            ([0.1, 0.2, 0.97], [0.0, 0.3, 0.95], [1.0, 0.1, -0.03], [-0.1, 1.0, -0.3], [0.2, 0.0, 0.05], [0.0, -0.3, 0.1]),
            ([0.1, 0.2, -0.97], [0.0, 0.3, 0.95], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.2], [1.0, 2.0, 3.0], [-3.0, 1.0, 0.5]),
            ([0, 0, 1], [0, 0, 1], [1e19, 0, 0], [0, 1e19, 0], z, z),
            ([0, 0, 1], [0, 0, 1], [1e-30, 0, 0], [0, 1e-30, 0], z, z),
            ([0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], z, z),
            ([-0.0, 0.0, -0.0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]),
        ]
        fr = np.array([np.concatenate([np.asarray(v, np.float64) for v in f]) for f in frames], F)
        rows = []
        for uv in uvs:
            for p in ps:
                for d in derivs:
                    for q in dp:
                        for f in fr:
                            rows.append(np.concatenate([uv, d, p, q, f]))
        inp = np.array(rows, F)
        return [dict(tex=t["id"], inp=inp, tag=t["tag"], variants=(0, 1, 2, 3) if t["simple"] else (0, 1)) for t in info["tex"]]


SETS = [TexelGrid(), TrilinearLevels(), EwaEllipse(), EwaSaturated(), Procedural2D(), Mappings(), Procedural3D(), Bump()]
SET_BY_NAME = {s.name: s for s in SETS}


# ---------------------------------------------------------------- running a set -----------------------------------------------------------------------------------------------
def batch_variants(ps, b):
    return b.get("variants", ps.variants)


def run_batches(scene, ps, batches, variant):
    """one (n, 3) — bump: (n, 6) — array per batch that has the variant, None for the others"""
    out = []
    for b in batches:
        if variant not in batch_variants(ps, b):
            out.append(None)
        elif ps.kind == "bump":
            out.append(scene.bump_probe_batch(b["tex"], b["inp"], variant))
        else:
            out.append(scene.texture_probe_batch(b["tex"], b["ctx"], variant))
    return out


def probe_work(orc, ps, batches):
    """(n, 2) per batch: footprint texels and noise calls of each probe, on the oracle.  A bump probe evaluates its texture three times: the work of the three contexts is summed."""
    out = []
    for b in batches:
        if ps.kind != "bump":
            out.append(orc.texture_probe_work(b["tex"], b["ctx"]))
            continue
        inp = b["inp"]; c = inp[:, :15]
        with np.errstate(all="ignore"):
            du = F(0.5) * (np.abs(c[:, 2]) + np.abs(c[:, 4])); du = np.where(du == 0, F(0.0005), du).astype(F)
            dv = F(0.5) * (np.abs(c[:, 3]) + np.abs(c[:, 5])); dv = np.where(dv == 0, F(0.0005), dv).astype(F)
            cu = c.copy(); cu[:, 0] = c[:, 0] + du; cu[:, 6:9] = c[:, 6:9] + du[:, None] * inp[:, 21:24]
            cv = c.copy(); cv[:, 1] = c[:, 1] + dv; cv[:, 6:9] = c[:, 6:9] + dv[:, None] * inp[:, 24:27]
        out.append(sum(orc.texture_probe_work(b["tex"], np.ascontiguousarray(x)) for x in (c, cu, cv)))
    return out


def thin_nans(batches, outs, key):
    """Probes whose oracle output holds a NaN stay in the set, where both sides must put the NaN in the same slot, but thinned at a fixed stride until they are at most NAN_SHARE
    of the set.  Decided on the oracle's output alone."""
    total = sum(len(b[key]) for b in batches)
    n_nan = sum(int(np.isnan(o).any(axis=1).sum()) for o in outs)
    if n_nan <= NAN_SHARE * total:
        return batches
    keep_every = int(math.ceil(n_nan / (NAN_SHARE * (total - n_nan) / (1.0 - NAN_SHARE))))
    while (n_nan + keep_every - 1) // keep_every > NAN_SHARE * (total - n_nan + (n_nan + keep_every - 1) // keep_every):   # the kept ones count towards the set they are a share of
        keep_every += 1
    thinned, seen = [], 0
    for b, o in zip(batches, outs):
        nan = np.isnan(o).any(axis=1)
        order = seen + np.cumsum(nan) - 1
        keep = ~nan | (order % keep_every == 0)
        seen += int(nan.sum())
        nb = dict(b); nb[key] = np.ascontiguousarray(b[key][keep])
        thinned.append(nb)
    return thinned


_prepared = {}


def prepared(name, host):
    """(set, oracle scene, batches, work per batch, {variant: oracle outputs per batch}) of one set: run through the oracle once, in libm mode 1, and left unchanged.  Raises if a
    probe is above a work cap: such a set is a mistake of the generator and goes to no device."""
    if name not in _prepared:
        ps = SET_BY_NAME[name]
        orc = OracleScene()
        info = ps.capture(orc, host)
        key = "inp" if ps.kind == "bump" else "ctx"
        set_libm_mode(1)
        try:
            batches = ps.cases(info)
            # NaNs are judged on the variant with differentials, which every batch has; the variants without can only lose NaNs that derivatives caused
            batches = thin_nans(batches, run_batches(orc, ps, batches, 0), key)
            work = probe_work(orc, ps, batches)
            for b, w in zip(batches, work):
                if len(w) and (int(w[:, 0].max()) > WORK_TEXELS or int(w[:, 1].max()) > WORK_NOISE):
                    i = int(np.argmax((w[:, 0] > WORK_TEXELS) | (w[:, 1] > WORK_NOISE)))
                    raise AssertionError(f"set {name} ({b['tag']}) probe {i}: {int(w[i, 0])} footprint texels, {int(w[i, 1])} noise calls: above the caps; inputs {hexf(b[key][i])}")
            want = {v: run_batches(orc, ps, batches, v) for v in ps.variants}
        finally:
            set_libm_mode(0)
        _prepared[name] = (ps, orc, batches, work, want)
    return _prepared[name]


def capture_product(name, host):
    """the set's scene on a device"""
    prod = pbrt_hip.Scene()
    SET_BY_NAME[name].capture(prod, host)
    return prod


def describe(name, b, i, key="ctx"):
    return f"set {name} texture {b['tex']} ({b['tag']}) probe {i}: {hexf(b[key][i])}"
