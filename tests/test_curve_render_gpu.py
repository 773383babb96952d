"""-m gpu: curves through the renderer.
  - closed forms: a straight flat curve under an orthographic camera and a constant sky covers exactly its strip, and the covered pixels carry Kd * L under the path and the
    Whitted integrator (tests/closed_form.py's conventions); a ribbon whose normals are perpendicular to the view has no width;
  - the reference's shape showcase less its loopsubdiv block (tests/golden/ref_scenes/shapes/all-shapes.pbrt), built call by call: the same film on one device, as tile parts,
    in sample-record bands and on several contexts; path, Whitted and direct lighting all render it;
  - `pbrt_hip_render --quadrics --curves` on the file equals that call-by-call build bit for bit;
  - at the file's own 800 x 400 @ 128 spp, the curves' half of the image against the reference's own render (renders/shapes/all-shapes.png), with the subdivision surface
    the fixture leaves out given back as a triangle mesh: without it that half differs from the reference's in 4 % of its pixels, curves or no curves."""
import re
import shutil
import subprocess

import numpy as np
import pytest

import closed_form as cf
import curve_restatement as cr
import driver_scene as ds
from loop_subdivision import loop_subdivide
import pbrt_hip
import reference_scenes as R
from test_band_plan_cpu import REC
from test_front_end_curves import FIXTURE
from test_front_end_quadrics_gpu import blackbody_through_the_c_abi

pytestmark = pytest.mark.gpu
IDENT = (pbrt_hip.IDENTITY.copy(), pbrt_hip.IDENTITY.copy())
MISS = 0xFFFFFFFF


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------------------------------
RES = 32          # the orthographic screen window is [-1, 1]^2: a pixel is 1/16 wide
STRIP_W = 0.25    # the strip |y| <= 1/8, |x| <= 3/8 ends on pixel boundaries: every pixel lies wholly in it or wholly outside
STRIP_CP = [[-0.375, 0, 0], [-0.125, 0, 0], [0.125, 0, 0], [0.375, 0, 0]]


def strip_scene(s, host, spp, ctype="flat", n=None):
    s.add_light_infinite(cf.LE)
    m = s.add_material_matte(cf.RHO_RGB)
    s.add_curve(IDENT[0], IDENT[1], ctype, STRIP_CP, [STRIP_W, STRIP_W], n, 2, m)
    # every camera sample at its pixel's centre: the strip's rim and end planes are inclusive and lie ON pixel boundaries, where the first Halton sample of a pixel (0, 0) falls
    cf._setup_view(s, host, RES, spp, cf.HALTON, cf.ortho_down(host, RES), at_center=True)
    s.build_accel(0, 4)


@pytest.mark.parametrize("integrator", ["path", "whitted"])
def test_straight_flat_curve_covers_its_strip_and_carries_kd_times_l(host, integrator):
    """A flat curve faces every ray, so the strip is a matte surface seen head-on under a uniform sky with nothing else in the scene: L_o = Kd * L in expectation (the spawned
    rays start 2 * hit_width off the strip — p_error — and none of them comes back within w / 2 of the axis).  Outside the strip the camera ray sees the sky itself."""
    with pbrt_hip.Scene() as s:
        strip_scene(s, host, 64)
        xyz, wt, st = s.render_path(max_depth=5) if integrator == "path" else s.render_whitted(max_depth=5)
        rgb = np.asarray(s.film_to_rgb(xyz, wt), np.float64)
    sky = np.all(np.abs(rgb - np.asarray(cf.LE)) < 1e-5, axis=-1)
    c = (np.arange(RES) + 0.5) / RES * 2.0 - 1.0
    want = (np.abs(c)[:, None] < STRIP_W / 2) & (np.abs(c)[None, :] < 0.375)        # rows = y, columns = x; the strip is symmetric in both
    assert want.sum() == 4 * 12
    assert np.array_equal(~sky, want), f"covered {int((~sky).sum())} pixels, the strip holds {int(want.sum())}"
    E = np.asarray(cf.RHO_RGB) * np.asarray(cf.LE)
    cf.assert_mean(rgb[want], E, se_target=0.02, wrongs={"the sky": cf.LE, "black": (0, 0, 0), "Kd L / pi": E / np.pi, "2 Kd L": 2 * E}, label=f"flat strip, {integrator}")
    assert st.regular_rays > st.camera_rays or integrator == "whitted"
    assert st.camera_rays == RES * RES * 64


def test_ribbon_seen_edge_on_has_no_width(host):
    """Ribbon normals perpendicular to the view direction: hit_width is scaled by |n_hit . d| / |d| = 0, and the film is the sky.  Face-on the same ribbon covers the strip."""
    for n, covered in (([[0, 1, 0], [0.1, 1, 0]], 0), ([[0, 0, 1], [0.05, 0, 1]], 48)):
        with pbrt_hip.Scene() as s:
            strip_scene(s, host, 16, "ribbon", n)
            xyz, wt, _ = s.render_whitted(max_depth=5)
            rgb = np.asarray(s.film_to_rgb(xyz, wt), np.float64)
        sky = np.all(np.abs(rgb - np.asarray(cf.LE)) < 1e-5, axis=-1)
        assert int((~sky).sum()) == covered, (n, int((~sky).sum()))


# ---- the shape showcase, call by call ---------------------------------------------------------------------------------------------------------------------------------
def all_shapes(s, host, spp, xres=800, yres=400, curves=True):
    """tests/golden/ref_scenes/shapes/all-shapes.pbrt through the C ABI, directive by directive.  Returns the primitive slots of the curve segments."""
    s.add_light_infinite((0.8, 0.9, 1.0))
    s.add_light_distant(R.blackbody("3000x1.5"), host.distant_direction(IDENT[0], (-30.0, 40.0, 100.0), (0.0, 0.0, 1.0)))
    matte = lambda: s.add_material_matte((0.5, 0.5, 0.5))
    T, Rt, Sc = host.translate, host.rotate, host.scale
    t = R.ctm(host, T((-5, 1, 0))); s.add_sphere(t[0], t[1], 1.0, None, None, 360.0, matte(), False)
    t = R.ctm(host, T((-3, 0, 0)), Rt(75, (1, 0, 0))); s.add_quadric("cylinder", t[0], t[1], 0.75, -1.0, 1.0, 270.0, matte(), False)
    t = R.ctm(host, T((-1, 0, -0.5)), Rt(45, (1, 0, 0))); s.add_quadric("cone", t[0], t[1], 0.75, 2.0, 0.0, 270.0, matte(), False)
    t = R.ctm(host, T((0.5, 0, -0.5)), Rt(65, (-1, 1, 1))); s.add_quadric("paraboloid", t[0], t[1], 1.0, 0.0, 1.0, 270.0, matte(), False)
    t = R.ctm(host, T((2.7, 0, 0.4)), Rt(45, (-1, 0, 0))); s.add_hyperboloid(t[0], t[1], (3.0, 1.2, 1.0), (0.65, -0.5, -1.0), 270.0, matte(), False)
    t = R.ctm(host, T((4.8, 1, 0.25)), Rt(45, (-1, 0, 0)), Sc((0.75, 0.75, 0.75))); s.add_hyperboloid(t[0], t[1], (3.0, 1.2, 1.0), (1.0, -0.5, -1.0), 270.0, matte(), False)
    t = R.ctm(host, T((0, 0, 2)), Rt(90, (1, 0, 0))); s.add_quadric("disk", t[0], t[1], 1.0, 0.0, 0.25, 270.0, matte(), False)
    slots = []
    if curves:
        first = 7
        for props in (dict(P=[-7, 0, 2, -7, 0, 3, -5, 0, 2, -5, 0, 3], degree=3, width=0.5, basis="bezier", curve_type="cylinder"),
                      dict(P=[-4, 0, 3, -3, 0, 2, -2, 0, 3], N=[-1, 1, 0, 1, -1, 0], degree=2, width=0.5, basis="bezier", curve_type="ribbon")):
            segs, warn = cr.from_props(**props)
            assert len(segs) == 1 and not warn
            m = matte()
            for g in segs:
                s.add_curve(IDENT[0], IDENT[1], g["type"], g["cp"], g["width"], g["n"], g["split_depth"], m, False)
                slots += list(range(first, first + (1 << g["split_depth"]))); first += 1 << g["split_depth"]
    else:
        matte(); matte()
    t = R.ctm(host, T((3.75, 0, 2.5)))
    tet = np.array([[0.9428, 0.0, -0.3333], [-0.4714, 0.8165, -0.3333], [-0.4714, -0.8165, -0.3333], [0.0, 0.0, 1.0]], np.float32)
    s.add_mesh(host.transform_points(t[0], tet), np.array([0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2], np.uint32), matte())
    t = R.ctm(host, T((0, 0, -1)))
    s.add_mesh(host.transform_points(t[0], R.quad(10.0)), R.QUAD_IDX, matte(), UV=R.QUAD_ST)
    R.camera_film(s, host, (0, 8, 0), (0, 0, 0), (0, 0, 1), 50.0, xres, yres, spp)
    s.build_accel_device_shapes(0, 4)
    return slots


SMALL = dict(spp=4, xres=96, yres=48)


def film_bits(xyz, wt):
    return np.ascontiguousarray(xyz, np.float32).view(np.uint32), np.ascontiguousarray(wt, np.float32).view(np.uint32)


def counters(st):
    d = st.as_dict()
    return {k: d[k] for k in ("camera_rays", "regular_rays", "shadow_rays")}


def test_every_integrator_renders_the_showcase(host):
    with pbrt_hip.Scene() as s, blackbody_through_the_c_abi():
        slots = all_shapes(s, host, **SMALL)
        assert len(slots) == 16
        for name, run in (("path", lambda: s.render_path(max_depth=5)), ("whitted", lambda: s.render_whitted(max_depth=5)), ("direct", lambda: s.render_direct("all", max_depth=5))):
            xyz, wt, st = run()
            assert np.isfinite(np.asarray(xyz)).all() and float(np.asarray(wt).min()) > 0, name
            # every material of the file is matte: Whitted recurses at specular lobes alone and traces no ray beyond the camera's; the path integrator's bounces and
            # estimate_direct's BSDF-sampled rays (path and direct lighting) are regular rays
            assert st.shadow_rays > 0 and (st.regular_rays == st.camera_rays if name == "whitted" else st.regular_rays > st.camera_rays), (name, counters(st))


@pytest.mark.parametrize("integrator", ["path", "whitted"])
def test_showcase_is_the_same_film_under_every_driver(host, integrator):
    """One device, three tile parts, a sample-record budget that forces at least three bands, several contexts: film, weights and counters bit-equal"""
    def render(s, **kw):
        return s.render_path(max_depth=5, **kw) if integrator == "path" else s.render_whitted(max_depth=5, **kw)
    with blackbody_through_the_c_abi():
        with pbrt_hip.Scene() as s:
            all_shapes(s, host, **SMALL)
            xyz, wt, st = render(s)
            want = film_bits(xyz, wt); want_st = counters(st)
            # tile parts: the parts' films add up tile by tile (each pixel belongs to one part's tiles under the box filter of radius 0.5)
            acc_x = np.zeros_like(np.asarray(xyz)); acc_w = np.zeros_like(np.asarray(wt)); acc = dict.fromkeys(want_st, 0)
            for p in range(3):
                x, w, t = render(s, tile_part=p, tile_parts=3)
                acc_x += np.asarray(x); acc_w += np.asarray(w)
                for k, v in counters(t).items(): acc[k] += v
            got = film_bits(acc_x, acc_w)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and acc == want_st, "tile parts"
            # bands: 96 x 48 is 6 x 3 tiles of 16 x 16; a budget of 6 tiles' records makes three bands
            s.set_sample_record_budget(6 * 256 * SMALL["spp"] * REC)
            x, w, t = render(s)
            got = film_bits(x, w)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and counters(t) == want_st, "bands"
        with pbrt_hip.Scene(devices=[0, 0, 0]) as s:
            all_shapes(s, host, **SMALL)
            x, w, t = (s.render_path(max_depth=5) if integrator == "path" else s.render_whitted_devices(max_depth=5))
            got = film_bits(x, w)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and counters(t) == want_st, "several contexts"


# ---- the front end ------------------------------------------------------------------------------------------------------------------------------------------------------
def run_front_end(tmp_path, spp=None, res=None, text=None):
    scene = tmp_path / "all-shapes.pbrt"
    text = open(FIXTURE).read() if text is None else text
    if spp is not None:
        text, n = re.subn(r'"integer pixelsamples" \d+', '"integer pixelsamples" %d' % spp, text); assert n == 1
    if res is not None:
        text = text.replace('"integer xresolution" [800]', '"integer xresolution" [%d]' % res[0]).replace('"integer yresolution" [400]', '"integer yresolution" [%d]' % res[1])
    scene.write_text(text)
    out = tmp_path / "out.pfm"
    r = subprocess.run([ds.RENDER_BIN, "--quadrics", "--curves", "--quiet", "--outfile", str(out), str(scene)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return ds.read_pfm(str(out))


def test_front_end_equals_the_c_abi_build_bit_for_bit(tmp_path, host):
    got = run_front_end(tmp_path, spp=8, res=(200, 100))
    with pbrt_hip.Scene() as s, blackbody_through_the_c_abi():
        all_shapes(s, host, spp=8, xres=200, yres=100)
        xyz, wt, _ = s.render_whitted(max_depth=5)
        want = np.ascontiguousarray(s.film_to_rgb(xyz, wt), np.float32)
    assert got.shape == want.shape
    diff = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not diff.any(), (int(diff.sum()), float(np.abs(got - want).max()))
    assert float(want.max()) > 0.05




def subdivision_surface_as_a_mesh():
    """The block the fixture leaves out — `Translate 6 0 2.5  Scale 4 4 4  Shape "loopsubdiv"` of a tetrahedron, nlevels 3 by default — as a `Shape "trianglemesh"` under
    the same transform: the surface the reference rendered, without the vertex normals (they shade the surface itself, which lies outside the compared window)"""
    P, idx = loop_subdivide([[0.9428, 0.0, -0.3333], [-0.4714, 0.8165, -0.3333], [-0.4714, -0.8165, -0.3333], [0.0, 0.0, 1.0]], [0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2], 3)
    assert len(idx) == 3 * 4 * 4 ** 3
    return ('  AttributeBegin\n    Material "matte"\n    Translate 6 0 2.5\n    Scale 4 4 4\n    Shape "trianglemesh"\n        "integer indices" [ %s ]\n        "point P" [ %s ]\n  AttributeEnd\n\n'
            % (" ".join(str(int(v)) for v in idx), " ".join("%.9g" % v for v in P.astype(np.float32).ravel())))


def test_the_references_render_of_the_shape_showcase(tmp_path, host):
    """The file at its own 800 x 400 @ 128 spp against renders/shapes/all-shapes.png on the curves' half of the image (world x < 0 = raster columns 0 .. 399, fixture made by
    tests/golden/make_all_shapes_crop.py), with the measures and bounds of test_front_end_reproduces_the_references_render_pixel_for_pixel (the project's general ones):
    same >= 0.999, le1 >= 0.9999, dmax <= 6.

    The half is NOT clear of the subdivision surface the fixture leaves out.  Measured on an MI355X with the fixture as it is: over the half same 0.95936, le1 0.97362,
    dmax 17; 4 220 pixels off by more than one level, 22 of them on a curve, this image brighter than the reference's by 1.6 - 2.1 levels there, the share of equal pixels
    falling from 1.000 in the top rows to 0.89 on the floor nearest the camera.  The curves have no part in it: with both curves taken out as well, adding or removing the surface
    changes the same half by the same amount (same 0.95956, dmax 17, 4 192 pixels off by more than one level, all on the floor).  With the surface given back as a plain
    triangle mesh (tests/loop_subdivision.py, written from loopsubdiv.rs) the half IS the reference's: same 1.00000, le1 1.00000, dmax 0, the curves' 4 958 pixels included.
    How a surface that small and that far reaches the floor of the other half is not established (the sky it hides looks too little; it also moves the scene's bound, which the
    lights' shadow rays are cut to).  So the test renders what the reference rendered — the fixture plus that mesh where the file had its loopsubdiv block — and asks what the
    comparison was set up to ask, on the same window, reference and bounds."""
    text = open(FIXTURE).read()
    floor = text.index('  AttributeBegin\n    Material "matte"\n    Translate 0 0 -1')
    original = open(FIXTURE).read()
    assert "loopsubdiv" not in original
    scene_text = text[:floor] + subdivision_surface_as_a_mesh() + text[floor:]
    mine = R.to_8bit(run_front_end(tmp_path, text=scene_text))[:, :400]
    ref = R.reference_render("shapes_all-shapes_left")
    assert mine.shape == ref.shape == (400, 400, 3)
    # the window holds the new ground: camera rays that hit a curve segment
    with pbrt_hip.Scene() as s, blackbody_through_the_c_abi():
        slots = all_shapes(s, host, spp=1)
        rays, _ = s.camera_rays_probe() if hasattr(s, "camera_rays_probe") else (None, None)
        if rays is None:
            # pixel centres of the left half through the camera of the file: LookAt 0 8 0 / 0 0 0 / 0 0 1, fov 50 over the shorter (y) axis, screen window [-2, 2] x [-1, 1]
            px = (np.arange(400) + 0.5) / 800 * 4.0 - 2.0; py = 1.0 - (np.arange(400) + 0.5) / 400 * 2.0
            tan = np.tan(np.radians(50.0) / 2)
            X, Y = np.meshgrid(px, py)
            d = np.stack([X.ravel() * tan, -np.ones(X.size), Y.ravel() * tan], 1)     # camera x = world x, camera y = world z, camera z = world -y
            r = np.zeros(len(d), pbrt_hip.RAY_DTYPE); r["o"] = (0, 8, 0); r["d"] = d.astype(np.float32); r["t_max"] = np.inf
            rays = r
        hits = s.intersect_batch(rays)
        on_curve = np.isin(hits["prim"], np.asarray(slots, np.uint32))
        assert on_curve.sum() > 300, int(on_curve.sum())
    d = np.abs(mine.astype(np.int32) - ref.astype(np.int32)).max(-1)
    same, le1, dmax = (d == 0).mean(), (d <= 1).mean(), d.max()
    dc = d.reshape(-1)[on_curve]
    rows = ", ".join("%d-%d: %.3f" % (r0, r0 + 50, (d[r0:r0 + 50] == 0).mean()) for r0 in range(0, 400, 50)); cols = ", ".join("%d-%d: %.3f" % (c0, c0 + 50, (d[:, c0:c0 + 50] == 0).mean()) for c0 in range(0, 400, 50))
    print("same by rows:", rows); print("same by columns:", cols)
    off = d.reshape(-1) > 1
    print("pixels off by more than 1: %d, of them on a curve %d; mean signed difference there %s" % (off.sum(), (off & on_curve).sum(), (mine.astype(np.int32) - ref.astype(np.int32)).reshape(-1, 3)[off].mean(0) if off.any() else "-"))
    print("all-shapes, left half: same %.5f le1 %.5f dmax %d; on the curves' %d pixels: same %.5f le1 %.5f dmax %d" % (same, le1, dmax, on_curve.sum(), (dc == 0).mean(), (dc <= 1).mean(), dc.max()))
    assert same >= 0.999 and le1 >= 0.9999 and dmax <= 6, (same, le1, dmax)
