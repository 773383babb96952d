"""-m gpu: `pbrt_hip_render --quadrics --curves --loopsubdiv` renders the reference's shape showcase from its own, unmodified text
(tests/golden/ref_scenes/shapes/all-shapes-loopsubdiv.pbrt = scenes/shapes/all-shapes.pbrt).  At a reduced size the image equals, bit for bit, the same scene built call by call
through the C ABI.  At the file's own 800 x 400 @ 128 spp it is compared with the reference's render (renders/shapes/all-shapes.png) under the project's bounds — same >= 0.999,
le1 >= 0.9999, dmax <= 6 — on the left half (tests/golden/ref_renders/shapes_all-shapes_left.npz) and on the window around the subdivision surface itself
(shapes_all-shapes_subdiv.npz, cut by tests/golden/make_all_shapes_subdiv_crop.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import all_shapes_surface as surf
import curve_restatement as cr
import driver_scene as ds
import loopsubdiv_cases as cases
import pbrt_hip
import reference_scenes as R
from test_front_end_loopsubdiv import FIXTURE
from test_front_end_quadrics_gpu import blackbody_through_the_c_abi

pytestmark = pytest.mark.gpu
IDENT = (pbrt_hip.IDENTITY.copy(), pbrt_hip.IDENTITY.copy())


def all_shapes(s, host, spp, xres=800, yres=400):
    """the fixture through the C ABI, directive by directive"""
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
    for props in (dict(P=[-7, 0, 2, -7, 0, 3, -5, 0, 2, -5, 0, 3], degree=3, width=0.5, basis="bezier", curve_type="cylinder"),
                  dict(P=[-4, 0, 3, -3, 0, 2, -2, 0, 3], N=[-1, 1, 0, 1, -1, 0], degree=2, width=0.5, basis="bezier", curve_type="ribbon")):
        segs, warn = cr.from_props(**props)
        assert len(segs) == 1 and not warn
        m = matte()
        for g in segs:
            s.add_curve(IDENT[0], IDENT[1], g["type"], g["cp"], g["width"], g["n"], g["split_depth"], m, False)
    t = R.ctm(host, T((3.75, 0, 2.5)))
    s.add_mesh(host.transform_points(t[0], cases.TETRA_P), np.array(cases.TETRA_IDX, np.uint32), matte())
    t = R.ctm(host, T((6, 0, 2.5)), Sc((4, 4, 4)))
    assert np.array_equal(t[0], surf.O2W) and np.array_equal(t[1], surf.W2O)
    first = s.loopsubdiv_mesh(cases.TETRA_P, cases.TETRA_IDX, 3, counts_only=True)
    assert first == (130, 256)
    s.add_loopsubdiv(cases.TETRA_P, cases.TETRA_IDX, 3, matte(), t[0], t[1])
    t = R.ctm(host, T((0, 0, -1)))
    s.add_mesh(host.transform_points(t[0], R.quad(10.0)), R.QUAD_IDX, matte(), UV=R.QUAD_ST)
    R.camera_film(s, host, (0, 8, 0), (0, 0, 0), (0, 0, 1), 50.0, xres, yres, spp)
    s.build_accel_device_shapes(0, 4)


def run_front_end(tmp_path, spp=None, res=None):
    scene = tmp_path / "all-shapes.pbrt"
    text = open(FIXTURE).read()
    if spp is not None:
        text, n = re.subn(r'"integer pixelsamples" \d+', '"integer pixelsamples" %d' % spp, text); assert n == 1
    if res is not None:
        text = text.replace('"integer xresolution" [800]', '"integer xresolution" [%d]' % res[0]).replace('"integer yresolution" [400]', '"integer yresolution" [%d]' % res[1])
    scene.write_text(text)
    out = tmp_path / "out.pfm"
    r = subprocess.run([ds.RENDER_BIN, "--quadrics", "--curves", "--loopsubdiv", "--quiet", "--outfile", str(out), str(scene)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
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


def measures(mine, ref):
    d = np.abs(mine.astype(np.int32) - ref.astype(np.int32)).max(-1)
    return float((d == 0).mean()), float((d <= 1).mean()), int(d.max())


def test_the_references_render_of_its_own_file(tmp_path, host):
    """The file as the reference has it, at its own 800 x 400 @ 128 spp, against renders/shapes/all-shapes.png with the project's bounds (same >= 0.999, le1 >= 0.9999,
    dmax <= 6): on the left half, which tests/test_curve_render_gpu.py compares with the surface pasted in as a float64 triangle mesh, and on the window around the surface."""
    image = R.to_8bit(run_front_end(tmp_path))
    assert image.shape == (surf.YRES, surf.XRES, 3)
    # the window, found again with the device's rays: the pixel centres whose camera ray hits the subdivided triangles, padded by 8
    with pbrt_hip.Scene() as s:
        s.add_loopsubdiv(cases.TETRA_P, cases.TETRA_IDX, 3, s.add_material_matte((0.5, 0.5, 0.5)), surf.O2W, surf.W2O)
        s.build_accel(0, 4)
        o, d = surf.pixel_centre_rays()
        rays = np.zeros(len(d), pbrt_hip.RAY_DTYPE); rays["o"] = o; rays["d"] = d.astype(np.float32); rays["t_max"] = np.inf
        mask = (s.intersect_batch(rays)["prim"] < 256).reshape(surf.YRES, surf.XRES)
    fixture = np.load(os.path.join(R.HERE, "golden", "ref_renders", "shapes_all-shapes_subdiv.npz"))
    r0, r1, c0, c1 = (int(v) for v in fixture["window"])
    assert surf.window(mask) == (r0, r1, c0, c1), (surf.window(mask), int(mask.sum()))
    assert mask.sum() > 4000 and c0 >= 400          # the surface lies in the right half: the two windows share no pixel
    left = measures(image[:, :400], R.reference_render("shapes_all-shapes_left"))
    print("all-shapes from the reference's own file, left half: same %.5f le1 %.5f dmax %d" % left)
    on = measures(image[r0:r1, c0:c1], fixture["rgb"])
    inside = measures(image[r0:r1, c0:c1][mask[r0:r1, c0:c1]][None], fixture["rgb"][mask[r0:r1, c0:c1]][None])
    print("window rows %d .. %d, columns %d .. %d (%d pixels on the surface): same %.5f le1 %.5f dmax %d; on the surface's pixels alone: same %.5f le1 %.5f dmax %d"
          % (r0, r1, c0, c1, int(mask.sum()), *on, *inside))
    assert left[0] >= 0.999 and left[1] >= 0.9999 and left[2] <= 6, left
    assert on[0] >= 0.999 and on[1] >= 0.9999 and on[2] <= 6, on
