"""-m gpu: the Whitted integrator on a handle over several devices (pbrt_hip_render_whitted_devices) and as tile parts (pbrt_hip_render_whitted_tiles_device).  One GPU serves
every context (the ordinals repeat, as in tests/test_multi_device_gpu.py).  Every comparison is on bits: `xyz` as uint32, the weights exactly, the three ray counters — against
the one-device film of pbrt_hip_render_whitted and against the CPU oracle's li_whitted (oracle_set_integrator(1) in libm mode 1)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch   # device buffers for the rank form.  At module level: first imported inside a test, after the library had run kernels in the process, torch found no device

import closed_form as cf
import driver_scene as ds
import pbrt_hip
import reference_scenes as R
import sphere_light_scenes as SL
from oracle_binding import OracleScene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 4
EXTRA_P = np.array([[-1.0, -1.6, 0.05], [0.6, -1.6, 0.05], [-0.2, -1.2, 1.1]], np.float32)


def stage(s, host, xres=48, yres=40, spp=4, sampler="halton", gaussian_crop=None, sphere_light=True, extra=False, build=True):
    """Every Whitted kernel in 48 x 40 pixels: a glass cube and a mirror (the binary recursion), a matte floor under a checkerboard (whitted_vertex_kernel), a cylinder and a
    sphere light (the <true> instantiations), an emissive quad of two triangles and a point light: four lights, 5 + 15 * 2 * 4 + 7 * 4 = 153 sampler dimensions at depth 4."""
    const = s.add_texture_constant
    floor = s.add_material_matte_tex(s.add_texture_checkerboard(const((0.15, 0.2, 0.6)), const((0.8, 0.8, 0.7)), 6.0, 6.0))
    glass = s.add_material_glass(kr=(0.9, 0.95, 1.0), kt=(0.95, 0.9, 0.85), eta=1.5)
    mirror = s.add_material_mirror((0.9, 0.8, 0.7))
    matte = s.add_material_matte((0.6, 0.3, 0.2))
    black = s.add_material_matte((0.0, 0.0, 0.0))
    s.add_mesh(R.quad(4.0), R.QUAD_IDX, floor, UV=R.QUAD_ST)
    t = R.ctm(host, host.translate((-0.9, 0.3, 0.6)), host.rotate(25.0, (0, 0, 1)), host.scale((0.5, 0.5, 0.6)))
    s.add_mesh(host.transform_points(t[0], R.CUBE_P), R.CUBE_IDX, glass)
    t = R.ctm(host, host.translate((1.0, 0.8, 0.9)), host.rotate(-20.0, (0, 0, 1)), host.rotate(80.0, (1, 0, 0)))
    s.add_mesh(host.transform_points(t[0], R.quad(0.9)), R.QUAD_IDX, mirror)
    t = R.ctm(host, host.translate((0.9, -1.0, 0.5)), host.rotate(15.0, (1, 0, 0)))
    s.add_quadric("cylinder", t[0], t[1], 0.35, -0.5, 0.5, 360.0, matte, False)
    if sphere_light:
        SL.add_sphere_light(s, R.ctm(host, host.translate((-1.5, -0.5, 4.0))), 0.8, material=black, L=(8.0, 8.0, 7.0))
    s.add_light_point((6.0, 7.0, 8.0), (2.5, -2.0, 3.0))
    first = s.add_light_diffuse_area((5.0, 5.0, 4.0), 2)
    t = R.ctm(host, host.translate((0.5, 2.5, 3.5)), host.rotate(150.0, (1, 0, 0)))
    s.add_mesh(host.transform_points(t[0], R.quad(0.6)), R.QUAD_IDX, matte, first_area_light=first)
    if extra:
        add_extra(s)
    _, c2w = host.look_at((0.3, -5.0, 2.2), (0.0, 0.3, 0.5), (0, 0, 1))
    s.set_camera_perspective(host.perspective_raster_to_camera(50.0, xres, yres, None), c2w)
    if gaussian_crop is None:
        radius = (0.5, 0.5)
        cb, table, sb = host.film_box(xres, yres)
    else:
        radius = (2.0, 2.0)
        cb, table, sb = host.film_filter("gaussian", xres, yres, radius, (2.0, 0.0), gaussian_crop)
    s.set_film(xres, yres, cb, radius, table)
    s.set_sampler(cf.SOBOL if sampler == "sobol" else cf.HALTON, spp, sb)
    if sampler == "sobol":
        s.set_sobol_tables(*cf.sobol_fixture())
    if build:
        s.build_accel(0, 4)


def add_extra(s):
    s.add_light_point((20.0, 18.0, 15.0), (0.2, -1.5, 1.0))
    s.add_mesh(EXTRA_P, [0, 1, 2], s.add_material_matte((0.8, 0.2, 0.2), 0.0))


def make(host, devices=None, **kw):
    s = pbrt_hip.Scene(devices=devices) if devices is not None else pbrt_hip.Scene()
    try:
        SL.capture(lambda s_, h: stage(s_, h, **kw), s, host)
    except Exception:
        s.close()
        raise
    return s


def oracle_film(host, depth=DEPTH, **kw):
    with OracleScene() as orc:
        SL.capture(lambda s_, h: stage(s_, h, **kw), orc, host)
        return SL.oracle_whitted(orc, max_depth=depth)


def assert_same_film(got, want, label=""):
    gxyz, gwt, gst = got
    oxyz, owt, ost = want
    assert gxyz.shape == oxyz.shape, label
    assert np.array_equal(gwt, owt), label
    diff = (gxyz.view(np.uint32) != oxyz.view(np.uint32)).any(-1)
    assert not diff.any(), (label, int(diff.sum()), float(np.abs(gxyz - oxyz).max()))
    for f in ("camera_rays", "regular_rays", "shadow_rays"):
        assert getattr(gst, f) == getattr(ost, f), (label, f, getattr(gst, f), getattr(ost, f))


@pytest.fixture(scope="module")
def base(host):
    """The one-device handle of the stage, its film (checked against the oracle's here, once), and its film at 2 spp for the tests that change the sampler"""
    one = make(host)
    want = one.render_whitted(max_depth=DEPTH)
    assert_same_film(want, oracle_film(host), "one device against the oracle")
    assert want[2].shadow_rays > 0 and want[2].regular_rays > want[2].camera_rays
    one.set_sampler(cf.HALTON, 2, one.sample_bounds)
    want2 = one.render_whitted(max_depth=DEPTH)
    one.set_sampler(cf.HALTON, 4, one.sample_bounds)
    yield one, want, want2
    one.close()


# ---- 1. the film ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 8])
def test_film_equals_one_device_and_the_oracle(host, base, n):
    """9 tiles over n contexts (with 8, all but one hold a single tile); `want` is the one-device film, which the fixture holds against the oracle's bit for bit"""
    one, want, want2 = base
    with make(host, devices=[0] * n) as multi:
        assert multi.devices() == [0] * n
        got = multi.render_whitted_devices(max_depth=DEPTH)
        assert_same_film(got, want, f"{n} contexts")
        for f in ("paths_total", "paths_zero_radiance", "extend_launches", "shadow_launches", "light_distributions_created"):
            assert getattr(got[2], f) == 0, f
        assert got[2].render_seconds > 0 and got[2].extend_seconds == 0
        assert_same_film(multi.render_whitted_devices(max_depth=DEPTH), want, "second frame: the replicas are reused")
        multi.set_sampler(cf.HALTON, 2, multi.sample_bounds)
        assert_same_film(multi.render_whitted_devices(max_depth=DEPTH), want2, "2 spp reach every context")


def test_one_device_handle_is_render_whitted(base):
    one, want, _ = base
    assert_same_film(one.render_whitted_devices(max_depth=DEPTH), want, "one-device handle")
    for part in range(2):
        assert_same_film(one.render_whitted_devices(max_depth=DEPTH, tile_part=part, tile_parts=2), one.render_whitted(max_depth=DEPTH, tile_part=part, tile_parts=2), f"part {part}")


def test_more_devices_than_tiles(host):
    """32 x 16 pixels are two tiles: six of the eight contexts own no pixel and hand over a zeroed buffer"""
    kw = dict(xres=32, yres=16)
    with make(host, **kw) as one, make(host, devices=[0] * 8, **kw) as multi:
        want = one.render_whitted(max_depth=DEPTH)
        assert_same_film(want, oracle_film(host, **kw), "one device against the oracle")
        assert_same_film(multi.render_whitted_devices(max_depth=DEPTH), want, "8 contexts, 2 tiles")


def test_overlapping_tiles_merge_in_tile_order(host):
    """A gaussian filter of radius 2 and a crop window off the tile grid: neighbouring tiles add to the same film pixels, so the order of the merge decides the bits"""
    kw = dict(gaussian_crop=(0.13, 0.87, 0.21, 0.9))
    with make(host, **kw) as one, make(host, devices=[0, 0, 0], **kw) as multi:
        want = one.render_whitted(max_depth=DEPTH)
        assert want[0].shape[0] < 40 and want[0].shape[1] < 48 and multi.tile_buffer_floats(16, 0, 1) > 4 * 48 * 40   # cropped; the tiles' pixel bounds reach into their neighbours'
        assert_same_film(want, oracle_film(host, **kw), "one device against the oracle")
        assert_same_film(multi.render_whitted_devices(max_depth=DEPTH), want, "3 contexts, gaussian")


def test_multi_handle_as_one_rank_of_several(host, base):
    """Two handles of two contexts each, tile_parts = 2: a four-way partition.  The box filter's tiles are disjoint, so the two partial films add exactly."""
    one, want, _ = base
    acc = np.zeros_like(want[0]); accw = np.zeros_like(want[1]); rays = [0, 0, 0]
    for part in range(2):
        with make(host, devices=[0, 0]) as m:
            x, w, st = m.render_whitted_devices(max_depth=DEPTH, tile_part=part, tile_parts=2)
            assert_same_film((x, w, st), one.render_whitted(max_depth=DEPTH, tile_part=part, tile_parts=2), f"part {part}")
        acc += x; accw += w
        rays = [a + b for a, b in zip(rays, (st.camera_rays, st.regular_rays, st.shadow_rays))]
    assert np.array_equal(acc.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(accw, want[1])
    assert rays == [want[2].camera_rays, want[2].regular_rays, want[2].shadow_rays]


def test_rank_form_parts_merge_to_the_whole_frame(base):
    one, want, _ = base
    bufs, rays = [], [0, 0, 0]
    for part in range(3):
        buf = torch.full((one.tile_buffer_floats(16, part, 3),), float("nan"), dtype=torch.float32, device="cuda")   # every slot has to be written
        st = one.render_whitted_tiles_device(buf.data_ptr(), max_depth=DEPTH, tile_part=part, tile_parts=3)
        assert (st.paths_total, st.extend_launches) == (0, 0)
        rays = [a + b for a, b in zip(rays, (st.camera_rays, st.regular_rays, st.shadow_rays))]
        bufs.append(buf)
    torch.cuda.synchronize()
    xyz, wt = one.merge_tiles_device([b.data_ptr() for b in bufs])
    assert np.array_equal(xyz.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(wt, want[1])
    assert rays == [want[2].camera_rays, want[2].regular_rays, want[2].shadow_rays]


def test_sample_record_budget_applies_to_every_context(host, base):
    """A tile's records are 256 * 4 * 20 = 20480 bytes: under 15000 no two tiles share a band, and either context holds four or five of the nine"""
    one, want, _ = base
    with make(host, devices=[0, 0]) as multi:
        multi.set_sample_record_budget(15000)
        got = multi.render_whitted_devices(max_depth=DEPTH)
        fp = multi.render_footprint()
        assert fp["bands"] > 1 and fp["record_budget"] == 15000, fp
        assert_same_film(got, want, "in bands")
        multi.set_sample_record_budget(0)
        got = multi.render_whitted_devices(max_depth=DEPTH)
        assert multi.render_footprint()["bands"] == 1
        assert_same_film(got, want, "one band again")


def test_path_and_whitted_alternate_on_one_handle(host):
    """The tile buffers and the replicas serve both integrators (no sphere light: the path integrator refuses one)"""
    kw = dict(sphere_light=False)
    with make(host, **kw) as one, make(host, devices=[0, 0, 0], **kw) as multi:
        path = one.render_path(max_depth=3, light_strategy=0)
        whitted = one.render_whitted(max_depth=DEPTH)
        assert (path[0].view(np.uint32) != whitted[0].view(np.uint32)).any()
        assert_same_film(multi.render_path(max_depth=3, light_strategy=0), path, "path first")
        assert_same_film(multi.render_whitted_devices(max_depth=DEPTH), whitted, "whitted between")
        assert_same_film(multi.render_path(max_depth=3, light_strategy=0), path, "path again")


def test_scene_change_reaches_every_context(host):
    """A light and a mesh added to a handle that has rendered, and the tree rebuilt: the film of a fresh one-device scene captured with them from the start"""
    with make(host, extra=True) as fresh, make(host, devices=[0, 0, 0]) as multi:
        want = fresh.render_whitted(max_depth=3)
        before = multi.render_whitted_devices(max_depth=3)
        add_extra(multi)
        multi.build_accel(0, 4)
        got = multi.render_whitted_devices(max_depth=3)
        assert_same_film(got, want, "after the change")
        assert (before[0].view(np.uint32) != got[0].view(np.uint32)).any() and before[2].shadow_rays != got[2].shadow_rays


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def _raw_devices(s, max_depth, tile_parts=1):
    h, w = s.film_shape
    xyz = np.full((h, w, 3), np.nan, np.float32); wt = np.full((h, w), -7.0, np.float32)
    pb = np.ascontiguousarray(s.sample_bounds, dtype=np.int32)
    fp = C.POINTER(C.c_float)
    rc = s.b.fn("render_whitted_devices")(s.h, max_depth, pb.ctypes.data_as(C.POINTER(C.c_int)), 16, 0, tile_parts, xyz.ctypes.data_as(fp), wt.ctypes.data_as(fp), None)
    return rc, bool(np.isnan(xyz).all() and (wt == -7.0).all())


def test_refusals_leave_outputs_and_handle_alone(host, base):
    one, want, _ = base
    with make(host, devices=[0] * 8) as multi:
        def still_renders(label):
            assert_same_film(multi.render_whitted_devices(max_depth=DEPTH), want, label)

        rc, untouched = _raw_devices(multi, 17)
        assert rc == pbrt_hip.ERR_INVALID_ARG and untouched, multi.last_error()
        still_renders("after max_depth 17")
        rc, untouched = _raw_devices(multi, DEPTH, tile_parts=9)   # 9 x 8 contexts = 72 parts, over the 64 a frame is dealt into
        assert rc == pbrt_hip.ERR_INVALID_ARG and untouched and "devices" in multi.last_error(), multi.last_error()
        still_renders("after too many parts")
        pb = np.ascontiguousarray(multi.sample_bounds, dtype=np.int32)
        for s in (one, multi):
            rc = s.b.fn("render_whitted_tiles_device")(s.h, DEPTH, pb.ctypes.data_as(C.POINTER(C.c_int)), 16, 0, 1, None, None)
            assert rc == pbrt_hip.ERR_INVALID_ARG and "tile buffer" in s.last_error(), s.last_error()
        rc = one.b.fn("render_whitted_tiles_device")(one.h, 17, pb.ctypes.data_as(C.POINTER(C.c_int)), 16, 0, 1, None, None)   # the integrator's own refusals come first
        assert rc == pbrt_hip.ERR_INVALID_ARG and "max_depth" in one.last_error(), one.last_error()
        still_renders("after a null tile buffer")
        # the 48 Sobol dimensions of tests/golden/sobol_subset.npz against the 153 the recursion may draw at depth 4; depth 1 draws 5 + 2 * 4 = 13
        multi.set_sampler(cf.SOBOL, 4, multi.sample_bounds)
        multi.set_sobol_tables(*cf.sobol_fixture())
        rc, untouched = _raw_devices(multi, DEPTH)
        assert rc == pbrt_hip.ERR_UNSUPPORTED and untouched and "Sobol" in multi.last_error(), multi.last_error()
        with make(host, sampler="sobol") as sob:
            assert_same_film(multi.render_whitted_devices(max_depth=1), sob.render_whitted(max_depth=1), "Sobol, depth 1, after the refusal")


# ---- 3. the front end -------------------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_renders_whitted_on_several_devices(tmp_path):
    """pbrt_hip_render --devices 0,0,0 on a scene file with Integrator "whitted" writes the image --device 0 writes"""
    exe = os.path.join(ROOT, "pbrt-v3-rs_amd", "pbrt_hip_render")
    scene = tmp_path / "s.pbrt"
    scene.write_text('LookAt 0 -4 1.2  0 0 0.4  0 0 1\nCamera "perspective" "float fov" 45\nFilm "image" "integer xresolution" 96 "integer yresolution" 64 "string filename" "o.pfm"\n'
                     'Sampler "halton" "integer pixelsamples" 4\nIntegrator "whitted" "integer maxdepth" 4\nWorldBegin\nLightSource "distant" "point from" [1 -2 4] "point to" [0 0 0] "rgb L" [1.5 1.4 1.3]\n'
                     'LightSource "point" "rgb I" [10 10 10] "point from" [0 -1 2.5]\nMaterial "matte" "rgb Kd" [0.6 0.5 0.4]\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -3 0 3 -3 0 3 3 0 -3 3 0]\n'
                     'Material "mirror" "rgb Kr" [0.9 0.85 0.8]\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 1.5 0 2 1.5 0 2 1.8 2 -2 1.8 2]\n'
                     'Material "glass" "rgb Kr" [0.9 0.9 1] "rgb Kt" [0.95 0.9 0.85] "float index" 1.5\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-0.8 -0.5 0.1 0.6 -0.7 0.1 0.6 -0.5 1.3 -0.8 -0.3 1.3]\nWorldEnd\n')
    digests = []
    for flags in (["--device", "0"], ["--devices", "0,0,0"]):
        out = tmp_path / ("a" + "".join(flags).replace(",", "_") + ".pfm")
        r = subprocess.run([exe, "--quiet", "--outfile", str(out)] + flags + [str(scene)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr
        digests.append(hashlib.sha256(out.read_bytes()).hexdigest())
        assert float(ds.read_pfm(str(out)).max()) > 0.05
    assert digests[0] == digests[1]
