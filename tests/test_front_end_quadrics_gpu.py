"""-m gpu: `pbrt_hip_render --quadrics` renders the reference's own scene files that hold quadric shapes (tests/golden/ref_scenes/).  The image it writes is, bit for bit, the
film of the same scene built call by call through the C ABI by the builders the other GPU tests use (tests/reference_scenes.py, tests/sphere_light_scenes.py): the front end adds
parameter reading, the CTM, orientation, the material override and the order of the calls, nothing numerical.  At the files' own sample counts the image is the reference's PNG
within the thresholds the C-ABI tests assert for the same scenes.  Each test runs the binary once."""
import contextlib
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

import driver_scene as ds
import pbrt_hip
import reference_scenes as R
import sphere_light_scenes as SL
from test_band_plan_cpu import REC
from test_front_end_quadrics import FILES, SCENES
from test_quadrics_gpu import generic_adders

pytestmark = pytest.mark.gpu
SPP = 8


def render(tmp_path, scene, *flags):
    """One run of the binary -> the PFM it wrote, top row first"""
    out = tmp_path / "out.pfm"
    r = subprocess.run([ds.RENDER_BIN, "--quadrics", "--quiet", "--outfile", str(out)] + list(flags) + [str(scene)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return ds.read_pfm(str(out))


def fixture_tree(tmp_path, name, spp=None):
    """The fixture tree, copied so that the Include and the image map resolve; `spp` replaces the file's pixelsamples (128 everywhere but samplers/halton.pbrt's 16)"""
    root = tmp_path / "scenes"
    shutil.copytree(SCENES, str(root))
    scene = root / name
    if spp is not None:
        text, n = re.subn(r'"integer pixelsamples" \d+', '"integer pixelsamples" %d' % spp, scene.read_text())
        assert n == 1
        scene.write_text(text)
    return scene


def build(s, host, name, spp, **kw):
    if name.startswith("textures/") and name != "textures/2d-mappings.pbrt": return R.textures_six_shapes(s, host, name[len("textures/"):-len(".pbrt")], spp=spp)
    if name == "textures/2d-mappings.pbrt": return R.textures_2d_mappings(s, host, spp=spp, **kw)
    if name == "cameras/depth-of-field.pbrt": return R.cameras_depth_of_field(s, host, spp=spp, **kw)
    if name == "materials/bump.pbrt": return R.materials_bump(s, host, spp=spp)
    if name == "samplers/halton.pbrt": return R.samplers_scene(s, host, "halton", spp=spp)
    if name == "lights/diffuse.pbrt": return SL.lights_diffuse(s, host, spp=spp)
    raise ValueError(name)


@contextlib.contextmanager
def blackbody_through_the_c_abi():
    """reference_scenes.blackbody takes the colour of `"blackbody L" [3000 1.5]` (the sun of cameras/depth-of-field.pbrt and materials/bump.pbrt) from
    tests/golden/blackbody_rgb.json, a numpy restatement that tests/test_host_driver.py holds to pbrt_hip_host_blackbody_rgb within 3e-6: the two differ in the last bits
    ((1.1025976, 0.52573085, 0.16947508) against (1.1025971, 0.52573097, 0.16947506)).  The front end has always made the colour with pbrt_hip_host_blackbody_rgb, as a host
    above the C ABI does, so with the JSON colour the sunlit pixels of these two scenes are one ulp apart (depth-of-field at 8 spp: 144408 pixels, at most 7.2e-7).  For the
    duration the builders get the C ABI's colour; nothing else about them changes, and the comparison stays bit for bit."""
    lib = pbrt_hip.default_binding().lib
    lib.pbrt_hip_host_blackbody_rgb.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]

    def blackbody(key):
        t, scale = (float(v) for v in key.split("x"))
        out = np.zeros(3, np.float32)
        lib.pbrt_hip_host_blackbody_rgb(t, scale, out.ctypes.data_as(C.POINTER(C.c_float)))
        return tuple(float(v) for v in out)
    saved = R.blackbody
    R.blackbody = blackbody
    try:
        yield
    finally:
        R.blackbody = saved


_abi_films = {}


def abi_film(host, name):
    """The scene at SPP samples through the C ABI, Integrator "whitted" at the files' default depth 5 -> RGB film; made once per scene"""
    if name not in _abi_films:
        with pbrt_hip.Scene() as s, generic_adders(), blackbody_through_the_c_abi():
            build(s, host, name, SPP)
            xyz, wt, _ = s.render_whitted(max_depth=5)
            _abi_films[name] = np.ascontiguousarray(s.film_to_rgb(xyz, wt), np.float32)
    return _abi_films[name]


def assert_same_bits(got, want, label):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    diff = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not diff.any(), (label, int(diff.sum()), float(np.abs(got - want).max()))
    assert float(want.max()) > 0.05, label


# ---- 1. the same bits as the C ABI -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FILES)
def test_fixture_scene_equals_the_c_abi_build_bit_for_bit(tmp_path, host, name):
    got = render(tmp_path, fixture_tree(tmp_path, name, SPP))
    assert_same_bits(got, abi_film(host, name), name)


def test_hlbvh_tree_of_a_quadric_scene(tmp_path, host):
    """Accelerator "bvh" "string splitmethod" "hlbvh" in front of lights/diffuse.pbrt: the front end has the device build that tree too (pbrt_hip_build_accel_device_shapes);
    the film is the one of the builder's host-built HLBVH tree"""
    scene = fixture_tree(tmp_path, "lights/diffuse.pbrt", SPP)
    text = scene.read_text()
    assert text.count("WorldBegin") == 1
    scene.write_text(text.replace("WorldBegin", 'Accelerator "bvh" "string splitmethod" "hlbvh"\nWorldBegin'))
    got = render(tmp_path, scene)
    with pbrt_hip.Scene() as s:
        SL.lights_diffuse(s, host, spp=SPP, split=1)
        xyz, wt, _ = s.render_whitted(max_depth=5)
        assert_same_bits(got, np.ascontiguousarray(s.film_to_rgb(xyz, wt), np.float32), "lights/diffuse.pbrt, hlbvh")


# ---- 2. defaults, orientation, partial shapes, the material override --------------------------------------------------------------------------------------------------
PROBE = '''LookAt 0 -15 7  0 0.5 0.5  0 0 1
Camera "perspective" "float fov" 42
Film "image" "integer xresolution" 64 "integer yresolution" 64 "string filename" "probe.pfm"
Sampler "halton" "integer pixelsamples" 4
Integrator "whitted"
WorldBegin
LightSource "infinite" "rgb L" [0.4 0.45 0.5]
LightSource "distant" "point from" [2 -3 5] "point to" [0 0 0] "rgb L" [2 1.9 1.8]
Material "matte" "rgb Kd" [0.6 0.5 0.4]
AttributeBegin
  Translate -4 0 1
  Shape "sphere"
AttributeEnd
AttributeBegin
  Translate -1.5 0 1
  Shape "cylinder"
AttributeEnd
AttributeBegin
  Translate 1 0 0
  Shape "cone"
AttributeEnd
AttributeBegin
  Translate 3.5 0 0
  Rotate 180 1 0 0
  Translate 0 0 -1
  Shape "paraboloid"
AttributeEnd
AttributeBegin
  Translate 4 -3 0.3
  Shape "disk"
AttributeEnd
AttributeBegin
  Translate 0 6 1
  Shape "hyperboloid"
AttributeEnd
AttributeBegin
  Translate -3.5 -4 1
  Rotate 40 1 0 0
  ReverseOrientation
  Material "glass" "rgb Kr" [0.3 0.3 0.3] "rgb Kt" [0.9 0.8 0.7] "float index" 1.4
  Shape "sphere" "float radius" 0.9 "float zmin" -0.5 "float zmax" 0.6 "float phimax" 250
AttributeEnd
AttributeBegin
  Translate -1 -4 0.6
  Scale 1 1 -1
  Material "glass" "rgb Kr" [0.3 0.3 0.3] "rgb Kt" [0.7 0.8 0.9] "float index" 1.4
  Shape "paraboloid" "float radius" 0.8 "float zmax" 0.9
AttributeEnd
AttributeBegin
  Translate 1.2 -4 0.5
  Rotate 25 0 1 0
  Shape "disk" "float radius" 1 "float innerradius" 0.45 "float height" 0.2 "float phimax" 300
AttributeEnd
AttributeBegin
  Translate 3.5 -6 1
  Material "matte" "rgb Kd" [0.9 0.9 0.9] "float sigma" 20
  Shape "cylinder" "rgb Kd" [0.1 0.7 0.2] "float radius" 0.7
AttributeEnd
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-9 -9 -0.01 9 -9 -0.01 9 9 -0.01 -9 9 -0.01]
WorldEnd
'''


def probe_through_the_c_abi(s, host):
    """PROBE call by call, with the reference's defaults written out (sphere.rs:503-506, cylinder.rs:360-363, cone.rs:330-332, paraboloid.rs:346-349, disk.rs:246-249,
    hyperboloid.rs:440-443)"""
    T, Rt, Sc = host.translate, host.rotate, host.scale
    s.add_light_infinite((0.4, 0.45, 0.5))
    s.add_light_distant((2.0, 1.9, 1.8), host.distant_direction(R._ident()[0], (2.0, -3.0, 5.0), (0.0, 0.0, 0.0)))
    m = s.add_material_matte((0.6, 0.5, 0.4))
    t = R.ctm(host, T((-4, 0, 1))); s.add_sphere(t[0], t[1], 1.0, -1.0, 1.0, 360.0, m)
    t = R.ctm(host, T((-1.5, 0, 1))); s.add_quadric("cylinder", t[0], t[1], 1.0, -1.0, 1.0, 360.0, m)
    t = R.ctm(host, T((1, 0, 0))); s.add_quadric("cone", t[0], t[1], 1.0, 1.0, 0.0, 360.0, m)
    t = R.ctm(host, T((3.5, 0, 0)), Rt(180, (1, 0, 0)), T((0, 0, -1))); s.add_quadric("paraboloid", t[0], t[1], 1.0, 0.0, 1.0, 360.0, m)
    t = R.ctm(host, T((4, -3, 0.3))); s.add_quadric("disk", t[0], t[1], 1.0, 0.0, 0.0, 360.0, m)
    t = R.ctm(host, T((0, 6, 1))); s.add_hyperboloid(t[0], t[1], (3.0, 1.2, 1.0), (1.0, -0.5, -1.0), 360.0, m)
    t = R.ctm(host, T((-3.5, -4, 1)), Rt(40, (1, 0, 0)))
    s.add_sphere(t[0], t[1], 0.9, -0.5, 0.6, 250.0, s.add_material_glass((0.3, 0.3, 0.3), (0.9, 0.8, 0.7), 0.0, 0.0, 1.4, True), reverse_orientation=True)
    t = R.ctm(host, T((-1, -4, 0.6)), Sc((1, 1, -1)))
    s.add_quadric("paraboloid", t[0], t[1], 0.8, 0.0, 0.9, 360.0, s.add_material_glass((0.3, 0.3, 0.3), (0.7, 0.8, 0.9), 0.0, 0.0, 1.4, True))
    t = R.ctm(host, T((1.2, -4, 0.5)), Rt(25, (0, 1, 0))); s.add_quadric("disk", t[0], t[1], 1.0, 0.2, 0.45, 300.0, m)
    t = R.ctm(host, T((3.5, -6, 1))); s.add_quadric("cylinder", t[0], t[1], 0.7, -1.0, 1.0, 360.0, s.add_material_matte((0.1, 0.7, 0.2), 20.0))   # the shape's Kd over the material's, whose sigma stays
    s.add_mesh(np.array([[-9, -9, -0.01], [9, -9, -0.01], [9, 9, -0.01], [-9, 9, -0.01]], np.float32), R.QUAD_IDX, m)
    R.camera_film(s, host, (0, -15, 7), (0, 0.5, 0.5), (0, 0, 1), 42.0, 64, 64, 4)
    s.build_accel(0, 4)


def test_defaults_orientation_partial_shapes_and_the_material_override(tmp_path, host):
    (tmp_path / "probe.pbrt").write_text(PROBE)
    got = render(tmp_path, tmp_path / "probe.pbrt")
    with pbrt_hip.Scene() as s:
        probe_through_the_c_abi(s, host)
        xyz, wt, st = s.render_whitted(max_depth=5)
        want = np.ascontiguousarray(s.film_to_rgb(xyz, wt), np.float32)
        assert st.regular_rays > st.camera_rays   # the glass shapes were met: the recursion ran, and with it the side of the surface a ray is on
        # every shape is in the picture: a wrong default on any of them moves pixels (dropping the glass sphere's reverse-orientation flag alone changes 72 of them)
        hit = s.intersect_batch(s.generate_camera_rays((0, 0, 64, 64), 0)[0])["prim"].reshape(-1)
        assert set(range(12)) <= set(int(p) for p in np.unique(hit)), np.unique(hit)   # each of the ten quadrics and both floor triangles is seen by a camera ray
    assert_same_bits(got, want, "probe")


# ---- 3. the reference's pixels -----------------------------------------------------------------------------------------------------------------------------------------
DOF_CROP = (0.25, 0.75, 0.3, 0.8)
PIXELS = [("samplers/halton.pbrt", "samplers_halton"), ("materials/bump.pbrt", "materials_bump"), ("textures/fbm.pbrt", "textures_fbm"), ("textures/2d-checkerboard.pbrt", "textures_2d-checkerboard"),
          ("textures/2d-mappings.pbrt", "textures_2d-mappings"), ("cameras/depth-of-field.pbrt", "cameras_depth-of-field"), ("lights/diffuse.pbrt", "lights_diffuse")]


@pytest.mark.parametrize("name,ref_name", PIXELS, ids=[r for _, r in PIXELS])
def test_front_end_reproduces_the_references_render_pixel_for_pixel(tmp_path, host, name, ref_name):
    """The files as they are, at their own 128 spp (halton: 16).  The thresholds are the ones tests/test_whitted_gpu.py (test_device_whitted_reproduces_the_references_render_pixel_for_pixel)
    and tests/test_sphere_light_gpu.py (..._render_of_lights_diffuse) assert for the same scenes built through the C ABI; those were measured on the mode-1 oracle against the
    reference's PNGs (the figures are in their docstrings), not on this code."""
    dof = name == "cameras/depth-of-field.pbrt"
    flags = ["--cropwindow"] + [str(v) for v in DOF_CROP] if dof else []
    mine = R.to_8bit(render(tmp_path, fixture_tree(tmp_path, name), *flags))
    ref = R.reference_render(ref_name)
    if dof:
        cb = [int(v) for v in host.film_box(800, 400, crop_window=DOF_CROP)[0]]
        ref = ref[cb[1]:cb[3], cb[0]:cb[2]]
    six = name.startswith("textures/") and name != "textures/2d-mappings.pbrt"
    if six and ref.shape[0] != 400:
        r0, r1, c0, c1 = R.TEX_CROP; mine = mine[r0:r1, c0:c1]
    assert mine.shape == ref.shape, (mine.shape, ref.shape)
    d = np.abs(mine.astype(np.int32) - ref.astype(np.int32)).max(-1)
    same, le1, dmax = (d == 0).mean(), (d <= 1).mean(), d.max()
    print(name, same, le1, dmax)
    if dof: assert same >= 0.999 and le1 >= 0.9999 and dmax <= 4, (same, le1, dmax)
    elif six or name == "textures/2d-mappings.pbrt": assert same >= 0.9995 and dmax <= 2, (same, dmax)
    else: assert same >= 0.999 and le1 >= 0.9999 and dmax <= 6, (same, le1, dmax)


# ---- 4. several devices and a budget -----------------------------------------------------------------------------------------------------------------------------------
BAND_TILES = 100   # of the 625 tiles of a 400 x 400 frame: seven bands on one device


@pytest.mark.parametrize("flags", [["--devices", "0,0,0"], ["--sample-record-budget", str(BAND_TILES * 256 * SPP * REC)],
                                   ["--devices", "0,0", "--sample-record-budget", str(BAND_TILES * 256 * SPP * REC)]], ids=["devices", "budget", "devices+budget"])
def test_six_shape_scene_on_several_devices_and_in_bands(tmp_path, host, flags):
    """Three contexts on one GPU, as tests/test_whitted_devices_gpu.py drives them; a budget of 100 tiles' records; both.  The same bits as the plain run, which
    test_fixture_scene_equals_the_c_abi_build_bit_for_bit holds to the C-ABI film compared against here."""
    name = "textures/mix.pbrt"
    assert 400 * 400 > 3 * BAND_TILES * 256   # more pixels than three bands hold, so than two devices' first bands
    got = render(tmp_path, fixture_tree(tmp_path, name, SPP), *flags)
    assert_same_bits(got, abi_film(host, name), name + " " + " ".join(flags))
