"""CPU tests of `pbrt_hip_render --quadrics` in --check mode (no GPU is touched, nothing is rendered): the reference's own scene files that hold quadric shapes
(tests/golden/ref_scenes/, copied byte for byte by tests/golden/make_ref_scenes.py) are read and counted; without the option they are refused as before, with the option named;
and what the library would refuse at a call that check mode never makes is refused by the front end itself."""
import json
import os
import subprocess

import pytest

import driver_scene as ds

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_scenes")
SIX_SHAPES = ["constant", "uv", "2d-checkerboard", "bilerp", "dots", "fbm", "marble", "mix", "scale", "windy", "wrinkled"]
QUADRICS = ["sphere", "cylinder", "cone", "paraboloid", "disk", "hyperboloid"]
# file -> quadrics, triangles, lights, xres, yres, spp: each read off the file
COUNTS = {"textures/%s.pbrt" % n: (6, 2, 1, 400, 400, 128) for n in SIX_SHAPES}   # sphere, hyperboloid, cone, paraboloid, cylinder, disk, the wall, the sky
COUNTS.update({
    "materials/bump.pbrt": (1, 2, 2, 400, 400, 128),             # sphere; floor; sky + distant
    "lights/diffuse.pbrt": (1, 12 + 2, 1, 400, 400, 128),        # the sphere, which is the one light; geometry/cube.pbrt + the floor
    "textures/2d-mappings.pbrt": (4, 2, 1, 800, 400, 128),       # four hyperboloids; wall; sky
    "cameras/depth-of-field.pbrt": (5, 2, 2, 800, 400, 128),     # five spheres; floor; sky + distant
    "samplers/halton.pbrt": (1, 0, 2, 64, 64, 16),               # sphere; no mesh; sky + distant
})
FILES = sorted(COUNTS)
OLD_PHRASE = "is outside the hot-path scope"


def run(args):
    return subprocess.run([ds.RENDER_BIN] + args, capture_output=True, text=True, timeout=120)


def check(tmp_path, text, *flags):
    p = tmp_path / "s.pbrt"
    p.write_text(text)
    r = run(["--check"] + list(flags) + [str(p)])
    return r, (json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None)


@pytest.mark.parametrize("name", FILES)
def test_fixture_scene_counts(name):
    r = run(["--check", "--quadrics", "--quiet", os.path.join(SCENES, name)])
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    q, t, l, xres, yres, spp = COUNTS[name]
    assert (info["quadrics"], info["triangles"], info["lights"], info["instances"]) == (q, t, l, 0), info
    assert (info["xres"], info["yres"], info["spp"]) == (xres, yres, spp), info
    assert info["integrator"] == "whitted" and info["max_depth"] == 5, info


@pytest.mark.parametrize("name", FILES)
def test_fixture_scene_is_refused_without_the_option(name):
    r = run(["--check", "--quiet", os.path.join(SCENES, name)])
    assert r.returncode == 1
    assert OLD_PHRASE in r.stderr and "--quadrics" in r.stderr, r.stderr


def test_only_the_six_quadric_names_are_pointed_to_the_option(tmp_path):
    for shape in QUADRICS:
        r, _ = check(tmp_path, 'WorldBegin\nShape "%s"\nWorldEnd\n' % shape)
        assert r.returncode == 1 and 'Shape "%s" %s' % (shape, OLD_PHRASE) in r.stderr and "--quadrics" in r.stderr, r.stderr
    for shape in ("loopsubdiv", "curve", "nurbs", "heightfield"):
        for flags in ((), ("--quadrics",)):
            r, _ = check(tmp_path, 'WorldBegin\nShape "%s"\nWorldEnd\n' % shape, *flags)
            assert r.returncode == 1 and 'Shape "%s" %s' % (shape, OLD_PHRASE) in r.stderr and "--quadrics" not in r.stderr, r.stderr


def test_bare_directives(tmp_path):
    r, info = check(tmp_path, 'Integrator "whitted"\nWorldBegin\nLightSource "infinite"\n' + "".join('Shape "%s"\n' % q for q in QUADRICS) + "WorldEnd\n", "--quadrics")
    assert r.returncode == 0, r.stderr
    assert info["quadrics"] == 6 and info["triangles"] == 0 and info["lights"] == 1 and info["warnings"] == 0, info


def test_meshes_and_instances_are_counted_as_before(tmp_path):
    tri = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\n'
    text = 'WorldBegin\nLightSource "infinite"\nObjectBegin "a"\n' + tri + 'ObjectEnd\nObjectInstance "a"\nShape "disk"\n' + tri + "WorldEnd\n"
    r, info = check(tmp_path, text, "--quadrics")
    assert r.returncode == 0, r.stderr
    assert (info["quadrics"], info["triangles"], info["instances"], info["lights"]) == (1, 2, 1, 1), info
    r, info = check(tmp_path, 'WorldBegin\nLightSource "infinite"\n' + tri + "WorldEnd\n", "--quadrics")   # a scene without quadrics says so
    assert r.returncode == 0 and info["quadrics"] == 0 and info["triangles"] == 1, (r.stderr, info)
    r, info = check(tmp_path, 'WorldBegin\nLightSource "infinite"\n' + tri + "WorldEnd\n")
    assert r.returncode == 0 and info["quadrics"] == 0, (r.stderr, info)


@pytest.mark.parametrize("shape", QUADRICS)
def test_quadric_inside_an_object_definition_is_refused(tmp_path, shape):
    r, _ = check(tmp_path, 'Integrator "whitted"\nWorldBegin\nLightSource "infinite"\nObjectBegin "a"\nShape "%s"\nObjectEnd\nObjectInstance "a"\nWorldEnd\n' % shape, "--quadrics")
    assert r.returncode == 1
    assert 'Shape "%s"' % shape in r.stderr and "ObjectBegin" in r.stderr and "not supported" in r.stderr, r.stderr


@pytest.mark.parametrize("shape", [q for q in QUADRICS if q != "sphere"])
def test_area_light_on_the_other_five_quadrics_is_refused(tmp_path, shape):
    r, _ = check(tmp_path, 'Integrator "whitted"\nWorldBegin\nAreaLightSource "diffuse" "rgb L" [2 2 2]\nShape "%s"\nWorldEnd\n' % shape, "--quadrics")
    assert r.returncode == 1
    assert "AreaLightSource" in r.stderr and 'Shape "%s"' % shape in r.stderr and "only the sphere" in r.stderr, r.stderr
    # an AttributeEnd takes the area light out of force: the same shape is then ordinary geometry
    r, info = check(tmp_path, 'Integrator "whitted"\nWorldBegin\nLightSource "infinite"\nAttributeBegin\nAreaLightSource "diffuse"\nAttributeEnd\nShape "%s"\nWorldEnd\n' % shape, "--quadrics")
    assert r.returncode == 0 and info["quadrics"] == 1 and info["lights"] == 1, (r.stderr, info)


def test_sphere_light_counts_as_one_light_and_needs_whitted(tmp_path):
    world = 'WorldBegin\nLightSource "distant"\nAreaLightSource "diffuse" "rgb L" [2 2 2] "rgb scale" [3 3 3] "bool twosided" "true"\nShape "sphere" "float radius" 0.5\nWorldEnd\n'
    r, info = check(tmp_path, 'Integrator "whitted"\n' + world, "--quadrics")
    assert r.returncode == 0, r.stderr
    assert (info["quadrics"], info["lights"], info["triangles"]) == (1, 2, 0), info
    for head in ('Integrator "path"\n', ""):   # "path" is also what a file without the directive gets
        r, _ = check(tmp_path, head + world, "--quadrics")
        assert r.returncode == 1
        assert "sphere light" in r.stderr and "whitted" in r.stderr, r.stderr
    r, _ = check(tmp_path, 'Integrator "whitted"\nWorldBegin\nAreaLightSource "laser"\nShape "sphere"\nWorldEnd\n', "--quadrics")
    assert r.returncode == 1 and 'AreaLightSource "laser" unknown' in r.stderr, r.stderr


def test_alpha_on_a_quadric_is_ignored_with_a_warning(tmp_path):
    text = 'Integrator "whitted"\nWorldBegin\nLightSource "infinite"\nTexture "a" "float" "constant" "float value" 0\nShape "sphere" "float alpha" 0\nShape "disk" "texture shadowalpha" "a"\nWorldEnd\n'
    r, info = check(tmp_path, text, "--quadrics")
    assert r.returncode == 0, r.stderr
    assert info["quadrics"] == 2 and info["warnings"] >= 2, info
    assert "'alpha'" in r.stderr and "'shadowalpha'" in r.stderr, r.stderr


def test_material_errors_reach_a_quadric_as_they_reach_a_mesh(tmp_path):
    """The effective material is made by the code meshes use: a shape parameter overrides the material's, and an out-of-scope material is an error, not a different image"""
    r, _ = check(tmp_path, 'WorldBegin\nMaterial "kdsubsurface"\nShape "cone"\nWorldEnd\n', "--quadrics")
    assert r.returncode == 1 and 'Material "kdsubsurface"' in r.stderr, r.stderr
    r, _ = check(tmp_path, 'WorldBegin\nTexture "c" "color" "ptex"\nMaterial "matte"\nShape "cylinder" "texture Kd" "c"\nWorldEnd\n', "--quadrics")
    assert r.returncode == 1 and "ptex" in r.stderr, r.stderr
    r, info = check(tmp_path, 'WorldBegin\nLightSource "infinite"\nMaterial "matte"\nShape "cylinder" "rgb Kd" [0.1 0.2 0.3]\nWorldEnd\n', "--quadrics")
    assert r.returncode == 0 and info["quadrics"] == 1, r.stderr


def test_usage_names_the_option():
    r = run(["--help"])
    assert r.returncode == 0 and "--quadrics" in r.stderr
