"""`pbrt_hip_render --quadrics --quadric-lights`: Shape "disk" / "cylinder" under AreaLightSource "diffuse" is an area light.  The --check tests need no GPU (check mode calls
nothing in the library, so the front end refuses by itself what the library would); the two tests marked gpu render a scene file with a disk and a cylinder light and compare
the image, bit for bit, with the same scene built call by call through the C ABI."""
import os

import numpy as np
import pytest

import pbrt_hip
import quadric_light_scenes as QS
from test_front_end_quadrics import OLD_PHRASE, SCENES, check, run

LIGHT = 'AreaLightSource "diffuse" "rgb L" [2 2 2] "rgb scale" [3 3 3] "bool twosided" "true"\n'
FLAGS = ("--quadrics", "--quadric-lights")


@pytest.mark.parametrize("integrator", ["whitted", "path", None])
@pytest.mark.parametrize("shape", ["disk", "cylinder"])
def test_disk_and_cylinder_lights_count_as_lights_under_both_integrators(tmp_path, shape, integrator):
    head = "" if integrator is None else 'Integrator "%s"\n' % integrator   # a file without the directive gets "path"
    world = 'WorldBegin\nLightSource "distant"\nAttributeBegin\nReverseOrientation\nScale -1 2 1\n' + LIGHT + 'Shape "%s" "float radius" 0.5 "float phimax" 200\nAttributeEnd\nShape "%s"\nWorldEnd\n' % (shape, shape)
    r, info = check(tmp_path, head + world, *FLAGS)
    assert r.returncode == 0, r.stderr
    assert (info["quadrics"], info["lights"], info["triangles"]) == (2, 2, 0), info   # the second shape stands outside the attribute block: plain geometry
    assert info["integrator"] == (integrator or "path")


@pytest.mark.parametrize("shape", ["cone", "paraboloid", "hyperboloid"])
def test_the_shapes_without_a_sample_stay_refused(tmp_path, shape):
    r, _ = check(tmp_path, 'Integrator "whitted"\nWorldBegin\n' + LIGHT + 'Shape "%s"\nWorldEnd\n' % shape, *FLAGS)
    assert r.returncode == 1
    assert "AreaLightSource" in r.stderr and 'Shape "%s"' % shape in r.stderr and "Shape::sample" in r.stderr and "todo!()" in r.stderr, r.stderr
    r, info = check(tmp_path, 'Integrator "whitted"\nWorldBegin\nLightSource "infinite"\nShape "%s"\nWorldEnd\n' % shape, *FLAGS)   # as plain geometry it is read as before
    assert r.returncode == 0 and info["quadrics"] == 1 and info["lights"] == 1, (r.stderr, info)


@pytest.mark.parametrize("shape", ["disk", "cylinder", "cone"])
def test_without_the_option_only_the_sphere_is_a_light(tmp_path, shape):
    r, _ = check(tmp_path, 'Integrator "whitted"\nWorldBegin\n' + LIGHT + 'Shape "%s"\nWorldEnd\n' % shape, "--quadrics")
    assert r.returncode == 1 and "only the sphere" in r.stderr, r.stderr
    r, _ = check(tmp_path, 'Integrator "whitted"\nWorldBegin\n' + LIGHT + 'Shape "%s"\nWorldEnd\n' % shape, "--quadric-lights")   # effective together with --quadrics only
    assert r.returncode == 1 and OLD_PHRASE in r.stderr and "--quadrics" in r.stderr, r.stderr


def test_other_refusals_stay(tmp_path):
    r, _ = check(tmp_path, 'Integrator "whitted"\nWorldBegin\nAreaLightSource "laser"\nShape "disk"\nWorldEnd\n', *FLAGS)
    assert r.returncode == 1 and 'AreaLightSource "laser" unknown' in r.stderr, r.stderr
    r, _ = check(tmp_path, 'WorldBegin\nObjectBegin "a"\n' + LIGHT + 'Shape "disk"\nObjectEnd\nWorldEnd\n', *FLAGS)
    assert r.returncode == 1 and "ObjectBegin" in r.stderr, r.stderr
    # a sphere light next to a disk light: the path integrator still wants --path-sphere-lights for the sphere
    world = 'WorldBegin\n' + LIGHT + 'Shape "disk"\nShape "sphere"\nWorldEnd\n'
    r, _ = check(tmp_path, 'Integrator "path"\n' + world, *FLAGS)
    assert r.returncode == 1 and "sphere light" in r.stderr, r.stderr
    r, info = check(tmp_path, 'Integrator "path"\n' + world, "--path-sphere-lights", *FLAGS)
    assert r.returncode == 0 and info["lights"] == 2, (r.stderr, info)
    r, info = check(tmp_path, 'Integrator "whitted"\n' + world, *FLAGS)
    assert r.returncode == 0 and info["lights"] == 2, (r.stderr, info)


def test_usage_and_readme_name_the_option():
    r = run(["--help"])
    assert r.returncode == 0 and "--quadric-lights" in r.stderr
    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    assert "--quadric-lights" in readme


def _scene_file(tmp_path, integrator):
    from test_front_end_quadrics_gpu import fixture_tree
    scene = fixture_tree(tmp_path, "lights/diffuse.pbrt")
    scene.write_text(QS.front_end_scene_text(scene.read_text(), integrator))
    return scene


@pytest.mark.parametrize("integrator", ["whitted", "path"])
def test_check_reads_the_scene_the_gpu_test_renders(tmp_path, integrator):
    r = run(["--check", "--quiet", *FLAGS, str(_scene_file(tmp_path, integrator))])
    assert r.returncode == 0, r.stderr
    import json
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert (info["quadrics"], info["lights"], info["triangles"], info["xres"], info["spp"], info["integrator"]) == (2, 2, 14, 64, 8, integrator), info


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["whitted", "path"])
def test_scene_file_equals_the_c_abi_build_bit_for_bit(tmp_path, host, integrator):
    from test_front_end_quadrics_gpu import assert_same_bits, render
    got = render(tmp_path, _scene_file(tmp_path, integrator), "--quadric-lights")
    with pbrt_hip.Scene() as s:
        QS.front_end_scene_abi(s, host)
        xyz, wt, _ = s.render_whitted(max_depth=5) if integrator == "whitted" else s.render_path(max_depth=5)   # the directives' defaults
        assert_same_bits(got, np.ascontiguousarray(s.film_to_rgb(xyz, wt), np.float32), "disk and cylinder lights under " + integrator)


@pytest.mark.gpu
def test_scene_file_on_two_contexts(tmp_path):
    from test_front_end_quadrics_gpu import assert_same_bits, render
    scene = _scene_file(tmp_path, "path")
    one = render(tmp_path, scene, "--quadric-lights")
    assert_same_bits(render(tmp_path, scene, "--quadric-lights", "--devices", "0,0"), one, "--devices 0,0")
