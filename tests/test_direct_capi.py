"""CPU tests of the direct-lighting integrator's interfaces: the three C entry points are declared, exported and mirrored in the binding, and the front end accepts
`Integrator "directlighting"` (direct_lighting.rs:169-213: "maxdepth" 5, "strategy" all / one, anything else a warning and all) in --check mode, reports the strategy for this
integrator alone, refuses a sphere light without --path-sphere-lights, and keeps refusing every other integrator name in the words tests/test_whitted_capi.py pins."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import driver_scene as ds
import pbrt_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = ('Integrator "{name}"{params}\nSampler "halton" "integer pixelsamples" 4\nFilm "image" "string filename" "x.pfm" "integer xresolution" [32] "integer yresolution" [24]\n'
         'WorldBegin\nLightSource "point" "rgb I" [1 1 1]\nMaterial "glass"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\nWorldEnd\n')
SPHERE_LIGHT = ('Integrator "directlighting"\nSampler "halton" "integer pixelsamples" 4\nFilm "image" "string filename" "x.pfm" "integer xresolution" [32] "integer yresolution" [24]\n'
                'WorldBegin\nAttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\nShape "sphere" "float radius" 0.5\nAttributeEnd\n'
                'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\nWorldEnd\n')
HEAD = "PbrtHipScene*, int strategy, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts, "
SIGNATURES = {"render_direct": HEAD + "float* out_xyz, float* out_weight, PbrtHipStats* out_stats",
              "render_direct_devices": HEAD + "float* out_xyz, float* out_weight, PbrtHipStats* out_stats",
              "render_direct_tiles_device": HEAD + "void* d_tile_buffer, PbrtHipStats* out_stats"}


def check(tmp_path, text, *flags):
    path = tmp_path / "scene.pbrt"
    path.write_text(text)
    return subprocess.run([ds.RENDER_BIN, "--check", *flags, str(path)], capture_output=True, text=True, timeout=120)


def info_of(r):
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_entry_is_declared_exported_and_mirrored(name):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    m = re.search(r"int pbrt_hip_%s\(([^;]*)\);" % name, header)
    assert m, f"pbrt_hip_{name} is not declared in include/pbrt_hip.h"
    assert " ".join(m.group(1).split()) == SIGNATURES[name]
    assert "direct_lighting.rs:110-166" in header and "common.rs:22-78" in header and "common.rs:89-133" in header and "common.rs:146-299" in header
    assert hasattr(C.CDLL(pbrt_hip.LIB_PATH), "pbrt_hip_" + name)
    assert pbrt_hip.default_binding().has(name)
    assert hasattr(pbrt_hip.Scene, name)


def test_front_end_accepts_directlighting_with_the_references_defaults(tmp_path):
    info = info_of(check(tmp_path, SCENE.format(name="directlighting", params=""), "--quiet"))
    assert (info["integrator"], info["max_depth"], info["strategy"], info["warnings"]) == ("directlighting", 5, "all", 0)
    info = info_of(check(tmp_path, SCENE.format(name="directlighting", params=' "integer maxdepth" 3 "string strategy" "one"'), "--quiet"))
    assert (info["integrator"], info["max_depth"], info["strategy"], info["warnings"]) == ("directlighting", 3, "one", 0)
    info = info_of(check(tmp_path, SCENE.format(name="directlighting", params=' "string strategy" "all" "integer pixelbounds" [2 3 20 10]'), "--quiet"))
    assert info["strategy"] == "all" and info["pixel_bounds"] == [2, 3, 20, 10]


def test_the_strategy_key_belongs_to_this_integrator_alone(tmp_path):
    for name in ("path", "whitted"):
        info = info_of(check(tmp_path, SCENE.format(name=name, params=""), "--quiet"))
        assert info["integrator"] == name and "strategy" not in info


def test_an_unknown_strategy_warns_once_and_means_all(tmp_path):
    r = check(tmp_path, SCENE.format(name="directlighting", params=' "string strategy" "most"'))
    info = info_of(r)
    assert info["strategy"] == "all" and info["warnings"] == 1
    assert r.stderr.count("Strategy 'most' for direct lighting unknown. Using 'all'.") == 1


def test_front_end_still_refuses_other_integrators_in_the_old_words(tmp_path):
    r = check(tmp_path, SCENE.format(name="bdpt", params=""), "--quiet")
    assert r.returncode == 1
    assert 'Integrator "bdpt" is outside the hot-path scope (supported: path, whitted)' in r.stderr
    assert "directlighting" in r.stderr.split("(supported: path, whitted)")[1]


def test_a_sphere_light_needs_the_switch(tmp_path):
    r = check(tmp_path, SPHERE_LIGHT, "--quiet", "--quadrics")
    assert r.returncode == 1
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and "sphere light" in lines[0] and '"directlighting"' in lines[0] and "--path-sphere-lights" in lines[0], r.stderr
    info = info_of(check(tmp_path, SPHERE_LIGHT, "--quiet", "--quadrics", "--path-sphere-lights"))
    assert info["integrator"] == "directlighting" and info["lights"] == 1
