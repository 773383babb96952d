"""CPU tests of the Whitted integrator's interfaces: the C entry point is declared and exported, and the front end accepts `Integrator "whitted"` (whitted.rs:121-150) in
--check mode while every other integrator name stays refused."""
import ctypes as C
import json
import os
import re
import subprocess

import driver_scene as ds
import pbrt_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = ('Integrator "{name}" "integer maxdepth" 3\nSampler "halton" "integer pixelsamples" 4\nFilm "image" "string filename" "x.pfm" "integer xresolution" [32] "integer yresolution" [24]\n'
         'WorldBegin\nLightSource "point" "rgb I" [1 1 1]\nMaterial "glass"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\nWorldEnd\n')


def check(tmp_path, text):
    path = tmp_path / "scene.pbrt"
    path.write_text(text)
    return subprocess.run([ds.RENDER_BIN, "--check", "--quiet", str(path)], capture_output=True, text=True, timeout=120)


def test_render_whitted_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    m = re.search(r"int pbrt_hip_render_whitted\(([^;]*)\);", header)
    assert m, "pbrt_hip_render_whitted is not declared in include/pbrt_hip.h"
    args = " ".join(m.group(1).split())
    assert args == "PbrtHipScene*, int max_depth, const int pixel_bounds[4], int tile_size, int tile_part, int tile_parts, float* out_xyz, float* out_weight, PbrtHipStats* out_stats"
    assert "whitted.rs" in header and "sampler_integrator.rs" in header
    lib = C.CDLL(pbrt_hip.LIB_PATH)
    assert hasattr(lib, "pbrt_hip_render_whitted")
    assert pbrt_hip.default_binding().has("render_whitted")
    assert hasattr(pbrt_hip.Scene, "render_whitted")


def test_front_end_accepts_whitted(tmp_path):
    r = check(tmp_path, SCENE.format(name="whitted"))
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["integrator"] == "whitted" and info["max_depth"] == 3
    r = check(tmp_path, SCENE.format(name="whitted").replace(' "integer maxdepth" 3', ""))
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["max_depth"] == 5     # whitted.rs: "maxdepth" defaults to 5
    r = check(tmp_path, SCENE.format(name="path"))
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["integrator"] == "path"


def test_front_end_still_refuses_other_integrators(tmp_path):
    r = check(tmp_path, SCENE.format(name="bdpt"))
    assert r.returncode == 1
    assert 'Integrator "bdpt" is outside the hot-path scope (supported: path, whitted)' in r.stderr
