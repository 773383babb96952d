"""not gpu: pbrt_hip_render_whitted_devices and pbrt_hip_render_whitted_tiles_device as far as they can be checked without a device — the declarations, the exports, the Python
mirror and its defaults — and the front end's --check on a scene file with Integrator "whitted"."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import driver_scene as ds
import pbrt_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["PbrtHipScene*", "int max_depth", "const int pixel_bounds[4]", "int tile_size", "int tile_part", "int tile_parts"]


def _declared(name):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, name + " is not declared in include/pbrt_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_both_entries_are_declared_and_exported(product):
    assert _declared("pbrt_hip_render_whitted_devices") == _declared("pbrt_hip_render_whitted") == COMMON + ["float* out_xyz", "float* out_weight", "PbrtHipStats* out_stats"]
    assert _declared("pbrt_hip_render_whitted_tiles_device") == COMMON + ["void* d_tile_buffer", "PbrtHipStats* out_stats"]
    assert _declared("pbrt_hip_render_path_tiles_device")[-2:] == ["void* d_tile_buffer", "PbrtHipStats* out_stats"]   # the output convention the rank form shares
    for name in ("render_whitted_devices", "render_whitted_tiles_device"):
        assert hasattr(product.lib, "pbrt_hip_" + name) and product.has(name)
    pb = (C.c_int * 4)(0, 0, 1, 1)
    assert product.fn("render_whitted_devices")(None, 1, pb, 16, 0, 1, None, None, None) != pbrt_hip.OK   # a null handle is an error, not a crash
    assert product.fn("render_whitted_tiles_device")(None, 1, pb, 16, 0, 1, None, None) != pbrt_hip.OK


def test_python_mirror_has_both_methods_with_the_stated_defaults():
    want = [("max_depth", 5), ("pixel_bounds", None), ("tile_size", 16), ("tile_part", 0), ("tile_parts", 1)]
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()][1:]
    assert sig(pbrt_hip.Scene.render_whitted_devices) == want == sig(pbrt_hip.Scene.render_whitted)
    assert sig(pbrt_hip.Scene.render_whitted_tiles_device) == [("d_tile_buffer_ptr", inspect.Parameter.empty)] + want
    assert [n for n, _ in sig(pbrt_hip.Scene.render_path_tiles_device)][0] == "d_tile_buffer_ptr"


def test_front_end_check_still_reports_the_whitted_integrator(tmp_path):
    scene = tmp_path / "s.pbrt"
    scene.write_text('LookAt 0 -4 1  0 0 0  0 0 1\nCamera "perspective" "float fov" 40\nFilm "image" "integer xresolution" 32 "integer yresolution" 24 "string filename" "o.pfm"\n'
                     'Sampler "halton" "integer pixelsamples" 2\nIntegrator "whitted" "integer maxdepth" 3\nWorldBegin\nLightSource "point" "rgb I" [10 10 10] "point from" [0 -1 2]\n'
                     'Material "mirror"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 0 2 -2 0 2 2 0 -2 2 0]\nWorldEnd\n')
    r = subprocess.run([ds.RENDER_BIN, "--check", str(scene)], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stderr
    assert '"integrator": "whitted"' in r.stdout, r.stdout
    assert not (tmp_path / "o.pfm").exists()
