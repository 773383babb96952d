"""not gpu: pbrt_hip_add_sphere_light as far as it can be checked without a device — the declaration, the export, the Python mirror — and the yardstick the device test of
scenes/lights/diffuse.pbrt relies on: the oracle's Whitted render in libm mode 1 (what the device computes) against the reference's own PNG."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import pbrt_hip
import reference_scenes as R
import sphere_light_scenes as SL
from oracle_binding import OracleScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_add_sphere_light_is_declared_and_exported(product):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    m = re.search(r"\bint\s+pbrt_hip_add_sphere_light\s*\(([^;]*)\)\s*;", header)
    assert m, "pbrt_hip_add_sphere_light is not declared in include/pbrt_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and args[0].startswith("PbrtHipScene") and args[-2].startswith("const float L_rgb") and args[-1] == "int two_sided", args
    assert hasattr(product.lib, "pbrt_hip_add_sphere_light")
    fp = C.POINTER(C.c_float)
    ident = np.eye(4, dtype=np.float32).ravel().ctypes.data_as(fp)
    L = np.ones(3, np.float32).ctypes.data_as(fp)
    f = product.fn("add_sphere_light")
    assert f(None, ident, ident, C.c_float(1), C.c_float(-1), C.c_float(1), C.c_float(360), 0, 0, L, 0) != pbrt_hip.OK   # a null handle is an error, not a crash
    assert f(None, None, None, C.c_float(1), C.c_float(-1), C.c_float(1), C.c_float(360), 0, 0, None, 0) != pbrt_hip.OK


def test_python_mirror_names_its_arguments_as_add_sphere_does():
    sphere = list(inspect.signature(pbrt_hip.Scene.add_sphere).parameters.values())
    light = list(inspect.signature(pbrt_hip.Scene.add_sphere_light).parameters.values())
    assert [p.name for p in light] == [p.name for p in sphere] + ["L", "two_sided"]
    assert [p.default for p in light[:len(sphere)]] == [p.default for p in sphere]
    assert light[-1].default is False


def test_mode1_oracle_whitted_reproduces_the_references_render_of_lights_diffuse(host):
    """The oracle in libm mode 1 — the mode the device equals bit for bit — at the reference's 400 x 400 and 128 spp, depth 5, against renders/lights/diffuse.png.  Measured:
    identical pixels 1.0, within one level 1.0, largest difference 0.  So the thresholds of test_oracle_whitted_reproduces_the_references_render_pixel_for_pixel (glibc mode)
    hold in mode 1 as they stand, and the device test asserts them unchanged."""
    with OracleScene() as s:
        info = SL.capture(lambda sc, h: SL.lights_diffuse(sc, h, spp=128, res=400), s, host)
        xyz, wt, st = SL.oracle_whitted(s, max_depth=info["max_depth"])
        rgb = s.film_to_rgb(xyz, wt)
    assert st.shadow_rays > 0
    d = np.abs(R.to_8bit(rgb).astype(np.int32) - R.reference_render(info["render"]).astype(np.int32)).max(-1)
    same, le1, dmax = (d == 0).mean(), (d <= 1).mean(), d.max()
    print("lights_diffuse, mode 1", same, le1, dmax)
    assert same >= 0.999 and le1 >= 0.9999 and dmax <= 6, (same, le1, dmax)
