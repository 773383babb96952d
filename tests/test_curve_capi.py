"""pbrt_hip_add_curve and pbrt_hip_curve_probe_batch as far as they can be checked without a GPU (tests/test_curve_gpu.py holds the refusals that need a handle): the symbols,
their behaviour on null arguments, and the plain header behind add_curve (csrc/curve_host.h) under the sanitizers through its stand-alone checker."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pbrt_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calls_are_declared_and_exported(product):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    for name in ("pbrt_hip_add_curve", "pbrt_hip_curve_probe_batch"):
        assert re.search(r"\bint\s+%s\s*\(\s*PbrtHipScene\s*\*" % name, header), name
        assert hasattr(product.lib, name), name
    decl = header[header.index("int pbrt_hip_add_curve"):]
    assert "int type, const float cp[12], const float width[2], const float* n" in decl and "int split_depth, uint32_t material_id, uint32_t flags" in decl
    assert "curve.rs" in header[header.index("Curve::create_segments"):header.index("int pbrt_hip_add_curve")]     # cites the reference lines it replaces
    assert "b0 = u, b1 = v" in header[:header.index("} PbrtHipHit;")]
    assert callable(pbrt_hip.Scene.add_curve) and callable(pbrt_hip.Scene.curve_probe)


def test_null_arguments_are_errors_not_crashes(product):
    fp = C.POINTER(C.c_float)
    ident = np.eye(4, dtype=np.float32).ravel()
    m = ident.ctypes.data_as(fp)
    cp = np.zeros(12, np.float32).ctypes.data_as(fp); w = np.ones(2, np.float32).ctypes.data_as(fp)
    L = product.lib
    assert product.fn("scene_create")(0) is None    # no device here: the handle is NULL
    assert L.pbrt_hip_add_curve(None, m, m, 0, cp, w, None, 3, 0, 0) != pbrt_hip.OK
    assert L.pbrt_hip_add_curve(None, None, None, 9, None, None, None, -1, 0, 0) != pbrt_hip.OK
    out = np.zeros(20, np.float32)
    assert L.pbrt_hip_curve_probe_batch(None, 0, 0, C.c_uint64(0), None, out.ctypes.data_as(fp)) != pbrt_hip.OK
    assert L.pbrt_hip_curve_probe_batch(None, 0, 1, C.c_uint64(1), None, None) != pbrt_hip.OK


def test_curve_host_header_under_the_sanitizers(tmp_path):
    """scripts/curve_host_check.cpp: CurveData::new, the segment ranges and bounds, and from_props' conversion, compiled with -fsanitize=address,undefined, against values worked out
    by hand in the checker itself; a non-zero exit or a sanitizer report fails"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "curve_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "pbrt-v3-rs_amd", "csrc"), os.path.join(ROOT, "scripts", "curve_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "curve_host_check: ok" in r.stdout
