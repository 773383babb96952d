"""not gpu: spherical area lights under the path integrator (pbrt_hip_set_path_sphere_lights, pbrt_hip_sphere_light_probe_batch, `pbrt_hip_render --path-sphere-lights`) as far as
they can be checked without a device.
  1. the declarations, the exports, the Python mirror, a null handle, and the front end's --check with and without the option;
  2. tests/sphere_pdf_restatement.py (numpy float32) proven on the oracle: its inside predicate names the branch the oracle's Sphere::sample_solid_angle took on the probe case
     set, its cone value is that branch's pdf bit for bit, and its offset_origin gives the shadow-ray origins the oracle's probe reports bit for bit;
  3. the two closed forms of tests/path_sphere_light_scenes.py hold for the oracle's Whitted integrator — a correct estimator of direct light — under closed_form.assert_mean, and
     tell it from the oracle's path render (the light-sampled half alone), from twice the answer and from 0.  The yardstick is proven before the device is held to it."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import closed_form as CF
import driver_scene as ds
import light_probe_cases as LP
import path_sphere_light_scenes as PS
import pbrt_hip
import sphere_light_scenes as SL
import sphere_pdf_restatement as SP
from oracle_binding import OracleScene, set_libm_mode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _declared(name):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, name + " is not declared in include/pbrt_hip.h"
    return [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in m.group(1).split(",")]


# ---- 1. the interface -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_both_entries_are_declared_exported_and_mirrored(product):
    assert _declared("pbrt_hip_set_path_sphere_lights") == ["PbrtHipScene*", "int on"]
    assert _declared("pbrt_hip_sphere_light_probe_batch") == ["PbrtHipScene*", "uint32_t light", "int op", "uint64_t n", "const float* ref", "const float* u", "const float* wi", "float* out"]
    probe = _declared("pbrt_hip_light_probe_batch")
    assert [a for a in probe if a != "int variant"] == _declared("pbrt_hip_sphere_light_probe_batch")   # the older probe's inputs and output, without the variant
    for name in ("set_path_sphere_lights", "sphere_light_probe_batch"):
        assert hasattr(product.lib, "pbrt_hip_" + name) and product.has(name)
    assert product.fn("set_path_sphere_lights")(None, 1) == pbrt_hip.ERR_INVALID_ARG   # a null handle is an error, not a crash
    assert product.fn("sphere_light_probe_batch")(None, 0, 0, 0, None, None, None, None) == pbrt_hip.ERR_INVALID_ARG
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()][1:]
    assert sig(pbrt_hip.Scene.set_path_sphere_lights) == [("on", True)]
    assert sig(pbrt_hip.Scene.sphere_light_probe_batch) == [("light", inspect.Parameter.empty), ("op", inspect.Parameter.empty), ("ref", inspect.Parameter.empty), ("u", None), ("wi", None)]


WORLD = 'WorldBegin\nLightSource "distant"\nAreaLightSource "diffuse" "rgb L" [2 2 2] "bool twosided" "true"\nShape "sphere" "float radius" 0.5\nWorldEnd\n'


def _check(tmp_path, text, *flags):
    p = tmp_path / "s.pbrt"
    p.write_text(text)
    r = subprocess.run([ds.RENDER_BIN, "--check"] + list(flags) + [str(p)], capture_output=True, text=True, timeout=120)
    return r, (json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None)


@pytest.mark.parametrize("head", ['Integrator "path"\n', 'Integrator "path" "integer maxdepth" 3 "string lightsamplestrategy" "uniform"\n', ""], ids=["path", "path_uniform", "no_directive"])
def test_front_end_check_accepts_a_sphere_light_under_path_with_the_option(tmp_path, head):
    r, info = _check(tmp_path, head + WORLD, "--quadrics", "--path-sphere-lights")
    assert r.returncode == 0, r.stderr
    assert info["integrator"] == "path" and (info["quadrics"], info["lights"], info["triangles"]) == (1, 2, 0), info
    r, _ = _check(tmp_path, head + WORLD, "--quadrics")   # without it: the old sentence, which now names the option
    assert r.returncode == 1
    assert "sphere light" in r.stderr and "whitted" in r.stderr and "--path-sphere-lights" in r.stderr, r.stderr
    r, _ = _check(tmp_path, head + WORLD, "--path-sphere-lights")   # the option does not read quadrics by itself
    assert r.returncode == 1 and "--quadrics" in r.stderr, r.stderr


def test_the_option_changes_nothing_else(tmp_path):
    r, info = _check(tmp_path, 'Integrator "whitted"\n' + WORLD, "--quadrics", "--path-sphere-lights")
    assert r.returncode == 0 and info["integrator"] == "whitted", (r.stderr, info)
    tri = 'WorldBegin\nLightSource "infinite"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\nWorldEnd\n'
    a, ia = _check(tmp_path, tri)
    b, ib = _check(tmp_path, tri, "--path-sphere-lights")
    assert a.returncode == b.returncode == 0 and ia == ib
    h = subprocess.run([ds.RENDER_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--path-sphere-lights" in h.stderr


# ---- 2. the restatement, on the oracle --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_oracle(host):
    orc = OracleScene()
    PS.build_probe_lights(orc, host)
    yield orc
    orc.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("k", range(len(PS.PROBE_LIGHTS)), ids=[p[0] for p in PS.PROBE_LIGHTS])
def test_restatement_names_the_oracles_branch_and_reproduces_its_origins(host, probe_oracle, k):
    name, steps, radius = PS.PROBE_LIGHTS[k][:3]
    ref, wi, u = PS.probe_cases(host, k)
    centre = SP.centre_of(PS.probe_transform(host, k)[0])
    set_libm_mode(1)
    try:
        out = probe_oracle.light_probe_batch(k, 0, ref, u, wi, variant=2)   # Sphere::sample_solid_angle behind DiffuseAreaLight::sample_li
    finally:
        set_libm_mode(0)
    inside = SP.is_inside(ref, centre, radius)
    cone = SP.sampled_cone_pdf(ref, centre, radius)   # sample_solid_angle's own spelling of uniform_cone_pdf's argument
    valid = out[:, LP.VALID] == 1.0
    assert inside.sum() >= 40 and (~inside).sum() >= 60 and valid.sum() >= 0.8 * len(ref), (name, int(inside.sum()), int(valid.sum()))
    # outside: the sample's pdf is uniform_cone_pdf — the restated value, bit for bit, whatever u was (infinity where cos_theta_max rounded to 1)
    o = valid & ~inside
    assert np.array_equal(_bits(out[o, LP.PDF]), _bits(cone[o])), (name, int((_bits(out[o, LP.PDF]) != _bits(cone[o])).sum()))
    # ... and Sphere::pdf_solid_angle's spelling (radius^2 / distance^2) is the same number up to the last bits of cos_theta_max
    pdf_li = SP.cone_pdf(ref, centre, radius)
    fin = ~inside & np.isfinite(cone) & np.isfinite(pdf_li)
    big = fin & (cone < 1e3)   # (1 - cos_theta_max loses its bits as the cone closes: the two spellings agree to 1e-6 only while it is wide)
    assert np.allclose(pdf_li[big], cone[big], rtol=1e-3), name
    assert np.isinf(pdf_li[~inside]).any(), name   # the case set reaches the rounding
    # inside: the area pdf turned into a solid-angle one at the sampled point — 1 / area * distance^2 / |n . -wi| of the point and normal the probe reports
    i = valid & inside
    area = PS.probe_light_area(k)
    with np.errstate(all="ignore"):
        want = (F(1) / area) * (SP.distance_squared(ref[i, 0:3], out[i, LP.VP]) / np.abs(SP.dot(out[i, LP.VN], -out[i, LP.WI])))
    assert np.allclose(out[i, LP.PDF], want, rtol=2e-5, atol=0.0), name   # (wi is renormalised between the two: not a bit-level statement)
    same_as_cone = _bits(out[i, LP.PDF]) == _bits(cone[i])
    assert same_as_cone.mean() < 0.05, (name, float(same_as_cone.mean()))
    # offset_origin: the shadow ray's origin is offset_origin(p, p_error, n, vp - p), where spawn_ray(hit, wi) uses offset_origin(p, p_error, n, wi)
    got = SP.offset_origin(ref[valid, 0:3], ref[valid, 3:6], ref[valid, 6:9], out[valid, LP.VP] - ref[valid, 0:3])
    assert np.array_equal(_bits(got), _bits(out[valid, LP.RO])), name


def test_first_three_probe_lights_share_their_cases(host):
    a, b, c = (PS.probe_cases(host, k) for k in range(3))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z))


# ---- 3. the closed forms, on the oracle's Whitted integrator ---------------------------------------------------------------------------------------------------------------
RES, SPP = 32, 64


def test_outside_closed_form_holds_for_the_oracles_whitted(host):
    with OracleScene() as orc:
        PS.outside_scene(host, RES, SPP)(orc)
        expect = PS.outside_pixel_expect(orc, RES)
        xyz, wt, _ = SL.oracle_whitted(orc, max_depth=1)
        ratio = orc.film_to_rgb(xyz, wt).astype(np.float64) / expect
        xyz, wt, _ = PS.oracle_path(orc, max_depth=1, light_strategy=0)
        half = CF.frame_stats(orc.film_to_rgb(xyz, wt).astype(np.float64) / expect)[0]
    mean, se = CF.assert_mean(ratio, 1.0, se_target=PS.SE_TARGET, wrongs=PS.wrongs_from(half, 1.0), label="outside, oracle Whitted")
    print("outside, oracle Whitted: ratio", mean, "se", se, "; oracle path (light half only):", half)
    assert np.all(half < 1.0)


@pytest.mark.parametrize("two_sided", [False, True], ids=["reversed", "two_sided"])
def test_inside_closed_form_holds_for_the_oracles_whitted(host, two_sided):
    with OracleScene() as orc:
        PS.inside_scene(host, two_sided, RES, SPP)(orc)
        xyz, wt, _ = SL.oracle_whitted(orc, max_depth=1)
        rgb = orc.film_to_rgb(xyz, wt)
        xyz, wt, _ = PS.oracle_path(orc, max_depth=1, light_strategy=0)
        half = CF.frame_stats(orc.film_to_rgb(xyz, wt))[0]
    mean, se = CF.assert_mean(rgb, PS.INSIDE_EXPECT, se_target=PS.SE_TARGET, wrongs=PS.wrongs_from(half, PS.INSIDE_EXPECT), label="inside, oracle Whitted")
    print("inside, oracle Whitted: mean", mean, "se", se, "; oracle path (light half only):", half)
    assert np.all(half < 0.5 * PS.INSIDE_EXPECT)
