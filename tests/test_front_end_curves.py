"""CPU tests of `pbrt_hip_render --curves` in --check mode (no GPU is touched, nothing is rendered): Shape "curve" is read as Curve::from_props reads it
(shapes/src/curve.rs:149-316) and its Curve segments are counted — 2^splitdepth per cubic Bezier segment —; every place where from_props panics is one sentence; without
the option the directive is refused with the sentence it always had; and the reference's shape showcase, scenes/shapes/all-shapes.pbrt with only its loopsubdiv block
removed (tests/golden/ref_scenes/shapes/all-shapes.pbrt), checks clean."""
import json
import os
import subprocess

import pytest

import driver_scene as ds

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ref_scenes", "shapes", "all-shapes.pbrt")
OLD_PHRASE = "is outside the hot-path scope"
P4 = "-1 0 0  0 1 0  1 -1 0  2 0 0"
P7 = P4 + "  3 1 0  4 -1 0  5 0 0"


def run(args):
    return subprocess.run([ds.RENDER_BIN] + args, capture_output=True, text=True, timeout=120)


def check(tmp_path, body, *flags, world=True):
    p = tmp_path / "s.pbrt"
    p.write_text(('WorldBegin\nLightSource "infinite"\n' + body + "\nWorldEnd\n") if world else body)
    r = run(["--check"] + list(flags) + [str(p)])
    return r, (json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None)


def curve(params):
    return 'Shape "curve" ' + params


@pytest.mark.parametrize("params,segments", [
    ('"point P" [%s]' % P4, 8),                                                          # one cubic Bezier, default splitdepth 3
    ('"point P" [%s] "integer splitdepth" 0' % P4, 1),
    ('"point P" [%s] "float splitdepth" 2' % P4, 4),                                     # read as a float first (:228)
    ('"point P" [%s] "float splitdepth" 2.9' % P4, 4),                                   # ... and truncated
    ('"point P" [%s] "float splitdepth" 5 "integer splitdepth" 1' % P4, 2),              # the integer wins (:229)
    ('"point P" [%s] "integer splitdepth" 1' % P7, 2 * 2),                               # two Bezier segments
    ('"point P" [%s] "integer degree" 2 "integer splitdepth" 1' % P7, 3 * 2),            # degree 2: (7 - 1) / 2
    ('"point P" [%s] "string basis" "bspline" "integer splitdepth" 0' % P7, 4),          # b-spline: 7 - 3
    ('"point P" [%s] "string basis" "bspline" "integer degree" 2 "integer splitdepth" 2' % P7, 5 * 4),
    ('"point P" [%s] "string type" "ribbon" "normal N" [0 0 1  0 1 1  0 1 0] "integer splitdepth" 0' % P7, 2),
    ('"point P" [%s] "string type" "cylinder" "float width0" 0.1 "float width1" 0.3' % P4, 8),
])
def test_segment_counts(tmp_path, params, segments):
    r, info = check(tmp_path, curve(params), "--curves")
    assert r.returncode == 0, r.stderr
    assert info["curves"] == segments and info["quadrics"] == 0 and info["triangles"] == 0 and info["warnings"] == 0, info


@pytest.mark.parametrize("params,sentence", [
    ('"point P" [%s] "integer degree" 4' % P4, "Invalid degree 4: only degree 2 and 3 curves are supported."),
    ('"point P" [%s] "string basis" "catmull"' % P4, "Invalid basis 'catmull'"),
    ('"point P" [%s  9 9 9]' % P4, "Invalid number of control points 5: for the degree 3 Bezier basis 4 + n * 3 are required"),
    ('"point P" [-1 0 0  0 1 0]', "Invalid number of control points 2"),
    ('', "Invalid number of control points 0"),
    ('"point P" [-1 0 0  0 1 0  1 0 0] "string basis" "bspline"', "Invalid number of control points 3: for the degree 3 b-spline basis, must have >= 4."),
    ('"point P" [%s] "string type" "ribbon"' % P4, "Must provide normals 'N' at curve endpoints with ribbon curves."),
    ('"point P" [%s] "string type" "ribbon" "normal N" [0 0 1  0 1 0]' % P7, "Invalid number of normals 2: must provide 3 normals for ribbon curves with 2 segments."),
    ('"point P" [%s] "integer splitdepth" 17' % P4, "splitdepth 17 is outside [0, 16]"),
    ('"point P" [%s] "integer splitdepth" -1' % P4, "splitdepth -1 is outside [0, 16]"),
])
def test_from_props_panics_are_sentences(tmp_path, params, sentence):
    r, _ = check(tmp_path, curve(params), "--curves")
    assert r.returncode == 1 and 'Shape "curve": ' + sentence in r.stderr, r.stderr
    assert len([l for l in r.stderr.strip().splitlines() if l.startswith("Error")]) == 1


def test_warnings(tmp_path):
    r, info = check(tmp_path, curve('"point P" [%s] "string type" "tube"' % P4), "--curves")
    assert r.returncode == 0 and info["warnings"] == 1 and "Unknown curve type 'tube'.  Using 'cylinder'." in r.stderr, r.stderr
    r, info = check(tmp_path, curve('"point P" [%s] "normal N" [0 0 1  0 1 0]' % P4), "--curves")          # N on a flat curve: dropped
    assert r.returncode == 0 and info["warnings"] == 1 and "Curve normals are only used with 'ribbon' type curves." in r.stderr, r.stderr
    r, info = check(tmp_path, curve('"point P" [%s] "float alpha" 0 "float shadowalpha" 0' % P4), "--curves")
    assert r.returncode == 0 and info["warnings"] == 2 and info["curves"] == 8 and "read no 'alpha'" in r.stderr and "read no 'shadowalpha'" in r.stderr, r.stderr


def test_placements_the_library_refuses(tmp_path):
    r, _ = check(tmp_path, 'ObjectBegin "o"\n' + curve('"point P" [%s]' % P4) + "\nObjectEnd", "--curves")
    assert r.returncode == 1 and "curves inside object definitions are not supported" in r.stderr, r.stderr
    r, _ = check(tmp_path, 'AttributeBegin\nAreaLightSource "diffuse"\n' + curve('"point P" [%s]' % P4) + "\nAttributeEnd", "--curves")
    assert r.returncode == 1 and "a curve cannot be an area light" in r.stderr and "todo!()" in r.stderr, r.stderr


def test_without_the_option_the_old_refusal_stays(tmp_path):
    for flags in ((), ("--quadrics",)):
        r, _ = check(tmp_path, curve('"point P" [%s]' % P4), *flags)
        assert r.returncode == 1 and 'Shape "curve" ' + OLD_PHRASE in r.stderr and "--curves" in r.stderr and "--quadrics" not in r.stderr, r.stderr
    for shape in ("loopsubdiv", "nurbs", "heightfield"):     # stay refused, and are not pointed to the option
        r, _ = check(tmp_path, 'Shape "%s"' % shape, "--quadrics", "--curves")
        assert r.returncode == 1 and 'Shape "%s" %s' % (shape, OLD_PHRASE) in r.stderr and "--curves" not in r.stderr, r.stderr


def test_help_names_the_option():
    r = run(["--help"])
    assert "--curves" in r.stdout + r.stderr


def test_the_shape_showcase_checks_clean():
    """The reference's scenes/shapes/all-shapes.pbrt less its loopsubdiv block: seven quadrics, two curves at the default splitdepth (2 x 8 segments), the tetrahedron and the floor"""
    r = run(["--check", "--quadrics", "--curves", FIXTURE])
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert (info["curves"], info["quadrics"], info["triangles"], info["lights"], info["instances"], info["warnings"]) == (16, 7, 6, 2, 0, 0), info
    assert (info["xres"], info["yres"], info["spp"], info["integrator"]) == (800, 400, 128, "whitted"), info
    text = open(FIXTURE).read()
    assert "loopsubdiv" not in text and text.count('Shape "curve"') == 2
    r = run(["--check", "--quadrics", FIXTURE])
    assert r.returncode == 1 and 'Shape "curve" ' + OLD_PHRASE in r.stderr
