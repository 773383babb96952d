"""CPU tests of `pbrt_hip_render --loopsubdiv` in --check mode (no GPU is touched, nothing is rendered): Shape "loopsubdiv" is read as LoopSubDiv::from_props reads it
(shapes/src/loopsubdiv.rs:668-689) and counted as F 4^nlevels triangles; its two panics and every mesh the library refuses are one sentence; without the option the directive
is refused with the sentence it always had; and the reference's shape showcase, scenes/shapes/all-shapes.pbrt UNCHANGED (tests/golden/ref_scenes/shapes/all-shapes-loopsubdiv.pbrt),
checks clean."""
import json
import os
import subprocess

import pytest

import driver_scene as ds

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ref_scenes", "shapes", "all-shapes-loopsubdiv.pbrt")
OLDER_FIXTURE = os.path.join(HERE, "golden", "ref_scenes", "shapes", "all-shapes.pbrt")
OLD_PHRASE = "is outside the hot-path scope"
TETRA = '"integer indices" [ 0 1 2  0 3 1  0 2 3  1 3 2 ] "point P" [ 0.9428 0 -0.3333  -0.4714 0.8165 -0.3333  -0.4714 -0.8165 -0.3333  0 0 1 ]'
TRI_P = '"point P" [0 0 0  1 0 0  0 1 0]'


def run(args):
    return subprocess.run([ds.RENDER_BIN] + args, capture_output=True, text=True, timeout=120)


def check(tmp_path, body, *flags):
    p = tmp_path / "s.pbrt"
    p.write_text('WorldBegin\nLightSource "infinite"\n' + body + "\nWorldEnd\n")
    r = run(["--check"] + list(flags) + [str(p)])
    return r, (json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None)


@pytest.mark.parametrize("params,triangles", [
    (TETRA + ' "integer nlevels" 0', 4), (TETRA + ' "integer nlevels" 1', 16), (TETRA + ' "integer nlevels" 3', 256), (TETRA, 256),     # the default is 3
    ('"integer indices" [0 1 2] ' + TRI_P + ' "integer nlevels" 2', 16),
    (TETRA + ' "integer nlevels" 13', 4 ** 14),        # the largest the library indexes: 3 * 4^14 still fits an int
])
def test_triangle_counts(tmp_path, params, triangles):
    r, info = check(tmp_path, 'Shape "loopsubdiv" ' + params, "--loopsubdiv")
    assert r.returncode == 0, r.stderr
    assert (info["triangles"], info["lights"], info["quadrics"], info["curves"], info["warnings"]) == (triangles, 1, 0, 0, 0), info


@pytest.mark.parametrize("params,sentence", [
    (TRI_P, "Vertex indices 'indices' not provided for LoopSubDiv shape."),
    ('"integer indices" [0 1 2]', "Vertex positions 'P' not provided for LoopSubDiv shape."),
    ('"integer indices" [0 1 3] ' + TRI_P, "Vertex index 3 is out of bounds (3 vertices)."),
    ('"integer indices" [0 1 -1] ' + TRI_P, "Vertex index -1 is out of bounds (3 vertices)."),
    ('"integer indices" [0 1 1] ' + TRI_P, "Face 0 names a vertex twice."),
    ('"integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 1 0  5 5 5]', "Start face for vertex 3 is not set. Check input mesh to ensure all vertices used."),
    ('"integer indices" [0 1 2  1 0 3  0 1 4] "point P" [0 0 0  1 0 0  0 1 0  0 -1 0  0 0 1]', "The edge between vertices 0 and 1 is in more than two faces."),
    ('"integer indices" [0 1 2  0 1 3] "point P" [0 0 0  1 0 0  0 1 0  0 -1 0]', "Faces 0 and 1 run through the edge between vertices 0 and 1 in the same direction."),
    ('"integer indices" [0 1 2] ' + TRI_P + ' "integer nlevels" -1', "nlevels -1 is negative."),
    ('"integer indices" [0 1 2] ' + TRI_P + ' "integer nlevels" 16', "The mesh after 16 levels does not fit 32-bit indices."),
    (TETRA + ' "integer nlevels" 14', "The mesh after 14 levels does not fit 32-bit indices."),
])
def test_each_refusal_is_one_sentence(tmp_path, params, sentence):
    r, _ = check(tmp_path, 'Shape "loopsubdiv" ' + params, "--loopsubdiv")
    assert r.returncode == 1 and 'Shape "loopsubdiv": ' + sentence in r.stderr, r.stderr
    assert len(r.stderr.strip().splitlines()) == 1, r.stderr


def test_warnings(tmp_path):
    r, info = check(tmp_path, 'Shape "loopsubdiv" "integer indices" [0 1 2 0] ' + TRI_P + ' "integer nlevels" 1', "--loopsubdiv")
    assert r.returncode == 0 and info["triangles"] == 4 and info["warnings"] == 1, (r.stderr, info)
    assert "4 indices are no multiple of 3; the last 1 are dropped" in r.stderr
    r, info = check(tmp_path, 'Shape "loopsubdiv" ' + TETRA + ' "float alpha" 0 "float shadowalpha" 0', "--loopsubdiv")
    assert r.returncode == 0 and info["triangles"] == 256 and info["warnings"] == 2, (r.stderr, info)
    assert "reads no 'alpha'" in r.stderr and "reads no 'shadowalpha'" in r.stderr


def test_inside_an_object_and_under_an_area_light(tmp_path):
    body = 'ObjectBegin "s"\nShape "loopsubdiv" ' + TETRA + ' "integer nlevels" 1\nObjectEnd\nObjectInstance "s"\nTranslate 3 0 0\nObjectInstance "s"\n'
    r, info = check(tmp_path, body, "--loopsubdiv")
    assert r.returncode == 0, r.stderr
    assert (info["triangles"], info["instances"], info["lights"]) == (2 * 16, 2, 1), info
    body = 'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [2 2 2]\nReverseOrientation\nScale 1 -2 1\nShape "loopsubdiv" ' + TETRA + ' "integer nlevels" 2 "rgb Kd" [0.2 0.3 0.4]\nAttributeEnd\n'
    r, info = check(tmp_path, body, "--loopsubdiv")
    assert r.returncode == 0, r.stderr
    assert (info["triangles"], info["lights"]) == (64, 1 + 64), info          # one DiffuseAreaLight per OUTPUT triangle: F 4^L


def test_without_the_option_the_old_refusal_stays(tmp_path):
    for flags in ((), ("--quadrics", "--curves")):
        r, _ = check(tmp_path, 'Shape "loopsubdiv" ' + TETRA, *flags)
        assert r.returncode == 1 and 'Shape "loopsubdiv" ' + OLD_PHRASE in r.stderr and "--loopsubdiv" in r.stderr, r.stderr
        assert "--quadrics" not in r.stderr and "--curves" not in r.stderr
    for shape in ("nurbs", "heightfield"):     # stay refused, and are not pointed to the option
        r, _ = check(tmp_path, 'Shape "%s"' % shape, "--loopsubdiv")
        assert r.returncode == 1 and 'Shape "%s" %s' % (shape, OLD_PHRASE) in r.stderr and "--loopsubdiv" not in r.stderr, r.stderr


def test_help_names_the_option():
    r = run(["--help"])
    assert r.returncode == 0 and "--loopsubdiv" in r.stderr and 'Shape "loopsubdiv"' in r.stderr


def test_the_references_own_shape_showcase_checks_clean():
    """scenes/shapes/all-shapes.pbrt as the reference has it: the older fixture plus its loopsubdiv block, a tetrahedron at the default 3 levels = 256 triangles"""
    text, older = open(FIXTURE).read(), open(OLDER_FIXTURE).read()
    assert text.count('Shape "loopsubdiv"') == 1 and "loopsubdiv" not in older
    at = text.index('    Translate 6 0 2.5\n    Scale 4 4 4\n    Shape "loopsubdiv"')
    end = text.index("  AttributeBegin", at)
    assert text[:at] + text[text.index("    Translate 0 0 -1", end):] == older          # nothing else differs
    r = run(["--check", "--quadrics", "--curves", "--loopsubdiv", FIXTURE])
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert (info["curves"], info["quadrics"], info["triangles"], info["lights"], info["instances"], info["warnings"]) == (16, 7, 6 + 256, 2, 0, 0), info
    assert (info["xres"], info["yres"], info["spp"], info["integrator"]) == (800, 400, 128, "whitted"), info
    r = run(["--check", "--quadrics", "--curves", FIXTURE])
    assert r.returncode == 1 and 'Shape "loopsubdiv" ' + OLD_PHRASE in r.stderr
