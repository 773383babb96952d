"""The escape-query predicate (pbrt-v3-rs_amd/csrc/mis_escape.h) on the CPU, through scripts/mis_escape_check.cpp: for which frames estimate_direct's BSDF-sampled ray is traced
as "does it hit anything", which rows of the traversal table are compiled for it, and what the binning makes of a marked bin key.  The table is restated here, not taken from
the header: the query is on exactly when the scene has no area light of any shape, its traversal row has neither alpha-mask textures (class 0 of 0 / 1 / 2) nor quadrics, and
traversal counting is off.  No GPU is needed."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 4096


def _fields(line):
    return {k: int(v) for k, v in (t.split("=") for t in line.split() if "=" in t)}


@pytest.fixture(scope="module")
def lines():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "mis_escape_check.sh")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


def test_every_combination_of_scene_features(lines):
    got = {}
    for l in lines:
        if l.startswith("eligible "):
            f = _fields(l.split("->")[0])
            got[(f["area"], f["alpha"], f["quadric"], f["counting"])] = int(l.split("->")[1])
    want = {(area, alpha, quadric, counting): int(not area and alpha == 0 and not quadric and not counting)
            for area, alpha, quadric, counting in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1))}
    assert len(want) == 24 and got == want
    assert sum(got.values()) == 1 and got[(0, 0, 0, 0)] == 1     # one combination in 24: a plain scene, timed


def test_rows_compiled_with_the_query(lines):
    got = {}
    for l in lines:
        if l.startswith("row "):
            f = _fields(l.split("->")[0])
            got[(f["alpha"], f["quadric"], f["counting"])] = int(l.split("->")[1])
    want = {(alpha, quadric, counting): int(alpha == 0 and not quadric and not counting) for alpha, quadric, counting in itertools.product((0, 1, 2), (0, 1), (0, 1))}
    assert len(want) == 12 and got == want


def test_joint_key_of_a_closest_hit_key(lines):
    seen = 0
    for l in lines:
        if not l.startswith("joint "):
            continue
        key = _fields(l.split("->")[0])["key"]
        f = _fields(l.split("->")[1])
        assert f["mark"] == int(key >= BINS)
        assert f["bin"] == key % BINS          # an unmarked key is binned as it always was, a marked one beside the extension rays of its cell
        seen += 1
    assert seen >= 8


def test_the_headers_constants():
    text = open(os.path.join(ROOT, "pbrt-v3-rs_amd", "csrc", "raysort_plan.h")).read()
    assert int(text.split("#define PH_SORT_BINS")[1].split()[0].rstrip("u")) == BINS
