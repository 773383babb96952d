"""The shade pass's row table (pbrt-v3-rs_amd/csrc/shade_shapes.h) on the CPU, through scripts/shade_rows_check.cpp: every combination of scene features
(infinite / area / delta lights present, Halton or Sobol, spatial light distribution on or off) maps to a row that compiles everything the combination can execute,
the headline combination maps to the lean row, and PBRT_HIP_SHADE_ROW=full maps everything to the row that compiles it all.
What "covers" means is restated here from the rows' printed members, not taken from the header's own predicate."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(line):
    return {k: int(v) for k, v in (t.split("=") for t in line.split() if "=" in t)}


@pytest.fixture(scope="module")
def table():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "shade_rows_check.sh")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    rows = {}
    for l in lines:
        if l.startswith("row "):
            rows[int(l.split()[1])] = dict(_fields(l), name=l.split()[2])
    picks = [_fields(l) for l in lines if l.startswith("pick ")]
    head = [l for l in lines if l.startswith("rows ")][0].split()
    return rows, picks, {"n": int(head[1]), "sky": int(head[3]), "full": int(head[5])}


def _covers(row, f):
    return ((not f["infinite"] or row["infinite"]) and (not f["area"] or row["area"]) and (not f["delta"] or row["delta"])
            and (row["sobol"] if f["sobol"] else row["halton"]) and (not f["spatial"] or row["spatial"]))


def test_every_feature_combination_has_a_row_that_covers_it(table):
    rows, picks, head = table
    assert len(rows) == head["n"] and len(picks) == 64
    seen = set()
    for p in picks:
        seen.add((p["infinite"], p["area"], p["delta"], p["sobol"], p["spatial"], p["full"]))
        assert 0 <= p["row"] < head["n"], p
        assert _covers(rows[p["row"]], p), p
        assert p["covers"] == 1, p
    assert seen == set(itertools.product((0, 1), repeat=6))


def test_the_headline_combination_takes_the_lean_row(table):
    rows, picks, head = table
    for p in picks:
        lean_scene = not p["area"] and not p["delta"] and not p["sobol"] and not p["spatial"]
        if p["full"]:
            assert p["row"] == head["full"], p
        elif lean_scene:   # infinite lights only — or no light at all —, Halton, no spatial distribution
            assert p["row"] == head["sky"], p
        else:
            assert p["row"] != head["sky"], p
    sky, full = rows[head["sky"]], rows[head["full"]]
    assert (sky["infinite"], sky["area"], sky["delta"], sky["halton"], sky["sobol"], sky["spatial"]) == (1, 0, 0, 1, 0, 0)
    assert all(full[k] == 1 for k in ("infinite", "area", "delta", "halton", "sobol", "spatial"))
    assert full["phi_skip"] == 0 and full["lean_lds"] == 0   # the kernel as it was before the table
