"""The shade pass's row table (pbrt-v3-rs_amd/csrc/shade_shapes.h) on the CPU, through scripts/shade_rows_check.cpp: every combination of scene features
(infinite / area / delta lights present, Halton or Sobol, spatial light distribution on or off) maps to a row that compiles everything the combination can execute,
the headline combination maps to the lean row, and PBRT_HIP_SHADE_ROW=full maps everything to the row that compiles it all.
What "covers" means is restated here from the rows' printed members, not taken from the header's own predicate.
The same program prints the two tables of what the shade side launches (ShadeVariants, TexVariants) and what their pickers answer: the ladders the render call used to walk are
restated here as plain Python, and every one of the 512 + 8 picks must be theirs."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(line):
    return {k: int(v) for k, v in (t.split("=") for t in line.split() if "=" in t)}


@pytest.fixture(scope="module")
def check_lines():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "shade_rows_check.sh")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def table(check_lines):
    lines = check_lines
    rows = {}
    for l in lines:
        if l.startswith("row "):
            rows[int(l.split()[1])] = dict(_fields(l), name=l.split()[2])
    picks = [_fields(l) for l in lines if l.startswith("pick ")]
    head = [l for l in lines if l.startswith("rows ")][0].split()
    return rows, picks, {"n": int(head[1]), "sky": int(head[3]), "full": int(head[5])}


@pytest.fixture(scope="module")
def variants(check_lines, table):
    """the same run's lines about the variant tables: (shade picks, texture picks, shade table, texture table, the row indices)"""
    by = lambda prefix: [_fields(l) for l in check_lines if l.startswith(prefix + " ")]
    return by("shade_pick"), by("tex_pick"), by("shade_variant"), by("tex_variant"), table[2]


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


def _shade_ladder(p, sky, full):
    """(gen, tex, quad, row) as the render call's ladder chose them: the full row whenever a trait is set, else the row of the features; then sky -> <F,F,F,Sky>,
    quadrics -> <T,T,T>, textured and general -> <T,T,F>, textured -> <F,T,F>, general -> <T,F,F>, otherwise <F,F,F>"""
    if p["general"] or p["textured"] or p["quadric"] or p["full"]:
        row = full
    else:   # (the row of the features, as test_the_headline_combination_takes_the_lean_row pins it)
        row = sky if not (p["area"] or p["delta"] or p["sobol"] or p["spatial"]) else full
    if row == sky:
        return (0, 0, 0, sky)
    if p["quadric"]:
        return (1, 1, 1, full)
    if p["textured"]:
        return (1, 1, 0, full) if p["general"] else (0, 1, 0, full)
    if p["general"]:
        return (1, 0, 0, full)
    return (0, 0, 0, full)


def _tex_ladder(p):
    """(simple, camera, waves, quadric) of the texture pass's launch site"""
    if p["camera"]:
        return (0, 1, 2, 1) if p["quadrics"] else (1, 1, 3, 0) if p["simple_textures"] else (0, 1, 2, 0)
    return (0, 0, 3, 1) if p["quadrics"] else (1, 0, 4, 0) if p["simple_textures"] else (0, 0, 3, 0)


def test_the_shade_picker_answers_as_the_ladder_did(variants):
    shade_picks, _, shade_table, _, head = variants
    assert len(shade_picks) == 512
    seen = set()
    for p in shade_picks:
        seen.add(tuple(p[k] for k in ("general", "textured", "quadric", "infinite", "area", "delta", "sobol", "spatial", "full")))
        assert (p["gen"], p["tex"], p["quad"], p["row"]) == _shade_ladder(p, head["sky"], head["full"]), p
        v = shade_table[p["variant"]]
        assert (v["gen"], v["tex"], v["quad"], v["row"]) == (p["gen"], p["tex"], p["quad"], p["row"]), p   # the printed members are the table entry's
    assert seen == set(itertools.product((0, 1), repeat=9))


def test_the_texture_picker_answers_as_the_ladder_did(variants):
    _, tex_picks, _, tex_table, _ = variants
    assert len(tex_picks) == 8
    assert {(p["camera"], p["simple_textures"], p["quadrics"]) for p in tex_picks} == set(itertools.product((0, 1), repeat=3))
    for p in tex_picks:
        assert (p["simple"], p["cam"], p["waves"], p["quad"]) == _tex_ladder(p) and p["launched"] == 1, p
        v = tex_table[p["variant"]]
        assert (v["simple"], v["cam"], v["waves"], v["quad"], v["launched"]) == (p["simple"], p["cam"], p["waves"], p["quad"], 1), p


def test_the_tables_hold_exactly_what_is_launched_and_the_two_anchors(variants):
    _, _, shade_table, tex_table, head = variants
    sky, full = head["sky"], head["full"]
    got = sorted((v["gen"], v["tex"], v["quad"], v["row"]) for v in shade_table)
    assert got == sorted([(0, 0, 0, sky), (1, 1, 1, full), (1, 1, 0, full), (0, 1, 0, full), (1, 0, 0, full), (0, 0, 0, full)])
    launched = sorted((v["simple"], v["cam"], v["waves"], v["quad"]) for v in tex_table if v["launched"])
    anchors = sorted((v["simple"], v["cam"], v["waves"], v["quad"]) for v in tex_table if not v["launched"])
    assert launched == sorted([(0, 1, 2, 1), (1, 1, 3, 0), (0, 1, 2, 0), (0, 0, 3, 1), (1, 0, 4, 0), (0, 0, 3, 0)])
    assert anchors == sorted([(0, 0, 4, 0), (0, 1, 3, 0)])
    assert len(shade_table) == 6 and len(tex_table) == 8
