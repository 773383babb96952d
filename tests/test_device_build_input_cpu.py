"""The input stage both device builders call before their first allocation (pbrt-v3-rs_amd/csrc/device_build_input.h), run on the CPU by scripts/device_build_input_check.cpp under
the address and undefined-behaviour sanitizers: one flat input and one forest (3 trees, 2 instances, one quadric slot in tree 0) are accepted; items without a forest, an empty tree
range, ranges that do not cover the items, an item that names no triangle (or no instance), an instance item outside tree 0, inst_tree equal to 0 or to n_trees, quadric slots without
bounds, a quadric slot inside an object's tree and a slot that names no quadric are each refused with -1 and a message; n_verts of a quadric-only, a mixed and a triangles-only input.
No GPU is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ACCEPTED = ("flat input", "forest of 3 trees, 2 instances, a quadric in tree 0", "no primitive at all")
# case -> words of the message that only the check meant to fire uses: a case refused by another check fails here
REFUSED = {"items without a forest": "an item list without its forest", "an empty tree range": "empty or unordered tree range",
           "ranges that end before the items do": "tree ranges do not cover the items", "ranges that begin behind the first item": "tree ranges do not cover the items",
           "an item that names no triangle": "an item names no triangle or instance", "an item that names no instance": "an item names no triangle or instance",
           "an instance item outside tree 0": "an item names no triangle or instance", "inst_tree equal to 0": "an instance names no object tree",
           "inst_tree equal to n_trees": "an instance names no object tree", "instances without their trees": "instances without object trees",
           "quadric slots without bounds (forest)": "quadric slots without their bounds", "quadric slots without bounds (flat)": "quadric slots without their bounds",
           "a quadric slot inside an object's tree": "a quadric slot inside an object's tree", "a slot that names no quadric (forest)": "one that names no quadric",
           "a slot that names no quadric (flat)": "one that names no quadric"}
COUNTS = (("n_verts, quadrics only", "0"), ("n_verts, mixed", "5"), ("n_verts, mixed, vertex 0 named by the quadric slot only", "4"), ("n_verts, triangles only", "5"))


def test_the_input_stage_accepts_and_refuses_as_both_builders_did():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "device_build_input_check.sh")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]     # (an unexpected answer, or a sanitizer report, ends the program with a non-zero status)
    lines = out.stdout.splitlines()
    assert lines[-1] == "all as expected" and not any("MISMATCH" in l for l in lines)
    for case in ACCEPTED:
        assert f"{case}: ok - accepted" in lines, case
    for case, words in REFUSED.items():
        got = [l for l in lines if l.startswith(f"{case}: ok - refused: device build: ")]
        assert len(got) == 1 and words in got[0][len(case):], (case, got)
    for case, n in COUNTS:
        assert f"{case}: ok - {n}" in lines, case
