"""The host's share of the HLBVH forest build on the device (pbrt-v3-rs_amd/csrc/hlbvh_forest_stitch.h: per-tree slices of the treelet list, the SAH over each tree's treelet roots,
forest-wide references, the host builder's node numbering), run on the CPU by scripts/hlbvh_forest_stitch_check.cpp under the address and undefined-behaviour sanitizers and
compared there with build_forest_host(.., split_method = 1, ..): a forest of three trees, a forest whose every tree is a single treelet, a forest in which one object has one
primitive, a forest with one deep treelet of 241 primitives, and scenes without objects — one tree of 1, 2, 3, 17, 300 and 5 000 triangles, where the array in the kernels'
numbering (what the device build ships for one tree) is also walked in step with the host tree; max_prims_in_node 1 and 4.  No GPU is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stitched_forest_equals_the_host_forest():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "hlbvh_forest_stitch_check.sh")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]     # (a difference, or a sanitizer report, ends the program with a non-zero status)
    lines = out.stdout.splitlines()
    assert lines[-1] == "all equal" and not any(l.startswith("MISMATCH") for l in lines)
    for case, trees in (("three trees", "3 trees"), ("single treelets, equal codes", "2 trees, 2 treelets"), ("an object of one primitive", "3 trees"),
                        ("deep treelets", "2 trees, 4 treelets"),      # one 241-primitive treelet: its nodes' numbers and references, renumbered
                        *((f"one tree of {n}", f"1 trees, ") for n in (1, 2, 3, 17, 300, 5000))):
        got = [l for l in lines if l.startswith(case + ": ")]
        assert len(got) == 2 and all(trees in l for l in got), (case, got)
