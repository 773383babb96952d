"""The oracle's EWA footprint loops and triangle's neighbour index where the float-to-isize conversions saturate (oracle/oracle_texture.hpp: MipMap::ewa, MipMap::triangle),
run on the CPU by scripts/ewa_loop_check.cpp under the address and undefined-behaviour sanitizers at -O0 and at -O2.  For st * w - 0.5 >= 2^63 both loop bounds are isize::MAX:
the reference's `t0..=t1` (core/src/mipmap/mod.rs:355-357) runs once; a C++ `for (it = t0; it <= t1; it++)` increments past INT64_MAX, which is undefined (at -O0 it never
returned).  The loops now leave at the last index, and `s0 + 1` wraps as the reference's release build does.  Both builds must end with status 0 within the time limit and print
the same bits.  The device's mip_ewa / mip_triangle (pbrt-v3-rs_amd/csrc/texture.h) carry the same two changes; tests/test_texture_probe_gpu.py compares them on these inputs.
No GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(level):
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "ewa_loop_check.sh"), level], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]   # (a sanitizer report ends the program with a non-zero status)
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def outputs():
    return _run("-O0"), _run("-O2")


def test_both_builds_return_and_cover_every_case(outputs):
    # 2 maps x 3 wrap modes x (1 + 14 coordinates x 3 placements x (3 derivative sets + one triangle per level)); the 4 x 4 map has 3 levels, the 2 x 16 map 5
    for lines in outputs:
        assert len(lines) == 3 * (1 + 14 * 3 * (3 + 3)) + 3 * (1 + 14 * 3 * (3 + 5))
        assert all(l.startswith(("lookup ", "triangle ")) and "->" in l for l in lines)


def test_same_bits_at_both_optimisation_levels(outputs):
    o0, o2 = outputs
    assert o0 == o2, [(a, b) for a, b in zip(o0, o2) if a != b][:5]


def test_the_case_the_defect_was_measured_on_is_finite(outputs):
    """4 x 4 map, max_anisotropy 8, st = (2^61, 0.3), derivatives (0.1, 0, 0, 0.1): the first line of the output; one footprint column per level, a weighted mean of texels."""
    line = outputs[0][0]
    assert line.startswith("lookup map=0 wrap=0 st=5e000000,3e99999a d=0 -> ")
    vals = [int(w, 16) for w in line.split("->")[1].split()]
    assert all((v & 0x7F800000) != 0x7F800000 for v in vals)   # finite
