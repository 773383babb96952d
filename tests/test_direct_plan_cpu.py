"""The sampler-dimension bound of the recursive integrators (pbrt-v3-rs_amd/csrc/direct_plan.h), which decides the UNSUPPORTED refusal of pbrt_hip_render_whitted and
pbrt_hip_render_direct, against li's recursion restated literally and counted by scripts/direct_plan_check.cpp, a plain host program built under the address and
undefined-behaviour sanitizers: scenes with neither specular kind, one kind and both; Whitted, direct lighting "all" and "one"; the Halton table (1000), the Sobol' table (1024)
and the Sobol' dimensions given.  No GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    return subprocess.run(["bash", os.path.join(ROOT, "scripts", "direct_plan_check.sh")], capture_output=True, text=True, timeout=600)


def _totals(out):
    lines = out.stdout.splitlines()
    assert len(lines) >= 2, out.stdout[-2000:] + out.stderr[-2000:]
    counts = lines[-2].split(); fails = lines[-1].split()
    assert counts[0] == "bound" and fails[0] == "failures", out.stdout[-2000:] + out.stderr[-2000:]
    return dict(zip(counts[0::2], map(int, counts[1::2]))), dict(zip(fails[1::2], map(int, fails[2::2])))


def test_the_bound_is_what_the_recursion_can_draw(report):
    _, fails = _totals(report)
    assert fails["bound"] == 0, report.stdout[:4000]


def test_the_refusal_stands_at_the_tables_edges(report):
    _, fails = _totals(report)
    assert fails["refusal"] == 0, report.stdout[:4000]


def test_clean_under_the_sanitizers_and_every_case_is_met(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-2000:]   # (a sanitizer report ends the program with a non-zero status)
    counts, _ = _totals(report)
    assert counts["bound"] == 3 * 4 * 17 * 17   # integrators x kinds of specular lobes x max_depth 0 .. 16 x light counts
    assert counts["ok"] > 1000 and counts["over_table"] > 1000 and counts["over_sobol_given"] > 100   # each answer is given many times
