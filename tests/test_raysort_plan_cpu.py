"""The slice plan of the ray binning between wavefront rounds (pbrt-v3-rs_amd/csrc/raysort_plan.h), run on the CPU by scripts/raysort_plan_check.cpp under the address and
undefined-behaviour sanitizers: which keys each block of the two passes owns, and how each of its two runs (closest-hit keys, any-hit keys) splits into a scalar head, a body of
16-byte loads and a scalar tail.  The contract is restated below in Python's unbounded integers, so an answer that wrapped at 32 bits differs from it.  No GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, FLOOR = 256, 16384          # PH_SORT_BLOCK, PH_SORT_FLOOR
LIMIT = 0x7FFF0000                 # ChunkPolicy::limit of the drivers: a round's queues hold fewer positions than this


def _header_constants():
    text = open(os.path.join(ROOT, "pbrt-v3-rs_amd", "csrc", "raysort_plan.h")).read()
    val = lambda name: int(text.split("#define " + name)[1].split()[0].rstrip("u"))
    return val("PH_SORT_BLOCK"), val("PH_SORT_FLOOR")


def slice_keys(n, grid, block, floor):
    each = -(-n // grid)
    return max(-(-each // block) * block, floor)


def n_cl_values(n):
    return sorted({v for v in (0, 1, 2, 3, 5, n) if v <= n})


def _cases():
    cases = []
    # every n in 0 .. 5000 against grids of 1, 3 and 1024, with n_cl at 0, 1, 2, 3, 5 and n: under the shipped floor (one block serves them all), and under a floor of one
    # block's width, where the same sizes spread over up to 20 blocks
    for floor in (FLOOR, BLOCK):
        for n in range(0, 5001):
            for grid in (1, 3, 1024):
                for n_cl in n_cl_values(n):
                    cases.append((n_cl, n - n_cl, grid, BLOCK, floor, 0, 0))
    # arrays that do not start on a 16-byte boundary
    for n in list(range(0, 40)) + [255, 256, 257, 1027, 1030]:
        for n_cl in n_cl_values(n):
            for mis_cl in range(4):
                for mis_sh in range(4):
                    cases.append((n_cl, n - n_cl, 3, BLOCK, BLOCK, mis_cl, mis_sh))
    # around the floor, around grid x floor, around the limit
    around = lambda c: [c + d for d in (-5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5)]
    for grid in (1, 3, 7, 1024):
        for n in around(FLOOR) + around(grid * FLOOR) + around(2 * FLOOR) + around(grid * (FLOOR + BLOCK)):
            for n_cl in n_cl_values(n) + [n // 2, n - 1]:
                cases.append((n_cl, n - n_cl, grid, BLOCK, FLOOR, 0, 0))
    for grid in (1, 3, 512, 1024, 2048):
        for n in [LIMIT - d for d in (0, 1, 2, 3, 4, 5, 255, 256, 257)]:
            for n_cl in (0, 1, 3, n // 2 + 1, n - 3, n):
                cases.append((n_cl, n - n_cl, grid, BLOCK, FLOOR, 0, 0))
                cases.append((n_cl, n - n_cl, grid, BLOCK, FLOOR, 3, 1))
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def answers():
    text = "".join("%d %d %d %d %d %d %d\n" % c for c in CASES)
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "raysort_plan_check.sh")], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]   # (a sanitizer report ends the program with a non-zero status)
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    got = []
    for line in lines:
        busy, rest = line.split("|")
        v = [int(w) for w in busy.split()]
        assert len(v) % 10 == 0
        idle, clean = (int(w) for w in rest.split())
        got.append(([tuple(v[i:i + 10]) for i in range(0, len(v), 10)], idle, clean))
    return got


def test_constants_are_the_headers():
    assert _header_constants() == (BLOCK, FLOOR)


def test_cases_cover_what_they_are_about():
    ns = {(c[0] + c[1], c[2]) for c in CASES if c[4] == FLOOR}
    for grid in (1, 3, 1024):
        assert all((n, grid) in ns for n in range(0, 5001))
        assert {(FLOOR - 1, grid), (FLOOR, grid), (FLOOR + 1, grid), (grid * FLOOR + 3, grid), (LIMIT, grid)} <= ns
    assert any(c[5] or c[6] for c in CASES)


def test_slices_partition_the_queue_in_block_order(answers):
    for case, (busy, idle, clean) in zip(CASES, answers):
        n_cl, n_sh, grid, block, floor = case[:5]
        n, per = n_cl + n_sh, slice_keys(n_cl + n_sh, grid, block, floor)
        at = 0
        for b, s in enumerate(busy):
            assert (s[0], s[1]) == (at, min(at + per, n)) and s[0] == b * per and s[0] < s[1], case
            at = s[1]
        assert at == n, case


def test_no_block_beyond_the_slices_needed_gets_work(answers):
    for case, (busy, idle, clean) in zip(CASES, answers):
        n_cl, n_sh, grid, block, floor = case[:5]
        n = n_cl + n_sh
        per = slice_keys(n, grid, block, floor)
        assert len(busy) == -(-n // per) and len(busy) + idle == grid and clean == 1, case


def test_runs_cover_the_slice_and_split_at_16_byte_boundaries(answers):
    for case, (busy, idle, clean) in zip(CASES, answers):
        n_cl, n_sh, grid, block, floor, mis_cl, mis_sh = case
        for s in busy:
            lo, hi = s[0], s[1]
            cl, sh = s[2:6], s[6:10]
            # the two runs are the slice: closest-hit positions [lo, hi) below n_cl, any-hit positions behind them, counted from the start of their own array
            assert (cl[0], cl[3]) == (min(lo, n_cl), min(hi, n_cl)), case
            assert (sh[0], sh[3]) == (max(lo, n_cl) - n_cl, max(hi, n_cl) - n_cl), case
            assert (cl[3] - cl[0]) + (sh[3] - sh[0]) == hi - lo, case
            for (head, body, tail, end), mis, size in ((cl, mis_cl, n_cl), (sh, mis_sh, n_sh)):
                assert head <= body <= tail <= end <= size, case
                assert body - head < 4 and end - tail < 4 and (tail - body) % 4 == 0, case
                if tail > body:
                    assert (body + mis) % 4 == 0, case        # 4-byte keys: the body starts on a 16-byte boundary of an array whose first key lies `mis` keys behind one
                if end - head >= 7:
                    assert tail > body, case                  # a run of seven keys holds an aligned four wherever it starts
                assert end <= 0xFFFFFFFF


def test_the_limit_fits_32_bits(answers):
    seen = 0
    for case, (busy, idle, clean) in zip(CASES, answers):
        if case[0] + case[1] == LIMIT:
            seen += 1
            assert busy[-1][1] == LIMIT and sum(s[1] - s[0] for s in busy) == LIMIT, case
    assert seen > 0
