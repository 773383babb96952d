"""The chunk planner the wavefront drivers share (pbrt-v3-rs_amd/csrc/chunk_plan.h), run on the CPU by scripts/chunk_plan_check.cpp: the samples per pixel it plans and the
bytes per path each driver's buffer table sums to, against what render_tiles (wavefront.hip) and render_whitted_tiles (whitted.hip) computed by hand before they shared it.
Those expressions are restated below from the drivers as they were, not taken from the header.  The record sizes are the ones the formulas were written for
(RayIn 32, HitOut 32, TexOut 128, WhSample 96, WhFrame 352 bytes, PH_WH_SLICE 4): a change to one of those records changes the estimate and belongs in this file too."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY, HIT, TEXOUT, WH_SAMPLE, WH_FRAME, SLICE = 32, 32, 128, 96, 352, 4
MI, KI, GB = 1 << 20, 1 << 10, 10 ** 9


def path_per_path(textured):
    """wavefront.hip, render_tiles: `per_path`"""
    return (2 * 2 * RAY + 2 * HIT + RAY + 1 + 2 * 4 + 6 * 2 * 16 + 2 * 4
            + 3 * 4 + 3 * 4 + (TEXOUT if textured else 0)
            + 4 + 2)


def whitted_per_sample(n_frames):
    """whitted.hip, render_whitted_tiles: `per_sample`"""
    return WH_SAMPLE + n_frames * WH_FRAME + 2 * RAY + HIT + 2 * SLICE * RAY + SLICE + 2 * 4


def _override(max_paths, env):
    if env is not None:
        try:
            v = int(env)       # atoll of the texts used here
        except ValueError:
            v = 0
        if v > 0:
            max_paths = v
    return max_paths


def path_chunk_spp(free_b, total_b, held, rec_need, rec_have, per_path, env, n_px, spp):
    """wavefront.hip, render_tiles"""
    max_paths = 128 << 20
    if total_b:
        avail = free_b // 10 * 8 + held
        short = rec_need - rec_have if rec_need > rec_have else 0
        avail = avail - short if avail > short else 0
        max_paths = max(1 << 20, min(max_paths, min(total_b // 10 * 3, avail) // per_path))
    max_paths = _override(max_paths, env)
    return max(1, min(spp, max_paths // max(n_px, 1)))


def whitted_chunk_spp(free_b, total_b, held, per_sample, env, n_px, spp):
    """whitted.hip, render_whitted_tiles"""
    max_paths = 32 << 20
    if total_b:
        avail = free_b // 10 * 8 + held
        max_paths = max(1 << 16, min(max_paths, min(total_b // 10 * 3, avail) // per_sample))
    max_paths = _override(max_paths, env)
    return max(1, min(spp, max_paths // max(n_px, 1)))


P, PT, W5 = path_per_path(False), path_per_path(True), whitted_per_sample(5)
HD = 1920 * 1080
# (what the case is about, driver, free, total, held, rec_need, rec_have, per_path, PBRT_HIP_MAX_PATHS, n_px, spp, chunk_spp worked out by hand from the expressions above)
CASES = [
    ("no memory info: the ceiling", "path", 0, 0, 0, 0, 0, P, None, MI, 1024, 128),
    ("no memory info: the ceiling", "whitted", 0, 0, 0, 0, 0, W5, None, MI, 1024, 32),
    ("plenty of memory: the ceiling", "path", 280 * GB, 288 * GB, 0, HD * 64 * 20, 0, P, None, HD, 1024, 64),             # 30 % of 288 GB / 463 B = 186 Mi > 128 Mi
    ("30 % of the device caps it", "path", 95 * GB, 100 * GB, 0, 0, 0, PT, None, MI, 1024, 48),                          # 30 GB / 591 B = 50 761 421 paths
    ("free memory caps it", "path", 20 * GB, 288 * GB, 0, 0, 0, P, None, MI, 1024, 32),                                 # 16 GB / 463 B = 34 557 235 paths
    ("held buffers count as available", "path", 20 * GB, 288 * GB, 16 * GB, 0, 0, P, None, MI, 1024, 65),               # 32 GB / 463 B = 69 114 470
    ("records still to allocate are set aside", "path", 20 * GB, 288 * GB, 0, 10 * GB, 2 * GB, P, None, MI, 1024, 16),   # 8 GB / 463 B = 17 278 617
    ("records already there need nothing", "path", 20 * GB, 288 * GB, 0, 2 * GB, 10 * GB, P, None, MI, 1024, 32),
    ("cap below the floor: the floor", "path", 100 * MI, 288 * GB, 0, 0, 0, P, None, 4 * KI, 1024, 256),                # 80 MiB / 463 B < 1 Mi
    ("cap below the floor: the floor", "whitted", 10 * MI, 288 * GB, 0, 0, 0, W5, None, KI, 1024, 64),                  # 8 MiB / 2 220 B < 64 Ki
    ("reserve above what is available: the floor", "path", 20 * GB, 288 * GB, 0, 40 * GB, 0, P, None, 4 * KI, 1024, 256),
    ("override below the memory cap", "path", 280 * GB, 288 * GB, 0, 0, 0, P, str(64 * 64 * 3), 64 * 64, 8, 3),
    ("override above the memory cap", "path", 20 * GB, 288 * GB, 0, 0, 0, P, str(512 * MI), MI, 1024, 512),
    ("override without memory info", "whitted", 0, 0, 0, 0, 0, W5, str(48 * 48 * 3 // 2), 48 * 48, 4, 1),
    ("override that is not positive is ignored", "whitted", 0, 0, 0, 0, 0, W5, "0", MI, 1024, 32),
    ("spp smaller than what fits", "path", 280 * GB, 288 * GB, 0, 0, 0, P, None, 64 * 64, 8, 8),
    ("spp smaller than what fits", "whitted", 280 * GB, 288 * GB, 0, 0, 0, W5, None, 48 * 48, 4, 4),
    ("more pixels than paths: one sample", "path", 280 * GB, 288 * GB, 0, 0, 0, P, None, 200 * MI, 16, 1),
    ("more pixels than paths: one sample", "whitted", 280 * GB, 288 * GB, 0, 0, 0, W5, str(1000), 48 * 48, 4, 1),
    ("no pixels", "path", 0, 0, 0, 0, 0, P, None, 0, 16, 16),
    ("whitted at 16 frames, memory bound", "whitted", 100 * GB, 288 * GB, 0, 0, 0, whitted_per_sample(16), None, HD, 64, 6),   # 80 GB / 6 092 B = 13 131 976 samples
]


def _expected(case):
    _, driver, free_b, total_b, held, need, have, per, env, n_px, spp, _ = case
    if driver == "path":
        return path_chunk_spp(free_b, total_b, held, need, have, per, env, n_px, spp)
    assert need == 0 and have == 0
    return whitted_chunk_spp(free_b, total_b, held, per, env, n_px, spp)


@pytest.fixture(scope="module")
def check_output():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("needs hipcc to compile the shared header for the host")
    lines = []
    for _, driver, free_b, total_b, held, need, have, per, env, n_px, spp, _ in CASES:
        ceiling, floor = (128 * MI, MI) if driver == "path" else (32 * MI, 64 * KI)
        reserve = need - have if need > have else 0     # what render_tiles hands over; the Whitted driver hands over 0
        lines.append(" ".join(str(v) for v in (ceiling, floor, free_b, total_b, held, reserve, per, env if env is not None else "-", n_px, spp)))
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "chunk_plan_check.sh")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


def test_hand_worked_values_follow_from_the_drivers_expressions():
    for case in CASES:
        assert _expected(case) == case[-1], case[:2]


def test_planned_chunk_spp_is_what_the_drivers_computed(check_output):
    got = [int(l.split("=")[1]) for l in check_output if l.startswith("plan =")]
    assert len(got) == len(CASES)
    for case, g in zip(CASES, got):
        assert g == _expected(case) == case[-1], (case[:2], g)


def test_table_sums_are_the_hand_formulas(check_output):
    tables = {l.split("=")[0].strip(): int(l.split("=")[1]) for l in check_output if l.startswith("table ")}
    want = {"table path general %d textured %d" % (g, t): path_per_path(bool(t)) for g in (0, 1) for t in (0, 1)}   # plain matte, general, textured, both
    want.update({"table whitted n_frames %d" % n: whitted_per_sample(n) for n in (1, 5, 16)})
    assert tables == want
    assert (P, PT, whitted_per_sample(1), W5, whitted_per_sample(16)) == (463, 591, 812, 2220, 6092)
