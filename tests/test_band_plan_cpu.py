"""The band planner of the wavefront drivers (pbrt-v3-rs_amd/csrc/band_plan.h), run on the CPU by scripts/band_plan_check.cpp under the address and undefined-behaviour
sanitizers: which runs of a rank's tiles have their sample records (20 B per camera sample) resident together, for budgets from below one tile's records to above the frame's.
The tile lists are restated here from the tile enumeration of the drivers (Film::get_sample_bounds, film/mod.rs:150-159; SamplerIntegrator::render, sampler_integrator.rs:252-259).
Also: the two entry points are exported and refuse a null handle.  No GPU is needed."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = 20


def rank_tile_pixels(crop, radius, tile=16, part=0, parts=1):
    """pixels of every tile of a rank, in increasing tile index"""
    sb = (math.floor(crop[0] + 0.5 - radius), math.floor(crop[1] + 0.5 - radius), math.ceil(crop[2] - 0.5 + radius), math.ceil(crop[3] - 0.5 + radius))
    ntx, nty = max((sb[2] - sb[0] + tile - 1) // tile, 0), max((sb[3] - sb[1] + tile - 1) // tile, 0)
    px = []
    for t in range(part, ntx * nty, parts):
        tx, ty = t % ntx, t // ntx
        x0, y0 = sb[0] + tx * tile, sb[1] + ty * tile
        px.append((min(x0 + tile, sb[2]) - x0) * (min(y0 + tile, sb[3]) - y0))
    return px


def greedy_bands(px, spp, budget):
    """the planner's contract restated: take tiles while the band's records stay within the budget; never less than one tile"""
    bands, cur = [], None
    for t, n in enumerate(px):
        if cur is None or (cur[3] + n) * spp * REC > budget:
            cur = [t, 0, sum(px[:t]), 0]
            bands.append(cur)
        cur[1] += 1
        cur[3] += n
    return [tuple(b) for b in bands]


FRAMES = [
    ("64x48, box filter: 12 whole tiles", rank_tile_pixels((0, 0, 64, 48), 0.5), 8),
    ("64x48, gaussian radius 2: 68x52 samples, ragged last column and row", rank_tile_pixels((0, 0, 64, 48), 2.0), 8),
    ("crop not aligned to tiles", rank_tile_pixels((5, 3, 59, 41), 0.5), 8),
    ("tile part 1 of 3", rank_tile_pixels((0, 0, 64, 48), 2.0, part=1, parts=3), 8),
    ("tile part 2 of 3 of a cropped frame", rank_tile_pixels((5, 3, 59, 41), 2.0, part=2, parts=3), 4),
    ("one tile", rank_tile_pixels((0, 0, 7, 5), 0.5), 3),
    ("more parts than tiles: a rank without pixels", rank_tile_pixels((0, 0, 16, 16), 0.5, part=3, parts=4), 8),
    ("no pixels at all", [], 16),
    ("1920x1080 at 8192 spp: products beyond 2^32", rank_tile_pixels((0, 0, 1920, 1080), 0.5), 8192),
]


def _budgets(px, spp):
    if not px:
        return [1, 10 ** 12]
    one, frame = max(px) * spp * REC, sum(px) * spp * REC
    return [1, min(px) * spp * REC - 1, min(px) * spp * REC, one - 1, one, one + 1, 3 * one, 5 * one, frame // 4, frame // 2, frame - 1, frame, frame + 1, 2 ** 63]


CASES = [(name, px, spp, b) for name, px, spp in FRAMES for b in _budgets(px, spp)]
# (rec_need, free, total, held, min_chunk, expected): one band where records and the smallest chunk fit into free + held or nothing is known about the memory, else half of 80 % free + held
GB = 10 ** 9
AUTO = [
    (21 * GB, 280 * GB, 288 * GB, 0, 1 * GB, 21 * GB),
    (279 * GB, 280 * GB, 288 * GB, 0, 1 * GB, 279 * GB),
    (279 * GB + 1, 280 * GB, 288 * GB, 0, 1 * GB, 112 * GB),
    (680 * GB, 280 * GB, 288 * GB, 0, 4 * GB, 112 * GB),
    (680 * GB, 200 * GB, 288 * GB, 80 * GB, 4 * GB, 120 * GB),
    (30 * GB, 10 * GB, 288 * GB, 25 * GB, 1 * GB, 30 * GB),
    (680 * GB, 0, 0, 0, 4 * GB, 680 * GB),
    (5, 0, 288 * GB, 0, 0, 1),
]


@pytest.fixture(scope="module")
def answers():
    lines = ["plan %d %d %d %s" % (spp, b, len(px), " ".join(map(str, px))) for _, px, spp, b in CASES]
    lines += ["auto %d %d %d %d %d" % a[:5] for a in AUTO]
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "band_plan_check.sh")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]   # (a sanitizer report ends the program with a non-zero status)
    got = out.stdout.splitlines()
    assert len(got) == len(CASES) + len(AUTO)
    bands = [[tuple(int(v) for v in w.split(":")) for w in l.split("=")[1].split()] for l in got[:len(CASES)]]
    return bands, [int(l.split("=")[1]) for l in got[len(CASES):]]


def test_frames_have_the_shapes_the_cases_are_about():
    shapes = {name: px for name, px, _ in FRAMES}
    assert shapes["64x48, box filter: 12 whole tiles"] == [256] * 12
    ragged = shapes["64x48, gaussian radius 2: 68x52 samples, ragged last column and row"]
    assert len(ragged) == 20 and sorted(set(ragged)) == [16, 64, 256]
    assert len(shapes["tile part 1 of 3"]) == 7 and shapes["more parts than tiles: a rank without pixels"] == []


def test_every_tile_is_in_exactly_one_band_in_order(answers):
    for (name, px, spp, budget), bands in zip(CASES, answers[0]):
        tile, pixel = 0, 0
        for t0, n, p0, npx in bands:
            assert (t0, p0) == (tile, pixel) and n >= 1, (name, budget)
            assert npx == sum(px[t0:t0 + n]), (name, budget)
            tile, pixel = tile + n, pixel + npx
        assert (tile, pixel) == (len(px), sum(px)), (name, budget)


def test_a_band_is_within_the_budget_or_a_single_tile(answers):
    for (name, px, spp, budget), bands in zip(CASES, answers[0]):
        for t0, n, p0, npx in bands:
            assert npx * spp * REC <= budget or n == 1, (name, budget)
        # ... and no band stops short: the next tile would not have fitted
        for (t0, n, p0, npx), nxt in zip(bands, bands[1:]):
            assert (npx + px[nxt[0]]) * spp * REC > budget, (name, budget)


def test_bands_are_the_greedy_runs(answers):
    for (name, px, spp, budget), bands in zip(CASES, answers[0]):
        assert bands == greedy_bands(px, spp, budget), (name, budget)


def test_budget_below_one_tile_gives_one_tile_per_band_and_a_frame_that_fits_one_band(answers):
    for (name, px, spp, budget), bands in zip(CASES, answers[0]):
        if px and budget < min(px) * spp * REC:
            assert [b[1] for b in bands] == [1] * len(px), (name, budget)
        if px and budget >= sum(px) * spp * REC:
            assert len(bands) == 1, (name, budget)


def test_no_pixels_no_bands(answers):
    for (name, px, spp, budget), bands in zip(CASES, answers[0]):
        if not px:
            assert bands == [], (name, budget)


def test_tiles_per_band_of_the_whole_tile_frame(answers):
    got = {(name, budget): bands for (name, px, spp, budget), bands in zip(CASES, answers[0])}
    one = 256 * 8 * REC
    name = "64x48, box filter: 12 whole tiles"
    assert [b[1] for b in got[(name, 3 * one)]] == [3, 3, 3, 3]
    assert [b[1] for b in got[(name, 5 * one)]] == [5, 5, 2]
    assert [b[1] for b in got[(name, one)]] == [1] * 12


def test_automatic_budget(answers):
    for case, got in zip(AUTO, answers[1]):
        assert got == case[5], case


def test_entry_points_are_exported_and_refuse_a_null_handle():
    import pbrt_hip
    b = pbrt_hip.default_binding()
    assert b.has("set_sample_record_budget") and b.has("get_render_footprint")
    assert b.fn("set_sample_record_budget")(None, 1 << 20) == pbrt_hip.ERR_INVALID_ARG
    out = (C.c_uint64 * 8)()
    assert b.fn("get_render_footprint")(None, out) == pbrt_hip.ERR_INVALID_ARG
    assert hasattr(pbrt_hip.Scene, "set_sample_record_budget") and hasattr(pbrt_hip.Scene, "render_footprint")
