"""The film probe's case sets (tests/film_probe_cases.py) proven on the CPU: the oracle's film probe (oracle_film_probe: get_film_tile, add_sample over the tile's pixels
row-major and then by sample index, the merge loop of its renders) against the float64 twin within gamma(n + 2) * sum|terms| per pixel, its layout against the tile
enumeration restated in the case module, its tiles against its film, and every family a case names counted in the case's own samples.  No GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import film_probe_cases as fc
import pbrt_hip
from oracle_binding import OracleScene


@pytest.fixture(scope="module")
def oracle_results():
    out = {}
    for case in fc.CASES:
        orc = OracleScene()
        case.setup(orc)
        px, L, pf = fc.samples(case)
        out[case.name] = (orc.film_probe_tiles(L, pf, case.tile), orc.film_probe_layout(case.tile))
    return out


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_oracle_is_within_the_twins_bound(case, oracle_results):
    (xyz, wt, tiles), _ = oracle_results[case.name]
    txyz, tw, bxyz, bw, st = fc.twin_of(case.name)
    assert np.isfinite(xyz).all() and np.isfinite(txyz).all()
    dx, dw = np.abs(xyz.astype(np.float64) - txyz), np.abs(wt.astype(np.float64) - tw)
    print(case.name, "largest error / bound: xyz %.3g weight %.3g" % (float((dx / np.maximum(bxyz, 1e-300)).max()), float((dw / np.maximum(bw, 1e-300)).max())))
    assert (dx <= bxyz).all(), (case.name, float((dx - bxyz).max()))
    assert (dw <= bw).all(), (case.name, float((dw - bw).max()))
    assert (wt[st_terms_zero(case)] == 0).all()


def st_terms_zero(case):
    """pixels the twin gives no term: the oracle's weight there is exactly 0"""
    _, tw, _, bw, _ = fc.twin_of(case.name)
    return bw == 0


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_every_family_of_the_case_is_present(case):
    st = fc.twin_of(case.name)[4]
    missing = [k for k in fc.ALWAYS + case.expect if not st[k] > 0]
    assert not missing, (case.name, missing, st)


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_layout_and_tiles_of_the_oracle(case, oracle_results):
    (xyz, wt, tiles), (px, pbs, _) = oracle_results[case.name]
    want_px, _ = fc.pixel_list(case)
    assert np.array_equal(px, want_px)
    sb, ntx, nty = fc.tile_grid(case)
    assert len(tiles) == ntx * nty == len(pbs)
    # the film is the tiles' sums in increasing tile order (Film::merge_film_tile), restated here in float32
    c = case.crop
    film = np.zeros((c[3] - c[1], c[2] - c[0], 3), np.float32); weight = np.zeros(film.shape[:2], np.float32)
    for pb, sums in tiles:
        if sums.size == 0:
            continue
        rgb = sums[..., :3]
        sl = (slice(pb[1] - c[1], pb[3] - c[1]), slice(pb[0] - c[0], pb[2] - c[0]))
        for k in range(3):
            film[sl + (k,)] += fc.XYZ[k, 0] * rgb[..., 0] + fc.XYZ[k, 1] * rgb[..., 1] + fc.XYZ[k, 2] * rgb[..., 2]
        weight[sl] += sums[..., 3]
    assert np.array_equal(fc.bits(film), fc.bits(xyz)) and np.array_equal(fc.bits(weight), fc.bits(wt))


def test_parts_of_the_oracle_are_the_frames_tiles_dealt_round_robin(oracle_results):
    case = fc.BY_NAME["parts 2 and 3"]
    (_, _, whole), _ = oracle_results[case.name]
    for parts in (2, 3):
        for part in range(parts):
            orc = OracleScene()
            case.setup(orc)
            px, L, pf = fc.for_part(case, part, parts)
            _, _, tiles = orc.film_probe_tiles(L, pf, case.tile, part, parts)
            assert len(tiles) == len(whole[part::parts])
            for (pb, sums), (wpb, wsums) in zip(tiles, whole[part::parts]):
                assert np.array_equal(pb, wpb) and np.array_equal(fc.bits(sums), fc.bits(wsums))


def test_case_constants():
    assert fc.lum(fc.C_EQ) == np.float32(fc.MAX_LUM) and fc.lum(fc.C_OVER) > np.float32(fc.MAX_LUM) and fc.lum(fc.C_LUM0) == 0
    assert fc.C_LUM0[0] > 0 > fc.C_LUM0[1]
    assert (fc.clamped(fc.C_EQ, fc.MAX_LUM) != fc.C_EQ).all()   # a clamp applied at equality would move every component
    names = {c.name for c in fc.CASES}
    assert {"hair under .5", "hair under 1.5", "hair under 2.5", "1.4998 from 4096", "17 .5: wider than a tile"} <= names
    assert {p for c in fc.CASES for p in c.parts} == {1, 2, 3, 64} and {b for c in fc.CASES for b in c.bands} == {None, "tile", "two"}
    assert {c.tile for c in fc.CASES} >= {1, 2, 3, 16, 64} and {c.max_lum for c in fc.CASES} == {fc.INF, 0.0, fc.MAX_LUM}


def test_entry_points_are_exported_and_refuse_a_null_handle():
    b = pbrt_hip.default_binding()
    assert b.has("film_probe") and b.has("film_probe_layout")
    out = (C.c_uint64 * 4)()
    assert b.fn("film_probe_layout")(None, 16, 0, 1, out, None, None) == pbrt_hip.ERR_INVALID_ARG
    assert b.fn("film_probe")(None, 16, 0, 1, 0, None, None, None, None, None, None) == pbrt_hip.ERR_INVALID_ARG
    assert hasattr(pbrt_hip.Scene, "film_probe") and hasattr(pbrt_hip.Scene, "film_probe_layout")
