"""-m gpu: the render's own film pass and tile merge (film_tiles_kernel, merge_kernel and the host code that sizes tile slots and lists tiles, csrc/wavefront.hip and
csrc/film_plan.h) on explicit camera samples (pbrt_hip_film_probe) against the oracle's FilmTile::add_sample / Film::merge_film_tile (oracle_film_probe), bit for bit as
uint32: the film, the weights and every part's tile buffer, slot by slot.  The cases are tests/film_probe_cases.py; tests/test_film_probe_cases_cpu.py proves them on the CPU.
Every case also asserts, on its own samples, that the families it is about are in it."""
import numpy as np
import pytest
import torch

import film_probe_cases as fc
import pbrt_hip
from oracle_binding import OracleScene

pytestmark = pytest.mark.gpu


def _oracle(case, part=0, parts=1):
    orc = OracleScene()
    case.setup(orc)
    _, L, pf = fc.for_part(case, part, parts)
    return orc.film_probe_tiles(L, pf, case.tile, part, parts)


def _budget(case, mode):
    return {None: 0, "tile": 1, "two": 2 * case.tile_records()}[mode]


def _same_film(got, want, label):
    assert np.array_equal(fc.bits(got[1]), fc.bits(want[1])), (label, "weights", int((fc.bits(got[1]) != fc.bits(want[1])).sum()))
    nb = int((fc.bits(got[0]) != fc.bits(want[0])).any(-1).sum())
    assert nb == 0, (label, "film pixels that differ", nb)


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_film_and_tiles_equal_the_oracles(case):
    st = fc.twin_of(case.name)[4]
    missing = [k for k in fc.ALWAYS + case.expect if not st[k] > 0]
    assert not missing, (case.name, missing)
    prod = pbrt_hip.Scene()
    case.setup(prod)
    whole = _oracle(case)
    for mode in case.bands:
        prod.set_sample_record_budget(_budget(case, mode))
        for parts in case.parts:
            bufs = []
            for part in range(parts):
                label = (case.name, mode, part, parts)
                want = whole if parts == 1 else _oracle(case, part, parts)
                mine, L, pf = fc.for_part(case, part, parts)
                px, pbs, slot = prod.film_probe_layout(case.tile, part, parts)
                assert np.array_equal(px, mine), label
                # into the handle's own tile buffer: the film of this part's tiles alone, and a host copy of the buffer
                xyz, wt, buf = prod.film_probe(L, pf, case.tile, part, parts, tiles=True)
                _same_film((xyz, wt), want, label)
                assert fc.tile_buffer_mismatches(buf, slot, pbs, want[2]) == 0, label
                if mode is not None:
                    fp = prod.render_footprint()
                    n_tiles = len(pbs)   # one tile per band; or at least two per band (edge tiles are smaller) and, the frame being many tiles, still several bands
                    assert fp["bands"] == n_tiles if mode == "tile" else 1 < fp["bands"] <= (n_tiles + 1) // 2, (label, fp, n_tiles)
                if parts > 1:   # ... and into a buffer of the caller's, every float of which has to be written
                    dev = torch.full((prod.tile_buffer_floats(case.tile, part, parts),), float("nan"), dtype=torch.float32, device="cuda")
                    none_xyz, none_wt, host = prod.film_probe(L, pf, case.tile, part, parts, d_tile_buffer_ptr=dev.data_ptr(), tiles=True)
                    assert none_xyz is None and none_wt is None
                    torch.cuda.synchronize()
                    assert np.array_equal(fc.bits(dev.cpu().numpy()), fc.bits(host)) and fc.tile_buffer_mismatches(host, slot, pbs, want[2]) == 0, label
                    bufs.append(dev)
            if parts > 1:   # the parts' buffers merged in increasing tile index: the one-part film
                _same_film(prod.merge_tiles_device([b.data_ptr() for b in bufs], case.tile), whole, (case.name, mode, "merged", parts))
    prod.set_sample_record_budget(0)


def test_bands_end_on_columns_and_rows_that_carry_rounded_up_samples():
    """one tile per band: every tile edge is a band edge.  Samples ON the next tile's first column / row must reach the pixels of the band they belong to and no other."""
    for name in ("bands box", "bands 1.5 across 1024"):
        case = fc.BY_NAME[name]
        st = fc.twin_of(name)[4]
        assert st["rounded_on_tile_edge_x"] > 0 and st["rounded_on_tile_edge_y"] > 0
        prod = pbrt_hip.Scene()
        case.setup(prod)
        _, L, pf = fc.for_part(case, 0, 1)
        prod.set_sample_record_budget(1)
        got = prod.film_probe(L, pf, case.tile)
        fp = prod.render_footprint()
        sb, ntx, nty = fc.tile_grid(case)
        assert fp["bands"] == ntx * nty and fp["band_tiles"] == 1
        _same_film(got, _oracle(case), name)


def test_a_part_without_tiles_gives_an_empty_film_and_a_zero_slot():
    case = fc.BY_NAME["64 parts, fewer tiles"]
    sb, ntx, nty = fc.tile_grid(case)
    assert ntx * nty < 64
    prod = pbrt_hip.Scene()
    case.setup(prod)
    px, pbs, slot = prod.film_probe_layout(case.tile, 63, 64)
    assert len(px) == 0 and len(pbs) == 0
    xyz, wt, buf = prod.film_probe(np.zeros((case.spp, 0, 3), np.float32), np.zeros((case.spp, 0, 2), np.float32), case.tile, 63, 64, tiles=True)
    assert not fc.bits(xyz).any() and not fc.bits(wt).any() and len(buf) == slot[0] * slot[1] * 4 and not fc.bits(buf).any()


def test_refusals_leave_the_handle_usable():
    case = fc.BY_NAME["1.5 1.25 crop not on tiles"]
    prod = pbrt_hip.Scene()
    with pytest.raises(pbrt_hip.PbrtHipError) as e:   # no film yet
        prod.film_probe_layout(16)
    assert e.value.code == pbrt_hip.ERR_STATE
    case.setup(prod)
    px, L, pf = fc.for_part(case, 0, 1)
    want = _oracle(case)

    def refused(L, pf, **kw):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            prod.film_probe(L, pf, kw.pop("tile", case.tile), **kw)
        assert e.value.code == pbrt_hip.ERR_INVALID_ARG, e.value

    i = int(np.flatnonzero(~np.isnan(pf[0, :, 0]))[0])
    for axis in (0, 1):   # outside [x, x + 1]: a step above the closed upper end, a step below the pixel; the ends themselves are cases of the sets
        for v in (fc.above(px[i, axis] + 1), fc.below(px[i, axis])):
            bad = pf.copy(); bad[0, i, axis] = v
            refused(L, bad)
    bad = pf.copy(); bad[0, i, 1] = np.nan      # only a NaN x marks "no sample"
    refused(L, bad)
    for v in (np.inf, -np.inf, np.nan):
        bad = L.copy(); bad[0, i, 2] = v        # (of a sample that was taken: where none was, the radiance is not read)
        refused(bad, pf)
    refused(L, pf, tile=0); refused(L, pf, tile_part=1, tile_parts=1); refused(L, pf, tile_part=-1, tile_parts=2); refused(L, pf, tile_parts=65)
    refused(L[:, :-1], pf[:, :-1])                 # not the list's length
    _same_film(prod.film_probe(L, pf, case.tile), want, "after the refusals")
