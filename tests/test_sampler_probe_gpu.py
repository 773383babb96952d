"""-m gpu: the device's Halton and Sobol samplers (csrc/pt_device.h, cursor_for in csrc/wf_device.h) against the oracle on explicit (pixel, sample number, dimension)
triples, through pbrt_hip_sampler_value_batch.  Every value must equal the oracle's bit for bit; under Halton the LDS copy of the first 54 dimensions' tables must
give the same bits as the global tables.  The case sets are probe_cases.py's (measured on the oracle by test_probe_cases_cpu.py).  No renders here."""
import os

import numpy as np
import pytest

import pbrt_hip
import probe_cases as pc
from oracle_binding import OracleScene, set_libm_mode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def sobol_tables(name):
    z = np.load(os.path.join(HERE, "golden", name))
    return z["m32"], z["vdc"], z["vdc_inv"]


def first_bad(got, want):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    return int(bad[0]) if len(bad) else -1


def assert_same(what, xy, smp, dim, got, want):
    i = first_bad(got, want)
    assert i < 0, f"{what}: pixel {tuple(xy[i])} sample {smp[i]} dimension {dim[i]}: device {float(got[i]).hex()} oracle {float(want[i]).hex()}"


@pytest.mark.parametrize("setup", pc.HALTON_SETUPS, ids=[s[0] for s in pc.HALTON_SETUPS])
def test_halton_values_bit_exact_with_and_without_lds(setup):
    name, bounds, spp = setup
    orc = OracleScene(); prod = pbrt_hip.Scene()
    orc.set_sampler(0, spp, bounds); prod.set_sampler(0, spp, bounds)
    xy, smp, dim = pc.halton_cases(bounds, spp)
    set_libm_mode(1)
    try:
        want = orc.sampler_value_batch(xy, smp, dim)
    finally:
        set_libm_mode(0)
    plain = prod.sampler_value_batch(xy, smp, dim, use_lds=False)
    lds = prod.sampler_value_batch(xy, smp, dim, use_lds=True)
    assert_same(f"halton {name}, global tables", xy, smp, dim, plain, want)
    assert_same(f"halton {name}, LDS tables", xy, smp, dim, lds, want)
    assert_same(f"halton {name}, LDS against global", xy, smp, dim, lds, plain)


def test_halton_at_pixel_centre():
    """sample_at_pixel_center: dimensions 0 and 1 are 0.5, the others unchanged."""
    bounds = (0, 0, 200, 150)
    orc = OracleScene(); prod = pbrt_hip.Scene()
    orc.set_sampler(0, 16, bounds, True); prod.set_sampler(0, 16, bounds, True)
    xy, smp, dim = pc.halton_cases(bounds, 16)
    want = orc.sampler_value_batch(xy, smp, dim)
    assert (want[dim < 2] == 0.5).all()
    for use_lds in (False, True):
        assert_same(f"halton at pixel centre, lds {use_lds}", xy, smp, dim, prod.sampler_value_batch(xy, smp, dim, use_lds=use_lds), want)


@pytest.mark.parametrize("fixture", ["sobol_subset.npz", "sobol_subset_64.npz"])
def test_sobol_values_bit_exact(fixture):
    m32, vdc, vdci = sobol_tables(fixture)
    n_dims = len(m32) // 52
    for res in pc.SOBOL_RESOLUTIONS:
        for mn in pc.SOBOL_MINIMA:
            orc = OracleScene(); prod = pbrt_hip.Scene()
            bounds, xy, smp, dim = pc.sobol_cases(res, mn, n_dims)
            for s in (orc, prod):
                s.set_sobol_tables(m32, vdc, vdci); s.set_sampler(1, 16, bounds)
            want = orc.sampler_value_batch(xy, smp, dim)
            assert_same(f"sobol {fixture} {res} from {mn}", xy, smp, dim, prod.sampler_value_batch(xy, smp, dim), want)
            assert_same(f"sobol {fixture} {res} from {mn} (use_lds is Halton's)", xy, smp, dim, prod.sampler_value_batch(xy, smp, dim, use_lds=True), want)


def test_refusals_leave_the_handle_usable():
    m32, vdc, vdci = sobol_tables("sobol_subset.npz")
    prod = pbrt_hip.Scene()

    def refused(code, *a):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            prod.sampler_value_batch(*a)
        assert e.value.code == code, (e.value.code, str(e.value))

    refused(pbrt_hip.ERR_STATE, [(0, 0)], [0], [0])                           # no sampler yet
    prod.set_sampler(1, 16, (0, 0, 100, 60))
    refused(pbrt_hip.ERR_STATE, [(0, 0)], [0], [0])                           # Sobol without tables
    prod.set_sobol_tables(m32, vdc, vdci)
    refused(pbrt_hip.ERR_UNSUPPORTED, [(0, 0)], [0], [len(m32) // 52])        # a dimension beyond the tables
    refused(pbrt_hip.ERR_INVALID_ARG, [(128, 0)], [0], [0])                   # a pixel outside the sampler's 128 x 128 square
    refused(pbrt_hip.ERR_INVALID_ARG, [(0, -1)], [0], [0])
    prod.set_sampler(1, 16, (0, 0, 1024, 1024))
    refused(pbrt_hip.ERR_UNSUPPORTED, [(0, 0)], [0], [0])                     # ten VdC matrices needed, nine given
    prod.set_sampler(0, 16, (0, 0, 100, 60))
    refused(pbrt_hip.ERR_INVALID_ARG, [(0, 0)], [0], [1000])                  # the Halton tables end at dimension 999
    orc = OracleScene(); orc.set_sampler(0, 16, (0, 0, 100, 60))
    xy, smp, dim = pc.halton_cases((0, 0, 100, 60), 16)
    assert_same("after the refusals", xy, smp, dim, prod.sampler_value_batch(xy, smp, dim, use_lds=True), orc.sampler_value_batch(xy, smp, dim))
