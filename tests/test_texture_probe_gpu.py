"""-m gpu: the device's texture code (csrc/texture.h: tex_eval in its four instantiations, alpha_prog_r, bump_shading, mip_lookup / mip_triangle / mip_ewa in both forms of
its loops, the procedural textures and the 2D mappings) against the oracle on explicit inputs, through pbrt_hip_texture_probe_batch and pbrt_hip_bump_probe_batch.  Per set of
texture_probe_cases.SETS and per variant, every output of every probe must equal the oracle's bits (sign of zero included; a NaN asks for a NaN in the same slot).  Every set
has been through the oracle before it reaches the device (texture_probe_cases.prepared), with its work per probe counted and capped there; test_texture_probe_cases_cpu.py
measures, on the oracle alone, which branches the sets reach.  No renders here."""
import numpy as np
import pytest

import pbrt_hip
import texture_probe_cases as tc
from probe_cases import first_difference, hexf

pytestmark = pytest.mark.gpu
F = np.float32
_prod = {}


def product_scene(name, host):
    if name not in _prod:
        _prod[name] = tc.capture_product(name, host)
    return _prod[name]


def assert_same(name, ps, batches, got, want, what):
    key = "inp" if ps.kind == "bump" else "ctx"
    n = 0
    for b, g, w in zip(batches, got, want):
        if w is None:
            assert g is None
            continue
        i = first_difference(g, w)
        assert i < 0, f"{what}: {tc.describe(name, b, i, key)}\n  device {hexf(g[i])}\n  oracle {hexf(w[i])}"
        n += len(w)
    assert n >= 500, n


def check(name, variant, host):
    ps, orc, batches, work, want = tc.prepared(name, host)   # raises, before any launch, if a probe is above a work cap
    prod = product_scene(name, host)
    assert_same(name, ps, batches, tc.run_batches(prod, ps, batches, variant), want[variant], f"variant {variant}")


SET_VARIANTS = [(s.name, v) for s in tc.SETS if s.name != "ewa_saturated" for v in s.variants]


@pytest.mark.parametrize("name,variant", SET_VARIANTS, ids=[f"{n}-{v}" for n, v in SET_VARIANTS])
def test_texture_probe_bit_exact(host, name, variant):
    check(name, variant, host)


@pytest.mark.parametrize("variant", tc.SET_BY_NAME["ewa_saturated"].variants)
def test_ewa_saturated_bit_exact(host, variant):
    """texel coordinates at +-2^62, +-2^63 and 3e38: the footprint loops' bounds are isize::MAX and must be visited once (scripts/ewa_loop_check.cpp runs the oracle's on the CPU)"""
    check("ewa_saturated", variant, host)


def test_refusals_leave_the_handle_usable(host):
    ps, orc, batches, work, want = tc.prepared("procedural_2d", host)
    prod = product_scene("procedural_2d", host)
    b = batches[0]   # a checkerboard: not a program of constants, image maps, scale and mix
    c4 = np.ascontiguousarray(b["ctx"][:4])
    n_tex = 64

    def refused(fn, code, word, *a):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            fn(*a)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert word in str(e.value) and prod.last_error() != ""

    i33 = np.zeros((4, 33), F)
    for fn, arg, who in ((prod.texture_probe_batch, c4, "texture_probe_batch"), (prod.bump_probe_batch, i33, "bump_probe_batch")):
        refused(fn, pbrt_hip.ERR_INVALID_ARG, who + ": unknown texture", n_tex, arg, 0)
        refused(fn, pbrt_hip.ERR_INVALID_ARG, who + ": unknown variant", b["tex"], arg, -1)
        refused(fn, pbrt_hip.ERR_UNSUPPORTED, who + ": variants 2 and above", b["tex"], arg, 2)
        refused(fn, pbrt_hip.ERR_UNSUPPORTED, who + ": variants 2 and above", b["tex"], arg, 3)
    refused(prod.texture_probe_batch, pbrt_hip.ERR_INVALID_ARG, "unknown variant", b["tex"], c4, 5)
    refused(prod.texture_probe_batch, pbrt_hip.ERR_UNSUPPORTED, "variants 2 and above", b["tex"], c4, 4)
    refused(prod.bump_probe_batch, pbrt_hip.ERR_INVALID_ARG, "unknown variant", b["tex"], i33, 4)
    fp = lambda a: a.ctypes.data_as(pbrt_hip.C.POINTER(pbrt_hip.C.c_float))
    out = np.zeros((4, 6), F)
    for name, arr in (("texture_probe_batch", c4), ("bump_probe_batch", i33)):
        fn = prod.b.fn(name)
        assert fn(prod.h, b["tex"], 0, 4, None, fp(out)) == pbrt_hip.ERR_INVALID_ARG and "null argument" in prod.last_error()     # null buffers with n > 0
        assert fn(prod.h, b["tex"], 0, 4, fp(arr), None) == pbrt_hip.ERR_INVALID_ARG and "null argument" in prod.last_error()
        assert fn(prod.h, b["tex"], 0, 2 ** 32, fp(arr), fp(out)) == pbrt_hip.ERR_INVALID_ARG and "too many probes" in prod.last_error()   # more than 2^32 - 1 probes
        assert fn(prod.h, b["tex"], 0, 0, None, None) == pbrt_hip.OK                                                                # nothing to do
        assert fn(None, b["tex"], 0, 4, fp(arr), fp(out)) == pbrt_hip.ERR_INVALID_ARG
    # the handle still answers, and as before
    assert_same("procedural_2d", ps, batches[:1], tc.run_batches(prod, ps, batches[:1], 0), want[0][:1], "after the refusals")
