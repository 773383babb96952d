"""-m gpu: the device's light code (light_le / light_sample_li / light_pdf_li of csrc/pt_device.h in both instantiations, the radiance-map functions of csrc/texture.h,
wh_light_sample_li / sphere_light_sample_li of csrc/sphere_light.h) against the oracle on explicit inputs, through pbrt_hip_light_probe_batch.  Per light set of
light_probe_cases.LIGHT_SETS, every output of every probe — the sample, the far end of its visibility tester and the shadow ray spawn_ray_to_hit makes of it, pdf_li, le —
must equal the oracle's bits (sign of zero included; a NaN asks for a NaN in the same slot).  test_light_probe_cases_cpu.py measures, on the oracle alone, which branches
the sets reach.  No renders here."""
import numpy as np
import pytest

import pbrt_hip
import light_probe_cases as lc
from oracle_binding import OracleScene, set_libm_mode
from probe_cases import first_difference, hexf

pytestmark = pytest.mark.gpu
F = np.float32
_cache = {}


def light_pair(name, host):
    """(product scene, batches, the oracle's outputs in libm mode 1) of one light set; computed once, shared by the tests below and left unchanged."""
    if name not in _cache:
        ls = lc.LIGHT_SET_BY_NAME[name]
        orc = OracleScene(); prod = pbrt_hip.Scene()
        ls.capture(orc, host); ls.capture(prod, host)
        batches = ls.cases(orc, host)   # the very set test_light_probe_cases_cpu.py measured
        set_libm_mode(1)
        try:
            want = lc.run_batches(orc, batches, ls.variant)
        finally:
            set_libm_mode(0)
        _cache[name] = (prod, batches, want)
    return _cache[name]


def assert_same(name, batches, got, want, what):
    for b, g, w in zip(batches, got, want):
        i = first_difference(g, w)
        assert i < 0, f"{what}: {lc.describe(name, b, i)}\n  device {hexf(g[i])}\n  oracle {hexf(w[i])}"


@pytest.mark.parametrize("name", [s.name for s in lc.LIGHT_SETS])
def test_light_probe_bit_exact(host, name):
    prod, batches, want = light_pair(name, host)
    variant = lc.LIGHT_SET_BY_NAME[name].variant
    assert_same(name, batches, lc.run_batches(prod, batches, variant), want, f"variant {variant}")


@pytest.mark.parametrize("name", [s.name for s in lc.LIGHT_SETS if s.variant == 0])
def test_texture_free_instantiation_equals_the_textured_one_and_the_oracle(host, name):
    """variant 1 = the MAP = false instantiations of the texture-free kernels, on every light of the set that holds no map"""
    prod, batches, want = light_pair(name, host)
    mapped = lc.LIGHT_SET_BY_NAME[name].mapped
    sub = [(b, w) for b, w in zip(batches, want) if b["light"] not in mapped]
    if not sub:
        assert name == "infinite_map"   # every light of that set holds a map: refused below
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            lc.run_batches(prod, batches[:1], 1)
        assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
        return
    bs, ws = [b for b, _ in sub], [w for _, w in sub]
    assert sum(len(b["ref"]) for b in bs) >= 500
    plain = lc.run_batches(prod, bs, 1)
    assert_same(name, bs, plain, ws, "variant 1 against the oracle")
    assert_same(name, bs, plain, lc.run_batches(prod, bs, 0), "variant 1 against variant 0")


@pytest.mark.parametrize("name", ["point_distant", "triangle", "infinite_map"])
def test_whitted_light_loop_equals_the_path_integrators_sample_li(host, name):
    """variant 2 on lights that are not spheres: wh_light_sample_li hands them to light_sample_li<true>"""
    prod, batches, want = light_pair(name, host)
    sub = [(b, w) for b, w in zip(batches, want) if b["op"] == 0]
    bs, ws = [b for b, _ in sub], [w for _, w in sub]
    assert_same(name, bs, lc.run_batches(prod, bs, 2), ws, "variant 2 against the oracle")


def test_refusals_leave_the_handle_usable(host):
    prod, batches, want = light_pair("projection", host)
    b = batches[0]
    n_lights = len(lc.PROJECTIONS)
    mapped = sorted(lc.LIGHT_SET_BY_NAME["projection"].mapped)[0]

    def refused(scene, code, *a, **kw):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            scene.light_probe_batch(*a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert scene.last_error() != ""

    ref = b["ref"][:4]
    refused(prod, pbrt_hip.ERR_INVALID_ARG, n_lights, 0, ref)                    # an unknown light
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, 3, ref)                           # an unknown op
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, -1, ref)
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, 0, ref, variant=3)                # an unknown variant
    refused(prod, pbrt_hip.ERR_INVALID_ARG, 0, 1, ref, variant=2)                # the Whitted light loop has sample_li only
    refused(prod, pbrt_hip.ERR_UNSUPPORTED, mapped, 0, ref, variant=1)           # a projected image under the texture-free code
    fn = prod.b.fn("light_probe_batch")
    out = np.zeros((4, 28), F)
    fp = lambda a: a.ctypes.data_as(pbrt_hip.C.POINTER(pbrt_hip.C.c_float))
    assert fn(prod.h, 0, 0, 0, 4, None, fp(b["u"][:4].copy()), fp(b["wi"][:4].copy()), fp(out)) == pbrt_hip.ERR_INVALID_ARG   # null buffers with n > 0
    assert fn(prod.h, 0, 0, 0, 4, fp(ref.copy()), fp(b["u"][:4].copy()), fp(b["wi"][:4].copy()), None) == pbrt_hip.ERR_INVALID_ARG
    assert fn(prod.h, 0, 0, 0, 2 ** 32, fp(ref.copy()), fp(b["u"][:4].copy()), fp(b["wi"][:4].copy()), fp(out)) == pbrt_hip.ERR_INVALID_ARG   # more than 2^32 - 1 probes
    assert prod.last_error() != ""
    assert fn(prod.h, 0, 0, 0, 0, None, None, None, None) == pbrt_hip.OK        # nothing to do
    # a spherical light under the path integrator's variants
    sph, sb, _ = light_pair("sphere", host)
    refused(sph, pbrt_hip.ERR_UNSUPPORTED, 0, 0, sb[0]["ref"][:4], variant=0)
    refused(sph, pbrt_hip.ERR_UNSUPPORTED, 0, 0, sb[0]["ref"][:4], variant=1)
    # no accelerator, an area light without its mesh
    bare = pbrt_hip.Scene()
    bare.add_light_point((1, 1, 1), (0, 0, 1))
    refused(bare, pbrt_hip.ERR_STATE, 0, 0, ref)
    lc.add_floor(bare); bare.build_accel(0, 4); bare.add_light_diffuse_area((1, 1, 1), 1)
    refused(bare, pbrt_hip.ERR_STATE, 1, 0, ref)
    assert bare.light_probe_batch(0, 0, ref).shape == (4, 28)
    # the handles still answer, and as before
    assert_same("projection", [b], [prod.light_probe_batch(b["light"], b["op"], b["ref"], b["u"], b["wi"])], [want[0]], "after the refusals")
    assert_same("sphere", sb[:1], lc.run_batches(sph, sb[:1], 2), light_pair("sphere", host)[2][:1], "after the refusals")
