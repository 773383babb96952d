"""-m gpu: the device's BSDF code (csrc/bsdf_general.h, the one-lobe matte path of csrc/pt_device.h) against the oracle on explicit inputs, through
pbrt_hip_bsdf_probe_batch.  Per material of probe_cases.MATERIALS, every probe of its case set — edge directions, sample values at the branch thresholds, seven flag
sets, frames whose normals disagree — must equal the oracle's output bit for bit (sign of zero and sampled type included; a NaN asks for a NaN in the same slot).
test_probe_cases_cpu.py measures, on the oracle alone, which branches the sets reach.  No renders here."""
import numpy as np
import pytest

import pbrt_hip
import probe_cases as pc
from oracle_binding import OracleScene, set_libm_mode

pytestmark = pytest.mark.gpu
F = np.float32
_cache = {}


def material_pair(name):
    """(product scene, material id, batches, the oracle's outputs in libm mode 1) of one probe material; computed once, shared by the tests below and left unchanged."""
    if name not in _cache:
        mat = pc.MATERIAL_BY_NAME[name]
        orc = OracleScene(); prod = pbrt_hip.Scene()
        mid = mat.make(orc)
        assert mat.make(prod) == mid
        batches = pc.bsdf_cases(mat, orc, mid)   # the very set test_probe_cases_cpu.py measured
        set_libm_mode(1)
        try:
            want = pc.run_batches(orc, mid, batches)
        finally:
            set_libm_mode(0)
        _cache[name] = (prod, mid, batches, want)
    return _cache[name]


def assert_same(name, batches, got, want, what):
    for b, g, w in zip(batches, got, want):
        i = pc.first_difference(g, w)
        assert i < 0, f"{what}: {pc.describe(name, b, i)}\n  device {pc.hexf(g[i])}\n  oracle {pc.hexf(w[i])}"


@pytest.mark.parametrize("name", [m.name for m in pc.MATERIALS])
def test_bsdf_probe_bit_exact(name):
    prod, mid, batches, want = material_pair(name)
    assert_same(name, batches, pc.run_batches(prod, mid, batches), want, "general BSDF")


@pytest.mark.parametrize("name", [m.name for m in pc.MATERIALS if m.matte])
def test_matte_one_lobe_path_equals_general_path_and_oracle(name):
    """path 1 = the Bsdf of shade_kernel<false>.  It has no flags: the probe admits the flag sets that hold its lobe's type, and those cases must match bit for bit."""
    prod, mid, batches, want = material_pair(name)
    sub, sub_want = [], []
    for b, w in zip(batches, want):
        keep = (b["flags"] & 5) == 5
        if keep.any():
            sub.append(dict(op=b["op"], frame=b["frame"], wo=b["wo"][keep], wi=b["wi"][keep], u=b["u"][keep], flags=b["flags"][keep])); sub_want.append(w[keep])
    assert sum(len(b["wo"]) for b in sub) > 5000
    one_lobe = pc.run_batches(prod, mid, sub, path=1)
    assert_same(name, sub, one_lobe, sub_want, "one-lobe matte BSDF against the oracle")
    assert_same(name, sub, one_lobe, pc.run_batches(prod, mid, sub, path=0), "one-lobe matte BSDF against the general BSDF")


def test_refusals_leave_the_handle_usable():
    _, mid, batches, want = material_pair("plastic")
    prod = pbrt_hip.Scene()   # a handle of its own: the refusals below add materials
    assert pc.MATERIAL_BY_NAME["plastic"].make(prod) == mid
    b = batches[1]
    args = (b["wo"][:4], b["wi"][:4], b["u"][:4], b["flags"][:4])

    def refused(code, *a, **kw):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            prod.bsdf_probe_batch(*a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert prod.last_error() != ""

    refused(pbrt_hip.ERR_UNSUPPORTED, mid, 0, *args, path=1)                  # path 1 on a material that is not matte
    refused(pbrt_hip.ERR_INVALID_ARG, mid + 1000, 0, *args)                   # an unknown material
    refused(pbrt_hip.ERR_INVALID_ARG, mid, 3, *args)                          # an unknown op
    tex = prod.add_texture_constant((0.5, 0.5, 0.5))
    refused(pbrt_hip.ERR_UNSUPPORTED, prod.add_material_matte_tex(tex, 0.0), 0, *args)   # a textured material, on either path
    bumped = prod.add_material_matte((0.5, 0.5, 0.5), 0.0)
    prod.set_material_bump(bumped, tex)
    refused(pbrt_hip.ERR_UNSUPPORTED, bumped, 0, *args, path=1)
    matte = prod.add_material_matte((0.5, 0.5, 0.5), 0.0)
    refused(pbrt_hip.ERR_INVALID_ARG, matte, 0, args[0], args[1], args[2], np.array([31, 31, 2, 31], np.uint32), path=1)   # path 1 has no flags to apply
    # the handle still answers, and as before
    got = prod.bsdf_probe_batch(mid, b["op"], b["wo"], b["wi"], b["u"], b["flags"])
    assert_same("plastic", [b], [got], [want[1]], "after the refusals")
