"""The probe case sets (probe_cases.py) measured on the oracle alone: the oracle's batch probes equal its single probes, and the cases reach the branches they
were built for — counted from the oracle's own outputs, so that the GPU comparison (test_bsdf_probe_gpu.py, test_sampler_probe_gpu.py) is known to cover them."""
import os

import numpy as np
import pytest

import pbrt_hip
import probe_cases as pc
from oracle_binding import OracleScene, oracle_binding

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CANONICAL = np.array([0, 0, 1, 0, 0, 1, 1, 0, 0], F)
_cache = {}


def material_set(name):
    """(oracle scene, material id, batches, oracle outputs) of one probe material, computed once."""
    if name not in _cache:
        orc = OracleScene()
        mat = pc.MATERIAL_BY_NAME[name]
        mid = mat.make(orc)
        batches = pc.bsdf_cases(mat, orc, mid)
        _cache[name] = (orc, mid, batches, pc.run_batches(orc, mid, batches))
    return _cache[name]


def coverage(mat, batches, outs):
    """What the oracle's outputs say the set reached (the counts DESIGN.md quotes)."""
    c = dict(probes=0, nan=0, failed=0, spec_refl=0, spec_trans=0, tir=0, refracted=0, blend_diffuse=0, blend_specular=0, opposite_zero=0, opposite_nonzero=0,
             above_switch=0, below_switch=0, critical_exact=0, ns_same_ng_opposite=0, ns_opposite_ng_same=0)
    n_all = outs[0][0, 0]   # the first batch is op 2 over FLAG_SETS: the lobes ALL matches, whose count divides a sampled lobe's pdf
    for b, o in zip(batches, outs):
        n = len(o); c["probes"] += n; c["nan"] += int(np.isnan(o).any(axis=1).sum())
        wo, wi, u, fl = b["wo"], b["wi"], b["u"], b["flags"]
        if b["op"] == 0 and b["frame"] is None:
            opp = (wi == -wo).all(axis=1)
            zero = (o[:, :3] == 0).all(axis=1)
            c["opposite_zero"] += int((opp & zero).sum()); c["opposite_nonzero"] += int((opp & ~zero).sum())
        if b["op"] == 0 and b["frame"] is not None:
            ns, ng = b["frame"][0:3].astype(np.float64), b["frame"][3:6].astype(np.float64)
            s_ns = (wo @ ns) * (wi @ ns) > 0; s_ng = (wo @ ng) * (wi @ ng) > 0
            c["ns_same_ng_opposite"] += int((s_ns & ~s_ng).sum()); c["ns_opposite_ng_same"] += int((~s_ns & s_ng).sum())
        if b["op"] != 1 or b["frame"] is not None:
            continue
        pdf, ty = o[:, 3], o[:, 7]
        ok = pdf > 0
        c["failed"] += int((pdf == 0).sum())
        c["spec_refl"] += int((ty == (pc.SPEC | pc.REFL)).sum()); c["spec_trans"] += int((ty == (pc.SPEC | pc.TRANS)).sum())
        if mat.eta is not None and mat.eta != 1.0:
            e = mat.eta if mat.eta > 1.0 else 1.0 / mat.eta
            dense = (wo[:, 2] < 0) if mat.eta > 1.0 else (wo[:, 2] > 0)
            s2 = (1.0 - wo[:, 2].astype(np.float64) ** 2) * e * e
            c["critical_exact"] += int((dense & (pc.refract_sin2_t(mat.eta, wo[:, 2]) == 1)).sum())
            if mat.fresnel_specular:   # FresnelSpecular past the critical angle: fr = 1, the reflection has all the probability of its lobe
                c["tir"] += int((dense & (s2 > 1.001) & (ty == (pc.SPEC | pc.REFL)) & (pdf * n_all == 1)).sum())
                c["refracted"] += int((dense & (s2 < 0.999) & (ty == (pc.SPEC | pc.TRANS))).sum())
            else:   # transmission lobes alone: the refraction fails past the critical angle, succeeds under it
                only_t = fl == (pc.ALL & ~pc.REFL)
                c["tir"] += int((only_t & dense & (s2 > 1.001) & (pdf == 0)).sum())
                c["refracted"] += int((only_t & dense & (s2 < 0.999) & ok & ((ty.astype(np.int64) & pc.TRANS) != 0)).sum())
        if mat.fresnel_blend:
            allf = fl == pc.ALL
            c["blend_diffuse"] += int((allf & ok & (u[:, 0] < 0.5)).sum()); c["blend_specular"] += int((allf & ok & (u[:, 0] >= 0.5)).sum())
        if mat.alpha is not None:
            with np.errstate(invalid="ignore"):
                z = pc.stretched_z(mat.alpha, wo)
                hi, lo = (z > pc.SWITCH, z <= pc.SWITCH) if mat.exact_alpha else (z > 0.99995, z < 0.99985)
            c["above_switch"] += int((ok & hi).sum()); c["below_switch"] += int((ok & lo).sum())
    return c


@pytest.mark.parametrize("name", [m.name for m in pc.MATERIALS])
def test_bsdf_case_set_reaches_its_branches(name):
    mat = pc.MATERIAL_BY_NAME[name]
    orc, mid, batches, outs = material_set(name)
    c = coverage(mat, batches, outs)
    print(name, c)
    assert 0 < c["probes"] <= pc.MAX_PROBES
    assert c["nan"] <= 0.01 * c["probes"], c
    assert c["failed"] >= 1, c                                  # a failed sample (pdf == 0): flag sets that match no lobe, grazing wo, ...
    assert c["ns_same_ng_opposite"] >= 1 and c["ns_opposite_ng_same"] >= 1, c
    if mat.fresnel_specular:
        assert c["spec_trans"] >= 1, c
        if mat.eta != 1.0:                                      # at eta = 1 the Fresnel reflectance is 0: nothing is ever reflected
            assert c["spec_refl"] >= 1, c
    if mat.transmission and mat.eta is not None and mat.eta != 1.0:
        assert c["tir"] >= 1 and c["refracted"] >= 1, c        # both sides of the critical angle
        if len(pc.critical_exact_z(mat.eta)):                    # ... and the angle itself, where float32 can meet g_refract's sin2_t == 1 at all (eta = 2)
            assert c["critical_exact"] >= 1, c
    if mat.fresnel_blend:
        assert c["blend_diffuse"] >= 1 and c["blend_specular"] >= 1, c
    if mat.alpha is not None:
        assert c["above_switch"] >= 1 and c["below_switch"] >= 1, c
    # wi = -wo.  BSDF::f sends such a pair to the transmission lobes only (its `reflect` test is -(wo . ng)^2 > 0, never true), so the `wh == 0` exits of
    # MicrofacetReflection::f and FresnelBlend::f cannot be reached through the BSDF, in any frame; what can be pinned is that a material without
    # transmission scatters nothing there
    assert c["opposite_zero"] + c["opposite_nonzero"] >= 1
    if not mat.transmission:
        assert c["opposite_nonzero"] == 0, c


@pytest.mark.parametrize("name", ["matte_oren", "glass_smooth_eta_1.5", "glass_anisotropic", "uber_opacity_0.6", "substrate", "mix_two_levels"])
def test_oracle_batch_probe_equals_single_probe(name):
    orc, mid, batches, outs = material_set(name)
    rng = np.random.default_rng(5)
    for b, o in zip(batches, outs):
        if b["frame"] is not None:
            continue
        for i in rng.choice(len(o), size=min(len(o), 60), replace=False):
            one = orc.bsdf_probe(mid, b["op"], b["wo"][i], b["wi"][i], b["u"][i], int(b["flags"][i]))
            assert pc.first_difference(o[i:i + 1], one.reshape(1, 8)) < 0 and pc.first_difference(one.reshape(1, 8), o[i:i + 1]) < 0, pc.describe(name, b, i)


@pytest.mark.parametrize("name", ["matte_lambert", "glass_rough_eta_1.5", "translucent"])
def test_canonical_frame_argument_changes_nothing(name):
    orc, mid, batches, outs = material_set(name)
    for b, o in zip(batches, outs):
        if b["frame"] is None:
            got = orc.bsdf_probe_batch(mid, b["op"], b["wo"], b["wi"], b["u"], b["flags"], frame=CANONICAL)
            i = pc.first_difference(got, o)
            assert i < 0, pc.describe(name, b, i)


def test_oracle_refuses_a_textured_material_and_an_unknown_one():
    orc = OracleScene()
    tex = orc.add_texture_constant((0.5, 0.5, 0.5))
    mid = orc.add_material_matte_tex(tex, 0.0)
    z = np.zeros((1, 3), F)
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        orc.bsdf_probe_batch(mid, 0, z, z, np.zeros((1, 2), F), [31])
    assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        orc.bsdf_probe_batch(mid + 1, 0, z, z, np.zeros((1, 2), F), [31])
    assert e.value.code == pbrt_hip.ERR_INVALID_ARG


# ---------------------------------------------------------------- samplers ----------------------------------------------------------------------------------------
def test_halton_batch_equals_single_value_and_spans_the_index_range():
    lib = oracle_binding().lib
    assert (pc.HALTON_SPP_MAX + 1) * pc.HALTON_STRIDE_MAX < 2 ** 32 <= (pc.HALTON_SPP_MAX + 2) * pc.HALTON_STRIDE_MAX
    for name, bounds, spp in pc.HALTON_SETUPS:
        s = OracleScene()
        s.set_sampler(0, spp, bounds)
        xy, smp, dim = pc.halton_cases(bounds, spp)
        got = s.sampler_value_batch(xy, smp, dim)
        assert ((got >= 0) & (got < 1)).all(), name
        for i in np.random.default_rng(3).choice(len(got), size=300, replace=False):
            one = lib.oracle_sampler_value(s.h, int(xy[i, 0]), int(xy[i, 1]), int(smp[i]), int(dim[i]))
            assert F(one).view(np.uint32) == got[i].view(np.uint32), (name, xy[i], smp[i], dim[i])
    # the last set-up's last sample sits within one stride of 2^32: the device's 32-bit index must hold it
    assert (pc.HALTON_SPP_MAX - 1) * pc.HALTON_STRIDE_MAX > 2 ** 32 - 3 * pc.HALTON_STRIDE_MAX


def sobol_tables(name):
    z = np.load(os.path.join(HERE, "golden", name))
    return z["m32"], z["vdc"], z["vdc_inv"]


def test_sobol_batch_reproduces_the_film_offsets(host):
    """The scene and pixel of test_oracle_kat.py::test_sobol_sampler_properties: dimensions 0 and 1 of samples 0..15 are the film offsets get_camera_sample adds to the pixel."""
    s = OracleScene()
    spec = pbrt_hip.SceneSpec(n_tris=4, xres=100, yres=60, spp=16)
    pbrt_hip.capture_spec(spec, s, host)
    s.set_sobol_tables(*sobol_tables("sobol_subset.npz"))
    s.set_sampler(1, 16, s.sample_bounds)
    k = np.arange(16, dtype=np.uint32)
    xy = np.tile(np.array([37, 21], np.int32), (16, 1))
    fx = s.sampler_value_batch(xy, k, np.zeros(16, np.uint32)); fy = s.sampler_value_batch(xy, k, np.ones(16, np.uint32))
    for i in range(16):
        _, pf = s.generate_camera_rays([37, 21, 38, 22], i)
        assert (F(37) + fx[i]).view(np.uint32) == pf[0, 0].view(np.uint32) and (F(21) + fy[i]).view(np.uint32) == pf[0, 1].view(np.uint32), i
    for nx, ny in ((4, 4), (16, 1), (1, 16), (2, 8), (8, 2)):   # the (0,2)-net that test asserts
        assert len({(int(x * nx), int(y * ny)) for x, y in zip(fx, fy)}) == 16, (nx, ny)


def test_sobol_cases_stay_inside_the_tables_and_refusals_are_reported():
    m32, vdc, vdci = sobol_tables("sobol_subset_64.npz")
    n_dims = len(m32) // 52
    assert n_dims == 64 and len(vdc) // 52 >= 9
    wide = 0
    for res in pc.SOBOL_RESOLUTIONS:
        for mn in pc.SOBOL_MINIMA:
            s = OracleScene()
            s.set_sobol_tables(m32, vdc, vdci)
            bounds, xy, smp, dim = pc.sobol_cases(res, mn, n_dims)
            s.set_sampler(1, 16, bounds)
            got = s.sampler_value_batch(xy, smp, dim)
            assert ((got >= 0) & (got < 1)).all(), (res, mn)
            m = int(np.ceil(np.log2(max(res))))
            assert int(smp.max()) << (2 * m) < 2 ** 52                      # the index stays within the 52 columns of a matrix ...
            wide += int(((smp.astype(np.uint64) << np.uint64(2 * m)) >= 2 ** 32).sum())   # ... and some need more than 32 of them
            with pytest.raises(pbrt_hip.PbrtHipError) as e:                 # a dimension the tables do not hold
                s.sampler_value_batch(xy[:1], smp[:1], [n_dims])
            assert e.value.code == pbrt_hip.ERR_UNSUPPORTED
    assert wide > 0


def test_an_index_meets_the_critical_angle_exactly():
    assert len(pc.critical_exact_z(2.0)) >= 1 and any(m.eta == 2.0 and m.transmission and not m.fresnel_specular for m in pc.MATERIALS)
