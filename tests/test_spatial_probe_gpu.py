"""-m gpu: the spatial light distribution on the device (csrc/spatial.h: spatial_voxel_of, spatial_claim, spatial_compute_kernel, the light pick of shade_kernel) against the
oracle on explicit points, through pbrt_hip_spatial_probe_begin / _batch / _voxel.  Per set of spatial_probe_cases.SETS every voxel index, every picked light, every word of
the pick's pdf, the voxel resolution and every word of the func / cdf / func_int tables read back must equal the oracle's (libm mode 1).  test_spatial_probe_cases_cpu.py
measures, on the oracle alone, which branches the sets reach.  The renders here are the two that show a probe leaves nothing behind."""
import numpy as np
import pytest

import pbrt_hip
import spatial_probe_cases as sc
from oracle_binding import OracleScene, set_libm_mode
from probe_cases import F, hexf
from test_spatial_gpu import _emissive_grid_scene

pytestmark = pytest.mark.gpu
_cache = {}


def pair(set_name, k, host):
    """(case, product scene, p, u, the oracle's (pi, light, pdf, nv) and {voxel: tables} in libm mode 1) of case k of a set; computed once, shared, left unchanged"""
    key = (set_name, k)
    if key not in _cache:
        case = sc.SETS[set_name][k]
        orc = OracleScene(); prod = pbrt_hip.Scene()
        case.capture(orc, host); case.capture(prod, host)
        set_libm_mode(1)   # the points too: the samples placed on a CDF entry must sit on the entries the device is compared with
        try:
            p, u = case.points(orc)
            want = orc.spatial_lookup_batch(p, u, case.strategy)
            tables = {}
            if len(case.voxels):
                vpi = orc.spatial_lookup_batch(case.voxels, np.full(len(case.voxels), 0.5, F))[0]
                tables = {tuple(int(x) for x in q): orc.spatial_voxel(q, case.n_lights) for q in vpi}
                for v, q in zip(case.voxels, vpi):   # every voxel whose CDF has an interior entry is sampled exactly on one
                    cdf = tables[tuple(int(x) for x in q)][1]
                    assert np.isin(u[(p == v).all(axis=1)], cdf[1:-1]).any(), (case.name, q)
        finally:
            set_libm_mode(0)
        _cache[key] = (case, prod, p, u, want, tables)
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_lookup(set_name, case, p, u, got, want):
    gpi, glight, gpdf = got[:3]; wpi, wlight, wpdf = want[:3]
    bad = (glight != wlight) | (bits(gpdf) != bits(wpdf))
    if case.strategy == 2:
        bad |= (gpi != wpi).any(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{sc.describe(set_name, case, p, u, i)}\n  device voxel {gpi[i]} light {glight[i]} pdf {hexf(gpdf[i:i + 1])}\n  oracle voxel {wpi[i]} light {wlight[i]} pdf {hexf(wpdf[i:i + 1])}")


def assert_tables(set_name, case, prod, tables):
    for q, (wf, wc, wi) in tables.items():
        gf, gc, gi = prod.spatial_probe_voxel(q, case.n_lights)
        for what, g, w in (("func", gf, wf), ("cdf", gc, wc), ("func_int", np.array([gi], F), np.array([wi], F))):
            d = np.flatnonzero(bits(g) != bits(w))
            assert len(d) == 0, f"set {set_name} case {case.name} voxel {q}: {what}[{d[0]}] device {hexf(g[d[0]:d[0] + 1])} oracle {hexf(w[d[0]:d[0] + 1])} ({len(d)} of {len(w)} words differ)"


def run_set(set_name, host):
    for k in range(len(sc.SETS[set_name])):
        case, prod, p, u, want, tables = pair(set_name, k, host)
        if case.strategy == 2:
            nv, cap = prod.spatial_probe_begin()
            assert nv == want[3], (case.name, nv, want[3])
            assert cap >= 1
        got = prod.spatial_probe_batch(p, u, case.strategy)
        assert_lookup(set_name, case, p, u, got, want)
        if case.strategy == 2:
            n_vox = len(np.unique(want[0], axis=0))
            assert list(got[3]) == [n_vox, n_vox, 0, 0], (case.name, list(got[3]), n_vox)
            assert_tables(set_name, case, prod, tables)
            # the same batch again: nothing new to claim, the distribution pass runs over no slot, the answers stay
            again = prod.spatial_probe_batch(p, u, 2)
            assert_lookup(set_name, case, p, u, again, want)
            assert list(again[3]) == [n_vox, n_vox, 0, 0]


def test_disk_and_cylinder_lights_against_the_float32_restatement(host):
    """`kinds`, the lights the oracle does not have: spatial_compute_kernel<true> reaches Disk::sample / Cylinder::sample through wh_light_sample_li.  Voxels apart from the
    lights, crossed by their surfaces, holding a whole light and inside the cylinder; tables, voxels, picks and pdfs bit for bit against spatial_probe_cases' float32
    restatement over quadric_light_restatement.sample_li, which test_quadric_lights_gpu.py compares with the device bit for bit."""
    from oracle_binding import oracle_binding
    case = sc.DISK_CYLINDER
    p, u, tables, wpi, wlight, wpdf, reached = sc.restated_points(case, host, oracle_binding().lib.oracle_radical_inverse)
    assert reached == sc.Q_OUTSIDE | sc.Q_STRADDLES | sc.Q_CONTAINS | sc.Q_INSIDE
    with pbrt_hip.Scene() as prod:
        case.capture(prod, host)
        nv, cap = prod.spatial_probe_begin()   # no switch: a disk or cylinder light selects the <true> instantiation by itself
        assert nv == (64, 64, 64)
        got = prod.spatial_probe_batch(p, u)
        assert_lookup("kinds", case, p, u, got, (wpi, wlight, wpdf))
        assert list(got[3]) == [len(tables), len(tables), 0, 0]
        assert_tables("kinds", case, prod, tables)


@pytest.mark.parametrize("name", ["grid", "flat", "resolution", "light_counts", "kinds", "pick"])
def test_spatial_probe_bit_exact(host, name):
    run_set(name, host)


def test_resolution_comes_from_the_rule(host):
    for k, extent in enumerate(sc.RESOLUTION_EXTENTS):
        case, prod, p, u, want, _ = pair("resolution", k, host)
        nv, _ = prod.spatial_probe_begin()
        assert nv == sc.resolution_rule(extent)[0] == want[3]


def test_many_voxels_counters_across_passes(host):
    """More new voxels in one pass than the distribution pass has blocks (its grid-stride leg); then one new voxel after a non-zero high-water mark; then one new voxel
    claimed by 5000 points at once."""
    case, prod, p, u, want, _ = pair("many_voxels", 0, host)
    orc = OracleScene(); case.capture(orc, host)
    nv, cap = prod.spatial_probe_begin()
    assert nv == (64, 64, 64) and cap >= sc.MANY_LATTICE ** 3 + 2
    rng = np.random.default_rng(9300)
    seen = set()
    for b in sc.many_voxel_batches():
        ub = rng.random(len(b)).astype(F)
        set_libm_mode(1)
        try:
            w = orc.spatial_lookup_batch(b, ub)
        finally:
            set_libm_mode(0)
        g = prod.spatial_probe_batch(b, ub)
        assert_lookup("many_voxels", case, b, ub, g, w)
        seen |= {tuple(q) for q in w[0]}
        assert list(g[3]) == [len(seen), len(seen), 0, 0]   # SP_CLAIMED == SP_DONE == distinct voxels so far, SP_OVERFLOW == 0, SP_BLOCKS == 0
    assert len(seen) == sc.MANY_LATTICE ** 3 + 2
    for q in ((1, 1, 1), (57, 57, 57), (62, 3, 7), (40, 41, 42)):   # the first slot, the last of the first pass, the two later passes' single slots
        set_libm_mode(1)
        try:
            wf, wc, wi = orc.spatial_voxel(q, 3)
        finally:
            set_libm_mode(0)
        assert_tables("many_voxels", case, prod, {q: (wf, wc, wi)})
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        prod.spatial_probe_voxel((0, 0, 0), 3)     # never touched
    assert e.value.code == pbrt_hip.ERR_STATE
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        prod.spatial_probe_voxel((64, 0, 0), 3)    # outside the grid
    assert e.value.code == pbrt_hip.ERR_INVALID_ARG


def test_film_after_a_probe_is_the_film_without_one(host):
    cap = _emissive_grid_scene(host, 4, res=24, spp=2)
    with pbrt_hip.Scene() as fresh:
        cap(fresh)
        x0, w0, st0 = fresh.render_path(max_depth=3, light_strategy=2)
    with pbrt_hip.Scene() as s:
        cap(s)
        nv, _ = s.spatial_probe_begin()
        rng = np.random.default_rng(9400)
        p = (rng.random((500, 3)) * 4.0 - 2.0).astype(F)
        s.spatial_probe_batch(p, rng.random(500).astype(F))
        s.spatial_probe_batch(p[:50], rng.random(50).astype(F), strategy=1)
        x1, w1, st1 = s.render_path(max_depth=3, light_strategy=2)
        with pytest.raises(pbrt_hip.PbrtHipError) as e:   # the render reset the tables: the probe's are gone
            s.spatial_probe_batch(p, rng.random(500).astype(F))
        assert e.value.code == pbrt_hip.ERR_STATE
        x2, w2, st2 = s.render_path(max_depth=3, light_strategy=1)
    assert np.array_equal(x0.view(np.uint32), x1.view(np.uint32)) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    assert st0.light_distributions_created == st1.light_distributions_created > 0
    with pbrt_hip.Scene() as fresh:
        cap(fresh)
        x3, w3, _ = fresh.render_path(max_depth=3, light_strategy=1)
    assert np.array_equal(x2.view(np.uint32), x3.view(np.uint32))


def test_pool_exhaustion_is_an_error_and_the_handle_stays_usable(host, monkeypatch):
    case, prod, _, _, _, _ = pair("many_voxels", 0, host)
    pts = sc.many_voxel_batches()[0][:200]   # 200 distinct voxels
    u = np.full(200, 0.5, F)
    monkeypatch.setenv("PBRT_HIP_SPATIAL_POOL_BYTES", str(64 * (2 * 3 + 2) * 4))   # room for 64 voxels of 3 lights
    nv, cap = prod.spatial_probe_begin()
    assert cap == 64
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        prod.spatial_probe_batch(pts, u)
    assert e.value.code == pbrt_hip.ERR_OOM
    # the same through the raw entry: the counters and the answers as the device left them — 200 claims, 64 distributions, the flag; a point whose voxel got no slot has pdf 0
    pi = np.zeros((200, 3), np.int32); light = np.zeros(200, np.uint32); pdf = np.full(200, -1.0, F); ctr = np.zeros(4, np.uint32)
    C = pbrt_hip.C
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    prod.spatial_probe_begin()
    rc = prod.b.fn("spatial_probe_batch")(prod.h, 200, ptr(pts, C.c_float), ptr(u, C.c_float), 2, ptr(pi, C.c_int32), ptr(light, C.c_uint32), ptr(pdf, C.c_float), ptr(ctr, C.c_uint32))
    assert rc == pbrt_hip.ERR_OOM and list(ctr) == [200, 64, 1, 0]
    assert int((pdf == 0).sum()) == 200 - 64 and int((pdf > 0).sum()) == 64
    monkeypatch.delenv("PBRT_HIP_SPATIAL_POOL_BYTES")
    nv, cap = prod.spatial_probe_begin()
    assert cap >= 200
    g = prod.spatial_probe_batch(pts, u)
    assert list(g[3]) == [200, 200, 0, 0] and (g[2] > 0).all()


def test_refusals(host):
    bare = pbrt_hip.Scene()
    bare.add_light_point((1, 1, 1), (0, 0, 3)); bare.add_light_point((1, 1, 1), (1, 0, 3))

    def refused(code, fn, *a, **kw):
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
    p = np.zeros((4, 3), F); u = np.full(4, 0.5, F)
    refused(pbrt_hip.ERR_STATE, bare.spatial_probe_begin)                      # no accelerator
    m = bare.add_material_matte((0.5, 0.5, 0.5), 0.0)
    sc.box_mesh(bare, (0, 0, 0), (1, 1, 1), m); bare.build_accel(0, 4)
    refused(pbrt_hip.ERR_STATE, bare.spatial_probe_batch, p, u)                # strategy 2 without begin
    refused(pbrt_hip.ERR_STATE, bare.spatial_probe_voxel, (0, 0, 0), 2)
    refused(pbrt_hip.ERR_INVALID_ARG, bare.spatial_probe_batch, p, u, strategy=3)
    assert bare.spatial_probe_batch(p, u, strategy=0)[1].tolist() == [1, 1, 1, 1]   # uniform over two lights: u = 0.5 picks the second
    case, one, _, _, _, _ = pair("pick", 2, host)                              # a single light: a render builds no tables
    refused(pbrt_hip.ERR_STATE, one.spatial_probe_begin)
    nv, cap = bare.spatial_probe_begin()
    assert nv == (64, 64, 64)
    assert bare.spatial_probe_batch(p, u)[3].tolist() == [1, 1, 0, 0]
    bare.add_light_point((1, 1, 1), (0, 1, 3))                                  # a third light: the slots were laid out for two
    refused(pbrt_hip.ERR_STATE, bare.spatial_probe_batch, p, u)
    refused(pbrt_hip.ERR_STATE, bare.spatial_probe_voxel, (0, 0, 0), 3)
    bare.spatial_probe_begin()
    assert bare.spatial_probe_batch(p, u)[3].tolist() == [1, 1, 0, 0] and len(bare.spatial_probe_voxel((0, 0, 0), 3)[0]) == 3
    sph = pbrt_hip.Scene()                                                      # a sphere light without the path integrator's switch
    m = sph.add_material_matte((0.5, 0.5, 0.5), 0.0)
    sph.add_light_point((1, 1, 1), (0, 0, 3))
    t = host.translate((0.5, 0.5, 0.5))
    sph.add_sphere_light(t[0], t[1], 0.2, None, None, 360.0, m, False, L=(1, 1, 1))
    sc.box_mesh(sph, (0, 0, 0), (1, 1, 1), m); sph.build_accel(0, 4)
    refused(pbrt_hip.ERR_UNSUPPORTED, sph.spatial_probe_begin)
    refused(pbrt_hip.ERR_UNSUPPORTED, sph.spatial_probe_batch, p, u, strategy=0)
    sph.set_path_sphere_lights(True)
    assert sph.spatial_probe_begin()[0] == (64, 64, 64)
