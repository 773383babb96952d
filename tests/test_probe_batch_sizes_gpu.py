"""-m gpu: a probe's answer for element i does not depend on the batch around it.  Every per-element probe entry point (csrc/probe.hip) stages its arrays on the device, launches
blocks of 128 or 256 threads and copies the results back; a size or a part taken wrong there shows where a batch ends inside a block or on its edge.  Per probe: 257 rows of a
batch the case modules build (past two blocks of 128 and one of 256; rows repeat if the batch is shorter) are run once, then their prefixes of 1, 127, 128 and 129 rows, and
each prefix's output must equal the first rows of the full output bit for bit (probe_cases.first_difference: a NaN asks for a NaN in the same slot).

The scenes, the batches and whatever the oracle did to place them are the existing tests' (their cached pairs and the case modules' `prepared`): nothing is compared with the
oracle here, the other probe tests do that."""
import numpy as np
import pytest

import curve_cases as CC
import pbrt_hip
import probe_cases as pc
import surface_probe_cases as sc
import texture_probe_cases as tc
import traverse_probe_cases as T
from test_bsdf_probe_gpu import material_pair
from test_curve_gpu import add_curve
from test_light_probe_gpu import light_pair
from test_spatial_probe_gpu import pair as spatial_pair
from test_surface_probe_gpu import subset, surface_pair

pytestmark = pytest.mark.gpu
F = np.float32
FULL = 257
PREFIXES = (1, 127, 128, 129)


def rows(a, dtype):
    """an output as (n, words): float32 where a NaN may stand for a NaN, uint32 where every bit counts"""
    a = np.ascontiguousarray(a)
    return a.view(dtype).reshape(len(a), -1)


def _bsdf(host):
    prod, mid, batches, _ = material_pair("plastic")
    b = next(b for b in batches if b["op"] == 1)   # sample_f: all eight output words
    return len(b["wo"]), lambda i: rows(prod.bsdf_probe_batch(mid, 1, b["wo"][i], b["wi"][i], b["u"][i], b["flags"][i], frame=b["frame"]), F)


def _sampler(host):
    _, bounds, spp = pc.HALTON_SETUPS[2]
    prod = pbrt_hip.Scene(); prod.set_sampler(0, spp, bounds)
    xy, smp, dim = pc.halton_cases(bounds, spp)
    return len(xy), lambda i: rows(prod.sampler_value_batch(xy[i], smp[i], dim[i], use_lds=True), F)


def _light(set_name, variant, sphere_entry=False):
    def make(host):
        prod, batches, _ = light_pair(set_name, host)
        b = next(b for b in batches if b["op"] == 0)   # sample_li: the sample, its far end and the shadow ray
        if sphere_entry:
            return len(b["ref"]), lambda i: rows(prod.sphere_light_probe_batch(b["light"], 0, b["ref"][i], b["u"][i], b["wi"][i]), F)
        return len(b["ref"]), lambda i: rows(prod.light_probe_batch(b["light"], 0, b["ref"][i], b["u"][i], b["wi"][i], variant=variant), F)
    return make


def _curve(host):
    c = CC.probe_curves(host)[0]
    prod = pbrt_hip.Scene()
    m = prod.add_material_matte((0.5, 0.5, 0.5)); prod.add_light_infinite((1.0, 1.0, 1.0))
    add_curve(prod, c, m)
    prod.build_accel(0, 4)
    rays = CC.probe_rays(c, FULL, np.random.default_rng(5))
    return len(rays), lambda i: rows(prod.curve_probe(c["seg"], rays[i], shadow=False), F)


def _surface(host):
    ss, prod, tpl, batches, _, _, _ = surface_pair("flags32", host)
    b = next(b for b in batches if b["op"] == 0)
    return len(b["prim"]), lambda i: rows(sc.run_batches(prod, host, tpl, [subset(b, i)], 1)[0], F)


def _texture(set_name, key):
    def make(host):
        ps, _, batches, _, _ = tc.prepared(set_name, host)
        prod = tc.capture_product(set_name, host)
        b = dict(batches[0])
        return len(b[key]), lambda i: rows(tc.run_batches(prod, ps, [dict(b, **{key: np.ascontiguousarray(b[key][i])})], 0)[0], F)
    return make


def _spatial(k):
    def make(host):
        case, prod, p, u, _, _ = spatial_pair("pick", k, host)
        assert case.strategy in (0, 1)

        def run(i):
            _, light, pdf, _ = prod.spatial_probe_batch(p[i], u[i], case.strategy)
            return np.concatenate([rows(light, np.uint32), rows(pdf, np.uint32)], axis=1)   # (a pick's pdf is a table entry, never a NaN: every bit counts)
        return len(p), run
    return make


def _traverse(host):
    p = T.prepared("flat", host)
    prod = pbrt_hip.Scene(); p.case.capture(prod)
    return len(p.pool), lambda i: rows(prod.traverse_probe(0, p.pool[i], blocks=1)[0], np.uint32)   # (a miss's words are NaN patterns: every bit counts)


PROBES = {
    "bsdf": _bsdf,
    "sampler": _sampler,
    "light_variant_0": _light("triangle", 0),
    "light_variant_2": _light("sphere", 2),
    "sphere_light": _light("sphere", 2, sphere_entry=True),
    "curve": _curve,
    "surface_op_0": _surface,
    "texture": _texture("procedural_2d", "ctx"),
    "bump": _texture("bump", "inp"),
    "spatial_pick_strategy_1": _spatial(0),
    "spatial_pick_strategy_0": _spatial(1),
    "traverse_mode_0": _traverse,
}


@pytest.mark.parametrize("name", list(PROBES))
def test_a_prefix_of_a_batch_gives_the_batchs_first_rows(host, name):
    n_rows, run = PROBES[name](host)
    assert n_rows > 0
    idx = np.arange(FULL) % n_rows
    full = run(idx)
    assert len(full) == FULL
    for k in PREFIXES:
        part = run(idx[:k])
        assert part.shape == (k, full.shape[1]), (name, k, part.shape)
        i = pc.first_difference(part, full[:k])
        assert i < 0, f"{name}: row {i} of the first {k} rows differs from row {i} of all {FULL}\n  prefix {part[i].view(np.uint32)}\n  full   {full[i].view(np.uint32)}"
