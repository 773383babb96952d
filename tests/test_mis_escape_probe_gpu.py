"""-m gpu: escape queries (csrc/mis_escape.h) in the mixed traversal kernel, through Scene.traverse_probe: an entry of `order` with bit 31 set marks its closest-hit ray as one
that only asks whether it hits anything.

For every launch, ray by ray:
  * the marked launch's `prim != 0xFFFFFFFF` equals the unmarked launch's and the oracle's intersect `found` (NOT intersect_p's: the closest-hit acceptance rule holds);
  * a marked ray's record is (t_max at its stop, 0 or 0xFFFFFFFF, 0, 0) and sixteen bytes the kernel did not write;
  * an unmarked ray's record and every any-hit ray's flag are byte for byte what the unmarked launch gives, which equals the oracle (the parent's behaviour).
Scenes: a 3 000-triangle soup with the rays the oracle records from a render of it (primary, bounce, MIS and shadow rays), its instanced form, and the chain-tree stack fixtures of
traverse_probe_cases.py (flat and instanced: stack heights through the LDS depth into the spill region, where a marked lane stops with entries still on its stack).
Batch sizes 1, 31, 32, 33, 64, 65 and 129 around the wave's batch of 64, each with no, every and every second closest-hit ray marked; marked rays with the any-hit queue empty;
marked rays only in the queue's last partial batch."""
import numpy as np
import pytest

import pbrt_hip
import scenes
import traverse_probe_cases as T
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1

pytestmark = pytest.mark.gpu

ESC, MISS = np.uint32(0x80000000), 0xFFFFFFFF
SIZES = (1, 31, 32, 33, 64, 65, 129)
MARKS = ("none", "all", "every second")


class Pool:
    pass


_pools = {}


def soup_pool(host, instances):
    """the soup on both sides, and the rays the oracle's render of it traces"""
    key = ("soup", instances)
    if key in _pools: return _pools[key]
    spec = pbrt_hip.SceneSpec(n_tris=3000, seed=5, xres=48, yres=40, spp=2, max_depth=4)
    p = Pool()
    p.capture = lambda s: pbrt_hip.capture_spec(spec, s, host, instances=instances)
    with libm1():
        orc = OracleScene(); p.capture(orc)
        orc.record_rays(1 << 20)
        orc.render_path_ex(max_depth=4)
        reg, sh = orc.recorded_rays(False), orc.recorded_rays(True)
        assert len(reg) > 1000 and len(sh) > 300
        g = np.random.default_rng(3)
        p.cl = reg[g.permutation(len(reg))[:1000]]; p.sh = sh[g.permutation(len(sh))[:300]]   # primary, bounce and MIS rays mixed
        p.hits, _ = orc.intersect_batch_stats(p.cl)
        p.occ, _ = orc.occluded_batch_stats(p.sh)
    _pools[key] = p
    return p


def chain_pool(host, name):
    if name in _pools: return _pools[name]
    c = T.prepared(name, host)
    p = Pool()
    p.capture = c.case.capture
    walk = np.flatnonzero(c.cats != "early")     # the chain rays and the fill: every stack height the fixture reaches
    p.cl = c.pool[walk]; p.sh = c.pool[walk][::3]
    p.hits = c.hits[walk]; p.occ = c.occ[walk][::3]
    _pools[name] = p
    return p


POOLS = {"soup": lambda h: soup_pool(h, 0), "soup_instanced": lambda h: soup_pool(h, 3), "chain_flat": lambda h: chain_pool(h, "chain_flat"),
         "chain_inst": lambda h: chain_pool(h, "chain_inst")}


def marks_of(kind, n_cl):
    m = np.zeros(n_cl, bool)
    if kind == "all": m[:] = True
    elif kind == "every second": m[::2] = True
    return m


def launch_pair(prod, p, n_cl, n_sh, marked, order=None, first=0, **kw):
    """the same queue twice, without and with the marks: (unmarked hits, marked hits, unmarked flags, marked flags)"""
    cl, sh = p.cl[first:first + n_cl], p.sh[:n_sh]
    base = np.arange(n_cl + n_sh, dtype=np.uint32) if order is None else order
    flag = np.concatenate([marked, np.zeros(n_sh, bool)])[base]
    h0, o0 = prod.traverse_probe(2, cl, sh, base, **kw)
    h1, o1 = prod.traverse_probe(2, cl, sh, base | np.where(flag, ESC, np.uint32(0)), **kw)
    return h0, h1, o0, o1


def check(p, n_cl, n_sh, marked, got, what, first=0):
    h0, h1, o0, o1 = got
    want = p.hits[first:first + n_cl]
    assert scenes.hits_equal(h0, want).all(), (what, "the unmarked launch differs from the oracle")
    assert np.array_equal(o0, p.occ[:n_sh]) and np.array_equal(o1, p.occ[:n_sh]), (what, "any-hit flags")
    found = want["prim"] != MISS
    assert np.array_equal(h1["prim"] != MISS, found), (what, "a marked launch's verdicts differ from the oracle's intersect")
    assert np.array_equal(h0["prim"] != MISS, found), what
    keep = ~marked
    assert np.array_equal(h1[keep].view(np.uint8), h0[keep].view(np.uint8)), (what, "an unmarked ray's record changed")
    m = h1[marked]
    assert np.isin(m["prim"], (0, MISS)).all() and (m["b0"].view(np.uint32) == 0).all() and (m["b1"].view(np.uint32) == 0).all(), (what, "a marked ray's record")
    assert (m["b2"].view(np.uint32) == MISS).all() and (m["pad"] == MISS).all(), (what, "a marked ray wrote more than sixteen bytes")
    miss = marked & ~found
    assert np.array_equal(h1["t"][miss].view(np.uint32), h0["t"][miss].view(np.uint32)), (what, "a marked ray that hit nothing keeps its t_max")


@pytest.mark.parametrize("name", list(POOLS))
def test_batch_sizes_and_marks(host, name):
    p = POOLS[name](host)
    prod = pbrt_hip.Scene(); p.capture(prod)
    reached = 0
    for n in SIZES:
        for kind in MARKS:
            marked = marks_of(kind, n)
            for n_sh, order, kw in ((n, None, dict(blocks=1)), (min(n, 40), "random", dict(blocks=2, n_heads=2, head_chunk=64))):
                o = np.random.default_rng(n).permutation(n + n_sh).astype(np.uint32) if order else None
                first = (7 * n) % (len(p.cl) - n)
                what = f"{name} n {n} marks {kind} n_sh {n_sh} order {order}"
                check(p, n, n_sh, marked, launch_pair(prod, p, n, n_sh, marked, o, first, **kw), what, first)
                reached += int((marked & (p.hits[first:first + n]["prim"] != MISS)).sum())
    assert reached > 50, "hardly a marked ray hit anything: the early stop was not reached"
    prod.close()


@pytest.mark.parametrize("name", list(POOLS))
def test_whole_pool_marked_on_several_blocks(host, name):
    """every closest-hit ray of the pool marked, in a random order over both queues, three blocks and eight heads: every wave refills beside lanes in mid-walk"""
    p = POOLS[name](host)
    prod = pbrt_hip.Scene(); p.capture(prod)
    n_cl, n_sh = len(p.cl), len(p.sh)
    marked = marks_of("all", n_cl)
    o = np.random.default_rng(11).permutation(n_cl + n_sh).astype(np.uint32)
    check(p, n_cl, n_sh, marked, launch_pair(prod, p, n_cl, n_sh, marked, o, blocks=3, n_heads=8, head_chunk=64), name + " whole pool")
    prod.close()


def test_marks_with_an_empty_any_hit_queue(host):
    p = POOLS["soup"](host)
    prod = pbrt_hip.Scene(); p.capture(prod)
    for n in (33, 129):
        for kind in ("all", "every second"):
            marked = marks_of(kind, n)
            check(p, n, 0, marked, launch_pair(prod, p, n, 0, marked, blocks=1), f"empty any-hit queue n {n} {kind}")
    prod.close()


def test_marks_only_in_the_last_partial_batch(host):
    p = POOLS["soup"](host)
    prod = pbrt_hip.Scene(); p.capture(prod)
    n_cl, n_sh = 150, 43                        # 193 positions: three batches of 64 and one ray
    o = np.concatenate([np.arange(n_cl, n_cl + n_sh), np.arange(n_cl)]).astype(np.uint32)   # any-hit rays first: the closest-hit rays 149 alone is the last batch
    marked = np.zeros(n_cl, bool); marked[149] = True
    check(p, n_cl, n_sh, marked, launch_pair(prod, p, n_cl, n_sh, marked, o, blocks=1), "one marked ray in the last batch")
    n_cl, n_sh = 150, 0                         # 150 positions: the last batch holds 128 .. 149, all marked and nothing else
    marked = np.zeros(n_cl, bool); marked[128:] = True
    check(p, n_cl, n_sh, marked, launch_pair(prod, p, n_cl, n_sh, marked, blocks=1), "marks in the last 22 positions")
    prod.close()


def test_marks_are_refused_where_no_kernel_reads_them(host):
    """an any-hit position, a mode other than 2, a counting row, a row with alpha masks: PBRT_HIP_ERR_INVALID_ARG, nothing launched, the handle usable"""
    p = POOLS["soup"](host)
    prod = pbrt_hip.Scene(); p.capture(prod)
    fn = prod.b.fn("traverse_probe")
    n = 65
    cl = np.ascontiguousarray(p.cl[:n]); sh = np.ascontiguousarray(p.sh[:n])
    hits = np.zeros(n, pbrt_hip.HIT_DTYPE); occ = np.zeros(n, np.uint8)
    ident = np.arange(2 * n, dtype=np.uint32)
    on_sh = ident.copy(); on_sh[n + 3] |= ESC
    on_cl = ident.copy(); on_cl[3] |= ESC
    call = lambda mode, order, n_sh=n: fn(prod.h, mode, cl.ctypes.data, n, sh.ctypes.data if n_sh else None, n_sh, order.ctypes.data, 1, 64, 1, hits.ctypes.data, occ.ctypes.data if n_sh else None)
    hits["prim"] = 12345
    assert call(2, on_sh) == pbrt_hip.ERR_INVALID_ARG and "traverse_probe" in prod.last_error()
    assert call(0, np.ascontiguousarray(on_cl[:n]), 0) == pbrt_hip.ERR_INVALID_ARG
    prod.set_traversal_counting(True)
    assert call(2, on_cl) == pbrt_hip.ERR_INVALID_ARG
    prod.set_traversal_counting(False)
    assert (hits["prim"] == 12345).all()
    assert call(2, on_cl) == pbrt_hip.OK
    prod.close()
    pa = T.prepared("alpha_imagemap", host)
    prod = pbrt_hip.Scene(); pa.case.capture(prod)
    cl = np.ascontiguousarray(pa.pool[:n]); sh = cl
    assert call(2, on_cl) == pbrt_hip.ERR_INVALID_ARG
    assert call(2, ident) == pbrt_hip.OK
    prod.close()
