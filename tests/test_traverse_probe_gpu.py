"""-m gpu: the traversal kernel's control logic — queue refill beside lanes in mid-walk, the multi-head queue and the order indirection, mixed launches with an empty queue, the
stack's two address spaces, the alpha wait phase, instance entry and exit — through Scene.traverse_probe on the case sets of traverse_probe_cases.py.

The reference is exact: for every scene, ray set and queue shape each ray's result equals the oracle's intersect / intersect_p of that ray in every bit; no tolerance appears.
What the cases reach (stack heights across both LDS depths and into the spill region, batch compositions around every refill threshold, 1 / 11 / 12 / 13 / 64 waiting lanes per
batch, the leaf-record sequences) is asserted on the CPU by test_traverse_probe_cases_cpu.py.  Every launch holds at most 2 305 + 2 305 rays on grids of 1 .. 9 blocks, so every
wave refills many times.

Out of scope by design: the stack-overflow path (error_flag -> PBRT_HIP_ERR_DEVICE): no builder produces a tree deep enough within float range to reach the flat cap of 64 or the
shared cap of 128, the oracle's own stack ends at 64, and no node array is hand-crafted for it.  Every input lies inside the probe's preconditions."""
import numpy as np
import pytest
import torch

import pbrt_hip
import scenes
import traverse_probe_cases as T

pytestmark = pytest.mark.gpu
NAMES = list(T.CASES)


def full_grid():
    """the resident grid: 6 blocks of 256 lanes per CU (ensure_traversal_workspace)"""
    return torch.cuda.get_device_properties(0).multi_processor_count * 6


def product_scene(p):
    prod = pbrt_hip.Scene()
    p.case.capture(prod)
    return prod


def probe(prod, p, q):
    return prod.traverse_probe(q.mode, p.pool[:q.n_cl], p.pool[:q.n_sh], q.order_array(), q.n_heads, q.head_chunk, q.blocks)


def assert_equals_oracle(p, q, hits, occ, what):
    eq = scenes.hits_equal(hits, p.hits[:q.n_cl])
    assert eq.all(), (what, f"{(~eq).sum()} of {q.n_cl} closest-hit rays differ; first at {np.flatnonzero(~eq)[:5]}: got {hits[~eq][:2]} want {p.hits[:q.n_cl][~eq][:2]}")
    ne = occ != p.occ[:q.n_sh]
    assert not ne.any(), (what, f"{ne.sum()} of {q.n_sh} any-hit rays differ; first at {np.flatnonzero(ne)[:5]}: got {occ[ne][:5]}")


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
@pytest.mark.parametrize("name", NAMES)
def test_every_queue_shape_equals_the_oracle(host, name, counting):
    p = T.prepared(name, host)
    prod = product_scene(p)
    inst = "Inst" in p.case.row
    if counting:
        prod.set_traversal_counting(True)
        prod.traversal_counts()
    first = {}
    for q in T.QUEUE_SHAPES:
        what = f"{name} {'counting' if counting else 'timed'} {q!r}"
        hits, occ = probe(prod, p, q)
        assert_equals_oracle(p, q, hits, occ, what)
        if counting:
            cnt = prod.traversal_counts()
            # the work of a ray does not depend on the queue it came through: the same tallies for every shape with these counts ...
            key = (q.n_cl, q.n_sh)
            assert first.setdefault(key, cnt) == cnt, (what, first[key], cnt)
            # ... and they are the oracle's: rays, primitive tests, and the reference's node visits = 1 + 2 x interior nodes passed per closest-hit ray.  With instances the
            # reference's tally also counts the root of every object aggregate entered, which the device's leaves out (tests/test_render_gpu.py).
            for kind, rs, n in (("closest", p.rs_cl, q.n_cl), ("any_hit", p.rs_sh, q.n_sh)):
                nodes, entered = int(rs["nodes_visited"][:n].sum()), int(rs["inst_entered"][:n].sum())
                assert (cnt[kind]["rays"], cnt[kind]["tri_tests"]) == (n, int(rs["tri_tests"][:n].sum())), (what, kind, cnt)
                assert nodes - entered <= cnt[kind]["ref_node_visits"] <= nodes, (what, kind, cnt, nodes, entered)
                if not inst:
                    assert cnt[kind]["ref_node_visits"] == nodes, (what, kind, cnt, nodes)
    prod.close()


@pytest.mark.parametrize("name", NAMES)
def test_full_grid_equals_the_batch_calls(host, name):
    """n_heads = 1, no order, the full resident grid: what intersect_batch / occluded_batch launch, with the grid they would have shrunk"""
    p = T.prepared(name, host)
    prod = product_scene(p)
    for mode, n in T.FULL_GRID_SHAPES:
        q = T.QueueShape(mode, n if mode == 0 else 0, n if mode == 1 else 0, blocks=full_grid())
        hits, occ = probe(prod, p, q)
        assert_equals_oracle(p, q, hits, occ, f"{name} full grid mode {mode} n {n}")
        if mode == 0:
            assert np.array_equal(hits.view(np.uint8), prod.intersect_batch(p.pool[:n]).view(np.uint8))   # every byte, padding included
        else:
            assert np.array_equal(occ, prod.occluded_batch(p.pool[:n]))
    prod.close()


def test_refusals_launch_nothing_and_leave_the_handle_usable(host):
    p = T.prepared("flat", host)
    prod = product_scene(p)
    fn = prod.b.fn("traverse_probe")
    n = 130
    rays = np.ascontiguousarray(p.pool[:n]); hits = np.zeros(n, pbrt_hip.HIT_DTYPE); occ = np.zeros(n, np.uint8)
    ident = np.arange(n, dtype=np.uint32)
    R, H, O = rays.ctypes.data, hits.ctypes.data, occ.ctypes.data

    def call(mode=0, r_cl=R, n_cl=n, r_sh=None, n_sh=0, order=None, n_heads=1, head_chunk=64, blocks=1, h=H, o=None):
        return fn(prod.h, mode, r_cl, n_cl, r_sh, n_sh, order, n_heads, head_chunk, blocks, h, o)
    dup = ident.copy(); dup[5] = 6
    out_of_range = ident.copy(); out_of_range[7] = n
    two = np.arange(2 * n, dtype=np.uint32); two[0] = 2 * n   # (mixed: positions run over both queues)
    refusals = {
        "null closest-hit rays": dict(r_cl=None),
        "null hits": dict(h=None),
        "null any-hit rays": dict(mode=1, n_cl=0, r_cl=None, n_sh=n, r_sh=None, o=O),
        "null occluded": dict(mode=1, n_cl=0, r_cl=None, n_sh=n, r_sh=R, o=None),
        "blocks 0": dict(blocks=0),
        "blocks above the resident grid": dict(blocks=full_grid() + 1),
        "n_heads 0": dict(n_heads=0),
        "n_heads above the heads buffer": dict(n_heads=9),
        "head_chunk 0": dict(n_heads=2, head_chunk=0),
        "head_chunk no multiple of the batch": dict(n_heads=2, head_chunk=96),
        "order with a duplicate": dict(order=dup.ctypes.data),
        "order out of range": dict(order=out_of_range.ctypes.data),
        "mixed order out of range": dict(mode=2, r_sh=R, n_sh=n, o=O, order=two.ctypes.data),
        "mode 0 with any-hit rays": dict(r_sh=R, n_sh=n, o=O),
        "mode 1 with closest-hit rays": dict(mode=1, r_sh=R, n_sh=n, o=O),
        "unknown mode": dict(mode=3),
        "negative mode": dict(mode=-1),
    }
    prod.set_traversal_counting(True)
    prod.traversal_counts()
    for what, kw in refusals.items():
        hits[:] = 0; hits["prim"] = 12345
        assert call(**kw) == pbrt_hip.ERR_INVALID_ARG, what
        assert "traverse_probe" in prod.last_error(), what
        assert (hits["prim"] == 12345).all(), what
        cnt = prod.traversal_counts()
        assert cnt["closest"]["rays"] == 0 and cnt["any_hit"]["rays"] == 0, (what, cnt)   # nothing was launched
        # the handle answers a valid probe next
        q = T.QueueShape(2, n, 65, order="interleave", n_heads=2, head_chunk=64, blocks=2)
        h2, o2 = probe(prod, p, q)
        assert_equals_oracle(p, q, h2, o2, "after refusal: " + what)
        cnt = prod.traversal_counts()
        assert (cnt["closest"]["rays"], cnt["any_hit"]["rays"]) == (n, 65)
    prod.set_traversal_counting(False)
    # head_chunk is only read with several heads
    assert call(n_heads=1, head_chunk=0) == pbrt_hip.OK and scenes.hits_equal(hits, p.hits[:n]).all()
    assert fn(None, 0, R, n, None, 0, None, 1, 64, 1, H, None) == pbrt_hip.ERR_INVALID_ARG
    prod.close()
    # no accelerator: a state error
    s = pbrt_hip.Scene()
    s.add_material_matte()
    with pytest.raises(pbrt_hip.PbrtHipError) as e:
        s.traverse_probe(0, rays, None, blocks=1)
    assert e.value.code == pbrt_hip.ERR_STATE
    s.build_accel(0, 4)   # an empty scene: every ray misses
    h3, _ = s.traverse_probe(0, rays, None, blocks=2)
    assert (h3["prim"] == T.MISS).all() and np.array_equal(h3["t"].view(np.uint32), rays["t_max"].view(np.uint32))
    s.close()
