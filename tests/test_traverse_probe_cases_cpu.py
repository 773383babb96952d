"""What the case sets of traverse_probe_cases.py reach, stated through the oracle's per-ray counters (no GPU): the depth of the stack fixture's tree and the device-style stack
peaks of its rays around both LDS depths, the reference's own stack inside its 64 entries, the composition of every 64-position batch, the mask candidates per batch, the
leaf-record sequences and instance forms met — and that the oracle's answer for a ray does not depend on where in a batch it stands.  The GPU test of the same cases
(test_traverse_probe_gpu.py) can then only pass by walking these edges.  The stack-overflow path is out of scope by design (see the case module's docstring)."""
import numpy as np
import pytest

import scenes
import traverse_probe_cases as T
from oracle_binding import OracleScene

NAMES = list(T.CASES)


@pytest.fixture(scope="module", params=NAMES)
def prep(request, host):
    return T.prepared(request.param, host)


def test_every_row_has_a_case(host):
    rows = {T.CASES[n](host).row for n in NAMES}
    assert rows == set(T.ROWS_NEEDED) and set(T.ROWS) == set(T.ROWS_NEEDED)


def test_queue_shapes_cover_the_issue():
    S = T.QUEUE_SHAPES
    plain = {(q.blocks, q.n_cl) for q in S if q.mode == 0 and q.n_heads == 1 and q.order is None}
    assert plain >= {(b, n) for b in (1, 2, 3, 9) for n in (0, 1, 63, 64, 65, T.N_BIG)}
    assert (T.N_BIG - 1) % (4 * 64) == 0 and (T.N_BIG - 1) // (4 * 64) >= 8
    mixed = [q for q in S if q.mode == 2]
    assert any(q.n_cl == 0 and q.n_sh for q in mixed) and any(q.n_sh == 0 and q.n_cl for q in mixed) and any(q.n_cl % 2 and q.n_sh % 2 for q in mixed)
    assert {(q.n_heads, q.head_chunk) for q in S} >= {(h, c) for h in (2, 8) for c in (64, 128, 49152)} | {(1, 49152)}
    for h in (2, 8):
        for c in (64, 128):
            ns = {q.n_cl + q.n_sh for q in S if (q.n_heads, q.head_chunk) == (h, c)}
            assert any(n < h * c for n in ns) and h * c in ns and h * c + 1 in ns          # heads dry from the start, an exact multiple, one ray into a new chunk
            assert any(n > h * c and n % c for n in ns)                                     # more than one chunk per head, the last one not full
    assert {q.order for q in S if q.mode != 2} >= {None, "identity", "reversed", "random"} and {q.order for q in S if q.mode == 2} >= {None, "reversed", "random", "interleave"}
    for q in S:
        assert q.n_cl <= T.N_BIG and q.n_sh <= T.N_BIG and 1 <= q.blocks <= 9 and (q.n_heads == 1 or q.head_chunk % T.BATCH == 0)
        assert (q.mode != 0 or q.n_sh == 0) and (q.mode != 1 or q.n_cl == 0)
        o = q.order_array()
        if o is not None:
            assert np.array_equal(np.sort(o), np.arange(q.n_cl + q.n_sh))
    o = T.QueueShape(2, 5, 3, order="interleave").order_array()
    assert o.tolist() == [0, 5, 1, 6, 2, 7, 3, 4]
    assert T.N_BIG < T.RESIDENT_LANES   # what makes a wave refill is the grid of 1 .. 9 blocks, not the ray count


def test_batch_compositions(prep):
    """every structured batch holds what the plan says, by the oracle's counters of the rays that stand in it — for the closest-hit and the any-hit walk"""
    case = prep.case
    cat = T.classify(case, prep.rs_cl)
    cat_sh = T.classify(case, prep.rs_sh)
    plan = T.batch_plan(case)
    seen = set()
    for b, comp in enumerate(plan):
        sl = slice(b * T.BATCH, (b + 1) * T.BATCH)
        assert sum(comp.values()) == T.BATCH
        for c, k in comp.items():
            assert int((cat[sl] == c).sum()) == k, (case.name, b, c, k, np.unique(cat[sl], return_counts=True))
            assert np.array_equal(prep.cats[sl] == c, cat[sl] == c)
            if c != "walker":
                assert int((cat_sh[sl] == c).sum()) == k, (case.name, b, "any-hit", c)
        seen.add(tuple(sorted(comp.items())))
    rm, rm_count = T.ROWS[case.row][0], T.COUNT_ROW[0]
    if case.alpha:
        masks = [(c.get("mask", 0), "early" in c) for c in plan]
        assert set(masks) == {(k, e) for k in T.ALPHA_COUNTS for e in (True, False)}
        assert T.ALPHA_MIN in T.ALPHA_COUNTS and T.ALPHA_MIN - 1 in T.ALPHA_COUNTS and T.ALPHA_MIN + 1 in T.ALPHA_COUNTS
        # exactly that many candidates' lanes wait: one candidate at least per mask ray, none on any other ray of the batch
        for b, comp in enumerate(plan):
            sl = slice(b * T.BATCH, (b + 1) * T.BATCH)
            for rs in (prep.rs_cl, prep.rs_sh):
                assert int((rs["alpha_candidates"][sl] > 0).sum()) == comp["mask"]
    else:
        early = {c["early"] for c in plan}
        assert early >= {0, 63, 64, rm - 1, rm, rm + 1, rm_count - 1, rm_count, rm_count + 1}
    # long walkers exist: lanes finish at very different times
    assert prep.rs_cl["nodes_visited"][cat == "walker"].max() >= 4 * max(case.walk_min, 8), prep.rs_cl["nodes_visited"].max()
    # the early rays are early for every reason listed
    e = prep.pool[cat == "early"]
    assert (e["t_max"] == 0).any() and np.isnan(e["d"]).any() and (e["d"] == 0).all(axis=1).any() and np.isinf(e["t_max"]).any()


def test_reference_stack_stays_inside_its_64_entries(prep):
    assert max(prep.rs_cl["ref_peak"].max(), prep.rs_sh["ref_peak"].max()) <= 64
    cap = 128 if "Inst" in prep.case.row else 64
    assert max(prep.rs_cl["dev_peak"].max(), prep.rs_sh["dev_peak"].max(), prep.rs_sh["dev_peak_count"].max()) < cap   # no launch is meant to overflow


def test_answer_does_not_depend_on_the_position_in_the_batch(prep):
    perm = np.random.default_rng(9).permutation(len(prep.pool))
    with T.libm1():
        h, _ = prep.orc.intersect_batch_stats(prep.pool[perm]); o, _ = prep.orc.occluded_batch_stats(prep.pool[perm])
        h1, _ = prep.orc.intersect_batch_stats(prep.pool[perm], threads=1)
    assert scenes.hits_equal(h, prep.hits[perm]).all() and np.array_equal(o, prep.occ[perm]) and scenes.hits_equal(h1, h).all()
    # and the per-ray counters sum to the batch's tallies: they describe the same walks
    assert int(prep.rs_cl["nodes_visited"].sum()) == prep.st_cl.nodes_visited and int(prep.rs_cl["tri_tests"].sum()) == prep.st_cl.tri_tests
    assert int(prep.rs_sh["nodes_visited"].sum()) == prep.st_sh.nodes_visited and int(prep.rs_sh["tri_tests"].sum()) == prep.st_sh.tri_tests
    assert np.array_equal(prep.rs_cl["found"] != 0, prep.hits["prim"] != T.MISS) and np.array_equal(prep.rs_sh["found"] != 0, prep.occ != 0)
    assert (prep.hits["prim"] != T.MISS).sum() >= 100 and (prep.occ != 0).sum() >= 100 and (prep.occ == 0).sum() >= 100


def chain_depth(nodes):
    """-> (interior nodes on the longest root-to-leaf path, True when every interior node has a leaf as its second child): the reference's linear layout puts the first child at
    index + 1 and the second at `offset`"""
    depth, pure, i = 0, True, 0
    while nodes[i]["n_primitives"] == 0:
        depth += 1
        pure &= bool(nodes[int(nodes[i]["offset"])]["n_primitives"] > 0)
        i += 1
    return depth, pure


def test_stack_fixture_flat(host):
    p = T.prepared("chain_flat", host)
    n = T.FLAT_CHAIN["n"]
    nodes = p.orc.bvh_nodes()
    assert len(nodes) == 2 * n - 1 and chain_depth(nodes) == (n - 1, True)      # a chain that peels one triangle per level: depth 28
    peaks = set(p.rs_cl["dev_peak"].tolist())
    assert peaks == set(range(n)), sorted(peaks)                                 # every height 0 .. 28
    for lds in (12, 11):
        assert peaks >= set(range(lds - 2, lds + 3))
    assert max(peaks) >= 2 * 12 and set(p.case.claims["peaks"]) <= peaks
    assert np.array_equal(p.rs_cl["dev_peak"], p.rs_cl["dev_peak_scene"]) and p.rs_cl["ref_peak"].max() == n - 1
    # the rays of one aim, family by family: peak n - 1 - j; family 0 ends on triangle j with every popped entry culled, family 1 on triangle j + 1, the first popped entry
    s_ = T.chain_scales(**T.FLAT_CHAIN)
    for fam in (0, 1):
        rays = T.chain_rays(s_, fam)
        st = p.orc.ray_stats_batch(rays); hits, _ = p.orc.intersect_batch_stats(rays)
        assert st["dev_peak"].tolist() == list(range(n - 1, -1, -1))
        want = np.arange(n) + fam; want[want == n] = T.MISS
        assert hits["prim"].tolist() == want.tolist()
        assert st["tri_tests"].tolist() == [min(1 + fam, n - j) for j in range(n)]
    P, _ = T.chain_mesh(s_)
    assert 2.0 ** -35 < np.abs(P).min() and np.abs(P).max() <= 2.0 ** 40   # fourth powers stay normal, cubes finite


def test_stack_fixture_instanced(host):
    p = T.prepared("chain_inst", host)
    n = T.INST_CHAIN["n"]
    nodes = p.orc.bvh_nodes()
    assert len(nodes) == 2 * n - 1 and chain_depth(nodes) == (n - 1, True)      # scene level: the instance and 33 triangles, depth 33; the object: the same chain
    rs = p.rs_cl
    peaks, scene_peaks = set(rs["dev_peak"].tolist()), set(rs["dev_peak_scene"].tolist())
    assert peaks == set(range(2 * n - 1)), sorted(peaks)                         # every shared height 0 .. 66: across 11, across the single-tree cap of 64, below 128
    assert max(scene_peaks) == n - 1 == p.case.claims["scene_peak"] and set(p.case.claims["peaks"]) <= peaks
    for lds in (12, 11):
        assert peaks >= set(range(lds - 2, lds + 3)) and scene_peaks >= set(range(lds - 2, lds + 3))
    assert max(peaks) > 64 and max(peaks) < 128 and max(peaks) >= 2 * 12
    inside = (rs["inst_entered"] > 0) & (p.cats == "walker")   # (the fixture's own rays: scenes.axis_rays() at the pool's end enter the instance elsewhere)
    assert rs["dev_peak"][inside].min() == n - 1 and (rs["dev_peak"][rs["inst_entered"] == 0] <= n - 1).all()   # the object's entries lie above the 33 scene-level ones
    assert rs["ref_peak"].max() == n - 1                                          # the reference recurses: each aggregate's own stack stays at 33
    assert p.rs_sh["dev_peak_count"].max() == 2 * n - 2
    assert np.isfinite(p.pool["o"][inside]).all() and (np.abs(p.pool["o"][inside]) >= 2.0 ** -120).all()   # origins stay normal floats


def test_alpha_cases_meet_both_record_positions_and_both_verdicts(host):
    for name in ("alpha_imagemap", "alpha_checkerboard", "instances_mp4_masked"):
        p = T.prepared(name, host)
        O = OracleScene
        seq = int(np.bitwise_or.reduce(p.rs_cl["leaf_seq"]))
        assert seq & O.SEQ_ALPHA_LAST and seq & O.SEQ_ALPHA_NOT_LAST, (name, bin(seq))   # the masked triangle as the last record of its leaf and not
        m = p.rs_cl["alpha_candidates"] > 0
        # some masks say 0 (the ray goes on: to the opaque triangle behind, or to nothing), some do not — for both ray kinds
        quad = p.hits["prim"][m]
        first = np.bincount(quad[quad != T.MISS]).argmax()
        assert 50 <= (quad == first).sum() + (quad == first + 1).sum() <= m.sum() - 50, (name, np.unique(quad, return_counts=True))
        msh = p.rs_sh["alpha_candidates"] > 0
        assert 50 <= p.occ[msh].sum() <= msh.sum() - 50


def test_instance_forms_and_leaf_sequences(host):
    O = OracleScene
    for name in NAMES:
        p = T.prepared(name, host)
        claims = p.case.claims.get("seq")
        if not claims: continue
        seq_cl, seq_sh = int(np.bitwise_or.reduce(p.rs_cl["leaf_seq"])), int(np.bitwise_or.reduce(p.rs_sh["leaf_seq"]))
        for c in claims:
            assert seq_cl & getattr(O, c), (name, c, bin(seq_cl))
            if c != "SEQ_HIT_IN_INST_THEN_NEARER":
                assert seq_sh & getattr(O, c), (name, "any-hit", c, bin(seq_sh))
        if p.case.claims.get("occluded_in_inst"):
            # any-hit rays occluded inside an instance: occluded although the scene without its instances would let them pass
            assert ((p.occ != 0) & (p.rs_sh["inst_entered"] > 0)).sum() >= 50
            assert ((p.hits["pad"][:, 1] != 0)).sum() >= 50 and ((p.hits["prim"] != T.MISS) & (p.hits["pad"][:, 1] == 0)).sum() >= 20
    # the projective instance is hit
    p = T.prepared("instances_mp4", host)
    assert (p.hits["pad"][:, 1] == 6 + 1).sum() >= 10, np.unique(p.hits["pad"][:, 1], return_counts=True)
