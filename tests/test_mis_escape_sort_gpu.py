"""The ray binning (csrc/raysort.h) with escape-query marks (csrc/mis_escape.h), through pbrt_hip_raysort_probe: a closest-hit key that carries PH_SORT_BINS on top of its bin.
For every case
  * `order & 0x7FFFFFFF` is a permutation of the queue positions;
  * the joint key never decreases along it, a marked closest-hit key counting as it is binned: beside the unmarked closest-hit rays of its cell (its bin without the mark), so
    all closest-hit rays still come before all any-hit rays;
  * bit 31 of an entry is set exactly where the entry's position holds a marked key;
  * the four positions one lane reads (an aligned group of four in the 16-byte body of a block's slice) stay consecutive in `order` where their keys are equal.
The last one is looked at where the lane's four are known from outside: the closest-hit run of a block's slice starts on a 16-byte boundary of an allocation of its own, so its
lanes hold the groups 4k .. 4k + 3 from the slice's start — those that go through the vector path (the rest of the body and the tail take one atomic per key, which promises nothing)."""
import ctypes as C

import numpy as np
import pytest

import pbrt_hip

pytestmark = pytest.mark.gpu

BINS, MARK, ESC = 4096, 4096, 0x80000000
SIZES = [5, 1027, 16384 + 3, 2 ** 20 + 5]


@pytest.fixture(scope="module")
def scene():
    s = pbrt_hip.Scene()   # no geometry: the probe needs a handle only
    yield s
    s.close()


def raysort(scene, keys_cl, keys_sh, sort_blocks):
    keys_cl = np.ascontiguousarray(keys_cl, dtype=np.uint32); keys_sh = np.ascontiguousarray(keys_sh, dtype=np.uint32)
    order = np.full(len(keys_cl) + len(keys_sh), 0xFFFFFFFF, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p) if a.size else None
    rc = scene.b.fn("raysort_probe")(scene.h, len(keys_cl), len(keys_sh), ptr(keys_cl), ptr(keys_sh), sort_blocks, ptr(order))
    assert rc == pbrt_hip.OK, (rc, scene.last_error())
    return order


def keys_for(n, share, seed, cells=BINS):
    """n closest-hit keys in runs of 1 .. 6 equal cells (a pixel's rays share a cell), a `share` of them marked; the mark falls ray by ray, so a lane's four hold both kinds"""
    g = np.random.default_rng(seed)
    runs = g.integers(1, 7, n)
    cell = np.repeat(g.integers(0, cells, n), runs)[:n].astype(np.uint32)
    marked = g.random(n) < share
    return cell | np.where(marked, MARK, 0).astype(np.uint32), marked


def check(scene, keys_cl, marked, keys_sh, sort_blocks):
    n_cl, n = len(keys_cl), len(keys_cl) + len(keys_sh)
    order = raysort(scene, keys_cl, keys_sh, sort_blocks)
    pos = order & np.uint32(ESC - 1)
    assert np.array_equal(np.sort(pos), np.arange(n, dtype=np.uint32)), "order & 0x7FFFFFFF is not a permutation of the queue positions"
    cl_bin = keys_cl.astype(np.int64) - MARK * marked
    bin_key = np.concatenate([cl_bin, BINS + keys_sh.astype(np.int64)])
    assert (np.diff(bin_key[pos]) >= 0).all(), "the joint key decreases along order"
    is_marked = np.concatenate([marked, np.zeros(len(keys_sh), bool)])
    assert np.array_equal((order >> 31).astype(bool), is_marked[pos]), "bit 31 is not exactly on the marked positions"
    assert (pos[:n_cl] < n_cl).all() and (pos[n_cl:] >= n_cl).all(), "a closest-hit ray lies behind an any-hit ray"
    # a lane's four: equal keys inside an aligned group of four at consecutive ranks, in position order.  The groups that go through the vector path (raysort_walk_run: four
    # 16-byte loads per lane and pass while that many are left; the rest of the body and the tail take one atomic per key, which promises nothing)
    rank = np.empty(n, np.int64); rank[pos] = np.arange(n)
    each = -(-n // sort_blocks)
    per = max(-(-each // 256) * 256, 16384)                            # raysort_slice_keys: a block's slice
    full = 0
    for lo in range(0, n_cl, per):                                      # a slice starts on a multiple of 256 of an allocation of its own: its closest-hit run has no scalar head
        hi = min(lo + per, n_cl)
        n_vec = (hi - lo) // 4
        v = np.arange(n_vec)
        v = v[1024 * (v // 1024) + v % 256 + 768 < n_vec]
        g0 = lo + 4 * v
        for a in range(3):
            for b in range(a + 1, 4):
                same = bin_key[g0 + a] == bin_key[g0 + b]
                between = np.ones(len(g0), np.int64)
                for c in range(a + 1, b):
                    between += bin_key[g0 + c] == bin_key[g0 + a]
                assert (rank[g0 + b][same] - rank[g0 + a][same] == between[same]).all(), "equal keys of one lane's four are not consecutive in order"
                full += int(same.sum())
    return full


@pytest.mark.parametrize("sort_blocks", [3, 1024])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("share", [0.0, 0.4, 1.0])
def test_marked_keys(scene, n, sort_blocks, share):
    n_cl = n - n // 3
    keys_cl, marked = keys_for(n_cl, share, n + int(10 * share))
    keys_sh = np.random.default_rng(n + 1).integers(0, BINS, n - n_cl).astype(np.uint32)
    pairs = check(scene, keys_cl, marked, keys_sh, sort_blocks)
    assert pairs > 1000 or n < 16384      # the two larger sizes reach the vector path


def test_few_cells_marked_and_unmarked_in_one_lane(scene):
    """two cells only: every lane's four hold equal bins with and without the mark — ONE run of equal keys, whose ranks are consecutive while the marks differ entry by entry"""
    keys_cl, marked = keys_for(16384 + 3, 0.5, 77, cells=2)
    assert check(scene, keys_cl, marked, np.zeros(0, np.uint32), 3) > 1000


def test_no_any_hit_queue_and_no_closest_hit_queue(scene):
    keys_cl, marked = keys_for(16384 + 3, 0.4, 5)
    check(scene, keys_cl, marked, np.zeros(0, np.uint32), 1024)
    check(scene, np.zeros(0, np.uint32), np.zeros(0, bool), np.random.default_rng(6).integers(0, BINS, 1027).astype(np.uint32), 3)


def test_unmarked_keys_give_the_order_they_gave(scene):
    """without a mark no entry has bit 31 and closest-hit rays come before any-hit rays, as test_raysort_probe_gpu.py states it"""
    keys_cl, marked = keys_for(16384 + 3, 0.0, 9)
    order = raysort(scene, keys_cl, np.arange(1027, dtype=np.uint32) % BINS, 1024)
    assert (order < ESC).all() and (order[:len(keys_cl)] < len(keys_cl)).all() and (order[len(keys_cl):] >= len(keys_cl)).all()


def test_refusals(scene):
    fn = scene.b.fn("raysort_probe")
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    keys = np.zeros(8, dtype=np.uint32); order = np.zeros(16, dtype=np.uint32)
    bad = keys.copy(); bad[3] = 2 * BINS                       # above every marked key
    assert fn(scene.h, 8, 8, p(bad), p(keys), 4, p(order)) == pbrt_hip.ERR_INVALID_ARG
    sh = keys.copy(); sh[3] = BINS                             # an any-hit key carries no mark
    assert fn(scene.h, 8, 8, p(keys), p(sh), 4, p(order)) == pbrt_hip.ERR_INVALID_ARG
    ok = keys.copy(); ok[3] = 2 * BINS - 1
    assert fn(scene.h, 8, 8, p(ok), p(keys), 4, p(order)) == pbrt_hip.OK
