"""The ray binning between wavefront rounds (csrc/raysort.h) on explicit keys, through pbrt_hip_raysort_probe, which runs the launch the path integrator's rounds use.
For every case `order` must be a permutation of the queue positions along which the joint key (a closest-hit ray's key, 4096 + an any-hit ray's key) never decreases,
so that all closest-hit rays come before all any-hit rays.  The order inside a bin is unspecified and is not looked at.  The shapes are the smallest at which the
code takes another path: empty queues, runs shorter than one 16-byte load, an any-hit run that starts off a 16-byte boundary, block boundaries, the slice floor
(PH_SORT_FLOOR, csrc/raysort_plan.h) and grids with idle trailing blocks."""
import ctypes as C

import numpy as np
import pytest

import pbrt_hip

pytestmark = pytest.mark.gpu

BINS, FLOOR, RENDER_BLOCKS = 4096, 16384, 1024


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


def check(scene, keys_cl, keys_sh, sort_blocks=RENDER_BLOCKS):
    keys_cl = np.asarray(keys_cl, dtype=np.uint32); keys_sh = np.asarray(keys_sh, dtype=np.uint32)
    order = raysort(scene, keys_cl, keys_sh, sort_blocks)
    n = len(keys_cl) + len(keys_sh)
    assert order.shape == (n,)
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), "order is not a permutation of the queue positions"
    joint = np.concatenate([keys_cl, BINS + keys_sh]).astype(np.int64)
    along = joint[order]
    assert (np.diff(along) >= 0).all(), "the joint key decreases along order"
    assert (order[:len(keys_cl)] < len(keys_cl)).all() and (order[len(keys_cl):] >= len(keys_cl)).all()


def cycling(n, start=0):
    return (np.arange(n, dtype=np.uint32) + start) % BINS


@pytest.mark.parametrize("n_cl, n_sh", [(0, 0), (0, 5), (5, 0), (1, 0), (0, 1), (1, 1)])
def test_counts_at_the_edges(scene, n_cl, n_sh):
    check(scene, cycling(n_cl, 7), cycling(n_sh, 4090))


@pytest.mark.parametrize("n_cl", [1, 2, 3, 5, 255, 256, 257])
def test_any_hit_run_off_a_16_byte_boundary(scene, n_cl):
    rng = np.random.default_rng(n_cl)
    check(scene, rng.integers(0, BINS, n_cl), rng.integers(0, BINS, 1027))
    check(scene, rng.integers(0, BINS, n_cl), rng.integers(0, BINS, 1027), sort_blocks=3)


@pytest.mark.parametrize("total", [FLOOR - 1, FLOOR, FLOOR + 1])
@pytest.mark.parametrize("n_cl_of", [lambda t: 0, lambda t: t, lambda t: t // 2 + 1, lambda t: 5], ids=["any-hit only", "closest-hit only", "half", "five closest-hit"])
def test_totals_around_the_slice_floor(scene, total, n_cl_of):
    n_cl = n_cl_of(total)
    rng = np.random.default_rng(total)
    check(scene, rng.integers(0, BINS, n_cl), rng.integers(0, BINS, total - n_cl))


@pytest.mark.parametrize("sort_blocks", [7, 1024])
def test_idle_trailing_blocks(scene, sort_blocks):
    total = 7 * FLOOR + 3       # grid x floor + 3 for the grid of 7: one slice is longer than the floor there, and 1024 blocks leave 1016 idle
    rng = np.random.default_rng(sort_blocks)
    n_cl = total // 3 + 2
    check(scene, rng.integers(0, BINS, n_cl), rng.integers(0, BINS, total - n_cl), sort_blocks)
    if sort_blocks == 1024:     # grid x floor + 3 for the render's grid as well: 16.8 M rays, every block at its floor but the last
        total = 1024 * FLOOR + 3
        n_cl = total - 2 * FLOOR - 1
        check(scene, rng.integers(0, BINS, n_cl), rng.integers(0, BINS, total - n_cl), sort_blocks)


@pytest.mark.parametrize("key", [0, BINS - 1])
def test_one_bin_takes_every_ray(scene, key):
    check(scene, np.full(3 * FLOOR + 5, key), np.full(FLOOR + 259, key))
    check(scene, np.full(3 * FLOOR + 5, key), np.full(FLOOR + 259, key), sort_blocks=2)


def test_keys_cycling_through_all_bins(scene):
    check(scene, cycling(5 * BINS + 3), cycling(3 * BINS + 1, 11))
    check(scene, cycling(5 * BINS + 3), cycling(3 * BINS + 1, 11), sort_blocks=5)


@pytest.fixture(scope="module")
def random_keys():
    rng = np.random.default_rng(20240607)
    return rng.integers(0, BINS, 2 ** 21 + 5).astype(np.uint32), rng.integers(0, BINS, 2 ** 20 + 3).astype(np.uint32)


@pytest.mark.parametrize("sort_blocks", [64, 1024])
def test_random_keys_over_many_blocks(scene, random_keys, sort_blocks):
    check(scene, random_keys[0], random_keys[1], sort_blocks)


def test_refusals_leave_the_handle_usable(scene):
    fn = scene.b.fn("raysort_probe")
    keys = np.zeros(8, dtype=np.uint32); order = np.zeros(16, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert fn(None, 8, 8, p(keys), p(keys), 4, p(order)) == pbrt_hip.ERR_INVALID_ARG
    assert fn(scene.h, 8, 8, p(keys), p(keys), 0, p(order)) == pbrt_hip.ERR_INVALID_ARG
    assert fn(scene.h, 8, 8, None, p(keys), 4, p(order)) == pbrt_hip.ERR_INVALID_ARG
    assert fn(scene.h, 8, 8, p(keys), p(keys), 4, None) == pbrt_hip.ERR_INVALID_ARG
    bad = keys.copy(); bad[5] = BINS
    assert fn(scene.h, 8, 8, p(keys), p(bad), 4, p(order)) == pbrt_hip.ERR_INVALID_ARG
    check(scene, cycling(300), cycling(40))
