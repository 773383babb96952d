"""not gpu: bench.py --dump-outputs writes what the last timed step returned — the whole film when it fits in 64 MiB, else a fixed, seeded
sample of its pixels with their indices — in float32 / float64 only."""
import os

import numpy as np

import bench
import pbrt_hip


def _stats():
    st = pbrt_hip.Stats()
    st.camera_rays, st.regular_rays, st.shadow_rays, st.paths_zero_radiance, st.paths_total = 100, 250, 75, 3, 100
    return st


def _film(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.random((h, w, 3), dtype=np.float32), rng.random((h, w), dtype=np.float32)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_film_is_written_whole(tmp_path):
    xyz, wt = _film(48, 64, 1)
    bench.dump_outputs(str(tmp_path / "out"), (xyz, wt), _stats())
    got = _load(tmp_path / "out")
    assert sorted(got) == ["film_weight", "film_xyz", "ray_counts"]
    assert got["film_xyz"].dtype == np.float32 and np.array_equal(got["film_xyz"], xyz)
    assert got["film_weight"].dtype == np.float32 and np.array_equal(got["film_weight"], wt)
    assert got["ray_counts"].dtype == np.float64 and got["ray_counts"].tolist() == [100, 250, 75, 3, 100]


def test_large_film_is_sampled_with_a_fixed_seed(tmp_path):
    xyz, wt = _film(2048, 2048, 2)   # 64 MiB of film: over the cap
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), (xyz, wt), _stats())
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["film_pixel_index", "film_weight", "film_xyz", "ray_counts"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= bench.DUMP_CAP_BYTES
    idx = a["film_pixel_index"]
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_SAMPLE_PIXELS and (np.diff(idx) > 0).all()
    i = idx.astype(np.int64)
    assert np.array_equal(a["film_xyz"], xyz.reshape(-1, 3)[i]) and np.array_equal(a["film_weight"], wt.reshape(-1)[i])
