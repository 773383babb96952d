"""-m gpu: bench.py's plain run (the headline only), --dump-outputs (the last timed frame, the same from run to run) and --full (roofline
counting pass + CPU baseline on top of the same frame)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--config", "1", "--steps", "2", "--warmup", "1", "--spp", "4", "--res", "160", "--n-tris", "8000"]


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + COMMON + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_timed_frame(tmp_path):
    a = _bench(["--dump-outputs", str(tmp_path / "a")])
    b = _bench(["--dump-outputs", str(tmp_path / "b")])
    assert a["steps"] == 2 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["value"] > 0
    assert a["metric"] == "Mrays/s" and a["unit"] == "Mrays/s" and a["higher_is_better"] is True and a["dtype"] == "f32"
    assert "cpu_baseline" not in a and a["roofline"]["achieved"] is None   # the plain run does no work beyond the timed steps
    for d in ("a", "b"):
        xyz, wt, rc = (np.load(tmp_path / d / f) for f in ("film_xyz.npy", "film_weight.npy", "ray_counts.npy"))
        assert xyz.shape == (160, 160, 3) and xyz.dtype == np.float32 and wt.shape == (160, 160) and wt.dtype == np.float32 and rc.dtype == np.float64
        assert hashlib.sha256(xyz.tobytes() + wt.tobytes()).hexdigest() == a["film_sha256"]
        assert int(rc[1] + rc[2]) == a["config"]["rays_per_frame"]
    assert a["film_sha256"] == b["film_sha256"]


def test_full_run_adds_roofline_and_cpu_baseline():
    plain = _bench([])
    full = _bench(["--full"])
    assert full["film_sha256"] == plain["film_sha256"] and full["config"]["rays_per_frame"] == plain["config"]["rays_per_frame"]
    assert full["roofline"]["achieved"] > 0 and full["roofline"]["closest_hit"]["rays"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["gpu_over_cpu"] > 0
