"""Times Shape "loopsubdiv" on the device (pbrt_hip_loopsubdiv_mesh): a synthetic control mesh — a jittered height field of --quads x --quads quads, two faces each — refined
--levels times.  Reports the kernels' time by HIP events (the levels, the limit positions, the normals and the world pass; uploads and downloads excluded: what the library
writes to stderr under PBRT_HIP_BUILD_PROFILE, as its device tree builders do — the measuring runs in a child process started with that switch) and the whole call's wall time, best
and median of --repeat after one warm-up call.  Prints one JSON object (and writes it to --out).
Run on the GPU box: python scripts/loopsubdiv_build_time.py --out profiles/loopsubdiv_build.json"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v3-rs_amd"))
import pbrt_hip  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=125)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help="the measuring process: prints the wall times; the library prints the kernels' to stderr")
    a = ap.parse_args()
    n = a.quads + 1
    rng = np.random.default_rng(1)
    g = np.stack(np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64)), -1).reshape(-1, 2)
    P = np.concatenate([g, rng.uniform(-0.3, 0.3, (len(g), 1))], 1).astype(np.float32)
    q = np.arange(a.quads)
    X, Y = np.meshgrid(q, q)
    v00 = (Y * n + X).ravel(); v10 = v00 + 1; v11 = v00 + n + 1; v01 = v00 + n
    idx = np.stack([v00, v10, v11, v00, v11, v01], 1).astype(np.uint32).ravel()
    host = pbrt_hip.Host()
    m, mi = host.compose(host.translate([1.0, 2.0, 3.0]), host.scale([2.0, 3.0, 0.5]))
    if a.child:
        with pbrt_hip.Scene() as s:
            nv, nt = s.loopsubdiv_mesh(P, idx, a.levels, counts_only=True)
            s.loopsubdiv_mesh(P, idx, a.levels, m, mi)     # warm-up: the code object loads
            wall = []
            for _ in range(a.repeat):
                t = time.perf_counter()
                s.loopsubdiv_mesh(P, idx, a.levels, m, mi)
                wall.append((time.perf_counter() - t) * 1e3)
        print(json.dumps({"out_vertices": nv, "out_triangles": nt, "wall": wall}))
        sys.exit(0)
    env = dict(os.environ, PBRT_HIP_BUILD_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--quads", str(a.quads), "--levels", str(a.levels), "--repeat", str(a.repeat)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(r.stdout + r.stderr)
    child = json.loads(r.stdout.strip().splitlines()[-1])
    dev = [float(v) for v in re.findall(r"loopsubdiv_device .*: kernels ([0-9.]+) ms", r.stderr)][1:]     # the first line is the warm-up call's
    assert len(dev) == a.repeat, r.stderr
    wall = child["wall"]
    res = {"control_faces": len(idx) // 3, "control_vertices": len(P), "levels": a.levels, "out_vertices": child["out_vertices"], "out_triangles": child["out_triangles"], "repeat": a.repeat,
           "device_ms_best": round(min(dev), 3), "device_ms_median": round(float(np.median(dev)), 3), "device_ms_all": [round(v, 3) for v in dev],
           "call_wall_ms_best": round(min(wall), 2), "call_wall_ms_median": round(float(np.median(wall)), 2)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
