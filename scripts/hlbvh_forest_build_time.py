"""Instanced scenes built with HLBVH on the device (bvh_device.hip, forest form) and on the host (build_forest_host): the arrays must be identical, a small film from either tree
the same bits; build times of both, alternating, best of `--repeat`.  Scenes: the configs[4] generator (pbrt_hip/sanmiguel.py) at `--sm-scale`, and one 10 k-triangle object
instanced 1 000 times.  Prints one JSON object (and writes it to --out).  Run on the GPU box: python scripts/hlbvh_forest_build_time.py --out profiles/hlbvh_forest_build.json"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v3-rs_amd"))
import pbrt_hip  # noqa: E402


def measure(name, capture, repeat):
    dev, hst = pbrt_hip.Scene(), pbrt_hip.Scene()
    capture(dev); capture(hst)      # (the captures build the SAH tree; the HLBVH builds below replace it)
    res = {"scene": name, "device_s": [], "host_s": [], "device_wall_s": [], "host_wall_s": []}
    for _ in range(repeat):
        if "device_error" in res or "host_error" in res:
            break
        for s, fn, key in ((dev, dev.build_accel_device, "device"), (hst, hst.build_accel, "host")):
            t = time.time()
            try:
                fn(1, 4)
            except pbrt_hip.PbrtHipError as e:
                res[key + "_error"] = [e.code, str(e)]
                res[key + "_refused_after_s"] = round(time.time() - t, 4)
                continue
            res[key + "_wall_s"].append(round(time.time() - t, 4)); res[key + "_s"].append(round(s.accel_stats()["build_seconds"], 4))
        print(name, {k: v for k, v in res.items() if k != "scene"}, flush=True)
    if "device_error" in res or "host_error" in res:
        res["same_refusal"] = res.get("device_error", [0])[0] == res.get("host_error", [0])[0]
        return res
    (dn, dr), (hn, hr) = dev.accel_copy(), hst.accel_copy()
    sd, sh = dev.accel_stats(), hst.accel_stats()
    res.update(interior_nodes=sd["interior_nodes"], leaf_records=sd["leaf_records"], depth=sd["depth"],
               arrays_identical=bool(np.array_equal(dn[:, 12:16], hn[:, 12:16]) and np.array_equal(dn[:, :12].view(np.float32), hn[:, :12].view(np.float32)) and np.array_equal(dr, hr)),
               stats_identical={k: v for k, v in sd.items() if k != "build_seconds"} == {k: v for k, v in sh.items() if k != "build_seconds"})
    films = []
    for s in (dev, hst):
        xyz, wt, st = s.render_path(max_depth=3)
        films.append((hashlib.sha256(xyz.tobytes() + wt.tobytes()).hexdigest()[:16], st.regular_rays, st.shadow_rays))
    res.update(film_device=films[0], film_host=films[1], films_identical=films[0] == films[1])
    res["device_best_s"], res["host_best_s"] = min(res["device_s"]), min(res["host_s"])
    dev.close(); hst.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sm-scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    host = pbrt_hip.Host()
    out = {"split_method": "hlbvh", "max_prims_in_node": 4, "host_threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"]), "scenes": []}
    from pbrt_hip.sanmiguel import SanMiguelScene
    sm = SanMiguelScene(host, scale=args.sm_scale)
    out["scenes"].append(measure(f"configs[4] generator, scale {args.sm_scale}", lambda s: sm.capture(s, 64, 36, 2), args.repeat))
    spec = pbrt_hip.SceneSpec(n_tris=10_000, seed=7, xres=64, yres=64, spp=2)
    out["scenes"].append(measure("one 10 k-triangle object x 1 000 instances", lambda s: pbrt_hip.capture_spec(spec, s, host, instances=1000), args.repeat))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
