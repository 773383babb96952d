"""Build times of the SAH device builder with quadric slots (csrc/bvh_sah_device.hip), on the GPU box.  Two measurements, one JSON object (--out):

benefit     1 M random triangles plus 64 spheres: Scene.build_accel_device_shapes(0, 4) on one handle against Scene.build_accel(0, 4) on another (the multi-threaded host builder, confined to
            --host-cpus CPUs: the process's affinity is cut to that many before the library is loaded), alternating, three counted builds each after one uncounted build each;
            medians of accel_stats()['build_seconds'], arrays compared.
triangles   configs[2]'s 4.3 M triangles, no quadric: Scene.build_accel_device(0, 4) of another build of the library (--parent-lib, the parent commit's) against this tree's.  One
            process per run, the libraries alternating; a process builds 1 000 triangles first (start-up: code objects, the first allocations), then the scene once.  Medians,
            the parent's own spread, a digest of the arrays.

    python scripts/sah_quadrics_build_time.py --parent-lib /path/to/parent/libpbrt_hip.so --out profiles/sah_quadrics_build.json
(--child-triangles N is the one-run process the second measurement starts.)"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v3-rs_amd"))


def digest(scene):
    nodes, recs = scene.accel_copy()
    return hashlib.sha256(nodes.tobytes() + recs.tobytes()).hexdigest()[:16]


def child_triangles(n_tris):
    import pbrt_hip
    host = pbrt_hip.Host()
    with pbrt_hip.Scene() as warm:
        P, idx = host.gen_random_tris(1000, 3)
        warm.add_mesh(P, idx, warm.add_material_matte((0.5, 0.5, 0.5), 0.0)); warm.build_accel_device(0, 4)
    P, idx = host.gen_random_tris(n_tris, 1)
    with pbrt_hip.Scene() as s:
        s.add_mesh(P, idx, s.add_material_matte((0.5, 0.5, 0.5), 0.0))
        s.build_accel_device(0, 4)
        st = s.accel_stats()
        print(json.dumps({"build_seconds": round(st["build_seconds"], 4), "interior_nodes": st["interior_nodes"], "leaves": st["leaves"], "digest": digest(s)}), flush=True)


def triangles(n_tris, parent_lib, runs):
    res = {"scene": f"configs[2] geometry: gen_random_tris({n_tris}, seed 1), one matte mesh; no quadric, so the build passes null tables",
           "per_process": "one start-up build of 1 000 triangles (not counted), then one counted build; the libraries alternate (parent, this tree, parent, ..)", "parent": [], "this_tree": []}
    for r in range(runs):
        for key, lib in (("parent", parent_lib), ("this_tree", None)):
            env = dict(os.environ)
            env.pop("PBRT_HIP_LIB", None)
            if lib: env["PBRT_HIP_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-triangles", str(n_tris)], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:      # nothing more is started on the GPU after a failure
                raise SystemExit(f"{key} run {r}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            res[key].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(key, res[key][-1], flush=True)
    for key in ("parent", "this_tree"):
        t = [x["build_seconds"] for x in res[key]]
        res[key] = {"build_seconds": t, "median": round(statistics.median(t), 4), "min": min(t), "max": max(t), "digests": sorted({x["digest"] for x in res[key]}),
                    "interior_nodes": res[key][0]["interior_nodes"], "leaves": res[key][0]["leaves"]}
    p, n = res["parent"], res["this_tree"]
    res["arrays_equal_by_digest"] = p["digests"] == n["digests"] and len(p["digests"]) == 1
    res["parent_spread"] = round(p["max"] - p["min"], 4)
    res["new_median_minus_parent_median"] = round(n["median"] - p["median"], 4)
    res["within_parent_spread"] = abs(n["median"] - p["median"]) <= p["max"] - p["min"] or n["median"] <= p["median"]
    return res


def benefit(n_tris, n_quadrics, host_threads):
    import numpy as np
    import pbrt_hip
    host = pbrt_hip.Host()
    P, idx = host.gen_random_tris(n_tris, 1)
    rng = np.random.default_rng(5)
    centres = rng.uniform(-0.9, 0.9, (n_quadrics, 3))

    def capture(s):
        m = s.add_material_matte((0.5, 0.5, 0.5), 0.0)
        half = 3 * (n_tris // 2)
        s.add_mesh(P, idx[:half], m)
        for c in centres:
            t = host.translate(tuple(float(v) for v in c))
            s.add_sphere(t[0], t[1], 0.05, None, None, 360.0, m, False)
        s.add_mesh(P, idx[half:], m)

    dev, hst = pbrt_hip.Scene(), pbrt_hip.Scene()
    capture(dev); capture(hst)
    res = {"scene": f"gen_random_tris({n_tris}, seed 1) as two meshes with {n_quadrics} spheres of radius 0.05 between them", "host_cpus": host_threads, "cpus_of_the_machine": os.cpu_count(),
           "order": "device, host, device, host, ..; the first build of each handle is listed apart", "device_s": [], "host_s": []}
    for k in range(4):
        dev.build_accel_device_shapes(0, 4); res["device_s"].append(round(dev.accel_stats()["build_seconds"], 4))
        hst.build_accel(0, 4); res["host_s"].append(round(hst.accel_stats()["build_seconds"], 4))
        print("benefit", k, res["device_s"][-1], res["host_s"][-1], flush=True)
    res["first_build_device_s"], res["first_build_host_s"] = res["device_s"].pop(0), res["host_s"].pop(0)
    res["device_median_s"], res["host_median_s"] = statistics.median(res["device_s"]), statistics.median(res["host_s"])
    (dn, dr), (hn, hr) = dev.accel_copy(), hst.accel_copy()
    res["arrays_identical"] = bool(np.array_equal(dn[:, 12:16], hn[:, 12:16]) and np.array_equal(dn[:, :12].view(np.float32), hn[:, :12].view(np.float32)) and np.array_equal(dr, hr))
    res["quadric_records"] = int(((dr[:, 7] & 128) != 0).sum())
    sd, sh = dev.accel_stats(), hst.accel_stats()
    res["stats_identical"] = {k: v for k, v in sd.items() if k != "build_seconds"} == {k: v for k, v in sh.items() if k != "build_seconds"}
    res.update(interior_nodes=sd["interior_nodes"], leaf_records=sd["leaf_records"], depth=sd["depth"])
    dev.close(); hst.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child-triangles", type=int, default=0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--n-tris", type=int, default=4_300_000)
    ap.add_argument("--host-cpus", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child_triangles:
        return child_triangles(args.child_triangles)
    cpus = sorted(os.sched_getaffinity(0))
    if len(cpus) > args.host_cpus:      # the host builder's threads share these CPUs
        os.sched_setaffinity(0, cpus[:args.host_cpus])
    out = {"what": "SAH device build with quadric slots on one MI355X (scripts/sah_quadrics_build_time.py)", "max_prims_in_node": 4}
    if args.parent_lib:
        out["triangles_only_against_parent"] = triangles(args.n_tris, os.path.abspath(args.parent_lib), args.runs)
    out["benefit_1m_triangles_64_quadrics"] = benefit(1_000_000, 64, len(os.sched_getaffinity(0)))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
