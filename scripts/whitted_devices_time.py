"""What the Whitted integrator's multi-device driver costs, on ONE GPU (contexts that share a GPU measure overhead, not speed-up).  Two measurements, one JSON object (--out):

unchanged   Scene.render_whitted of another build of the library (--parent-lib, the parent commit's) against this tree's: one process per run, the libraries alternating, the
            parent first and last.  A process renders the frame once uncounted, then three times; its figure is the median.  Both sides' spread over their processes is reported.
devices     Scene.render_whitted_devices of this tree with 1, 2 and 4 contexts on the GPU (ordinal 0 repeated), one process each, the same four frames: what partition,
            exchange and merge add to the one-device frame.

The frame is the lights/diffuse-shaped scene of tests/sphere_light_scenes.py (a sphere light over the cube and the checkered floor) at 400 x 400, 128 spp, depth 5.  Every
process runs under its own time limit, and nothing more is started after one that fails.

    python scripts/whitted_devices_time.py --parent-lib /path/to/parent/libpbrt_hip.so --out profiles/whitted_devices.json
(--child N is the one-process run: N = 0 renders with render_whitted, N >= 1 with render_whitted_devices on N contexts.)"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v3-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
RES, SPP, DEPTH, FRAMES = 400, 128, 5, 3


def child(n_contexts):
    import pbrt_hip
    import sphere_light_scenes as SL
    host = pbrt_hip.Host()
    with (pbrt_hip.Scene(devices=[0] * n_contexts) if n_contexts else pbrt_hip.Scene()) as s:
        SL.lights_diffuse(s, host, spp=SPP, res=RES)
        render = (lambda: s.render_whitted_devices(max_depth=DEPTH)) if n_contexts else (lambda: s.render_whitted(max_depth=DEPTH))
        render()   # start-up: code objects, workspaces, the replicas
        wall, dev = [], []
        for _ in range(FRAMES):
            t = time.perf_counter(); xyz, wt, st = render(); wall.append(time.perf_counter() - t); dev.append(st.render_seconds)
        print(json.dumps({"wall_ms": [round(1e3 * v, 2) for v in wall], "device_ms": [round(1e3 * v, 2) for v in dev], "wall_ms_median": round(1e3 * statistics.median(wall), 2),
                          "device_ms_median": round(1e3 * statistics.median(dev), 2), "rays": st.camera_rays + st.regular_rays + st.shadow_rays,
                          "film_sha256_12": hashlib.sha256(xyz.tobytes() + wt.tobytes()).hexdigest()[:12]}), flush=True)


def run_child(n_contexts, lib, limit):
    env = dict(os.environ)
    env.pop("PBRT_HIP_LIB", None)
    if lib: env["PBRT_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_contexts)], env=env, capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:      # nothing more is started on the GPU after a failure
        raise SystemExit(f"child {n_contexts} ({lib or 'this tree'}): exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def side(rows):
    w = [r["wall_ms_median"] for r in rows]; d = [r["device_ms_median"] for r in rows]
    return {"processes": rows, "wall_ms_median": round(statistics.median(w), 2), "wall_ms_min": min(w), "wall_ms_max": max(w), "wall_ms_spread": round(max(w) - min(w), 2),
            "device_ms_median": round(statistics.median(d), 2), "device_ms_spread": round(max(d) - min(d), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pairs", type=int, default=2, help="parent / this-tree pairs before the closing parent run")
    ap.add_argument("--limit", type=int, default=120, help="seconds a process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child >= 0:
        return child(args.child)
    out = {"what": "Whitted integrator, one device against several contexts on ONE MI355X (scripts/whitted_devices_time.py)",
           "frame": f"tests/sphere_light_scenes.py lights_diffuse, {RES} x {RES}, {SPP} spp, depth {DEPTH}; per process one uncounted frame, then {FRAMES}; wall = the call, device = PbrtHipStats::render_seconds",
           "note": "the contexts shared one GPU: these are the costs of partition, exchange and merge, not a scaling curve; a measured 1 -> N curve is outstanding"}
    if args.parent_lib:
        parent_lib = os.path.abspath(args.parent_lib)
        rows = {"parent": [], "this_tree": []}
        for _ in range(args.pairs):
            rows["parent"].append(run_child(0, parent_lib, args.limit)); print("parent", rows["parent"][-1], flush=True)
            rows["this_tree"].append(run_child(0, None, args.limit)); print("this tree", rows["this_tree"][-1], flush=True)
        rows["parent"].append(run_child(0, parent_lib, args.limit)); print("parent", rows["parent"][-1], flush=True)
        p, n = side(rows["parent"]), side(rows["this_tree"])
        out["render_whitted_parent_against_this_tree"] = {
            "order": "parent, this tree, .., parent", "parent": p, "this_tree": n,
            "films_equal_by_digest": len({r["film_sha256_12"] for r in rows["parent"] + rows["this_tree"]}) == 1,
            "this_tree_median_minus_parent_median_wall_ms": round(n["wall_ms_median"] - p["wall_ms_median"], 2),
            "this_tree_inside_parent_range": p["wall_ms_min"] <= n["wall_ms_median"] <= p["wall_ms_max"]}
    dev = {}
    for n in (1, 2, 4):
        dev[str(n)] = run_child(n, None, args.limit); print("contexts", n, dev[str(n)], flush=True)
    out["render_whitted_devices_contexts_on_one_gpu"] = dev
    out["devices_films_equal_by_digest"] = len({r["film_sha256_12"] for r in dev.values()}) == 1
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
