#!/usr/bin/env python3
"""Cost of the traversal kernel's (inst, quadric) rows on a large instanced frame, without a target: one object of N_TRIS random triangles placed N_INST times (capture_spec's
lattice), a few hundred small spheres scattered through the lattice, 512 x 512 @ 16 spp, depth 5 — next to the same scene WITHOUT the spheres, which runs the plain instancing
row.  Prints and writes (argv[1], default profiles/quadric_instances_frame.json) the frame, traversal and shade times of both, the median of STEPS renders after one warm-up.

    python scripts/quadric_instances_frame.py [OUT.json]"""
import json
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(_root, "pbrt-v3-rs_amd"), os.path.join(_root, "tests")]

import numpy as np

import pbrt_hip

N_TRIS, N_INST, N_SPHERES, RES, SPP, DEPTH, STEPS = 10000, 1000, 300, 512, 16, 5, 3


def capture(host, spheres):
    s = pbrt_hip.Scene()
    if spheres:   # ahead of the lattice in the primitive list; centres uniform in [-1, 1]^3, the cube capture_spec's lattice of instances fills (cell 0.2 wide at 1 000 instances); radius about a third of a cell
        g = np.random.default_rng(77)
        m = s.add_material_matte((0.7, 0.3, 0.2))
        for c in g.uniform(-1.0, 1.0, (N_SPHERES, 3)):
            t = host.compose((pbrt_hip.IDENTITY.copy(), pbrt_hip.IDENTITY.copy()), host.translate(c))
            s.add_sphere(t[0], t[1], 0.03, None, None, 360.0, m, False)
    spec = pbrt_hip.SceneSpec(n_tris=N_TRIS, seed=1, xres=RES, yres=RES, spp=SPP, max_depth=DEPTH)
    pbrt_hip.capture_spec(spec, s, host, instances=N_INST)     # host builders (a scene with a quadric is not built on the device)
    return s


def measure(s):
    rows = []
    for k in range(STEPS + 1):
        _, _, st = s.render_path(max_depth=DEPTH)
        if k:
            rows.append(st.as_dict())
    med = lambda f: float(np.median([r[f] for r in rows]))
    rays = rows[0]["regular_rays"] + rows[0]["shadow_rays"]
    return {"rays": rays, "render_seconds": med("render_seconds"), "traversal_seconds": med("extend_seconds") + med("shadow_seconds"), "shade_seconds": med("shade_seconds"),
            "mrays_per_s": rays / med("render_seconds") * 1e-6, "runs": [{f: r[f] for f in ("render_seconds", "extend_seconds", "shadow_seconds", "shade_seconds")} for r in rows]}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_root, "profiles", "quadric_instances_frame.json")
    host = pbrt_hip.Host()
    res = {"scene": {"object_triangles": N_TRIS, "instances": N_INST, "spheres": N_SPHERES, "sphere_radius": 0.03, "res": RES, "spp": SPP, "max_depth": DEPTH, "steps": STEPS}}
    for name, spheres in (("instances_only", False), ("instances_and_spheres", True)):
        with capture(host, spheres) as s:
            res[name] = measure(s)
        print(name, json.dumps({k: v for k, v in res[name].items() if k != "runs"}), flush=True)
    res["traversal_ratio"] = res["instances_and_spheres"]["traversal_seconds"] / res["instances_only"]["traversal_seconds"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("traversal ratio (with spheres / without):", round(res["traversal_ratio"], 3))


if __name__ == "__main__":
    main()
