#!/usr/bin/env python3
"""What a sample-record budget costs, and the frame that needs one (film bands).

    python scripts/film_bands_cost.py cost OUT.json           configs[1] (100 k triangles, 512^2 @ 64 spp, depth 5) in one band, with the budget at a quarter and at a
                                                              sixteenth of its need: wall and device time per frame, footprint, film hash (which must not change)
    python scripts/film_bands_cost.py large SPP OUT.json      1920 x 1080, depth 1, 12 triangles under a constant sky at SPP samples per pixel, automatic budget: choose SPP so
                                                              that 1920 * 1080 * SPP * 20 B exceeds the card's free memory (8192: 340 GB); run a smaller SPP first for the rate
"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-v3-rs_amd"))
import pbrt_hip  # noqa: E402


def cost(out_path):
    host = pbrt_hip.Host()
    s = pbrt_hip.Scene(device=0)
    pbrt_hip.capture_spec(pbrt_hip.SceneSpec(n_tris=100_000, seed=1, xres=512, yres=512, spp=64, max_depth=5), s, host, device_build=True)
    need = 512 * 512 * 64 * 20
    rows = []
    for label, budget in (("one band", 0), ("a quarter of the need", need // 4), ("one band, again", 0), ("a quarter, again", need // 4), ("a sixteenth", need // 16)):
        s.set_sample_record_budget(budget)
        s.render_path(max_depth=5)   # the buffers of this size exist before the timed frames
        wall = []
        for _ in range(5):
            t = time.perf_counter(); xyz, wt, st = s.render_path(max_depth=5); wall.append(time.perf_counter() - t)
        rows.append(dict(label=label, budget=budget, footprint=s.render_footprint(), wall_ms=[round(1e3 * v, 2) for v in wall], device_ms_last=round(1e3 * st.render_seconds, 2),
                         film_sha256_12=hashlib.sha256(xyz.tobytes() + wt.tobytes()).hexdigest()[:12], rays=st.regular_rays + st.shadow_rays))
        print(rows[-1], flush=True)
    assert len({r["film_sha256_12"] for r in rows}) == 1, "the film depends on the budget"
    json.dump(rows, open(out_path, "w"), indent=1)


def large(spp, out_path):
    import torch
    host = pbrt_hip.Host()
    s = pbrt_hip.Scene(device=0)
    pbrt_hip.capture_spec(pbrt_hip.SceneSpec(n_tris=12, seed=5, xres=1920, yres=1080, spp=spp, max_depth=1), s, host)
    free_b, total_b = torch.cuda.mem_get_info(0)
    t = time.perf_counter(); xyz, wt, st = s.render_path(max_depth=1); wall = time.perf_counter() - t
    rec = dict(scene="12 random triangles under a constant sky, 1920 x 1080, depth 1", spp=spp, record_bytes_whole_frame=1920 * 1080 * spp * 20, device_free_bytes_before=free_b,
               device_total_bytes=total_b, result="PBRT_HIP_OK", footprint=s.render_footprint(), wall_seconds=round(wall, 3), device_seconds=round(st.render_seconds, 3),
               camera_rays=st.camera_rays, regular_rays=st.regular_rays, shadow_rays=st.shadow_rays, film_mean=float(xyz.mean()), weight_min=float(wt.min()), weight_max=float(wt.max()))
    print(rec, flush=True)
    json.dump(rec, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "cost":
        cost(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "large":
        large(int(sys.argv[2]), sys.argv[3])
    else:
        sys.exit(__doc__)
