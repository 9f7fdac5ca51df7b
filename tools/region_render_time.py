"""Times ptmi_render_region against ptmi_render: what a call costs as the rectangle shrinks, and prints one JSON record.

On the named scene (default tris1m, 1920 x 1080, depth 10, the reference's default arithmetic), warm calls of --iterations (32):

  render             the whole image through ptmi_render
  region 1/1         the whole image through ptmi_render_region
  region 1/4 .. 1/256   centred rectangles of that share of the area (both sides halved from one to the next)

Each as the host clock around the call and ptmi_synchronize: median and min .. max of --reps (5) calls after one warm-up call of
the same rectangle, and paths per second at the median.  With the record go the persistent grid of the context's launches
(ptmi_scheduler_stats: resident workgroups x lanes) - a launch fills it while the region has that many pixels x iterations to
hand out - and, as a check, whether the accumulators after the region calls equal a render of the same iterations there.

usage: python tools/region_render_time.py [--scene tris1m] [--size 1920x1080] [--depth 10] [--iterations 32] [--reps 5]
                                          [--out profiles/region_render_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402


def timed_ms(be, call, reps):
    """wall ms of `reps` calls, each waited for, after one warm-up call"""
    runs = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        call()
        be.synchronize()
        if k:
            runs.append((time.perf_counter() - t0) * 1e3)
    return runs


def row(name, region, n, runs):
    med = float(np.median(runs))
    paths = region[2] * region[3] * n
    return {"call": name, "region": list(region), "pixels": region[2] * region[3], "ms_median": round(med, 3), "ms_min": round(min(runs), 3),
            "ms_max": round(max(runs), 3), "ms_all": [round(r, 3) for r in runs], "paths_per_s": round(paths / (med * 1e-3)),
            "us_per_kilopath": round(med * 1e3 / (paths / 1e3), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = map(int, a.size.split("x"))
    n = a.iterations
    sc = bvh_create(scenes.build(a.scene, W, H), device=a.device)
    be = Backend().setup_context(W, H, a.depth, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC)
    rec = {"scene": a.scene, "triangles": len(sc.triangulation), "image": [W, H], "depth": a.depth, "iterations_per_call": n, "reps": a.reps,
           "clock": "host, around the call and ptmi_synchronize"}
    try:
        be.initialize_memory(sc)
        whole = (0, 0, W, H)
        rows = [row("ptmi_render", whole, n, timed_ms(be, lambda: be.render(0, n), a.reps))]
        stats = be.scheduler_stats()
        rec["grid"] = {"resident_workgroups": stats.get("resident_workgroups"), "workgroup_lanes": stats.get("workgroup_lanes")}
        if rec["grid"]["resident_workgroups"] and rec["grid"]["workgroup_lanes"]:
            rec["grid"]["lanes"] = rec["grid"]["resident_workgroups"] * rec["grid"]["workgroup_lanes"]
            rec["grid"]["pixels_that_fill_it_once"] = -(-rec["grid"]["lanes"] // n)
        for k in range(5):
            w, h = W >> k, H >> k
            r = ((W - w) // 2, (H - h) // 2, w, h)
            rows.append(row(f"ptmi_render_region 1/{4 ** k}", r, n, timed_ms(be, lambda: be.render_region(*r, 0, n), a.reps)))
        rec["calls"] = rows
        full = rows[0]["ms_median"]
        for r in rows:
            r["of_the_frame_time"] = round(r["ms_median"] / full, 4)
            r["of_the_frame_area"] = round(r["pixels"] / (W * H), 5)
        # the check: a rectangle rendered twice by region calls holds what ptmi_render leaves there
        small = rows[-1]["region"]
        be.clear()
        be.render(0, 2)
        want = be.read_region(*small)[0].view(np.uint32).copy()
        be.clear()
        be.render_region(*small, 0, 2)
        rec["identical"] = bool(np.array_equal(want, be.read_region(*small)[0].view(np.uint32)))
        assert rec["identical"]
    finally:
        be.release()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
