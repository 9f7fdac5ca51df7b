"""Rate of ptmi_query_rays_device on the tris1m scene, next to the integrator's own segment rate in the same run.

2^22 rays of two kinds - pinhole rays of a 2048 x 2048 image from the scene's camera (coherent: neighbouring lanes walk the
same nodes) and segments between random points of the scene's box (incoherent) - for PTMI_QUERY_CLOSEST and PTMI_QUERY_ANY, with
device pointers (torch tensors), timed by HIP events on the context's stream after a warm-up, median of --reps.
The yardstick: ptmi_counters.segments / ptmi_kernel_time of a 4-iteration render of the same context (closest-hit queries of
the integrator, its shadow rays not counted), so the ratio says what a query costs in units of the integrator's own traversal.

usage: python tools/query_rate.py [--scene tris1m] [--log2-rays 22] [--reps 5] [--out profiles/ray_query_rate_tris1m.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402

f32 = np.float32


def pinhole(sc, side):
    y, x = np.mgrid[0:side, 0:side]
    # 8 x 8 pixel tiles in a row, so that a wave's 64 rays are a tile (as the integrator lays its paths out)
    order = (((y // 8) * (side // 8) + (x // 8)) * 64 + (y % 8) * 8 + (x % 8)).ravel().argsort()
    sx = (((x.ravel()[order] + 0.5) / side) - 0.5).astype(f32)[:, None]
    sy = (((y.ravel()[order] + 0.5) / side) - 0.5).astype(f32)[:, None]
    d = (np.asarray(sc.cameraDirection, f32) + np.asarray(sc.cameraRight, f32) * sx + np.asarray(sc.cameraUp, f32) * sy).astype(f32)
    return backend.make_rays(np.tile(np.asarray(sc.cameraPosition, f32), (len(d), 1)), d)


def segments(sc, n, seed=1):
    rs = np.random.default_rng(seed)
    box = sc.bvh[0]["trianglesAABB"]
    lo, hi = np.asarray(box["pMin"], np.float64)[:3], np.asarray(box["pMax"], np.float64)[:3]
    p, q = rs.uniform(lo, hi, (n, 3)).astype(f32), rs.uniform(lo, hi, (n, 3)).astype(f32)
    o = np.concatenate([p, np.full((n, 1), np.asarray(sc.cameraPosition, f32)[3], f32)], axis=1)
    return backend.make_rays(o, q - p)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--log2-rays", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query_rate_tris1m.json"))
    a = ap.parse_args()
    side = 1 << (a.log2_rays // 2)
    n = side * side
    w, h, depth = 1920, 1080, 10
    sc = bvh_create(scenes.build(a.scene, w, h), device=a.device)
    torch.cuda.set_device(a.device)
    stream = torch.cuda.Stream(torch.device("cuda", a.device))
    rec = {"scene": a.scene, "triangles": len(sc.triangulation), "max_depth": int(sc.bvhMaxDepth), "rays": n, "reps": a.reps, "arithmetic": "default"}
    be = Backend().setup_context(w, h, depth, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC | backend.FLAG_NO_HISTOGRAMS)
    try:
        be.initialize_memory(sc)
        # the integrator's own rate: a warm-up render, then 4 iterations
        be.render(0, 4)
        be.synchronize()
        be.kernel_time()
        be.clear()
        be.render(0, 4)
        ms, launches = be.kernel_time()
        c = be.counters()
        rec["integrator"] = {"image": [w, h], "depth": depth, "iterations": 4, "kernel_ms": round(ms, 3), "launches": launches, "segments": c["segments"],
                             "shadow_rays": c["shadow_rays"], "box_tests_per_segment": round(c["box_tests"] / (c["segments"] + c["shadow_rays"]), 2),
                             "msegments_per_s": round(c["segments"] / ms / 1e3, 1), "mrays_per_s": round((c["segments"] + c["shadow_rays"]) / ms / 1e3, 1)}
        be.set_stream(stream.cuda_stream)
        rec["queries"] = {}
        for rays_name, rays in (("pinhole", pinhole(sc, side)), ("segments", segments(sc, n))):
            d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 12)).cuda()
            d_hits = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for any_hit in (False, True):
                times = []
                for rep in range(a.reps + 1):  # (the first is the warm-up)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    be.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit)
                    t1.record(stream)
                    t1.synchronize()
                    times.append(t0.elapsed_time(t1))
                hits = d_hits.cpu().numpy().view(S.RAY_HIT).reshape(-1)
                med = float(np.median(times[1:]))
                q = {"ms_median": round(med, 3), "ms_all": [round(t, 3) for t in times[1:]], "ms_warm_up": round(times[0], 3), "mrays_per_s": round(n / med / 1e3, 1),
                     "hit_fraction": round(float((hits["triangle_id"] != S.RAY_MISS).mean()), 4), "box_tests_per_ray": round(float(hits["box_tests"].mean()), 2),
                     "triangle_tests_per_ray": round(float(hits["triangle_tests"].mean()), 2)}
                q["vs_integrator_segments"] = round(q["mrays_per_s"] / rec["integrator"]["msegments_per_s"], 3)
                q["vs_integrator_rays"] = round(q["mrays_per_s"] / rec["integrator"]["mrays_per_s"], 3)
                rec["queries"][f"{rays_name}_{'any' if any_hit else 'closest'}"] = q
        be.set_stream(None)
    finally:
        be.release()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
