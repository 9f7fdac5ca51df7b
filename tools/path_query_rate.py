"""Paths per second of ptmi_trace_paths_device, next to ptmi_render with PTMI_FLAG_MEGAKERNEL over the same paths in the same run.

The rays are the built-in camera's own (built on the device in float32 from the JITTERED sample centres: the rate does not need
the sampler's exact values, only rays of the same coherence), one per pixel of a 1920 x 1080 image of the scene, traced for
--spp iterations with first_index = 0 and index_stride = W * H - the seeds ptmi_render uses.  The one-path-per-lane render
kernel runs the same loops per lane (one lane owns one pixel for all the iterations of a launch) and is the yardstick: it does the
same work plus the framebuffer, minus 96 bytes of ray and sum per lane.  Both are timed by HIP events around the launches of one
call after a warm-up, median of --reps.

usage: python tools/path_query_rate.py [--scene tris1m] [--spp 8] [--reps 5] [--out profiles/path_query_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402


def camera_rays(scene, w, h, torch):
    """float32[W*H, 12] ptmi_ray records on the device: the camera ray through every pixel centre"""
    cam = {k: torch.tensor(np.asarray(v, np.float32), device="cuda") for k, v in
           (("o", scene.cameraPosition), ("d", scene.cameraDirection), ("r", scene.cameraRight), ("u", scene.cameraUp))}
    gx = torch.arange(w, device="cuda", dtype=torch.float32).repeat(h)
    gy = torch.arange(h, device="cuda", dtype=torch.float32).repeat_interleave(w)
    sx, sy = ((gx + 0.5) / w - 0.5)[:, None], ((gy + 0.5) / h - 0.5)[:, None]
    rays = torch.zeros((w * h, 12), dtype=torch.float32, device="cuda")
    rays[:, 0:4] = cam["o"]
    rays[:, 4:8] = cam["u"] * sy + (cam["r"] * sx + cam["d"])
    rays[:, 8] = float("inf")
    return rays


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_query_rate.json"))
    a = ap.parse_args()
    w, h, depth = 1920, 1080, 10
    sc = bvh_create(scenes.build(a.scene, w, h), device=a.device)
    torch.cuda.set_device(a.device)
    stream = torch.cuda.Stream(torch.device("cuda", a.device))
    flags = backend.FLAG_DEFAULT_ARITHMETIC | backend.FLAG_NO_HISTOGRAMS | backend.FLAG_MEGAKERNEL
    rec = {"scene": a.scene, "image": [w, h], "iterations": a.spp, "reps": a.reps, "depth": depth, "arithmetic": "default", "paths_per_call": w * h * a.spp}
    be = Backend().setup_context(w, h, depth, sc.lightsSize, S.JITTERED, device=a.device, flags=flags)
    try:
        be.initialize_memory(sc)
        render_ms = []
        for k in range(a.reps + 1):  # (the first is the warm-up)
            be.clear()
            be.synchronize()
            be.kernel_time()
            be.render(0, a.spp)
            ms, launches = be.kernel_time()
            render_ms.append(ms)
        render_counters = None
        be.clear()
        be.render(0, a.spp)
        render_counters = be.counters()

        be.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            rays = camera_rays(sc, w, h, torch)
            sums = torch.zeros((w * h, 12), dtype=torch.float32, device="cuda")
        stream.synchronize()
        trace_ms = []
        for k in range(a.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            be.trace_paths_device(rays.data_ptr(), w * h, sums.data_ptr(), first_iteration=0, n_iterations=a.spp, first_index=0, index_stride=w * h)
            t1.record(stream)
            t1.synchronize()
            trace_ms.append(t0.elapsed_time(t1))
        host = np.ascontiguousarray(sums.cpu().numpy()).view(S.PATH_SUM).reshape(-1)
        be.set_stream(None)
    finally:
        be.release()
    paths = w * h * a.spp
    r, t = float(np.median(render_ms[1:])), float(np.median(trace_ms[1:]))
    rec["render_megakernel"] = {"ms_median": round(r, 3), "ms_all": [round(x, 3) for x in render_ms[1:]], "launches_per_call": launches,
                                "paths_per_s": round(paths / r * 1e3), "segments": render_counters["segments"]}
    rec["trace_paths_device"] = {"ms_median": round(t, 3), "ms_all": [round(x, 3) for x in trace_ms[1:]], "paths_per_s": round(paths / t * 1e3),
                                 "segments": int(host["segments"].sum())}
    rec["trace_over_render_rate"] = round(r / t, 3)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
