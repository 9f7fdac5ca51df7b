"""Cost of ptmi_render_guides_device on the tris1m scene, next to ptmi_render of the same iterations in the same run.

One 1920 x 1080 call of 1 and one of 4 iterations, all five planes, to device pointers (torch tensors), timed by HIP events
on the context's stream after a warm-up, median of --reps.  The thing to hold it against is taken from this very library in the
same run: ptmi_kernel_time of ptmi_render for the same iterations (a render iteration traces several segments and their shadow
rays where a guide iteration traces one segment), so guide_vs_render_per_iteration says what a guide iteration costs in units
of a render iteration.

usage: python tools/guide_rate.py [--scene tris1m] [--reps 5] [--out profiles/guide_rate_tris1m.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_rate_tris1m.json"))
    a = ap.parse_args()
    w, h, depth = 1920, 1080, 10
    sc = bvh_create(scenes.build(a.scene, w, h), device=a.device)
    torch.cuda.set_device(a.device)
    stream = torch.cuda.Stream(torch.device("cuda", a.device))
    rec = {"scene": a.scene, "triangles": len(sc.triangulation), "max_depth": int(sc.bvhMaxDepth), "image": [w, h], "depth": depth,
           "reps": a.reps, "arithmetic": "default", "render": {}, "guides": {}}
    be = Backend().setup_context(w, h, depth, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC | backend.FLAG_NO_HISTOGRAMS)
    try:
        be.initialize_memory(sc)
        be.render(0, 4)  # warm-up
        be.synchronize()
        be.kernel_time()
        for n in (1, 4):
            be.clear()
            be.synchronize()
            be.kernel_time()
            be.render(0, n)
            ms, launches = be.kernel_time()
            c = be.counters()
            rec["render"][str(n)] = {"iterations": n, "kernel_ms": round(ms, 3), "launches": launches, "segments": c["segments"],
                                     "shadow_rays": c["shadow_rays"], "ms_per_iteration": round(ms / n, 3)}
        be.set_stream(stream.cuda_stream)
        planes = {name: torch.zeros((h, w) if name == "hit_count" else (h, w, 4), dtype=torch.int32 if name == "ids" else torch.float32, device="cuda")
                  for name in backend.GUIDE_PLANES}
        pointers = {name: t.data_ptr() for name, t in planes.items()}
        torch.cuda.synchronize()
        for n in (1, 4):
            times = []
            for rep in range(a.reps + 1):  # (the first is the warm-up)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                be.render_guides_device(0, n, **pointers)
                t1.record(stream)
                t1.synchronize()
                times.append(t0.elapsed_time(t1))
            med = float(np.median(times[1:]))
            hit_fraction = float(planes["hit_count"].sum().item()) / (n * w * h)
            g = {"iterations": n, "ms_median": round(med, 3), "ms_all": [round(t, 3) for t in times[1:]], "ms_warm_up": round(times[0], 3),
                 "ms_per_iteration": round(med / n, 3), "msegments_per_s": round(n * w * h / med / 1e3, 1), "hit_fraction": round(hit_fraction, 4)}
            g["guide_vs_render_per_iteration"] = round(g["ms_per_iteration"] / rec["render"][str(n)]["ms_per_iteration"], 4)
            rec["guides"][str(n)] = g
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
