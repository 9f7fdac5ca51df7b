"""Cost of ptmi_reproject_device at 1920 x 1080, next to one ptmi_render iteration of the same scene in the same run.

The inputs are real: --spp iterations of the scene in torch tensors (the previous image) with the guide planes of the same
iterations, and the guide planes of a second camera.  Two cases: the previous camera IS the current one (every tap falls on its
own pixel: the gathers are as coherent as they get), and the previous camera is the current one orbited by --degrees about the
point the image's centre sees (the gathers of a tile land on a shifted, slightly turned tile).  A timed window is --calls calls
between two HIP events on the context's stream (one call is a fraction of a millisecond, too short to time alone), after a
warm-up, median of --reps windows.  Beside the times: the bytes a call must move at the least - it reads the three current
planes (36 bytes per pixel), touches each pixel of the five previous planes about once (56) and writes the result (20) - and the
time that takes at the HBM rate a float4 copy reaches on this part, 6.3 TB/s.

usage: python tools/reproject_rate.py [--scene tris1m] [--out profiles/reproject_rate_1080p.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402

CURRENT_BYTES, PREVIOUS_BYTES, WRITE_BYTES, HBM_BYTES_PER_S = 36, 56, 20, 6.3e12
PLANES = ("normal", "position", "hit_count")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--degrees", type=float, default=1.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_rate_1080p.json"))
    a = ap.parse_args()
    w, h, depth = 1920, 1080, 10
    sc = bvh_create(scenes.build(a.scene, w, h), device=a.device)
    torch.cuda.set_device(a.device)
    stream = torch.cuda.Stream(torch.device("cuda", a.device))
    floor_bytes = (CURRENT_BYTES + PREVIOUS_BYTES + WRITE_BYTES) * w * h
    rec = {"scene": a.scene, "image": [w, h], "spp": a.spp, "reps": a.reps, "calls_per_window": a.calls, "arithmetic": "default",
           "defaults": backend.REPROJECT_DEFAULTS, "orbit_degrees": a.degrees,
           "floor": {"current_bytes_per_pixel": CURRENT_BYTES, "previous_bytes_per_pixel": PREVIOUS_BYTES, "write_bytes_per_pixel": WRITE_BYTES,
                     "bytes": floor_bytes, "hbm_bytes_per_s": HBM_BYTES_PER_S, "ms": round(floor_bytes / HBM_BYTES_PER_S * 1e3, 4)}}
    be = Backend().setup_context(w, h, depth, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC | backend.FLAG_NO_HISTOGRAMS)
    try:
        be.initialize_memory(sc)
        be.render(0, a.spp)  # warm-up
        be.synchronize()
        be.clear()
        be.synchronize()
        be.kernel_time()
        be.render(0, 1)
        ms, launches = be.kernel_time()
        rec["render_one_iteration_ms"] = round(ms, 3)
        be.render(1, a.spp - 1)
        be.synchronize()

        def planes():
            t = {name: torch.zeros((h, w) if name == "hit_count" else (h, w, 4), dtype=torch.float32, device="cuda") for name in PLANES}
            torch.cuda.synchronize()
            be.render_guides_device(0, a.spp, **{name: x.data_ptr() for name, x in t.items()})
            be.synchronize()
            return t

        home = (sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp)
        color, count = (torch.from_numpy(x).cuda() for x in be.read_image())
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the context's stream is not torch's)
        previous = planes()
        # the point the centre of the image sees (the mean of the hit points around it), to orbit about
        centre = previous["position"][h // 2 - 8:h // 2 + 8, w // 2 - 8:w // 2 + 8, :3].sum((0, 1)) / previous["hit_count"][h // 2 - 8:h // 2 + 8, w // 2 - 8:w // 2 + 8].sum().clamp(min=1)
        moved = scenes.orbit_camera(home, centre.cpu().numpy(), a.degrees)
        be.set_camera(*moved)
        current = planes()
        be.set_stream(stream.cuda_stream)
        ptr = lambda t: {name: x.data_ptr() for name, x in t.items()}  # noqa: E731

        def window(cur):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(a.calls):
                be.reproject_device(out[0].data_ptr(), out[1].data_ptr(), home, ptr(previous), color.data_ptr(), count.data_ptr(), ptr(cur))
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1) / a.calls

        for name, cur in (("identical_camera", previous), ("small_orbit", current)):
            times = [window(cur) for _ in range(a.reps + 1)][1:]  # (the first is the warm-up)
            med = float(np.median(times))
            kept = float((out[1] > 0).float().mean().item())
            rec[name] = {"ms_median": round(med, 4), "ms_all": [round(x, 4) for x in times], "over_floor": round(med / rec["floor"]["ms"], 2),
                         "vs_render_iteration": round(med / ms, 4), "pixels_with_history": round(kept, 4)}
        be.set_stream(None)
    finally:
        be.release()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
