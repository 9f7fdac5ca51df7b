"""Cost of the display stage at 1920 x 1080: the device time of the tone-map kernel in each pixel format and of the luminance
histogram kernel, and the wall time of ptmi_read_display_tonemapped beside ptmi_read_display in the same run.

The image is real: --spp iterations of the scene in the context's accumulators (the sum form), and the same sums divided by
their counts in a tensor (the mean form).  A timed window is --calls device-form calls between two HIP events on the context's
stream (one call is tens of microseconds, too short to time alone), after a warm-up, median of --reps windows.  Beside the
times: the bytes a call must move - 20 per pixel read in the sum form, 16 in the mean form, 3 or 4 written - and the time that
takes at the HBM rate a float4 copy reaches on this part, 6.3 TB/s.  The host calls are timed with the wall clock, alternating,
--host-reps times each, into pageable memory and into memory page-locked with ptmi_pin_host_buffer: both move 3 bytes per pixel
over the bus, so their times should agree to within the spread the file records.

usage: python tools/display_rate.py [--scene cornell] [--out profiles/display_rate_1080p.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def spread(times):
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "ms_max": round(float(np.max(times)), 4)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=30)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display_rate_1080p.json"))
    a = ap.parse_args()
    w, h, depth = 1920, 1080, 4
    stride = (3 * w + 3) & ~3
    sc = bvh_create(scenes.build(a.scene, w, h), device=a.device)
    torch.cuda.set_device(a.device)
    stream = torch.cuda.Stream(torch.device("cuda", a.device))
    rec = {"scene": a.scene, "image": [w, h], "spp": a.spp, "reps": a.reps, "calls_per_window": a.calls, "host_reps": a.host_reps,
           "defaults": {k: (v if np.isfinite(v) else "inf") for k, v in backend.DISPLAY_DEFAULTS.items()}, "hbm_bytes_per_s": HBM_BYTES_PER_S}
    be = Backend().setup_context(w, h, depth, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC | backend.FLAG_NO_HISTOGRAMS)
    try:
        be.initialize_memory(sc)
        be.render(0, a.spp)
        be.synchronize()
        color, count = be.read_image()
        with np.errstate(all="ignore"):
            mean = torch.from_numpy(np.where(count[..., None] > 0, color / count[..., None], np.float32(0)).astype(np.float32)).cuda()
        pixels = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        words = torch.zeros(backend.LUMINANCE_WORDS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the context's stream is not torch's)
        be.set_stream(stream.cuda_stream)

        def window(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(a.calls):
                call()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1) / a.calls

        def device_time(call, bytes_per_pixel):
            times = [window(call) for _ in range(a.reps + 1)][1:]  # (the first is the warm-up)
            floor = bytes_per_pixel * w * h / HBM_BYTES_PER_S * 1e3
            med = float(np.median(times))
            return {"ms_median": round(med, 4), "ms_all": [round(x, 4) for x in times], "bytes_per_pixel": bytes_per_pixel,
                    "floor_ms": round(floor, 4), "over_floor": round(med / floor, 2)}

        rec["device_ms"] = {
            "tonemap_bgr24_sums": device_time(lambda: be.display_device(pixels.data_ptr()), 23),
            "tonemap_rgba32_sums": device_time(lambda: be.display_device(pixels.data_ptr(), rgba=True), 24),
            "tonemap_bgr24_means": device_time(lambda: be.display_device(pixels.data_ptr(), mean.data_ptr()), 19),
            "tonemap_rgba32_means": device_time(lambda: be.display_device(pixels.data_ptr(), mean.data_ptr(), rgba=True), 20),
            "histogram_sums": device_time(lambda: be.luminance_histogram_device(words.data_ptr()), 20),
            "histogram_means": device_time(lambda: be.luminance_histogram_device(words.data_ptr(), mean.data_ptr()), 16),
        }
        be.set_stream(None)
        be.synchronize()

        # the host calls, alternating, the wall clock around each
        rows = np.empty((h, stride), np.uint8)
        params = be.display_params()
        calls = {"read_display": lambda: be._check(be._lib.ptmi_read_display(be._ctx, rows.ctypes.data, stride)),
                 "read_display_tonemapped": lambda: be._check(be._lib.ptmi_read_display_tonemapped(be._ctx, C.byref(params), rows.ctypes.data)),
                 "luminance_histogram": be.luminance_histogram}
        rec["host_wall_ms"] = {}
        for memory in ("pageable", "page_locked"):
            if memory == "page_locked":
                be.pin_host_buffer(rows)
            times = {name: [] for name in calls}
            for rep in range(a.host_reps + 2):
                for name, call in calls.items():
                    t0 = time.perf_counter()
                    call()
                    if rep >= 2:  # (two warm-up rounds)
                        times[name].append((time.perf_counter() - t0) * 1e3)
            rec["host_wall_ms"][memory] = {name: spread(t) for name, t in times.items()}
            r = rec["host_wall_ms"][memory]
            r["tonemapped_over_read_display"] = round(r["read_display_tonemapped"]["ms_median"] / r["read_display"]["ms_median"], 3)
        be.unpin_host_buffer(rows)
    finally:
        be.release()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
