"""Cost of ptmi_denoise_device at 1920 x 1080, next to one ptmi_render iteration of the same scene in the same run, and the A/B
of the two forms of the a-trous kernel at steps 1 and 2.

The inputs are real: --spp iterations of the scene in the context's accumulators and its guide planes over the same iterations,
in torch tensors.  A timed window is --calls denoise calls between two HIP events on the context's stream (one call is a
fraction of a millisecond, too short to time alone; 200 of five passes are 0.12 s), after a warm-up, median of --reps windows.
passes = 0 .. 5 are timed, so the pass at step 1 << k costs t(k + 1) - t(k); t(0) is the prepass writing the image.  Beside the times: the bytes a pass must
move at the least with the library's layout - it reads e, g1, g2 (16 + 16 + 8 bytes) and writes e (16) per pixel - and the time
that takes at the HBM rate a float4 copy reaches on this part, 6.3 TB/s.

The A/B alternates, window by window, the form that stages a 32 x 8 tile and its halo in LDS (the default) with the form that
reads every tap from memory (PTMI_DENOISE_UNTILED) - the same binary, a flag of the call - at passes = 1 and 2.

usage: python tools/denoise_rate.py [--scene tris1m] [--out profiles/denoise_rate_1080p.json] [--ab profiles/denoise_tile_ab.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402

READ_BYTES, WRITE_BYTES, HBM_BYTES_PER_S = 40, 16, 6.3e12
GUIDE_NAMES = ("albedo", "normal", "position", "hit_count")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_rate_1080p.json"))
    ap.add_argument("--ab", default=os.path.join(ROOT, "profiles", "denoise_tile_ab.txt"))
    a = ap.parse_args()
    w, h, depth = 1920, 1080, 10
    sc = bvh_create(scenes.build(a.scene, w, h), device=a.device)
    torch.cuda.set_device(a.device)
    stream = torch.cuda.Stream(torch.device("cuda", a.device))
    floor_bytes = (READ_BYTES + WRITE_BYTES) * w * h
    rec = {"scene": a.scene, "image": [w, h], "spp": a.spp, "reps": a.reps, "calls_per_window": a.calls, "arithmetic": "default",
           "defaults": backend.DENOISE_DEFAULTS, "pass_floor": {"read_bytes_per_pixel": READ_BYTES, "write_bytes_per_pixel": WRITE_BYTES,
                                                               "bytes": floor_bytes, "hbm_bytes_per_s": HBM_BYTES_PER_S,
                                                               "ms": round(floor_bytes / HBM_BYTES_PER_S * 1e3, 4)}}
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

        be.set_stream(stream.cuda_stream)
        guides = {name: torch.zeros((h, w) if name == "hit_count" else (h, w, 4), dtype=torch.float32, device="cuda") for name in GUIDE_NAMES}
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        pointers = {name: t.data_ptr() for name, t in guides.items()}
        be.render_guides_device(0, a.spp, **pointers)
        be.synchronize()

        def window(passes, untiled):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(a.calls):
                be.denoise_device(out.data_ptr(), pointers, passes=passes, guide_iterations=a.spp, untiled=untiled)
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1) / a.calls

        def timed(passes, untiled):
            times = [window(passes, untiled) for _ in range(a.reps + 1)]  # (the first is the warm-up)
            return times[1:]

        # the same words from both forms, at the size that is timed
        be.denoise_device(out.data_ptr(), pointers, passes=5, guide_iterations=a.spp, untiled=False)
        be.synchronize()
        tiled_words = out.clone()
        be.denoise_device(out.data_ptr(), pointers, passes=5, guide_iterations=a.spp, untiled=True)
        be.synchronize()
        same = bool(((tiled_words.view(torch.int32) == out.view(torch.int32)) | (tiled_words.isnan() & out.isnan())).all().item())
        rec["forms_agree_word_for_word"] = same

        calls = {}
        for passes in range(6):
            t = timed(passes, False)
            calls[passes] = float(np.median(t))
            rec.setdefault("call_ms", {})[str(passes)] = {"ms_median": round(calls[passes], 4), "ms_all": [round(x, 4) for x in t]}
        rec["prepass_ms"] = round(calls[0], 4)
        rec["pass_ms_at_step"] = {str(1 << k): round(calls[k + 1] - calls[k], 4) for k in range(5)}
        rec["pass_over_floor"] = {s: round(v / rec["pass_floor"]["ms"], 2) for s, v in rec["pass_ms_at_step"].items()}
        rec["whole_call_ms"] = round(calls[5], 4)
        rec["whole_call_vs_render_iteration"] = round(calls[5] / ms, 4)

        # A/B, alternating window by window
        ab = {(p, u): [] for p in (0, 1, 2) for u in (False, True)}
        for key in ab:
            window(*key)  # warm-up
        for _ in range(a.reps):
            for key in ab:
                ab[key].append(window(*key))
        med = {key: float(np.median(v)) for key, v in ab.items()}
        lines = [f"denoise a-trous kernel, {w} x {h}, {a.scene} at {a.spp} spp: LDS-tiled (32 x 8 tile + halo) against direct reads, same binary,",
                 f"windows of {a.calls} calls alternated, median of {a.reps}; ms per call.  the two forms agree word for word: {same}", ""]
        for p in (0, 1, 2):
            lines.append(f"passes={p}  tiled {med[p, False]:.4f}  [{' '.join(f'{x:.4f}' for x in ab[p, False])}]   "
                         f"direct {med[p, True]:.4f}  [{' '.join(f'{x:.4f}' for x in ab[p, True])}]")
        lines.append("")
        for k, step in ((0, 1), (1, 2)):
            tiled, direct = med[k + 1, False] - med[k, False], med[k + 1, True] - med[k, True]
            lines.append(f"step {step}: tiled {tiled:.4f} ms, direct {direct:.4f} ms, tiled / direct = {tiled / direct:.3f}")
            rec.setdefault("tile_ab", {})[str(step)] = {"tiled_ms": round(tiled, 4), "direct_ms": round(direct, 4), "ratio": round(tiled / direct, 3)}
        be.set_stream(None)
    finally:
        be.release()
    print(json.dumps(rec), flush=True)
    print("\n".join(lines), flush=True)
    for path, text in ((a.out, json.dumps(rec, indent=1) + "\n"), (a.ab, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
