"""Times the in-place edits of a loaded scene's materials, lights and sky against the upload they replace, on the named scene
given one 2x2 texture, and prints one JSON record.

Each as the median of --reps warm calls (wall clock around the call, which is synchronous):

  materials_ms           ptmi_update_materials, a new colour: no screen (with its ptmi_material_update_info)
  materials_screen_ms    ptmi_update_materials, the plain material turned textured: the screen kernel reads the DShade records
                         of every triangle on the device and one word comes back.  The way back (textured -> plain, no screen)
                         runs between two such calls and is timed as materials_back_ms
  lights_ms              ptmi_update_lights, the light moved
  sky_ms                 ptmi_set_sky, another rotation
  initialize_memory_ms   ptmi_initialize_memory of the same scene on the same context: what each of these edits cost before

After the timed calls the context renders two iterations with the textured material and its image is compared, bit for bit, with
a context that was initialised with the edited scene.

usage: python tools/material_update_time.py [--scene tris1m] [--reps 5] [--out profiles/material_update_time.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from opencl_pathtracer_amd import Backend, backend, bvh_create, scenes, structs as S  # noqa: E402

W, H, DEPTH = 160, 90, 4
f32 = np.float32


def raw_copy(a):
    return np.frombuffer(bytearray(np.ascontiguousarray(a).tobytes()), dtype=a.dtype)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def median_of(reps, fn, between=None):
    """(median wall ms, all wall ms, the median call's result) after one warm-up call; `between` runs, untimed, after every call"""
    runs = []
    for k in range(reps + 1):
        run = timed(fn)
        if k:
            runs.append(run)
        if between:
            between()
    k = int(np.argsort([r[0] for r in runs])[len(runs) // 2])
    return round(runs[k][0], 3), [round(r[0], 3) for r in runs], runs[k][1]


def rounded(info):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in info.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sc = bvh_create(scenes.build(a.scene, W, H), device=a.device)
    texels = np.concatenate([np.ascontiguousarray(sc.texturesData).reshape(-1, 4),
                             np.array([[230, 40, 40, 0], [40, 230, 40, 0], [40, 40, 230, 0], [230, 230, 40, 0]], np.uint8)])
    sc.texturesData = texels
    sc.textures = np.array(list(sc.textures) + [(2, 2, len(texels) - 4)], dtype=S.Texture)
    plain = raw_copy(sc.materiaux[:1])
    recoloured = raw_copy(plain)
    recoloured["simpleColor"][0] = f32([0.8, 0.3, 0.2, 0])
    textured = raw_copy(plain)
    textured["isSimpleColor"], textured["textureId"] = 0, len(sc.textures) - 1
    lights = raw_copy(sc.lights)
    lights["position"][0, :3] += f32([0.5, -0.25, 0.125])
    sky = sc.sky.copy()
    sky["cosRotationAngle"], sky["sinRotationAngle"] = f32(np.cos(0.5)), f32(np.sin(0.5))
    rec = {"scene": a.scene, "triangles": len(sc.triangulation), "materials": len(sc.materiaux), "lights": sc.lightsSize, "image": [W, H],
           "reps": a.reps}
    be = Backend().setup_context(W, H, DEPTH, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC)
    try:
        rec["init_first_call_ms"] = round(timed(lambda: be.initialize_memory(sc))[0], 3)
        rec["materials_ms"], rec["materials_ms_all"], info = median_of(a.reps, lambda: be.update_materials(0, recoloured))
        rec["materials_info"] = rounded(info)
        back = []
        rec["materials_screen_ms"], rec["materials_screen_ms_all"], info = median_of(
            a.reps, lambda: be.update_materials(0, textured), between=lambda: back.append(timed(lambda: be.update_materials(0, plain))[0]))
        rec["materials_screen_info"] = rounded(info)
        assert info["screened_triangles"] == len(sc.triangulation) and (info["plain_before"], info["plain_after"]) == (1, 0), info
        rec["materials_back_ms"] = round(float(np.median(back[1:])), 3)
        # the bytes the screen must read where every record's materials are textured (64 of a record's 112), at the 6.3 TB/s a
        # float4 copy reaches (profiles/): the floor of the kernel inside validate_ms
        rec["screen_floor_ms"] = round(64 * len(sc.triangulation) / 6.3e12 * 1e3, 5)
        rec["lights_ms"], rec["lights_ms_all"], _ = median_of(a.reps, lambda: be.update_lights(lights))
        rec["sky_ms"], rec["sky_ms_all"], _ = median_of(a.reps, lambda: be.set_sky(sky))
        rec["synchronize_ms"], _, _ = median_of(a.reps, be.synchronize)
        be.update_materials(0, textured)
        be.clear()
        be.render(0, 2)
        edited_image = be.read_image()[0].view(np.uint32).copy()
        edited = copy.copy(sc)
        edited.materiaux, edited.lights, edited.sky = textured, lights, sky
        rec["initialize_memory_ms"], rec["initialize_memory_ms_all"], _ = median_of(a.reps, lambda: be.initialize_memory(edited))
        be.render(0, 2)
        rec["identical"] = bool(np.array_equal(edited_image, be.read_image()[0].view(np.uint32)))
        assert rec["identical"]
        for key in ("materials_ms", "materials_screen_ms", "lights_ms", "sky_ms"):
            rec["init_vs_" + key[:-3]] = round(rec["initialize_memory_ms"] / rec[key], 1)
    finally:
        be.release()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
