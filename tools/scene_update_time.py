"""Times the ways of getting a moved scene onto the device, on the named scenes, and writes one JSON record per scene.

Every vertex is displaced by a small seeded offset (normals and boxes recomputed); then, each as the median of --reps warm calls:

  update_ms            ptmi_update_triangles (with its ptmi_update_info: checks, upload, device work)
  update_device_ms     ptmi_update_triangles_device from a torch tensor that holds the same displaced records (with its info:
                       there validate_ms is the host checks, the screen kernel and its one word back, upload_ms is 0 on one
                       device); the two forms alternate inside one loop, so that both see the same machine
  host_refit_ms        ptmi_bvh_refit of the caller's tree
  init_refit_tree_ms   ptmi_initialize_memory of (new triangles, that tree) - what the update replaces
  rebuild_ms           ptmi_bvh_create_device + ptmi_initialize_memory - a new tree for the new triangles
  set_camera_ms        ptmi_set_camera, next to synchronize_ms (ptmi_synchronize of an idle context) and init_refit_tree_ms

The first update of a scene also derives the refit's schedule and allocates its scratch: first_update_ms.  After the timed
updates the context renders two iterations and its image is compared, bit for bit, with a context that was initialised with
(new triangles, host-refit tree).

usage: python tools/scene_update_time.py [--scenes tris20k,tris1m,mayalike] [--reps 3] [--out profiles/scene_update_time.json]
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
from opencl_pathtracer_amd import Backend, PtmiError, backend, bvh_create, bvh_refit, scenes, structs as S  # noqa: E402

W, H, DEPTH = 160, 90, 4
f32 = np.float32


def displaced(tris, seed, amplitude):
    rs = np.random.default_rng(seed)
    t = np.frombuffer(bytearray(np.ascontiguousarray(tris).tobytes()), dtype=S.Triangle)
    for name in ("S1", "S2", "S3"):
        v = t[name].copy()
        v[:, :3] += rs.uniform(-amplitude, amplitude, (len(t), 3)).astype(f32)
        t[name] = v
    s1, s2, s3 = t["S1"][:, :3], t["S2"][:, :3], t["S3"][:, :3]
    c = scenes._cross3(s2 - s1, s3 - s1)
    nrm = (c / np.sqrt(scenes._dot3(c, c)).astype(f32)[:, None]).astype(f32)
    flip = scenes._dot3(nrm, t["N"][:, :3]) < 0
    nrm[flip] = -nrm[flip]
    N = t["N"].copy()
    N[:, :3] = nrm
    t["N"] = N
    p = np.stack([t["S1"], t["S2"], t["S3"]], axis=1)
    box = t["AABB"].copy()
    box["pMin"], box["pMax"] = p.min(axis=1), p.max(axis=1)
    box["centroid"] = (box["pMin"] + box["pMax"]) / f32(2)
    t["AABB"] = box
    return t


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def median_of(reps, fn):
    """(median wall ms, all wall ms, the median call's result) after one warm-up call"""
    fn()
    runs = [timed(fn) for _ in range(reps)]
    k = int(np.argsort([r[0] for r in runs])[len(runs) // 2])
    return round(runs[k][0], 3), [round(r[0], 3) for r in runs], runs[k][1]


def alternating(reps, fns):
    """Per function (median wall ms, all wall ms, the median call's result): one warm-up call each, then `reps` rounds in which
    the functions take turns."""
    for fn in fns:
        fn()
    runs = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            runs[k].append(timed(fn))
    out = []
    for r in runs:
        k = int(np.argsort([x[0] for x in r])[len(r) // 2])
        out.append((round(r[k][0], 3), [round(x[0], 3) for x in r], r[k][1]))
    return out


def rounded(info):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in info.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="tris20k,tris1m,mayalike")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()  # (before the library's first device call: torch's runtime does not find the device after it)
    records = []
    for name in a.scenes.split(","):
        sc = bvh_create(scenes.build(name, W, H), device=a.device)
        box = sc.bvh[0]["trianglesAABB"]
        diagonal = float(np.linalg.norm((box["pMax"] - box["pMin"])[:3]))
        amplitude = 1e-4 * diagonal
        tris = displaced(sc.triangulation, 1, amplitude)
        rec = {"scene": name, "triangles": len(tris), "nodes": len(sc.bvh), "max_depth": int(sc.bvhMaxDepth), "image": [W, H],
               "displacement": amplitude, "reps": a.reps}
        be = Backend().setup_context(W, H, DEPTH, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC)
        try:
            rec["init_first_call_ms"] = round(timed(lambda: be.initialize_memory(sc))[0], 3)
            try:
                rec["first_update_ms"], first = timed(lambda: be.update_triangles(tris))
                rec["first_update_ms"] = round(rec["first_update_ms"], 3)
                rec["first_update_info"] = rounded(first)
                d_tris = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(len(tris), 336).view(np.float32)).to(f"cuda:{a.device}")
                torch.cuda.synchronize()
                rec["first_update_device_ms"], first = timed(lambda: be.update_triangles_device(d_tris.data_ptr(), len(tris)))
                rec["first_update_device_ms"] = round(rec["first_update_device_ms"], 3)
                rec["first_update_device_info"] = rounded(first)
                host, dev = alternating(a.reps, [lambda: be.update_triangles(tris), lambda: be.update_triangles_device(d_tris.data_ptr(), len(tris))])
                rec["update_ms"], rec["update_ms_all"], rec["update_info"] = host[0], host[1], rounded(host[2])
                rec["update_device_ms"], rec["update_device_ms_all"], rec["update_device_info"] = dev[0], dev[1], rounded(dev[2])
                rec["update_vs_update_device"] = round(rec["update_ms"] / rec["update_device_ms"], 2)
                # the bytes the screen must read, at the 6.3 TB/s a float4 copy reaches (profiles/): the floor of its validate_ms
                rec["screen_floor_ms"] = round(336 * len(tris) / 6.3e12 * 1e3, 5)
                rec["screen_vs_floor"] = round(rec["update_device_info"]["validate_ms"] / rec["screen_floor_ms"], 1)
                del d_tris
                be.clear()
                be.render(0, 2)
                updated = be.read_image()[0].view(np.uint32).copy()
            except PtmiError as e:  # (a scene an update cannot express: said, not hidden)
                rec["update_refused"] = str(e)
                updated = None
            moved = copy.copy(sc)
            moved.triangulation = tris
            moved.bvh = np.frombuffer(bytearray(sc.bvh.tobytes()), dtype=S.Node)
            rec["host_refit_ms"], rec["host_refit_ms_all"], _ = median_of(a.reps, lambda: bvh_refit(moved))
            rec["init_refit_tree_ms"], rec["init_refit_tree_ms_all"], _ = median_of(a.reps, lambda: be.initialize_memory(moved))
            if updated is not None:
                be.render(0, 2)
                rec["identical"] = bool(np.array_equal(updated, be.read_image()[0].view(np.uint32)))
                assert rec["identical"], name

            def rebuild():
                fresh = copy.copy(sc)
                fresh.triangulation = np.frombuffer(bytearray(tris.tobytes()), dtype=S.Triangle)
                be.initialize_memory(bvh_create(fresh, device=a.device))
            rec["rebuild_ms"], rec["rebuild_ms_all"], _ = median_of(a.reps, rebuild)
            be.initialize_memory(moved)
            be.synchronize()
            camera = (sc.cameraPosition + f32([amplitude, 0, 0, 0]), sc.cameraDirection, sc.cameraRight, sc.cameraUp)
            rec["set_camera_ms"], rec["set_camera_ms_all"], _ = median_of(a.reps, lambda: be.set_camera(*camera))
            rec["synchronize_ms"], _, _ = median_of(a.reps, be.synchronize)
            if "update_ms" in rec:
                rec["update_vs_init_refit_tree"] = round(rec["init_refit_tree_ms"] / rec["update_ms"], 2)
                rec["update_vs_rebuild"] = round(rec["rebuild_ms"] / rec["update_ms"], 2)
            rec["set_camera_vs_init"] = round(rec["init_refit_tree_ms"] / rec["set_camera_ms"], 1)
        finally:
            be.release()
        print(json.dumps(rec), flush=True)
        records.append(rec)
        if a.out:  # (after every scene: a long run that is cut short keeps what it has measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
