"""Times ptmi_bvh_create (host) against ptmi_bvh_create_device on the named scenes and writes one JSON record per scene.

Wall time is from the caller's arrays in to the arrays out: one warm-up call first (its time is reported separately as
the first-call cost, HIP runtime and code-object load included), then the median of --reps calls.  The device record
carries ptmi_bvh_build_info: the kernels' share (HIP events), upload, download, reordering of the triangles, peak
workspace.  Both trees are compared byte for byte on every call.

usage: python tools/bvh_build_time.py [--scenes tris20k,tris1m,mayalike,tris4m] [--reps 3] [--out FILE]
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
from opencl_pathtracer_amd import backend, scenes, structs as S  # noqa: E402


def call(lib, tris, device):
    t = np.frombuffer(bytearray(tris.tobytes()), dtype=S.Triangle)
    n = len(t)
    nodes = np.zeros(2 * n - 1, dtype=S.Node)
    size, depth = C.c_uint32(0), C.c_uint32(0)
    info = backend.BvhBuildInfo()
    args = (t.ctypes.data_as(C.c_void_p), n, nodes.ctypes.data_as(C.c_void_p), C.byref(size), C.byref(depth))
    t0 = time.perf_counter()
    rc = lib.ptmi_bvh_create(*args) if device is None else lib.ptmi_bvh_create_device(device, *args, C.byref(info))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.ptmi_last_error(None).decode()
    return wall, info, nodes[:size.value].tobytes(), t.tobytes(), depth.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="tris20k,tris1m,mayalike,tris4m")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = backend.load_library()
    records = []
    for name in a.scenes.split(","):
        tris = np.ascontiguousarray(scenes.build(name, 160, 90).triangulation)
        host_ms, _, h_nodes, h_tris, h_depth = call(lib, tris, None)
        first_ms, first_info, _, _, _ = call(lib, tris, a.device)
        walls, infos = [], []
        for _ in range(a.reps):
            wall, info, nodes, t, depth = call(lib, tris, a.device)
            assert info.built_on_device == 1 and nodes == h_nodes and t == h_tris and depth == h_depth, name
            walls.append(wall)
            infos.append(info.as_dict())
        k = int(np.argsort(walls)[len(walls) // 2])
        rec = {"scene": name, "triangles": len(tris), "nodes": len(h_nodes) // S.Node.itemsize, "max_depth": h_depth,
               "host_ms": round(host_ms, 2), "device_first_call_ms": round(first_ms, 2), "device_wall_ms": round(walls[k], 2),
               "device_wall_ms_all": [round(w, 2) for w in walls], "speedup": round(host_ms / walls[k], 2),
               "device_info": {key: (round(v, 3) if isinstance(v, float) else v) for key, v in infos[k].items()},
               "identical": True}
        print(json.dumps(rec), flush=True)
        records.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
