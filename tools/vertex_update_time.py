"""Times ptmi_update_vertices and ptmi_update_vertices_device next to the record forms they end in, on the named scenes, and
writes one JSON record per scene.

The scene becomes an indexed mesh (scenes.mesh_from_triangulation) whose topology is bound once; every VERTEX is displaced by a
seeded offset of at most 1e-4 of the scene's diagonal per axis.  The 336-byte records of the same motion (ptmi_assemble_triangles,
on the host) feed ptmi_update_triangles and ptmi_update_triangles_device: the parent's calls, the yardstick.  The four calls take
turns inside one loop, so that all see the same machine; each is reported as the median and the min..max of --reps warm calls,
with the ptmi_update_info of its median call.

  assemble_ms          what the vertex device form adds on the device, as a DIFFERENCE of two medians: its device_ms (the assemble
                       kernel's HIP events plus the update's) less the record device form's device_ms
  assemble_floor_ms    the bytes the assemble kernel must move - 336 n written, the topology (72 bytes per triangle) and every
                       vertex's position and normal once (24 bytes per vertex; a vertex shared by several corners is gathered
                       again from cache) - at the 6.3 TB/s a float4 copy reaches
  host_saving_ms       ptmi_update_triangles less ptmi_update_vertices: about that call's validate_ms + upload_ms less the vertex copy

After the timed updates the context renders two iterations and its image is compared, bit for bit, with a context that was
initialised with (the assembled records, the host-refit tree).

usage: python tools/vertex_update_time.py [--scenes tris20k,tris1m,mayalike] [--reps 3] [--out profiles/vertex_update_time.json]
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def alternating(reps, fns):
    """Per function (median wall ms, [min, max], the median call's result): one warm-up call each, then `reps` rounds in which
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
        out.append((round(r[k][0], 3), [round(min(x[0] for x in r), 3), round(max(x[0] for x in r), 3)], r[k][1]))
    return out


def rounded(info):
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in info.items()}


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
        mesh = scenes.mesh_from_triangulation(sc.triangulation)
        n, nv = len(mesh.indices), len(mesh.positions)
        rs = np.random.default_rng(1)
        positions = (mesh.positions + rs.uniform(-amplitude, amplitude, mesh.positions.shape).astype(f32)).astype(f32)
        normals = mesh.normals
        tris = backend.assemble_triangles(mesh, positions=positions)  # the same motion as 336-byte records
        rec = {"scene": name, "triangles": n, "vertices": nv, "nodes": len(sc.bvh), "max_depth": int(sc.bvhMaxDepth), "image": [W, H],
               "displacement": amplitude, "reps": a.reps}
        be = Backend().setup_context(W, H, DEPTH, sc.lightsSize, S.JITTERED, device=a.device, flags=backend.FLAG_DEFAULT_ARITHMETIC)
        try:
            be.initialize_memory(sc)
            try:
                rec["bind_ms"] = round(timed(lambda: be.bind_mesh(mesh))[0], 3)
                dev = f"cuda:{a.device}"
                d_tris = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(n, 336).view(np.float32)).to(dev)
                d_pos, d_nrm = torch.from_numpy(positions).to(dev), torch.from_numpy(np.ascontiguousarray(normals)).to(dev)
                torch.cuda.synchronize()
                names = ["update_triangles", "update_triangles_device", "update_vertices", "update_vertices_device"]
                got = alternating(a.reps, [lambda: be.update_triangles(tris),
                                           lambda: be.update_triangles_device(d_tris.data_ptr(), n),
                                           lambda: be.update_vertices(positions, normals),
                                           lambda: be.update_vertices_device(nv, d_pos.data_ptr(), d_nrm.data_ptr())])
                for key, (ms, span, info) in zip(names, got):
                    rec[key + "_ms"], rec[key + "_ms_min_max"], rec[key + "_info"] = ms, span, rounded(info)
                rec["assemble_ms"] = round(rec["update_vertices_device_info"]["device_ms"] - rec["update_triangles_device_info"]["device_ms"], 4)
                rec["assemble_bytes"] = 336 * n + 72 * n + 24 * nv  # (the mesh carries uvp and uvn, and normals)
                rec["assemble_floor_ms"] = round(rec["assemble_bytes"] / 6.3e12 * 1e3, 5)
                rec["assemble_vs_floor"] = round(rec["assemble_ms"] / rec["assemble_floor_ms"], 1)
                rec["vertices_device_less_triangles_device_ms"] = round(rec["update_vertices_device_ms"] - rec["update_triangles_device_ms"], 3)
                rec["host_saving_ms"] = round(rec["update_triangles_ms"] - rec["update_vertices_ms"], 3)
                rec["update_triangles_vs_update_vertices"] = round(rec["update_triangles_ms"] / rec["update_vertices_ms"], 2)
                del d_tris
                be.clear()
                be.render(0, 2)
                updated = be.read_image()[0].view(np.uint32).copy()
            except PtmiError as e:  # (a scene an update cannot express: said, not hidden)
                rec["update_refused"] = str(e)
                updated = None
            if updated is not None:
                moved = copy.copy(sc)
                moved.triangulation = tris
                moved.bvh = np.frombuffer(bytearray(sc.bvh.tobytes()), dtype=S.Node)
                bvh_refit(moved)
                be.initialize_memory(moved)
                be.render(0, 2)
                rec["identical"] = bool(np.array_equal(updated, be.read_image()[0].view(np.uint32)))
                assert rec["identical"], name
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
