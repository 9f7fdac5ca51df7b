#!/usr/bin/env python3
"""A mesh deformed on the GPU from its vertex buffer: the caller moves vertices, the library derives the triangle records.

    python examples/deform_vertices.py --scene tris20k --width 512 --height 512 --frames 12 --spp 4
    python examples/deform_vertices.py --out wave          # -> wave_00.bmp, wave_01.bmp, ...

The scene becomes an indexed mesh once (scenes.mesh_from_triangulation: a (V, 3) vertex tensor, an (F, 3) index tensor) and its
topology is bound once (ptmi_bind_mesh).  Every frame the travelling wave of examples/deform.py displaces the (V, 3) rest
positions in torch, smooth vertex normals are summed from the face normals with index_add_, and ptmi_update_vertices_device does
what deform.py does by hand and more: the geometric normal from the face's winding (so a triangle that turns over is shaded on
the side it now shows), the shading normals N1..N3 from the new vertex normals, the bounding box, the corners in the importer's
lexicographic order.  About 12 bytes per vertex are read instead of 336 per triangle being written by the caller.  Then
ptmi_clear, --spp iterations, and the frame comes back tone-mapped and quantised (ptmi_read_display_tonemapped).
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, structs as S  # noqa: E402


def deformed(rest, phase, amplitude, wavelength, torch):
    """`rest` (V, 3) with every vertex lifted along y by a wave that travels along x"""
    moved = rest.clone()
    moved[:, 1] = rest[:, 1] + amplitude * torch.sin(rest[:, 0] * (2 * math.pi / wavelength) - phase)
    return moved


def smooth_normals(positions, faces, torch):
    """(V, 3): per vertex the sum of the (area-weighted) normals of the faces around it; the library normalises them, and
    falls back to the face's own normal where a sum is shorter than one half"""
    p0, p1, p2 = positions[faces[:, 0]], positions[faces[:, 1]], positions[faces[:, 2]]
    face = torch.linalg.cross(p1 - p0, p2 - p0)
    face = face / torch.linalg.vector_norm(face, dim=1, keepdim=True).clamp_min(1e-30)
    normals = torch.zeros_like(positions)
    for k in range(3):
        normals.index_add_(0, faces[:, k], face)
    return normals.contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="tris20k", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--spp", type=int, default=4, help="iterations rendered per frame")
    ap.add_argument("--amplitude", type=float, default=0.01, help="the wave's height, in scene diagonals")
    ap.add_argument("--wavelength", type=float, default=0.5, help="in scene diagonals")
    ap.add_argument("--out", default="deform_vertices", help="prefix of the BMPs")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # (before the library's first device call: torch's runtime does not find the device after it)

    w, h = args.width, args.height
    scene = pt.bvh_create(pt.scenes.build(args.scene, w, h))
    box = scene.bvh[0]["trianglesAABB"]
    diagonal = float(np.linalg.norm((box["pMax"] - box["pMin"])[:3]))
    mesh = pt.scenes.mesh_from_triangulation(scene.triangulation)
    device = f"cuda:{args.device}"
    rest = torch.from_numpy(mesh.positions).to(device)                    # (V, 3) float32: stride 12
    faces = torch.from_numpy(mesh.indices.astype(np.int64)).to(device)    # (F, 3)
    be = pt.Backend().setup_context(w, h, 4, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    be.bind_mesh(mesh)  # the topology goes up once
    spent, levels = [], 0
    for frame in range(args.frames):
        moved = deformed(rest, 2 * math.pi * frame / max(args.frames, 1), args.amplitude * diagonal, args.wavelength * diagonal, torch)
        normals = smooth_normals(moved, faces, torch)
        torch.cuda.synchronize(args.device)  # (the context reads the tensors on its own stream)
        info = be.update_vertices_device(len(mesh.positions), moved.data_ptr(), normals.data_ptr())
        spent.append(info["total_ms"])
        levels = info["levels"]
        be.clear()
        be.render(0, max(args.spp, 1))
        output.save_bmp_rows(f"{args.out}_{frame:02d}.bmp", be.display(), w, h)
    be.release()
    print(f"{args.out}_NN.bmp: {args.frames} frames of {len(mesh.indices)} triangles on {len(mesh.positions)} vertices, {w}x{h}, "
          f"{args.spp} iterations each" + (f"; an update took {np.median(spent):.3f} ms (median), {levels} level passes" if spent else ""))


if __name__ == "__main__":
    main()
