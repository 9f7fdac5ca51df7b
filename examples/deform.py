#!/usr/bin/env python3
"""A mesh deformed on the GPU and rendered where it is: no triangle record crosses the bus after the first frame.

    python examples/deform.py --scene tris20k --width 512 --height 512 --frames 12 --spp 4
    python examples/deform.py --out wave          # -> wave_00.bmp, wave_01.bmp, ...

The scene's 336-byte triangle records go up once, as a float32 (n, 84) torch tensor.  Every frame a travelling wave displaces the
vertices of that rest pose in torch; the geometric normal and the bounding box of every triangle follow in torch (what
ptmi_update_triangles asks of its caller: N on the side it was, AABB = the box of the three vertices).  Then
ptmi_update_triangles_device checks the records on the device, rewrites the scene's records from them and refits the tree;
ptmi_clear, --spp iterations, and the frame comes back tone-mapped and quantised (ptmi_read_display_tonemapped): 3 bytes per
pixel.  A refit keeps the tree's topology: a wave that is large against the triangles makes the boxes overlap and the render
slower, never wrong.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, structs as S  # noqa: E402


def column(*path):
    """The float32 column at which the field path[0].path[1]... of structs.Triangle starts"""
    dtype, at = S.Triangle, 0
    for name in path:
        dtype, offset = dtype.fields[name][:2]
        at += offset
    assert at % 4 == 0
    return at // 4


S1, S2, S3, N = column("S1"), column("S2"), column("S3"), column("N")
P_MIN, P_MAX, CENTROID = column("AABB", "pMin"), column("AABB", "pMax"), column("AABB", "centroid")


def deformed(rest, phase, amplitude, wavelength, torch):
    """`rest` with every vertex lifted along y by a wave that travels along x; N and AABB follow (scene_update_cases.follow_vertices)"""
    t = rest.clone()
    for c in (S1, S2, S3):
        t[:, c + 1] = rest[:, c + 1] + amplitude * torch.sin(rest[:, c] * (2 * math.pi / wavelength) - phase)
    s1, s2, s3 = t[:, S1:S1 + 3], t[:, S2:S2 + 3], t[:, S3:S3 + 3]
    normal = torch.linalg.cross(s2 - s1, s3 - s1)
    normal = normal / torch.linalg.vector_norm(normal, dim=1, keepdim=True)
    flip = (normal * rest[:, N:N + 3]).sum(dim=1, keepdim=True) < 0
    t[:, N:N + 3] = torch.where(flip, -normal, normal)
    corners = torch.stack([t[:, S1:S1 + 4], t[:, S2:S2 + 4], t[:, S3:S3 + 4]])
    t[:, P_MIN:P_MIN + 4] = corners.amin(dim=0)
    t[:, P_MAX:P_MAX + 4] = corners.amax(dim=0)
    t[:, CENTROID:CENTROID + 4] = (t[:, P_MIN:P_MIN + 4] + t[:, P_MAX:P_MAX + 4]) / 2
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="tris20k", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--spp", type=int, default=4, help="iterations rendered per frame")
    ap.add_argument("--amplitude", type=float, default=0.01, help="the wave's height, in scene diagonals")
    ap.add_argument("--wavelength", type=float, default=0.5, help="in scene diagonals")
    ap.add_argument("--out", default="deform", help="prefix of the BMPs")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # (before the library's first device call: torch's runtime does not find the device after it)

    w, h = args.width, args.height
    scene = pt.bvh_create(pt.scenes.build(args.scene, w, h))
    box = scene.bvh[0]["trianglesAABB"]
    diagonal = float(np.linalg.norm((box["pMax"] - box["pMin"])[:3]))
    n = len(scene.triangulation)
    records = np.ascontiguousarray(scene.triangulation).view(np.uint8).reshape(n, S.Triangle.itemsize).view(np.float32)
    rest = torch.from_numpy(records).to(f"cuda:{args.device}")  # the only time the records cross the bus
    be = pt.Backend().setup_context(w, h, 4, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    spent = []
    for frame in range(args.frames):
        moved = deformed(rest, 2 * math.pi * frame / max(args.frames, 1), args.amplitude * diagonal, args.wavelength * diagonal, torch)
        torch.cuda.synchronize(args.device)  # (the context reads the tensor on its own stream)
        info = be.update_triangles_device(moved.data_ptr(), n)
        spent.append(info["total_ms"])
        be.clear()
        be.render(0, max(args.spp, 1))
        output.save_bmp_rows(f"{args.out}_{frame:02d}.bmp", be.display(), w, h)
    be.release()
    print(f"{args.out}_NN.bmp: {args.frames} frames of {n} triangles, {w}x{h}, {args.spp} iterations each; "
          f"an update took {np.median(spent):.3f} ms (median), {info['levels']} level passes")


if __name__ == "__main__":
    main()
