#!/usr/bin/env python3
"""Denoiser inputs and a pick buffer: what the camera sees per pixel, without rendering it.

    python examples/guides.py --scene cornell --width 512 --height 512 --iterations 8 --pixel 100 380
    python examples/guides.py --scene matmix --out matmix          # -> matmix_albedo.bmp, matmix_normal.bmp

Loads a scene and asks for its first-hit guide buffers (ptmi_render_guides) over --iterations samples per pixel, the very
primary rays a render of those iterations traces.  Writes the mean albedo (the sum over the iterations - a surface's colour on a
hit, the sky's on a miss - divided by their number) and the mean shading normal of the hits mapped from [-1, 1] to [0, 1] as
BMPs, and prints what lies under --pixel from the id plane: triangle, material, side, coverage.  No image is rendered.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, structs as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--pixel", type=int, nargs=2, default=None, metavar=("X", "Y"), help="the pixel to pick (default: the centre)")
    ap.add_argument("--out", default="guides", help="prefix of the BMPs")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    w, h, n = args.width, args.height, max(args.iterations, 1)
    scene = pt.bvh_create(pt.scenes.build(args.scene, w, h))
    be = pt.Backend().setup_context(w, h, 4, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    g = be.render_guides(0, n)
    be.release()

    samples = np.full((h, w), n, np.float32)
    output.save_bmp(args.out + "_albedo.bmp", g["albedo"], samples)
    hits = g["hit_count"]
    normal = np.where(hits[..., None] > 0, g["normal"] * np.float32(0.5) + hits[..., None] * np.float32(0.5), np.float32(0))  # sum of (Ns + 1) / 2
    output.save_bmp(args.out + "_normal.bmp", normal, np.maximum(hits, 1))
    print(f"{args.out}_albedo.bmp, {args.out}_normal.bmp: {w}x{h}, {n} samples per pixel, {100 * float((hits > 0).mean()):.1f} % of the pixels covered")

    x, y = tuple(args.pixel) if args.pixel else (w // 2, h // 2)
    triangle, material, front, _ = (int(v) for v in g["ids"][y, x])
    if triangle == S.RAY_MISS:
        print(f"pixel ({x}, {y}): nothing under the first sample; {int(hits[y, x])} of {n} samples hit")
    else:
        p = g["position"][y, x, :3] / max(hits[y, x], 1)
        print(f"pixel ({x}, {y}): triangle {triangle} ({'front' if front else 'back'}), material {material} "
              f"(type {int(scene.materiaux[material]['type'])}), {int(hits[y, x])} of {n} samples hit, mean position {p.tolist()}")


if __name__ == "__main__":
    main()
