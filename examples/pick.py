#!/usr/bin/env python3
"""Viewport picking: which triangle lies under a pixel of the scene a context holds.

    python examples/pick.py --scene cornell --width 512 --height 512 --pixel 100 380
    python examples/pick.py --scene matmix --pixel 10 10 --any     # first accepted triangle instead of the closest

Loads a scene, then asks the integrator's own tree (ptmi_query_rays) for the camera ray through the centre of the image and
the one through --pixel: triangle id, the material on the side that was hit, and the distance.  No image is rendered.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import structs as S  # noqa: E402


def camera_ray(scene, w, h, x, y):
    """The ray the kernel shoots through the centre of pixel (x, y): direction + right * sx + up * sy, sx, sy in [-0.5, 0.5]
    (FullKernel.cl:1213); the origin is the camera position, w included (the plane equation is a 4-wide dot product)."""
    sx, sy = np.float32((x + 0.5) / w - 0.5), np.float32((y + 0.5) / h - 0.5)
    d = np.asarray(scene.cameraDirection, np.float32) + np.asarray(scene.cameraRight, np.float32) * sx + np.asarray(scene.cameraUp, np.float32) * sy
    return np.asarray(scene.cameraPosition, np.float32), d.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--pixel", type=int, nargs=2, default=None, metavar=("X", "Y"), help="a second pixel to pick (default: a quarter in)")
    ap.add_argument("--any", action="store_true", help="PTMI_QUERY_ANY: stop at the first accepted triangle (an occlusion probe)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    w, h = args.width, args.height
    scene = pt.bvh_create(pt.scenes.build(args.scene, w, h))
    be = pt.Backend().setup_context(w, h, 4, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    pixels = [(w // 2, h // 2), tuple(args.pixel) if args.pixel else (w // 4, h // 4)]
    rays = [camera_ray(scene, w, h, x, y) for x, y in pixels]
    hits = be.query_rays(np.stack([o for o, _ in rays]), np.stack([d for _, d in rays]), any_hit=args.any)
    be.release()
    for (x, y), hit in zip(pixels, hits):
        if hit["triangle_id"] == S.RAY_MISS:
            print(f"pixel ({x}, {y}): nothing ({hit['box_tests']} box tests, {hit['triangle_tests']} triangle tests)")
            continue
        tri = scene.triangulation[hit["triangle_id"]]
        material = int(tri["materialWithPositiveNormalIndex"] if hit["front"] else tri["materialWithNegativeNormalIndex"])
        print(f"pixel ({x}, {y}): triangle {hit['triangle_id']} ({'front' if hit['front'] else 'back'}), material {material} "
              f"(type {int(scene.materiaux[material]['type'])}), distance {np.sqrt(hit['squared_distance']):.4f} at "
              f"{hit['point'][:3].tolist()}  [{hit['box_tests']} box tests, {hit['triangle_tests']} triangle tests]")


if __name__ == "__main__":
    main()
