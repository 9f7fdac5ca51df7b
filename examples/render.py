#!/usr/bin/env python3
"""Render one of the built-in scenes (or a Wavefront OBJ) on the MI355X and save what the reference's viewer would
save: a 24-bit BMP of min(255 * sum / n, 255) (Alone/PathTracer_Dialog.cpp:161-185).

    python examples/render.py --scene cornell --width 512 --height 512 --spp 64 --depth 4 -o cornell.bmp
    python examples/render.py --obj mesh.obj --spp 32 -o mesh.bmp
    python examples/render.py --scene matmix --orbit 24 -o turn.bmp      # turn_000.bmp .. turn_023.bmp around the scene

The pixels are quantised on the device (ptmi_read_display): 3 bytes per pixel cross the bus.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd.output import save_bmp_rows as save_bmp  # noqa: E402  (SaveBMP, Alone/PathTracer_bitmap.cpp:146-205)


def orbit_camera(scene, angle):
    """The scene's camera turned by `angle` about the axis through the middle of the scene's bounding box along the camera's up."""
    box = scene.bvh[0]["trianglesAABB"]
    centre = (np.asarray(box["pMin"], np.float64) + np.asarray(box["pMax"], np.float64))[:3] / 2
    up = np.asarray(scene.cameraUp, np.float64)[:3]
    k = up / np.linalg.norm(up)
    c, s = np.cos(angle), np.sin(angle)

    def turn(v):  # Rodrigues
        v = np.asarray(v, np.float64)[:3]
        return v * c + np.cross(k, v) * s + k * np.dot(k, v) * (1 - c)

    def f4(xyz, like):
        return np.float32([xyz[0], xyz[1], xyz[2], np.asarray(like, np.float32)[3]])

    position = centre + turn(np.asarray(scene.cameraPosition, np.float64)[:3] - centre)
    return (f4(position, scene.cameraPosition), f4(turn(scene.cameraDirection), scene.cameraDirection),
            f4(turn(scene.cameraRight), scene.cameraRight), f4(turn(scene.cameraUp), scene.cameraUp))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--obj", help="a Wavefront OBJ file instead of a built-in scene (opencl_pathtracer_amd.obj_import)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--strict-arithmetic", action="store_true",
                    help="the strict arithmetic instead of the reference's own build's (both bit-exact modes, DESIGN.md 2)")
    ap.add_argument("--orbit", type=int, default=0, metavar="N",
                    help="N frames around the scene instead of one image: the camera moves with set_camera, the scene stays on the "
                         "device; writes <output>_000.bmp ... (ptmi_set_camera + ptmi_clear per frame)")
    ap.add_argument("-o", "--output", default="render.bmp")
    args = ap.parse_args()

    w, h = args.width, args.height
    if args.obj:
        from opencl_pathtracer_amd import obj_import
        scene = obj_import.scene_from_obj(args.obj, w, h)
    else:
        scene = pt.scenes.build(args.scene, w, h)
    scene = pt.bvh_create(scene, device=args.device)  # the tree on the device it renders on (the host's tree, byte for byte)
    flags = 0 if args.strict_arithmetic else pt.backend.FLAG_DEFAULT_ARITHMETIC  # default: the reference kernel's own pixels
    be = pt.Backend().setup_context(w, h, args.depth, scene.lightsSize, pt.structs.JITTERED, device=args.device, flags=flags)
    be.initialize_memory(scene)
    if args.orbit > 0:
        stem = args.output[:-4] if args.output.lower().endswith(".bmp") else args.output
        t0 = time.time()
        for k in range(args.orbit):
            be.set_camera(*orbit_camera(scene, 2 * np.pi * k / args.orbit))
            be.clear()
            be.render(0, args.spp)
            save_bmp(f"{stem}_{k:03d}.bmp", be.read_display(), w, h)
        dt = time.time() - t0
        be.release()
        print(f"{stem}_000.bmp .. {stem}_{args.orbit - 1:03d}.bmp: {args.orbit} frames of {w}x{h}, {args.spp} spp, depth {args.depth} "
              f"in {dt * 1e3:.1f} ms ({dt * 1e3 / args.orbit:.1f} ms per frame, one upload)")
        return
    t0 = time.time()
    be.render(0, args.spp)
    be.synchronize()
    dt = time.time() - t0
    rows = be.read_display()  # uint8[h, stride]: B,G,R scanlines, image row 0 first, padded to 4 bytes
    c = be.counters()
    be.release()
    save_bmp(args.output, rows, w, h)
    print(f"{args.output}: {w}x{h}, {args.spp} spp, depth {args.depth}: {c['segments'] / dt / 1e6:.1f} Msamples/s "
          f"({c['paths'] / dt / 1e6:.1f} Mpaths/s) in {dt * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
