#!/usr/bin/env python3
"""Look development with a render region: edit one material, then refine only the rectangle that shows it.

    python examples/region.py --region 150,260,200,180 --spp 16 --region-spp 256
    python examples/region.py --obj mesh.obj --material 0 --region 0,0,256,256 -o look.bmp

The scene (the Cornell box, or a Wavefront OBJ) goes up once and the frame renders at --spp.  Then one material changes
(ptmi_update_materials: 32 bytes to the device).  What the frame holds of it is stale only where the object shows, so only the
rectangle given by --region x,y,w,h is cleared - read back, zeroed on the host, written again - and rendered anew, to the
higher sample count --region-spp (ptmi_render_region): the paths are the very paths ptmi_render would trace for those pixels,
and no pixel outside the rectangle is read or written.  The BMP shows the old frame around the refined rectangle.
(ptmi_clear would wipe the whole frame, and there is no write of a rectangle: clearing it this way moves the WHOLE frame across
the bus once each way, 20 bytes per image pixel - once per edit, not per render call.)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, scenes, structs as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--obj", help="a Wavefront OBJ file instead of the Cornell box (opencl_pathtracer_amd.obj_import)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16, help="iterations of the whole frame")
    ap.add_argument("--region", default=None, help="x,y,w,h of the rectangle to refine (default: the middle quarter of the frame)")
    ap.add_argument("--region-spp", type=int, default=256, help="iterations of the rectangle after the edit")
    ap.add_argument("--material", type=int, default=0, help="index of the material that changes")
    ap.add_argument("--color", default="0.85,0.25,0.2", help="its new colour, r,g,b")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", default="region.bmp")
    args = ap.parse_args()

    w, h = args.width, args.height
    if args.obj:
        from opencl_pathtracer_amd import obj_import
        scene = obj_import.scene_from_obj(args.obj, w, h)
    else:
        scene = scenes.build("cornell", w, h)
    scene = pt.bvh_create(scene)
    x, y, rw, rh = map(int, args.region.split(",")) if args.region else (w // 4, h // 4, w // 2, h // 2)

    be = pt.Backend().setup_context(w, h, args.depth, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    t0 = time.perf_counter()
    be.render(0, max(args.spp, 1))
    be.synchronize()
    frame_ms = (time.perf_counter() - t0) * 1e3

    edited = np.zeros(1, S.Material)
    edited[0] = scenes.material_create(S.MAT_STANDART, color=(*map(float, args.color.split(",")), 0.0))
    be.update_materials(args.material, edited)
    # clear the rectangle alone: the rest of the frame keeps its samples
    color, count = be.read_image()
    color[y:y + rh, x:x + rw] = 0
    count[y:y + rh, x:x + rw] = 0
    be.write_image(color, count)
    t0 = time.perf_counter()
    be.render_region(x, y, rw, rh, 0, max(args.region_spp, 1))
    be.synchronize()
    region_ms = (time.perf_counter() - t0) * 1e3

    output.save_bmp_rows(args.output, be.display(), w, h)
    be.release()
    print(f"{args.output}: {w}x{h}, the frame at {args.spp} iterations in {frame_ms:.1f} ms; material {args.material} edited, rectangle "
          f"({x}, {y}, {rw}, {rh}) rendered anew at {args.region_spp} iterations in {region_ms:.1f} ms")


if __name__ == "__main__":
    main()
