#!/usr/bin/env python3
"""An interactive viewer's orbit, two ways: clearing the image at every camera move, and carrying it along.

    python examples/orbit.py --scene cornell --width 512 --height 512 --steps 12 --degrees 2 --spp 2
    python examples/orbit.py --out turn          # -> turn_clear_00.bmp ..., turn_reprojected_00.bmp ...

The camera turns about the point the middle of the image sees, --degrees per step, and --spp iterations are rendered per step.
One context calls ptmi_clear after every move, as a caller had to: each of its frames shows --spp samples per pixel.  The other
moves with ptmi_set_camera_reprojected: every pixel whose surface the previous camera saw too keeps its mean and its sample count,
only the revealed ones restart, and ptmi_denoise filters what is left of the noise.  One BMP per step and way, to be flipped
through side by side.

    python examples/orbit.py --tone filmic --transfer srgb --exposure auto

With --tone, --transfer or --exposure the frames are displayed on the device (ptmi_read_display_tonemapped; guides, filter and
ptmi_display_device between tensors for the carried image), `auto` choosing the exposure from the luminance histogram of each
frame: 3 bytes per pixel cross the bus, no float plane.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, structs as S  # noqa: E402
import display_options  # noqa: E402


def main():
    d = pt.backend.REPROJECT_DEFAULTS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--degrees", type=float, default=2.0, help="the camera's turn per step")
    ap.add_argument("--spp", type=int, default=2, help="iterations rendered per step")
    ap.add_argument("--position-tolerance", type=float, default=d["position_tolerance"])
    ap.add_argument("--normal-tolerance", type=float, default=d["normal_tolerance"])
    ap.add_argument("--max-history", type=float, default=d["max_history"])
    ap.add_argument("--out", default="orbit", help="prefix of the BMPs")
    ap.add_argument("--device", type=int, default=0)
    display_options.add_arguments(ap)
    args = ap.parse_args()
    display = display_options.chosen(args)

    w, h, n = args.width, args.height, max(args.spp, 1)
    scene = pt.bvh_create(pt.scenes.build(args.scene, w, h))
    contexts = []
    for _ in range(2):
        be = pt.Backend().setup_context(w, h, 4, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
        contexts.append(be.initialize_memory(scene))
    clearing, carrying = contexts
    camera = (scene.cameraPosition, scene.cameraDirection, scene.cameraRight, scene.cameraUp)
    guides = clearing.render_guides(0, 1, planes=("position", "hit_count"))
    middle = (slice(h // 2 - 2, h // 2 + 2), slice(w // 2 - 2, w // 2 + 2))
    hits = guides["hit_count"][middle].sum()
    centre = guides["position"][middle][..., :3].sum((0, 1)) / hits if hits else np.asarray(camera[0][:3]) + np.asarray(camera[1][:3])

    kept = []
    for step in range(args.steps):
        first = step * n
        if step:
            camera = pt.scenes.orbit_camera(camera, centre, args.degrees)
            clearing.set_camera(*camera)
            clearing.clear()
            carrying.set_camera_reprojected(*camera, position_tolerance=args.position_tolerance, normal_tolerance=args.normal_tolerance,
                                            max_history=args.max_history, guide_first_iteration=first, guide_iterations=n)
            if display:  # (word 256: the pixels without a sample - no plane is read back)
                kept.append(1.0 - float(carrying.luminance_histogram()[256]) / (w * h))
            else:
                kept.append(float((carrying.read_image()[1] > 0).mean()))
        for be in contexts:
            be.render(first, n)
        if display:
            output.save_bmp_rows(f"{args.out}_clear_{step:02d}.bmp", clearing.display(exposure=display_options.exposure_of(clearing, args), **display), w, h)
            rows = display_options.denoised_rows(carrying, display_options.exposure_of(carrying, args), display, guide_first_iteration=first,
                                                 guide_iterations=n)
            output.save_bmp_rows(f"{args.out}_reprojected_{step:02d}.bmp", rows, w, h)
            continue
        output.save_bmp(f"{args.out}_clear_{step:02d}.bmp", *clearing.read_image())
        output.save_bmp(f"{args.out}_reprojected_{step:02d}.bmp", carrying.denoise(guide_first_iteration=first, guide_iterations=n))
    for be in contexts:
        be.release()
    share = f", {100 * np.mean(kept):.1f} % of the pixels kept their history at a move" if kept else ""
    print(f"{args.out}_clear_NN.bmp, {args.out}_reprojected_NN.bmp: {args.steps} steps of {args.degrees} degrees, {w}x{h}, {n} iterations per step{share}")


if __name__ == "__main__":
    main()
