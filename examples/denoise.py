#!/usr/bin/env python3
"""A few samples per pixel, filtered on the device: the raw and the denoised image side by side.

    python examples/denoise.py --scene cornell --width 512 --height 512 --spp 4
    python examples/denoise.py --scene matmix --sigma-position 0.5 --out matmix     # -> matmix_raw.bmp, matmix_denoised.bmp

Renders --spp iterations of a scene and filters the mean image with ptmi_denoise: an edge-avoiding a-trous wavelet filter guided
by the first-hit albedo, normal and position of the same iterations, which the call renders itself.  --sigma-position is in
scene units.  Only the filtered image crosses the bus, 16 bytes per pixel; the raw one is read here for the comparison.

    python examples/denoise.py --tone filmic --transfer srgb --exposure auto

With --tone, --transfer or --exposure both images are displayed on the device instead (ptmi_read_display_tonemapped for the raw
one; guides, filter and ptmi_display_device between tensors for the denoised one): 3 bytes per pixel cross the bus, no float plane.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, structs as S  # noqa: E402
import display_options  # noqa: E402


def main():
    d = pt.backend.DENOISE_DEFAULTS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--passes", type=int, default=d["passes"])
    ap.add_argument("--sigma-color", type=float, default=d["sigma_color"])
    ap.add_argument("--sigma-normal", type=float, default=d["sigma_normal"])
    ap.add_argument("--sigma-position", type=float, default=d["sigma_position"])
    ap.add_argument("--no-demodulation", action="store_true", help="filter the image itself, not the image divided by the albedo")
    ap.add_argument("--out", default="denoise", help="prefix of the BMPs")
    ap.add_argument("--device", type=int, default=0)
    display_options.add_arguments(ap)
    args = ap.parse_args()
    display = display_options.chosen(args)

    w, h, n = args.width, args.height, max(args.spp, 1)
    scene = pt.bvh_create(pt.scenes.build(args.scene, w, h))
    be = pt.Backend().setup_context(w, h, 4, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    be.render(0, n)
    filter_options = dict(passes=args.passes, sigma_color=args.sigma_color, sigma_normal=args.sigma_normal, sigma_position=args.sigma_position,
                          demodulate=not args.no_demodulation, guide_first_iteration=0, guide_iterations=n)
    if display:
        exposure = display_options.exposure_of(be, args)
        output.save_bmp_rows(args.out + "_raw.bmp", be.display(exposure=exposure, **display), w, h)
        output.save_bmp_rows(args.out + "_denoised.bmp", display_options.denoised_rows(be, exposure, display, **filter_options), w, h)
        be.release()
    else:
        color, count = be.read_image()
        denoised = be.denoise(**filter_options)
        be.release()
        output.save_bmp(args.out + "_raw.bmp", color, count)
        output.save_bmp(args.out + "_denoised.bmp", denoised)  # (already a mean: its fourth word is the sample count)
    print(f"{args.out}_raw.bmp, {args.out}_denoised.bmp: {w}x{h}, {n} samples per pixel, {args.passes} passes")


if __name__ == "__main__":
    main()
