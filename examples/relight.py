#!/usr/bin/env python3
"""One scene, uploaded once, looked at under two looks: a material and the light change between the renders.

    python examples/relight.py --width 512 --height 512 --spp 64
    python examples/relight.py --out look          # -> look_before.bmp, look_after.bmp

The small stage of the feature scenes (a floor, a wall, a sphere, one point light) goes up once.  It renders; then the sphere's
material becomes glass (ptmi_update_materials: 32 bytes to the device) and the point light a spot light from the other side
(ptmi_update_lights: 64 bytes); ptmi_clear, and it renders again.  No triangle is touched, no tree rebuilt, nothing uploaded
again.  The first look is all plain colours under a point light, which the integrator renders with its plain instantiation;
the edit leaves it, and the library says so (plain_before, plain_after).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, scenes, structs as S  # noqa: E402

BALL = 2  # scenes.feature_scene: the sphere's material


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64, help="iterations rendered per look")
    ap.add_argument("--out", default="relight", help="prefix of the two BMPs")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    w, h = args.width, args.height
    scene = pt.bvh_create(scenes.build("feat_plain", w, h))
    be = pt.Backend().setup_context(w, h, 6, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    be.render(0, max(args.spp, 1))
    output.save_bmp_rows(f"{args.out}_before.bmp", be.display(), w, h)

    glass = np.zeros(1, S.Material)
    glass[0] = scenes.material_create(S.MAT_GLASS, color=(0.9, 0.95, 1.0, 0), opacity=0.1)
    spot = np.zeros(1, S.Light)
    spot[0] = scenes.light_spot((-3.0, -4.0, 6.0), (0.45, 0.7, -1.0), cone_angle=0.8, penumbra_angle=0.3, color=(0.9, 0.9, 1, 1), intensity=3.0)
    info = be.update_materials(BALL, glass)
    be.update_lights(spot)
    be.clear()
    be.render(0, max(args.spp, 1))
    output.save_bmp_rows(f"{args.out}_after.bmp", be.display(), w, h)
    be.release()
    print(f"{args.out}_before.bmp, {args.out}_after.bmp: {w}x{h}, {args.spp} iterations each; the material update took "
          f"{info['total_ms']:.3f} ms (plain shading {info['plain_before']} -> {info['plain_after']})")


if __name__ == "__main__":
    main()
