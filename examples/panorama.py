#!/usr/bin/env python3
"""Two camera models the built-in pinhole does not have, from rays built here in NumPy: ptmi_trace_paths.

    python examples/panorama.py --scene cornell --spp 16
    python examples/panorama.py --scene matmix --width 512 --height 256 --aperture 6 --out-dir /tmp

Writes <scene>_panorama.bmp, an equirectangular 360 x 180 degree view from the camera's position, and <scene>_thin_lens.bmp,
the camera's own view through a lens of radius --aperture focused at --focus (depth of field).  Every pixel is one ray of the
caller's; the library traces each as a full path (every light, every bounce) for --spp iterations and returns the sum.

No direction component is exactly zero: a +0 component makes the reference's box test fail every box, so a ray
along an axis would see nothing.  The generators below cannot produce one except at isolated pixel centres, and `nudge` moves
those by one part in a million.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import opencl_pathtracer_amd as pt  # noqa: E402
from opencl_pathtracer_amd import output, structs as S  # noqa: E402


def nudge(d):
    d = np.asarray(d, np.float32)
    return np.where(d == 0, np.float32(1e-6), d)


def camera_frame(scene):
    """(position float32[4], unit forward, right, up float64[3]) of the scene's camera"""
    f, r, u = (np.asarray(v, np.float64)[:3] for v in (scene.cameraDirection, scene.cameraRight, scene.cameraUp))
    return np.asarray(scene.cameraPosition, np.float32), f / np.linalg.norm(f), r / np.linalg.norm(r), u / np.linalg.norm(u)


def panorama_rays(scene, w, h):
    """Pixel (x, y): longitude 2 pi (x + 0.5) / w - pi around the camera's up axis, latitude pi (y + 0.5) / h - pi / 2."""
    o, f, r, u = camera_frame(scene)
    lon = (2 * np.pi * (np.arange(w) + 0.5) / w - np.pi)[None, :]
    lat = (np.pi * (np.arange(h) + 0.5) / h - np.pi / 2)[:, None]
    d = (np.cos(lat) * np.sin(lon))[..., None] * r + (np.sin(lat) * np.ones_like(lon))[..., None] * u + (np.cos(lat) * np.cos(lon))[..., None] * f
    return np.tile(o, (w * h, 1)), nudge(d.reshape(-1, 3))


def thin_lens_rays(scene, w, h, aperture, focus, rng):
    """The pinhole's ray through the pixel centre fixes the point in focus (at distance `focus` along it); the ray starts at a
    random point of the lens disk and aims there."""
    o, f, r, u = camera_frame(scene)
    sx = ((np.arange(w) + 0.5) / w - 0.5)[None, :, None]
    sy = ((np.arange(h) + 0.5) / h - 0.5)[:, None, None]
    pinhole = np.asarray(scene.cameraDirection, np.float64)[:3] + np.asarray(scene.cameraRight, np.float64)[:3] * sx + np.asarray(scene.cameraUp, np.float64)[:3] * sy
    pinhole /= np.linalg.norm(pinhole, axis=-1, keepdims=True)
    target = o[:3].astype(np.float64) + pinhole * focus
    rad, phi = aperture * np.sqrt(rng.random((h, w, 1))), 2 * np.pi * rng.random((h, w, 1))
    lens = o[:3].astype(np.float64) + rad * np.cos(phi) * r + rad * np.sin(phi) * u
    origins = np.concatenate([lens, np.full((h, w, 1), float(o[3]))], axis=-1).reshape(-1, 4)
    return origins.astype(np.float32), nudge((target - lens).reshape(-1, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell", help="cornell | mayalike | matmix | tris<N>[k|m] (opencl_pathtracer_amd.scenes.build)")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--spp", type=int, default=16, help="iterations per ray (at most backend.MAX_PATH_ITERATIONS per call)")
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--aperture", type=float, default=None, help="lens radius in scene units (default: 1 % of the scene's extent)")
    ap.add_argument("--focus", type=float, default=None, help="distance of the plane in focus (default: the scene's centre)")
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    w, h = args.width, args.height
    scene = pt.bvh_create(pt.scenes.build(args.scene, w, h))
    t = scene.triangulation
    points = np.concatenate([t["S1"][:, :3], t["S2"][:, :3], t["S3"][:, :3]]).astype(np.float64)
    centre, extent = (points.min(axis=0) + points.max(axis=0)) / 2, float((points.max(axis=0) - points.min(axis=0)).max())
    aperture = 0.01 * extent if args.aperture is None else args.aperture
    focus = float(np.linalg.norm(centre - np.asarray(scene.cameraPosition, np.float64)[:3])) if args.focus is None else args.focus

    be = pt.Backend().setup_context(w, h, args.depth, scene.lightsSize, S.JITTERED, device=args.device, flags=pt.backend.FLAG_DEFAULT_ARITHMETIC)
    be.initialize_memory(scene)
    views = {"panorama": panorama_rays(scene, w, h), "thin_lens": thin_lens_rays(scene, w, h, aperture, focus, np.random.default_rng(1))}
    for name, (origins, directions) in views.items():
        sums = be.trace_paths(origins, directions, n_iterations=args.spp)  # index_stride = the ray count: every path its own random numbers
        image = sums["radiance"].reshape(h, w, 4)
        path = os.path.join(args.out_dir, f"{args.scene}_{name}.bmp")
        output.save_bmp(path, image, np.full((h, w), np.float32(args.spp)))
        print(f"{path}: {w} x {h} rays x {args.spp} iterations, {int(sums['segments'].sum())} segments, {int(sums['shadow_rays'].sum())} shadow rays")
    be.release()


if __name__ == "__main__":
    main()
