"""Exact float32 arithmetic for the yardsticks (guide_cases.py, leaf_cull_cases.py, ray_query_cases.py): the one rounding, the
one fused multiply-add and the one camera expression they build their rays with.  No product code is involved."""
import ctypes as C
from fractions import Fraction

import numpy as np

f32 = np.float32


def round_to_f32(q):
    """The float32 nearest to the Fraction q, ties to even."""
    near = f32(float(q))
    best = None
    for c in (np.nextafter(near, f32(-np.inf)), near, np.nextafter(near, f32(np.inf))):
        if not np.isfinite(c):
            continue
        key = (abs(Fraction(float(c)) - q), int(c.view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def fma(a, b, c, exact=False):
    """fmaf(a, b, c) on float32 scalars: one rounding of the exact a * b + c.  exact=True: every finite case through Fractions."""
    a, b, c = f32(a), f32(b), f32(c)
    with np.errstate(all="ignore"):
        s = np.float64(a) * np.float64(b) + np.float64(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return f32(s)  # (infinities and NaNs: nothing to round)
    # float64 holds the product exactly and rounds the sum once; rounding that to float32 is the fused result unless the
    # float64 sum sits exactly half way between two float32 values (or is zero, or tiny): those few go through exact fractions
    if not exact and int(s.view(np.uint64)) & 0x1FFFFFFF != 0x10000000 and abs(s) > 1e-30:
        return f32(s)
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:  # IEEE 754 6.3: an exact zero sum is +0 unless both addends are -0
        product_negative = bool(np.signbit(a)) != bool(np.signbit(b))
        both_zero = (a == 0 or b == 0) and c == 0
        return f32(-0.0) if both_zero and product_negative and np.signbit(c) else f32(0.0)
    return round_to_f32(q)


def mad(a, b, c, fused):
    """a * b + c in float32, on scalars or per component of arrays that broadcast: two rounded operations (the strict
    arithmetic), or one fused multiply-add (what the reference's default build makes of it)."""
    a, b, c = np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)
    if not fused:
        return a * b + c
    if a.ndim == b.ndim == c.ndim == 0:
        return fma(a, b, c)
    a, b, c = np.broadcast_arrays(a, b, c)
    return np.array([fma(x, y, z) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())], f32).reshape(a.shape)


def camera_direction(scene, sample, fused):
    """cameraDirection + cameraRight * sample.x + cameraUp * sample.y as cl:1213 nests it (un-normalised: Ray3D_Create does that)."""
    direction, right, up = (np.asarray(v, f32).reshape(4) for v in (scene.cameraDirection, scene.cameraRight, scene.cameraUp))
    with np.errstate(all="ignore"):
        return mad(up, sample[1], mad(right, sample[0], direction, fused), fused)


def c4(v):
    return (C.c_float * 4)(*[float(x) for x in v])


def bits(x):
    return np.asarray(x, f32).view(np.uint32)
