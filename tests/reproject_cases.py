"""The yardstick of ptmi_reproject_device / ptmi_set_camera_reprojected (test_reproject_model.py, test_reproject_gpu.py): the
reprojection's arithmetic as ptmi.h and DESIGN 1g state it, in NumPy, vectorised over the pixels with a Python loop over the four
taps.  No product code is involved.  The host part (the rows that invert the previous camera) is float64 rounded to float32
once; everything else is np.float32 arrays and scalars, so no operation is promoted, and every line is one IEEE binary32
operation per pixel in the written order.  Below it: the generators of the synthetic cases and the previous cameras the tests
use, and the grid the shipped defaults are held against."""
import numpy as np

f32 = np.float32
ZERO, ONE, HALF = f32(0), f32(1), f32(0.5)


def dot3(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z over the last axis"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def camera_rows(camera):
    """camera = (position, direction, right, up), float32 each -> (det, r0, r1, r2): det in float64, the rows float32"""
    direction, right, up = (np.asarray(v, f32)[:3].astype(np.float64) for v in camera[1:])
    c = cross(right, up)
    det = (direction[0] * c[0] + direction[1] * c[1]) + direction[2] * c[2]
    with np.errstate(all="ignore"):
        rows = [(v / det).astype(f32) for v in (c, cross(up, direction), cross(direction, right))]
    return det, rows[0], rows[1], rows[2]


def reproject(previous_camera, previous, current, position_tolerance, normal_tolerance, max_history, details=None):
    """previous = dict(normal, position, hit_count, color, ray_nb), current = dict(normal, position, hit_count): [H,W,4] and [H,W]
    float32 planes -> (out_color[H,W,4], out_ray_nb[H,W]).  details: a dict that receives u, w_ and the history mask."""
    prev = {k: np.asarray(previous[k], f32) for k in ("normal", "position", "hit_count", "color", "ray_nb")}
    cur = {k: np.asarray(current[k], f32) for k in ("normal", "position", "hit_count")}
    height, width = cur["hit_count"].shape
    _, r0, r1, r2 = camera_rows(previous_camera)
    cam = np.asarray(previous_camera[0], f32)[:3]
    tp = f32(position_tolerance) * f32(position_tolerance)
    tn = f32(normal_tolerance) * f32(normal_tolerance)
    Wf, Hf, cap = f32(width), f32(height), f32(max_history)
    with np.errstate(all="ignore"):
        h = cur["hit_count"]
        P = cur["position"][..., :3] / h[..., None]
        N = cur["normal"][..., :3] / h[..., None]
        v = P - cam
        t, a, b = dot3(r0, v), dot3(r1, v), dot3(r2, v)
        u = (a / t + HALF) * Wf - HALF
        w_ = (b / t + HALF) * Hf - HALF
        ok = (h > 0) & (t > 0) & (u > -ONE) & (u < Wf) & (w_ > -ONE) & (w_ < Hf)
        x0, y0 = np.floor(u), np.floor(w_)
        fx, fy = u - x0, w_ - y0
        lim = tp * dot3(v, v)
        gx1, gy1 = ONE - fx, ONE - fy
        weights = (gx1 * gy1, fx * gy1, gx1 * fy, fx * fy)
        assert all(x.dtype == f32 for x in (P, N, v, t, a, b, u, w_, x0, fx, lim) + weights)
        ix = np.where(ok, x0, ZERO).astype(np.int64)
        iy = np.where(ok, y0, ZERO).astype(np.int64)
        sw = np.zeros((height, width), f32)
        sn = np.zeros((height, width), f32)
        sm = np.zeros((height, width, 4), f32)
        for k in range(4):
            qx, qy = ix + (k & 1), iy + (k >> 1)
            inside = ok & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
            cx, cy = np.clip(qx, 0, width - 1), np.clip(qy, 0, height - 1)  # (what lies outside is masked, never used)
            w = weights[k]
            hq, nq = prev["hit_count"][cy, cx], prev["ray_nb"][cy, cx]
            dP = prev["position"][cy, cx, :3] / hq[..., None] - P
            dN = prev["normal"][cy, cx, :3] / hq[..., None] - N
            mq = prev["color"][cy, cx] / nq[..., None]
            finite = ((mq - mq) == 0).all(-1)
            taken = inside & (w > 0) & (hq > 0) & (nq > 0) & (dot3(dP, dP) <= lim) & (dot3(dN, dN) <= tn) & finite
            new_sw, new_sm, new_sn = sw + w, sm + w[..., None] * mq, sn + w * nq
            assert all(x.dtype == f32 for x in (dP, dN, mq, new_sw, new_sm, new_sn))
            sw = np.where(taken, new_sw, sw)
            sm = np.where(taken[..., None], new_sm, sm)
            sn = np.where(taken, new_sn, sn)
        mean_n = sn / sw
        n = np.floor(np.where(mean_n < cap, mean_n, cap))
        history = (sw > 0) & (n >= 1)
        out_color = np.where(history[..., None], (sm / sw[..., None]) * n[..., None], ZERO)
        out_ray_nb = np.where(history, n, ZERO)
    assert out_color.dtype == f32 and out_ray_nb.dtype == f32
    if details is not None:
        details.update(u=u, w_=w_, ok=ok, history=history)
    return out_color, out_ray_nb


def describe_difference(got, want):
    """'' where every word of both planes is equal (the yardstick's planes hold no NaN: neither may the kernel's)"""
    for name, g, w in zip(("color", "ray_nb"), got, want):
        g, w = np.asarray(g, f32), np.asarray(w, f32)
        if g.shape != w.shape:
            return f"{name}: shape {g.shape}, not {w.shape}"
        if np.isnan(g).any():
            return f"{name}: {int(np.isnan(g).sum())} NaN words in the result"
        same = g.view(np.uint32) == w.view(np.uint32)
        if not same.all():
            bad = np.argwhere(~same)
            where = tuple(int(i) for i in bad[0])
            return f"{name}: {len(bad)} words differ of {same.size}; first at (y, x[, c]) = {where}: got {g[where]!r}, want {w[where]!r}"
    return ""


# ---------------------------------------------------------------------------------------------- the synthetic world

# A pinhole camera at the origin looks along +z at two planes: a NEAR strip at z = 4 that covers x in [-1.1, 0.3] and a FAR wall at
# z = 8 behind it, with square holes (no hit) in the wall - a blocky hit mask that is fixed in the world, so every camera sees the
# same holes.  The planes carry different shading normals.
Z_NEAR, Z_FAR = 4.0, 8.0
NEAR_X = (-1.1, 0.3)
N_NEAR, N_FAR = (0.0, 0.6, -0.8), (0.0, 0.0, -1.0)
HOLE = 0.9  # edge of the wall's blocks, in world units


def camera(position=(0, 0, 0), direction=(0, 0, 1), right=(1, 0, 0), up=(0, 0.75, 0)):
    """(position, direction, right, up) as float32[4] each (w = 0)"""
    return tuple(np.array(list(v) + [0.0], f32) for v in (position, direction, right, up))


CURRENT = camera()


def _hole(x, y):
    bx, by = np.floor(x / HOLE).astype(np.int64), np.floor(y / HOLE).astype(np.int64)
    return ((bx * 7 + by * 13) % 5) == 0


def guides(cam, width, height, seed=0):
    """The planes a guide call would give for the synthetic world under `cam`, at exact pixel centres (float64, rounded once),
    summed over a seeded per-pixel number of iterations 1..3: dict(normal, position, hit_count)."""
    pos, direction, right, up = (np.asarray(v, f32)[:3].astype(np.float64) for v in cam)
    yy, xx = np.mgrid[0:height, 0:width]
    sx, sy = (xx + 0.5) / width - 0.5, (yy + 0.5) / height - 0.5
    d = direction + sx[..., None] * right + sy[..., None] * up
    with np.errstate(all="ignore"):
        t_near = (Z_NEAR - pos[2]) / d[..., 2]
        t_far = (Z_FAR - pos[2]) / d[..., 2]
        p_near = pos + t_near[..., None] * d
        p_far = pos + t_far[..., None] * d
        near = (t_near > 0) & (p_near[..., 0] >= NEAR_X[0]) & (p_near[..., 0] <= NEAR_X[1])
        far = ~near & (t_far > 0) & ~_hole(p_far[..., 0], p_far[..., 1])
    point = np.where(near[..., None], p_near, p_far)
    normal = np.where(near[..., None], np.array(N_NEAR), np.array(N_FAR))
    hits = np.random.default_rng(seed).integers(1, 4, (height, width)).astype(np.float64) * (near | far)
    four = lambda v3: np.concatenate([np.nan_to_num(v3) * hits[..., None], np.zeros((height, width, 1))], -1).astype(f32)  # noqa: E731
    return dict(normal=four(normal), position=four(point), hit_count=hits.astype(f32)), near, far


def image(width, height, seed, odd=True):
    """A seeded previous image: means over six decades, counts 1..24; with `odd`, about 3 % of the pixels with a zero count and
    about 3 % with a NaN or infinite channel (one of each kind at least, where there is room): dict(color, ray_nb)."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 25, (height, width)).astype(f32)
    decades = f32(10.0) ** rng.integers(-3, 3, (height, width, 1)).astype(f32)
    color = (rng.random((height, width, 4)).astype(f32) * decades * n[..., None]).astype(f32)
    if odd:
        kinds = np.array([np.nan, np.inf, -np.inf], f32)
        n[rng.random((height, width)) < 0.03] = 0
        for y, x in np.argwhere(rng.random((height, width)) < 0.03):
            color[y, x, rng.integers(0, 4)] = kinds[rng.integers(0, 3)]
        if width * height >= 15:
            for kind in kinds:
                color[rng.integers(0, height), rng.integers(0, width), rng.integers(0, 4)] = kind
            n[rng.integers(0, height), rng.integers(0, width)] = 0
    return dict(color=color, ray_nb=n)


def rotated_about_y(degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return camera(direction=(s, 0, c), right=(c, 0, -s))


def previous_cameras(width, height):
    """name -> the previous camera; the current one is CURRENT.  At depth z a pixel is z / width wide (|right| = 1)."""
    return {
        "identical": camera(),
        "pan_one_pixel_at_near": camera(position=(Z_NEAR / width, 0, 0)),
        "pan_fraction": camera(position=(0.37 * Z_NEAR / width, -1.21 * 0.75 * Z_NEAR / height, 0)),
        "dolly": camera(position=(0.05, -0.02, -0.6)),
        "rotated": rotated_about_y(3.0),
        "skewed": camera(position=(0.1, 0, 0), right=(1, 0.2, 0.1), up=(0.1, 0.75, 0.05)),
        "behind": camera(position=(0, 0, Z_FAR + 1.0)),
    }


CAMERAS = tuple(previous_cameras(1, 1))


def synthetic_params(width, height):
    """The position tolerance is relative to the distance and a pixel is 1 / width of it wide: a pixel and a half passes, the step
    between the planes (half the far distance) never does."""
    return dict(position_tolerance=min(0.25, 1.5 / min(width, height)), normal_tolerance=0.3, max_history=12.0)


def case(width, height, name, seed=None, odd=True):
    """-> (previous_camera, previous planes incl. the image, current planes)"""
    seed = width * 1000 + height if seed is None else seed
    prev_cam = previous_cameras(width, height)[name]
    previous, _, _ = guides(prev_cam, width, height, seed)
    previous.update(image(width, height, seed + 1, odd))
    current, _, _ = guides(CURRENT, width, height, seed + 2)
    return prev_cam, previous, current


# ---------------------------------------------------------------------------------------------- the defaults' grid

# The shipped defaults (backend.REPROJECT_DEFAULTS) must be the RMSE minimum over this grid on the Cornell box at 64 x 48: 16
# iterations at camera A, the camera orbited by ORBIT_DEGREES about the box's centre, the reprojection, 4 iterations at B, against
# 1024 further iterations at B (test_reproject_gpu.py::test_defaults_are_the_grids_minimum).  What spans it: neighbouring pixels
# of a 64-pixel row lie 1/64 = 1.6 % of their distance apart, so the relative position tolerance runs from a fraction of a pixel
# (hardly a tap passes on a slanted wall) to 16 times the distance (position says nothing: no two points of that box are so far
# apart, seen from outside it, so the top values must give one and the same image and the test can tell a saturated axis from a
# grid that ends too early); unit normals are at most 2 apart, so from 1/16 to 4
# (normals say nothing); and the history cap from 1 (a carried pixel weighs as one new sample) to infinity, with 16 iterations
# before the move the most there is to carry.
GRID_POSITION_TOLERANCE = (0.005, 0.01, 0.02, 0.04, 0.08, 0.16, 0.64, 2.56, 16.0)
GRID_NORMAL_TOLERANCE = (0.0625, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0)
GRID_MAX_HISTORY = (1.0, 2.0, 4.0, 8.0, 16.0, float("inf"))
ORBIT_DEGREES = 4.0


def rmse(image_, truth):
    """root mean square error of the r, g, b means, in float64"""
    a, b = np.asarray(image_, np.float64)[..., :3], np.asarray(truth, np.float64)[..., :3]
    return float(np.sqrt(np.mean((a - b) ** 2)))
