"""ptmi_reproject_device / ptmi_set_camera_reprojected without a GPU: the new ABI (symbols, struct layout) held against the header,
the yardstick of the GPU tests (reproject_cases.py) held bit for bit against a second restatement of the contract - a scalar
loop over pixels and taps - and the properties that make it a reprojection."""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import backend
from abi_cases import exported_symbols, header_values
import reproject_cases as R

f32 = np.float32
NAMES = {"ptmi_reproject_device", "ptmi_set_camera_reprojected"}


# ---------------------------------------------------------------------------------------------- ABI and layout

def test_library_exports_the_reproject_entry_points(built):
    """Both calls exist and refuse a NULL context with PTMI_ERR_INVALID_ARGUMENT, before they look at anything else."""
    assert NAMES <= exported_symbols()
    assert NAMES <= set(backend.ABI_SYMBOLS)
    lib = backend.load_library()
    assert lib.ptmi_abi_version() == 4
    p = backend.Backend.reproject_params()
    assert lib.ptmi_reproject_device(None, C.byref(p), None, None, None, None, None, None, None) == -1
    assert lib.ptmi_set_camera_reprojected(None, None, None, None, None, C.byref(p)) == -1
    assert lib.ptmi_set_camera_reprojected(None, None, None, None, None, None) == -1


LAYOUT = """
    SIZE(ptmi_reproject_params);
    OFFSET(ptmi_reproject_params, struct_size); OFFSET(ptmi_reproject_params, flags); OFFSET(ptmi_reproject_params, guide_first_iteration);
    OFFSET(ptmi_reproject_params, guide_iterations); OFFSET(ptmi_reproject_params, position_tolerance);
    OFFSET(ptmi_reproject_params, normal_tolerance); OFFSET(ptmi_reproject_params, max_history); OFFSET(ptmi_reproject_params, reserved);
""".splitlines()


def test_ctypes_struct_matches_the_header():
    out = header_values(LAYOUT)
    want = {"ptmi_reproject_params": 32}
    for field, _ in backend.ReprojectParams._fields_:
        want[f"ptmi_reproject_params.{field}"] = getattr(backend.ReprojectParams, field).offset
    assert out == want
    assert C.sizeof(backend.ReprojectParams) == 32
    assert [out[f"ptmi_reproject_params.{f}"] for f, _ in backend.ReprojectParams._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    p = backend.Backend.reproject_params()
    assert p.struct_size == 32 and p.flags == 0 and p.reserved == 0 and p.guide_iterations == 1
    assert {k: getattr(p, k) for k in backend.REPROJECT_DEFAULTS} == {k: f32(v) for k, v in backend.REPROJECT_DEFAULTS.items()}


# ---------------------------------------------------------------------------------------------- the second restatement

def scalar_reproject(previous_camera, prev, cur, position_tolerance, normal_tolerance, max_history):
    """The contract of ptmi.h read again, one pixel and one tap at a time, in np.float32 scalars."""
    height, width = cur["hit_count"].shape
    direction, right, up = (np.asarray(v, f32)[:3].astype(np.float64) for v in previous_camera[1:])
    c = R.cross(right, up)
    det = (direction[0] * c[0] + direction[1] * c[1]) + direction[2] * c[2]
    r0, r1, r2 = ((v / det).astype(f32) for v in (c, R.cross(up, direction), R.cross(direction, right)))
    cam = np.asarray(previous_camera[0], f32)
    tp, tn = f32(position_tolerance) * f32(position_tolerance), f32(normal_tolerance) * f32(normal_tolerance)
    Wf, Hf, cap, half, one = f32(width), f32(height), f32(max_history), f32(0.5), f32(1)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    out_color, out_count = np.zeros((height, width, 4), f32), np.zeros((height, width), f32)
    with np.errstate(all="ignore"):
        for y in range(height):
            for x in range(width):
                h = cur["hit_count"][y, x]
                if not h > 0:
                    continue
                P = [cur["position"][y, x, i] / h for i in range(3)]
                N = [cur["normal"][y, x, i] / h for i in range(3)]
                v = [P[i] - cam[i] for i in range(3)]
                t, a, b = dot(r0, v), dot(r1, v), dot(r2, v)
                if not t > 0:
                    continue
                u, w_ = (a / t + half) * Wf - half, (b / t + half) * Hf - half
                if not (u > -one and u < Wf and w_ > -one and w_ < Hf):
                    continue
                x0, y0 = np.floor(u), np.floor(w_)
                fx, fy = u - x0, w_ - y0
                lim = tp * dot(v, v)
                sw, sn, sm = f32(0), f32(0), [f32(0)] * 4
                taps = (((0, 0), (one - fx) * (one - fy)), ((1, 0), fx * (one - fy)), ((0, 1), (one - fx) * fy), ((1, 1), fx * fy))
                for (dx, dy), w in taps:
                    qx, qy = int(x0) + dx, int(y0) + dy
                    if qx < 0 or qx >= width or qy < 0 or qy >= height or not w > 0:
                        continue
                    hq, nq = prev["hit_count"][qy, qx], prev["ray_nb"][qy, qx]
                    if not (hq > 0 and nq > 0):
                        continue
                    dP = [prev["position"][qy, qx, i] / hq - P[i] for i in range(3)]
                    dN = [prev["normal"][qy, qx, i] / hq - N[i] for i in range(3)]
                    if not (dot(dP, dP) <= lim and dot(dN, dN) <= tn):
                        continue
                    mq = [prev["color"][qy, qx, i] / nq for i in range(4)]
                    if not all(m - m == 0 for m in mq):
                        continue
                    sw = sw + w
                    sm = [sm[i] + w * mq[i] for i in range(4)]
                    sn = sn + w * nq
                assert all(type(z) is f32 for z in (t, u, fx, lim, sw, sn, *sm))
                if not sw > 0:
                    continue
                mean_n = sn / sw
                n = np.floor(mean_n if mean_n < cap else cap)
                if n >= 1:
                    out_color[y, x] = [(sm[i] / sw) * n for i in range(4)]
                    out_count[y, x] = n
    return out_color, out_count


@pytest.mark.parametrize("name", R.CAMERAS)
def test_yardstick_equals_the_scalar_restatement(name):
    prev_cam, previous, current = R.case(13, 9, name)
    for params in (R.synthetic_params(13, 9), dict(position_tolerance=0.5, normal_tolerance=4.0, max_history=float("inf"))):
        got = R.reproject(prev_cam, previous, current, **params)
        assert not R.describe_difference(got, scalar_reproject(prev_cam, previous, current, **params))
        if name != "behind":
            assert (got[1] > 0).any() and (got[1] == 0).any()  # (something is carried, something restarts)


# ---------------------------------------------------------------------------------------------- it is a reprojection

W2, H2 = 16, 8  # powers of two: pixel centres, the one-pixel pan and the projection are exact in binary32
OPEN = dict(position_tolerance=0.05, normal_tolerance=0.3)


def test_identical_camera_returns_every_hit_pixel():
    """Exact pixel centres project onto themselves: the weights are (1, 0, 0, 0), so the mean is the pixel's own m = color / n
    and the sum (m * n') is within two roundings of m * n' in real numbers - a relative 2^-23 - where n' = min(n, max_history)."""
    prev_cam, previous, current = R.case(W2, H2, "identical", odd=False)
    previous.update(R.guides(prev_cam, W2, H2, seed=5)[0])  # (guides of other iteration counts: the means are the same)
    for cap in (4.0, float("inf")):
        details = {}
        color, count = R.reproject(prev_cam, previous, current, max_history=cap, details=details, **OPEN)
        hit = current["hit_count"] > 0
        assert hit.any() and not hit.all()
        assert np.array_equal(details["u"][hit], np.mgrid[0:H2, 0:W2][1][hit]) and np.array_equal(details["w_"][hit], np.mgrid[0:H2, 0:W2][0][hit])
        assert np.array_equal(count, np.where(hit, np.minimum(previous["ray_nb"], f32(cap)), 0))
        mean = previous["color"].astype(np.float64) / previous["ray_nb"][..., None]
        want = mean * count[..., None]
        assert (np.abs(color[hit] - want[hit]) <= 2.0 ** -23 * np.abs(want[hit])).all()
        assert not color[~hit].any() and not count[~hit].any()  # a miss carries nothing


def test_one_pixel_pan_shifts_the_image_by_one_pixel():
    """The previous camera stood one near-plane pixel to the right, so a near-plane point lay one pixel further LEFT in its
    image: new pixel x shows previous pixel x - 1, exactly."""
    prev_cam, previous, current = R.case(W2, H2, "pan_one_pixel_at_near", odd=False)
    _, near_now, _ = R.guides(R.CURRENT, W2, H2)
    _, near_before, _ = R.guides(prev_cam, W2, H2)
    color, count = R.reproject(prev_cam, previous, current, max_history=float("inf"), **OPEN)
    checked = 0
    for y, x in np.argwhere(near_now):
        if x >= 1 and near_before[y, x - 1]:
            m = previous["color"][y, x - 1] / previous["ray_nb"][y, x - 1]
            assert count[y, x] == previous["ray_nb"][y, x - 1] and np.array_equal(color[y, x], m * count[y, x])
            checked += 1
    assert checked >= 3 * H2


def test_sideways_move_reveals_pixels_and_never_mixes_the_planes():
    """A colour per plane: near red, far blue.  Far pixels next to the near strip's edge were hidden before the move and restart
    at count 0; no output pixel holds both colours."""
    w, h = 48, 12
    prev_cam = R.camera(position=(0.5, 0, 0))
    previous, near_before, far_before = R.guides(prev_cam, w, h, 1)
    current, near_now, far_now = R.guides(R.CURRENT, w, h, 2)
    n = np.full((h, w), 4, f32)
    color = np.zeros((h, w, 4), f32)
    color[near_before, 0] = 4
    color[far_before, 2] = 4
    out, count = R.reproject(prev_cam, dict(previous, color=color, ray_nb=n), current, max_history=8.0, **OPEN)
    assert not ((out[..., 0] > 0) & (out[..., 2] > 0)).any()
    assert not out[far_now, 0].any() and not out[near_now, 2].any()
    # the wall behind the strip's edges: its previous-frame position is covered by the strip there
    revealed = far_now & (count == 0)
    columns = np.unique(np.argwhere(revealed)[:, 1])
    edge_columns = [x for x in range(1, w - 1) if (near_now[:, x] != near_now[:, x + 1]).any() or (near_now[:, x] != near_now[:, x - 1]).any()]
    assert len(columns) and min(abs(int(c) - e) for c in columns for e in edge_columns) <= 1
    assert (count[near_now] == 4).sum() > near_now.sum() // 2 and (count[far_now] == 4).sum() > far_now.sum() // 2


def test_camera_behind_gives_all_zeros():
    prev_cam, previous, current = R.case(13, 9, "behind")
    previous.update(R.guides(R.CURRENT, 13, 9)[0])  # (planes that would pass every other test)
    color, count = R.reproject(prev_cam, previous, current, position_tolerance=1e3, normal_tolerance=4.0, max_history=8.0)
    assert not color.view(np.uint32).any() and not count.view(np.uint32).any()


def test_bad_previous_pixels_appear_nowhere():
    """Every finite previous mean is below 1000, the bad ones are NaN, infinite, or have no count: with one bad pixel among a tap's
    four the output stays finite and inside the range of the good ones."""
    for name in ("identical", "pan_fraction", "rotated"):
        prev_cam, previous, current = R.case(33, 9, name)
        n, c = previous["ray_nb"], previous["color"]
        bad = (n == 0) | ~np.isfinite(c).all(-1)
        assert bad.sum() >= 4 and np.isnan(c).any() and np.isinf(c).any()
        color, count = R.reproject(prev_cam, previous, current, **R.synthetic_params(33, 9))
        assert np.isfinite(color).all() and np.isfinite(count).all()
        with np.errstate(all="ignore"):
            top = np.where(bad[..., None], 0, c / n[..., None]).max()
        mean = color[count > 0] / count[count > 0][..., None]
        assert (count > 0).any() and (mean >= 0).all() and (mean <= top * (1 + 1e-6)).all()
        assert np.array_equal(count, np.floor(count)) and count.max() <= R.synthetic_params(33, 9)["max_history"]
        # and with the bad pixels repaired the output differs only around them
        repaired = dict(previous, color=np.where(bad[..., None], f32(1), c), ray_nb=np.where(bad, f32(1), n))
        other, _ = R.reproject(prev_cam, repaired, current, **R.synthetic_params(33, 9))
        assert not np.array_equal(other, color)


def test_constant_image_stays_constant():
    """Every previous mean is (0.5, 0.25, 2, 1) at varying counts: whatever is carried has that mean, to the rounding of a
    four-term weighted mean of equal values (sum of w*m over sum of w: 5 roundings each way, then * n) - a relative 2^-20."""
    value = np.array([0.5, 0.25, 2.0, 1.0], f32)
    for name in R.CAMERAS:
        prev_cam, previous, current = R.case(33, 9, name, odd=False)
        previous["color"] = (value * previous["ray_nb"][..., None]).astype(f32)
        color, count = R.reproject(prev_cam, previous, current, **R.synthetic_params(33, 9))
        kept = count > 0
        assert kept.any() or name == "behind"
        want = value.astype(np.float64) * count[kept][..., None]
        assert (np.abs(color[kept] - want) <= 2.0 ** -20 * want).all()
        assert not color[~kept].any()
