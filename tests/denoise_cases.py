"""The yardstick of ptmi_denoise (test_denoise_model.py, test_denoise_gpu.py): the filter's arithmetic as ptmi.h and DESIGN 1e
state it, in NumPy float32, vectorised over the pixels with a Python loop over taps and passes.  No product code is involved.
Every intermediate is an np.float32 array (or scalar), so no operation is promoted, and every line is one IEEE binary32
operation per pixel in the written order.  Below it: the generators of the synthetic planes the tests filter, and the grid of
sigmas the shipped defaults are held against."""
import numpy as np

f32 = np.float32
DEMODULATE = 1  # PTMI_DENOISE_DEMODULATE_ALBEDO
B = (f32(0.375), f32(0.25), f32(0.0625))
ZERO, ONE, FLOOR = f32(0), f32(1), f32(1e-3)


def dot3(v):
    """(v.x*v.x + v.y*v.y) + v.z*v.z over the last axis"""
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def prepass(color, ray_nb, albedo, normal, position, hit_count, guide_iterations, flags):
    """-> e0[H,W,3], d[H,W,3], n[H,W], hit[H,W] (bool), nrm[H,W,3], pos[H,W,3]"""
    color, ray_nb, albedo, normal, position, hit_count = (np.asarray(a, f32) for a in (color, ray_nb, albedo, normal, position, hit_count))
    with np.errstate(all="ignore"):
        n = ray_nb
        m = np.where((n > 0)[..., None], color[..., :3] / n[..., None], ZERO).astype(f32)
        a = albedo[..., :3] / f32(guide_iterations)
        h = hit_count
        hit = h > 0
        nrm = np.where(hit[..., None], normal[..., :3] / h[..., None], ZERO).astype(f32)
        pos = np.where(hit[..., None], position[..., :3] / h[..., None], ZERO).astype(f32)
        d = np.where(a > FLOOR, a, FLOOR).astype(f32) if flags & DEMODULATE else np.ones_like(a)
        e0 = m / d
    assert all(x.dtype == f32 for x in (m, a, nrm, pos, d, e0))
    return e0, d, n, hit, nrm, pos


def one_pass(e, hit, nrm, pos, k, sigma_color, sigma_normal, sigma_position):
    """e(k) -> e(k+1)"""
    height, width = hit.shape
    s = 1 << k
    inv_c = f32(1 << (2 * k)) / (f32(sigma_color) * f32(sigma_color))
    inv_n = ONE / (f32(sigma_normal) * f32(sigma_normal))
    inv_p = ONE / (f32(sigma_position) * f32(sigma_position))
    sw = np.zeros((height, width), f32)
    se = np.zeros((height, width, 3), f32)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                # the pixels p whose tap q = p + s * (dx, dy) lies inside the image
                y0, y1 = max(0, -s * dy), min(height, height - s * dy)
                x0, x1 = max(0, -s * dx), min(width, width - s * dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                b = B[abs(dy)] * B[abs(dx)]
                xc = dot3(e[Q] - e[P]) * inv_c
                xn = dot3(nrm[Q] - nrm[P]) * inv_n
                xp = dot3(pos[Q] - pos[P]) * inv_p
                w = b / (((ONE + xc) * (ONE + xn)) * (ONE + xp))
                assert w.dtype == f32
                taken = (hit[Q] == hit[P]) & (w > 0)
                sw[P] = np.where(taken, sw[P] + w, sw[P])
                se[P] = np.where(taken[..., None], se[P] + w[..., None] * e[Q], se[P])
        out = np.where((sw > 0)[..., None], se / sw[..., None], e)
    assert out.dtype == f32
    return out


def denoise(color, ray_nb, albedo, normal, position, hit_count, passes, flags=DEMODULATE, guide_iterations=1, sigma_color=1.0,
            sigma_normal=1.0, sigma_position=1.0, every_pass=None):
    """out[H,W,4] = (e * d, n).  every_pass: a list that receives e(0), e(1), ... e(passes)."""
    e, d, n, hit, nrm, pos = prepass(color, ray_nb, albedo, normal, position, hit_count, guide_iterations, flags)
    if every_pass is not None:
        every_pass.append(e)
    for k in range(passes):
        e = one_pass(e, hit, nrm, pos, k, sigma_color, sigma_normal, sigma_position)
        if every_pass is not None:
            every_pass.append(e)
    with np.errstate(all="ignore"):
        out = np.concatenate([e * d, n[..., None]], axis=-1)
    assert out.dtype == f32
    return out


def describe_difference(got, want):
    """'' where every word is equal; a NaN in `want` asks for a NaN, sign and payload left open"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    if got.shape != want.shape:
        return f"shape {got.shape}, not {want.shape}"
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if same.all():
        return ""
    bad = np.argwhere(~same)
    y, x, c = (int(v) for v in bad[0])
    return f"{len(bad)} words differ of {same.size}; first at (x={x}, y={y}, c={c}): got {got[y, x, c]!r}, want {want[y, x, c]!r}"


# ---------------------------------------------------------------------------------------------- synthetic planes

def synthetic(width, height, seed, guide_iterations=3):
    """Seeded planes that take every branch of the filter: colour sums over several decades; about 2 % of the pixels with a zero
    count; about 1 % with a NaN or an infinite channel; a random blocky hit mask; zero albedo in places; normals and positions
    that are smooth inside a block and jump between blocks.  -> dict(color, ray_nb, albedo, normal, position, hit_count)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    block = (yy // 5) * 1000 + xx // 7
    per_block = rng.random(1000 * (height // 5 + 1) + width // 7 + 1)
    n = rng.integers(1, 9, (height, width)).astype(f32)
    n[rng.random((height, width)) < 0.02] = 0
    decades = f32(10.0) ** rng.integers(-3, 3, (height, width, 1)).astype(f32)
    color = (rng.random((height, width, 4)).astype(f32) * decades * n[..., None]).astype(f32)
    odd = rng.random((height, width)) < 0.01
    kinds = np.array([np.nan, np.inf, -np.inf], f32)
    for y, x in np.argwhere(odd):
        color[y, x, rng.integers(0, 3)] = kinds[rng.integers(0, 3)]
    if width * height >= 15:  # (a small image has one of each kind all the same)
        for kind in kinds:
            color[rng.integers(0, height), rng.integers(0, width), rng.integers(0, 3)] = kind
        n[rng.integers(0, height), rng.integers(0, width)] = 0
    g = f32(guide_iterations)
    hits = np.where(per_block[block] < 0.3, 0, rng.integers(1, guide_iterations + 1, (height, width))).astype(f32)
    if width * height > 1:
        hits.flat[rng.integers(0, hits.size)] = 0  # (at least one miss, one hit where there is room for both)
        hits.flat[rng.integers(0, hits.size)] = g
    albedo = (rng.random((height, width, 4)).astype(f32) * g).astype(f32)
    albedo[per_block[block] > 0.9] = 0
    albedo[rng.random((height, width)) < 0.01, 1] = np.nan
    tilt = (per_block[block] * 6.0).astype(f32)
    normal = np.stack([np.cos(tilt), np.sin(tilt), f32(0.01) * xx, np.zeros_like(tilt)], -1).astype(f32) * hits[..., None]
    position = np.stack([f32(0.1) * xx, f32(0.1) * yy, (per_block[block] * 4.0), np.ones_like(tilt)], -1).astype(f32) * hits[..., None]
    position = (position + rng.random((height, width, 4)).astype(f32) * f32(0.01)).astype(f32)
    return dict(color=color, ray_nb=n, albedo=albedo, normal=normal.astype(f32), position=position, hit_count=hits), guide_iterations


SYNTHETIC_SIGMAS = dict(sigma_color=0.7, sigma_normal=0.4, sigma_position=0.9)

# ---------------------------------------------------------------------------------------------- the defaults' grid

# The shipped defaults (backend.DENOISE_DEFAULTS) must be the RMSE minimum over this grid on the Cornell box at 64 x 48, 4 spp
# against 1024 spp, passes = 5 and demodulation on (test_denoise_gpu.py::test_defaults_are_the_grids_minimum).
# What spans it: sigma_position is in scene units, and that box is 555 units wide - neighbouring pixels of a 64-pixel row lie
# about 10 units apart on its walls, a step-16 tap 160 - so from 4 units (hardly a neighbour counts) to 4096 (position says
# nothing); unit normals are at most 2 apart, so from 0.25 to 4 (normals say nothing); the demodulated colours are of order 1, so
# from a quarter of that to 16 (colour says nothing).
GRID_SIGMA_COLOR = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
GRID_SIGMA_NORMAL = (0.25, 0.5, 1.0, 2.0, 4.0)
GRID_SIGMA_POSITION = (4.0, 16.0, 64.0, 256.0, 1024.0, 4096.0)


def rmse(image, truth):
    """root mean square error of the r, g, b means, in float64"""
    a, b = np.asarray(image, np.float64)[..., :3], np.asarray(truth, np.float64)[..., :3]
    return float(np.sqrt(np.mean((a - b) ** 2)))
