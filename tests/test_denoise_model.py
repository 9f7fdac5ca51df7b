"""ptmi_denoise without a GPU: the new ABI is held against the header, the entry points validate their arguments, the yardstick
of the GPU tests (denoise_cases.py) is held against a second, scalar restatement of the contract, and the properties that make
the contract a denoiser are checked on the yardstick."""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import backend
from abi_cases import declared_symbols, exported_symbols, header_values
import denoise_cases as D

NEW_SYMBOLS = {"ptmi_denoise", "ptmi_denoise_device"}
f32 = np.float32


# ---------------------------------------------------------------------------------------------- ABI

def test_header_binding_list_and_library_agree(built):
    declared = set(declared_symbols())
    assert NEW_SYMBOLS <= declared and declared == set(backend.ABI_SYMBOLS)
    assert NEW_SYMBOLS <= exported_symbols()
    assert backend.load_library().ptmi_abi_version() == 4


LAYOUT = ['VALUE("sizeof", sizeof(ptmi_denoise_params));', 'VALUE("demodulate", PTMI_DENOISE_DEMODULATE_ALBEDO);',
          'VALUE("untiled", PTMI_DENOISE_UNTILED);'] + [
    f'VALUE("{field}", offsetof(ptmi_denoise_params, {field}));' for field in
    "struct_size passes flags guide_first_iteration guide_iterations sigma_color sigma_normal sigma_position reserved".split()]


def test_ctypes_struct_matches_the_header():
    out = header_values(LAYOUT)
    want = {"sizeof": C.sizeof(backend.DenoiseParams), "demodulate": backend.DENOISE_DEMODULATE_ALBEDO, "untiled": backend.DENOISE_UNTILED}
    want.update({name: getattr(backend.DenoiseParams, name).offset for name, _ in backend.DenoiseParams._fields_})
    assert out == want
    assert C.sizeof(backend.DenoiseParams) == 40 and D.DEMODULATE == backend.DENOISE_DEMODULATE_ALBEDO


def test_default_parameters_are_a_point_of_the_committed_grid():
    d = backend.DENOISE_DEFAULTS
    assert d["passes"] == 5
    assert d["sigma_color"] in D.GRID_SIGMA_COLOR and d["sigma_normal"] in D.GRID_SIGMA_NORMAL and d["sigma_position"] in D.GRID_SIGMA_POSITION
    p = backend.Backend.denoise_params()
    assert (p.struct_size, p.passes, p.flags, p.guide_first_iteration, p.guide_iterations) == (40, 5, 1, 0, 1)
    assert (p.sigma_color, p.sigma_normal, p.sigma_position) == tuple(f32(d[k]) for k in ("sigma_color", "sigma_normal", "sigma_position"))
    assert list(p.reserved) == [0, 0]


def test_argument_validation_needs_no_gpu(built):
    lib = backend.load_library()
    good = backend.Backend.denoise_params()
    bad = backend.Backend.denoise_params(passes=6)
    bad.struct_size -= 8
    guides = backend.Guides(C.sizeof(backend.Guides), 0)
    image = np.zeros((2, 2, 4), f32)
    for p in (C.byref(good), C.byref(bad), None):  # a NULL context: refused for good and bad parameters alike
        assert lib.ptmi_denoise(None, p, image.ctypes.data_as(C.c_void_p)) == -1
        assert lib.ptmi_denoise(None, p, None) == -1
        assert lib.ptmi_denoise_device(None, p, C.byref(guides), None, None, None) == -1
        assert lib.ptmi_denoise_device(None, p, None, 256, 256, 256) == -1


# ---------------------------------------------------------------------------------------------- the yardstick against a second restatement

def scalar_denoise(planes, passes, flags, guide_iterations, sigma_color, sigma_normal, sigma_position):
    """The contract once more, one pixel and one tap at a time in np.float32 scalars, written from ptmi.h and sharing nothing
    with denoise_cases.denoise but the three spline weights."""
    color, ray_nb, albedo, normal, position, hit_count = (planes[k] for k in ("color", "ray_nb", "albedo", "normal", "position", "hit_count"))
    height, width = ray_nb.shape
    zero, one = f32(0), f32(1)

    def sq(a, b):
        x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return (x * x + y * y) + z * z

    e, d, hit, nrm, pos = {}, {}, {}, {}, {}
    G = f32(guide_iterations)
    for y in range(height):
        for x in range(width):
            n = ray_nb[y, x]
            m = [color[y, x, c] / n for c in range(3)] if n > 0 else [zero] * 3
            a = [albedo[y, x, c] / G for c in range(3)]
            h = hit_count[y, x]
            hit[y, x] = bool(h > 0)
            nrm[y, x] = [normal[y, x, c] / h for c in range(3)] if h > 0 else [zero] * 3
            pos[y, x] = [position[y, x, c] / h for c in range(3)] if h > 0 else [zero] * 3
            d[y, x] = [(v if v > f32(1e-3) else f32(1e-3)) for v in a] if flags & 1 else [one] * 3
            e[y, x] = [m[c] / d[y, x][c] for c in range(3)]
    for k in range(passes):
        s = 1 << k
        inv_c = f32(1 << (2 * k)) / (f32(sigma_color) * f32(sigma_color))
        inv_n = one / (f32(sigma_normal) * f32(sigma_normal))
        inv_p = one / (f32(sigma_position) * f32(sigma_position))
        nxt = {}
        for y in range(height):
            for x in range(width):
                sw, se = zero, [zero] * 3
                for dy in (-2, -1, 0, 1, 2):
                    for dx in (-2, -1, 0, 1, 2):
                        qx, qy = x + s * dx, y + s * dy
                        if not (0 <= qx < width and 0 <= qy < height) or hit[qy, qx] != hit[y, x]:
                            continue
                        b = D.B[abs(dy)] * D.B[abs(dx)]
                        xc = sq(e[qy, qx], e[y, x]) * inv_c
                        xn = sq(nrm[qy, qx], nrm[y, x]) * inv_n
                        xp = sq(pos[qy, qx], pos[y, x]) * inv_p
                        w = b / (((one + xc) * (one + xn)) * (one + xp))
                        if not w > 0:
                            continue
                        sw = sw + w
                        se = [se[c] + w * e[qy, qx][c] for c in range(3)]
                nxt[y, x] = [se[c] / sw for c in range(3)] if sw > 0 else e[y, x]
        e = nxt
    out = np.zeros((height, width, 4), f32)
    for (y, x), v in e.items():
        out[y, x] = [v[0] * d[y, x][0], v[1] * d[y, x][1], v[2] * d[y, x][2], ray_nb[y, x]]
    return out


@pytest.mark.parametrize("flags", [0, 1], ids=["plain", "demodulated"])
def test_yardstick_equals_a_scalar_restatement(flags):
    planes, g = D.synthetic(13, 9, seed=5)
    assert np.isnan(planes["color"]).any() or np.isinf(planes["color"]).any()
    assert (planes["ray_nb"] == 0).any() and (planes["hit_count"] == 0).any() and (planes["hit_count"] > 0).any()
    with np.errstate(all="ignore"):
        want = scalar_denoise(planes, 5, flags, g, **D.SYNTHETIC_SIGMAS)
    got = D.denoise(**planes, passes=5, flags=flags, guide_iterations=g, **D.SYNTHETIC_SIGMAS)
    assert not D.describe_difference(got, want)
    assert not np.array_equal(got.view(np.uint32), D.denoise(**planes, passes=0, flags=flags, guide_iterations=g).view(np.uint32))


# ---------------------------------------------------------------------------------------------- what makes the contract a denoiser

def flat_planes(width, height, value=0.5, hit=1.0, albedo=1.0):
    return dict(color=np.full((height, width, 4), value, f32), ray_nb=np.ones((height, width), f32),
                albedo=np.full((height, width, 4), albedo, f32), normal=np.tile(f32([0, 0, hit, 0]), (height, width, 1)),
                position=np.zeros((height, width, 4), f32), hit_count=np.full((height, width), hit, f32))


@pytest.mark.parametrize("flags", [0, 1])
def test_no_passes_return_the_demodulated_mean_times_its_divisor(flags):
    planes, g = D.synthetic(33, 9, seed=2)
    e0, d, n, _, _, _ = D.prepass(**planes, guide_iterations=g, flags=flags)
    with np.errstate(all="ignore"):
        want = np.concatenate([e0 * d, n[..., None]], -1)
    assert not D.describe_difference(D.denoise(**planes, passes=0, flags=flags, guide_iterations=g), want)
    if not flags:  # d = 1: the plain mean, and 0 where nothing was sampled
        with np.errstate(all="ignore"):
            mean = np.where((n > 0)[..., None], planes["color"][..., :3] / n[..., None], f32(0))
        assert not D.describe_difference(want[..., :3], mean)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_pixel_that_is_not_a_number_keeps_its_words_and_reaches_nobody(bad):
    """Against the same input with that pixel replaced by its left neighbour: the bad pixel's own words stay what e0 * d makes of
    them, and every pixel outside the replaced pixel's reach differs nowhere - inside it (any pixel the replacement could have
    fed) the bad pixel must have had weight 0, which is what the second assertion pins: the result with the bad pixel equals the
    result with that pixel struck from every footprint, modelled by a one-pixel hole in the hit mask."""
    rng = np.random.default_rng(11)
    planes = flat_planes(40, 24)
    planes["color"] = (planes["color"] + rng.random((24, 40, 4)).astype(f32) * f32(0.1)).astype(f32)
    y, x = 12, 20
    with_bad = {k: v.copy() for k, v in planes.items()}
    with_bad["color"][y, x, 1] = bad
    out = D.denoise(**with_bad, passes=5, flags=1, sigma_color=0.5)
    e0 = D.denoise(**with_bad, passes=0, flags=1)
    assert np.array_equal(out[y, x].view(np.uint32), e0[y, x].view(np.uint32)) or (np.isnan(bad) and np.isnan(out[y, x, 1]) and
                                                                                  np.array_equal(out[y, x, [0, 2, 3]], e0[y, x, [0, 2, 3]]))
    # struck from every footprint: the same planes with that pixel alone on the other side of the hit mask
    struck = {k: v.copy() for k, v in planes.items()}
    struck["hit_count"][y, x] = 0
    reference = D.denoise(**struck, passes=5, flags=1, sigma_color=0.5)
    others = np.ones((24, 40), bool)
    others[y, x] = False
    assert np.array_equal(out[others].view(np.uint32), reference[others].view(np.uint32))
    # ... while a finite replacement (the left neighbour's value) does reach its neighbours
    replaced = {k: v.copy() for k, v in planes.items()}
    replaced["color"][y, x] = replaced["color"][y, x - 1]
    assert not np.array_equal(D.denoise(**replaced, passes=5, flags=1, sigma_color=0.5)[others], out[others])
    assert np.isfinite(out[others]).all()


def test_no_value_crosses_the_hit_mask():
    """Two constant regions split by the mask each stay constant, to the rounding bound of a 25-term weighted mean.

    The bound.  Inside a region every accepted tap has e_q = c (the region's constant) and, the guides being constant too, xc =
    xn = xp = 0 exactly, so w = b exactly (b / 1).  With u = 2^-24: each product w * c carries one rounding, (1 + u); each of the
    at most 25 additions of se and of sw one more, so se = c * sum(w) * (1 + t1), |t1| <= 26 u, and sw = sum(w) * (1 + t2),
    |t2| <= 25 u - in fact t2 = 0 here, the partial sums of the spline weights being multiples of 2^-8 below 2 - and the division
    one more: |e' - c| <= 27 u |c| to first order.  A pass feeds the next one values within that bound of c, for which xc is of
    the order of (27 u c)^2 / sigma^2, far below u: the weights stay b to within an ulp or two and the mean of values within
    delta of c stays within delta + 27 u |c| + (a few u) |c|.  Five passes: 5 * 30 u |c| is asserted, relative."""
    width, height = 48, 32
    planes = flat_planes(width, height)
    yy, xx = np.mgrid[0:height, 0:width]
    miss = (xx + yy // 3) % 16 < 6  # a slanted, striped mask: every footprint at every step straddles it somewhere
    planes["hit_count"][miss] = 0
    planes["normal"][miss] = 0
    c_hit, c_miss = f32(0.7231), f32(13.37)
    planes["color"][~miss] = c_hit
    planes["color"][miss] = c_miss
    passes = []
    D.denoise(**planes, passes=5, flags=0, every_pass=passes)
    bound = 5 * 30 * 2.0 ** -24
    for e in passes:
        assert np.abs(e[~miss].astype(np.float64) / float(c_hit) - 1).max() <= bound
        assert np.abs(e[miss].astype(np.float64) / float(c_miss) - 1).max() <= bound


def test_every_pass_lowers_the_variance_of_a_noisy_flat_region():
    rng = np.random.default_rng(3)
    planes = flat_planes(64, 48)
    planes["color"][..., :3] = (f32(0.5) + (rng.random((48, 64, 3)).astype(f32) - f32(0.5)) * f32(0.2)).astype(f32)
    passes = []
    D.denoise(**planes, passes=5, flags=1, sigma_color=0.5, every_pass=passes)
    variances = [float(np.var(e.astype(np.float64))) for e in passes]
    assert len(variances) == 6 and all(b < a for a, b in zip(variances, variances[1:])), variances
    assert variances[-1] < 0.05 * variances[0]
