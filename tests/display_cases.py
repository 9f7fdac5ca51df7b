"""The yardstick of the display stage (test_display_model.py, test_display_gpu.py): the contract of include/ptmi.h, "displaying an
image", restated in NumPy.  No product code is involved.

Every float operation of the contract is one np.float32 operation on one line, in the written order; `_f` asserts that the
result is still float32, so that no line silently runs in double.  NumPy on the host keeps denormals and divides with correct
rounding, which is what the contract asks of the device.  The transfer tables come from the double formulae, evaluated here with
math.pow, independently of the product's generated file.
"""
import math

import numpy as np

f32 = np.float32
CLAMP, REINHARD, FILMIC = 0, 1, 2      # PTMI_TONE_*
LINEAR, SRGB, GAMMA22 = 0, 1, 2        # PTMI_TRANSFER_*
TONES, TRANSFERS = (CLAMP, REINHARD, FILMIC), (LINEAR, SRGB, GAMMA22)
WORDS = 260                            # PTMI_LUMINANCE_WORDS


def _f(a):
    assert a.dtype == np.float32, a.dtype
    return a


# ---------------------------------------------------------------------------------------------- the tables

def eotf(transfer, v):
    """encoded value in [0, 1] -> linear value, in double"""
    if transfer == LINEAR:
        return v
    if transfer == SRGB:
        return v / 12.92 if v <= 0.04045 else math.pow((v + 0.055) / 1.055, 2.4)
    assert transfer == GAMMA22
    return math.pow(v, 2.2)


_tables = {}


def tables():
    """{transfer: float32[256]}: T[0] = 0, T[k] = (float) EOTF((k - 0.5) / 255.0)"""
    if not _tables:
        for transfer in TRANSFERS:
            t = np.array([0.0] + [eotf(transfer, (k - 0.5) / 255.0) for k in range(1, 256)], np.float64).astype(f32)
            t.setflags(write=False)
            _tables[transfer] = t
    return _tables


# ---------------------------------------------------------------------------------------------- the arithmetic

def mean(color, count):
    """step 1: float32[H, W, 3].  count None: `color` is a mean plane (its fourth word is ignored)"""
    c = _f(np.asarray(color)[..., :3])
    if count is None:
        return c.copy()
    n = _f(np.asarray(count))[..., None]
    with np.errstate(all="ignore"):
        q = _f(c / n)
    return _f(np.where(n > 0, q, f32(0)))


def tone(x, operator, white=np.inf):
    """step 3 on exposed values x >= 0: t = min(operator(x), 1)"""
    one = f32(1)
    with np.errstate(all="ignore"):
        if operator == CLAMP:
            t = x
        elif operator == REINHARD:
            w2 = f32(white) * f32(white)
            assert type(w2) is f32
            a = _f(x / w2)
            a = _f(one + a)
            a = _f(x * a)
            b = _f(one + x)
            t = _f(a / b)
        else:
            assert operator == FILMIC
            a = _f(f32(2.51) * x)
            a = _f(a + f32(0.03))
            a = _f(x * a)
            b = _f(f32(2.43) * x)
            b = _f(b + f32(0.59))
            b = _f(x * b)
            b = _f(b + f32(0.14))
            t = _f(a / b)
        return _f(np.where(t < one, t, one))  # min(a, b) = a < b ? a : b: a NaN becomes 1


def tonemap(color, count, params):
    """steps 1 to 4: uint8[H, W, 3] = r, g, b.  params: dict(tone, transfer, exposure, white)"""
    m = mean(color, count)
    with np.errstate(all="ignore"):
        x = _f(m * f32(params.get("exposure", 1.0)))
    x = _f(np.where(x > 0, x, f32(0)))  # NaN and negative values go to 0
    t = tone(x, params["tone"], params.get("white", np.inf))
    T = tables()[params["transfer"]]
    return np.searchsorted(T[1:], t, side="right").astype(np.uint8)  # the largest k with T[k] <= t


def pack_bgr24(rgb, row_stride):
    h, w, _ = rgb.shape
    assert 3 * w <= row_stride <= 3 * w + 3
    rows = np.zeros((h, row_stride), np.uint8)
    rows[:, :3 * w] = rgb[..., ::-1].reshape(h, 3 * w)
    return rows


def pack_rgba32(rgb):
    h, w, _ = rgb.shape
    return np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], -1)


def luminance(color, count):
    m = mean(color, count)
    with np.errstate(all="ignore"):
        a = _f(f32(0.2126) * m[..., 0])
        b = _f(f32(0.7152) * m[..., 1])
        a = _f(a + b)
        b = _f(f32(0.0722) * m[..., 2])
        return _f(a + b)


def histogram(color, count):
    """uint32[260]: quarter-octave bins of the positive finite luminances, then the not-positive ones, the infinite ones, 0, 0"""
    Y = luminance(color, count).ravel()
    positive = Y > 0
    infinite = Y == np.inf
    binned = positive & ~infinite
    bins = np.clip((Y[binned].view(np.uint32) >> 21).astype(np.int64) - 380, 0, 255)
    out = np.zeros(WORDS, np.uint32)
    out[:256] = np.bincount(bins, minlength=256)
    out[256] = np.count_nonzero(~positive)
    out[257] = np.count_nonzero(infinite)
    return out


def bin_start(b):
    """where bin b of the histogram starts (bin 128: 1.0)"""
    return (1 + (b & 3) / 4) * 2.0 ** ((b >> 2) - 32)


# ---------------------------------------------------------------------------------------------- synthetic planes

def threshold_values():
    """For every k of every transfer: T[k], its predecessor and its successor in float32 (T[0] = 0: -0, its predecessor in
    the order of the bits that still compares equal to it, stands in for a value below it, with the smallest denormal above)."""
    out = []
    for transfer in TRANSFERS:
        T = tables()[transfer]
        for k in range(256):
            below = f32(-0.0) if k == 0 else np.nextafter(T[k], f32(-1))
            out += [below, T[k], np.nextafter(T[k], f32(2))]
    return np.array(out, f32)


SPECIALS = np.array([0.0, -0.0, -1.5, -1e-30, np.nan, np.inf, -np.inf, 1e-40, 1.4e-45, 3.0e38], f32)   # (two denormals)
COUNTS = np.array([0.0, -0.0, -2.0, np.nan, 1.0, 1.0, 3.0, 1e6, 16777216.0, np.inf, 1e-40], f32)


def synthetic(w, h, seed):
    """(color float32[H, W, 4], count float32[H, W]).  Read as sums with the counts, or as means without them.
      * threshold pixels, up to half of the image and up to all 768: count 1, and in the three channels three consecutive values
        of threshold_values() (768 x 3 = the whole list), so that with exposure 1 and CLAMP t = x = the value exactly, in either
        form.  An image too small for the whole list takes a stretch of it that starts with the seed;
      * special pixels, an eighth of the rest: SPECIALS in one or more channels, any count of COUNTS;
      * ordinary pixels: means spread over 2^-40 .. 2^40 (half of them) or over 0 .. 2 where the tone curves bend (the other
        half), times a count of 1 .. 4096 or, now and then, a count of COUNTS.
    The fourth word of the colour is noise, NaNs included: nothing may read it."""
    rng = np.random.default_rng(seed)
    npix = w * h
    color = np.empty((npix, 4), f32)
    count = rng.integers(1, 4097, npix).astype(f32)
    wide = np.ldexp(rng.uniform(1.0, 2.0, (npix, 3)), rng.integers(-40, 41, (npix, 3))).astype(f32)
    bend = rng.uniform(0.0, 2.0, (npix, 3)).astype(f32)
    color[:, :3] = np.where(rng.random((npix, 1)) < 0.5, wide, bend) * count[:, None]
    odd = rng.random(npix) < 0.1
    count[odd] = rng.choice(COUNTS, int(odd.sum()))
    order = rng.permutation(npix)
    values = threshold_values()
    n_threshold = min(len(values) // 3, npix // 2)
    first = seed % (len(values) // 3)
    for i, p in enumerate(order[:n_threshold]):
        k = (first + i) % (len(values) // 3)
        color[p, :3] = values[3 * k:3 * k + 3]
        count[p] = 1
    rest = order[n_threshold:]
    special = rest[:max(len(rest) // 8, min(len(rest), 1))]
    for p in special:
        channels = rng.random(3) < 0.5
        channels[rng.integers(0, 3)] = True
        color[p, :3][channels] = rng.choice(SPECIALS, int(channels.sum()))
        count[p] = rng.choice(COUNTS)
    color[:, 3] = rng.choice(np.array([np.nan, 0.0, 7.0, -np.inf], f32), npix)
    return color.reshape(h, w, 4), count.reshape(h, w)
