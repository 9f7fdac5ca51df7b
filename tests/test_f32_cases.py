"""f32_cases.py against itself and against the oracle: the float64 fast path of its fused multiply-add equals the path through
exact fractions, and its camera expression gives the ray whose first hit pto_trace_path records."""
import numpy as np

import f32_cases as F
import guide_cases as G

f32 = np.float32


def assert_both_paths(a, b, c, want=None):
    fast, exact = F.fma(a, b, c), F.fma(a, b, c, exact=True)
    assert F.bits(fast) == F.bits(exact), (a, b, c, fast, exact)
    if want is not None:
        assert F.bits(fast) == F.bits(want) or (np.isnan(want) and np.isnan(fast)), (a, b, c, fast, want)


def test_fma_fast_path_equals_exact_fractions_on_random_triples():
    """100 000 triples of magnitudes 2^-20 .. 2^20; every fourth has c within a few ulps of -(a * b), which cancels."""
    rs = np.random.default_rng(20)
    n = 100000
    a, b, c = ((rs.uniform(1, 2, n) * 2.0 ** rs.integers(-20, 21, n) * rs.choice([-1, 1], n)).astype(f32) for _ in range(3))
    near = (-(a.astype(np.float64) * b.astype(np.float64))).astype(f32)
    c[::4] = (near.view(np.int32) + rs.integers(-2, 3, n).astype(np.int32)).view(f32)[::4]
    cancelled = 0
    for x, y, z in zip(a, b, c):
        assert_both_paths(x, y, z)
    with np.errstate(all="ignore"):
        cancelled = int((np.abs(a.astype(np.float64) * b + c) < 1e-6 * np.abs(c))[::4].sum())
    assert cancelled > 20000


def test_fma_constructed_cases():
    one, ulp = f32(1), f32(2.0 ** -23)
    # exact halfway sums: 1 * (1 + k ulp) + ulp / 2 lies between 1 + k ulp and 1 + (k + 1) ulp; ties go to the even neighbour
    assert_both_paths(one, f32(1 + 2.0 ** -23 * 2), ulp / 2, want=f32(1 + 2.0 ** -23 * 2))  # lower neighbour even: stays
    assert_both_paths(one, f32(1 + 2.0 ** -23), ulp / 2, want=f32(1 + 2.0 ** -23 * 2))      # lower neighbour odd: goes up
    # ... and with a product that float32 cannot hold: (1 + ulp)^2 = 1 + 2 ulp + ulp^2, plus what brings it half way
    x = f32(1 + 2.0 ** -23)
    assert_both_paths(x, x, f32(2.0 ** -24) - f32(2.0 ** -46), want=f32(1 + 2.0 ** -23 * 2))
    assert_both_paths(x, x, f32(2.0 ** -24 * 3) - f32(2.0 ** -46), want=f32(1 + 2.0 ** -23 * 4))
    # an exact zero sum: +0, unless the product and the addend are both -0
    for sa in (1, -1):
        for sc in (1, -1):
            assert_both_paths(f32(sa * 1.5), f32(2), f32(-sa * 3), want=f32(0.0))
            assert_both_paths(f32(sa * 0.0), f32(2), f32(sc * 0.0), want=f32(-0.0) if sa < 0 and sc < 0 else f32(0.0))
            assert_both_paths(f32(sa * 0.0), f32(-2), f32(sc * 0.0), want=f32(-0.0) if sa > 0 and sc < 0 else f32(0.0))
    # results below 1e-30, down into the subnormals, where float32's halfway points lie elsewhere in a float64
    tiny = f32(2.0 ** -126)
    assert_both_paths(f32(2.0 ** -70), f32(2.0 ** -70), f32(0), want=f32(2.0 ** -140))
    assert_both_paths(tiny, f32(0.5), f32(2.0 ** -149), want=f32(2.0 ** -127 + 2.0 ** -149))
    assert_both_paths(f32(2.0 ** -149), f32(0.5), f32(0), want=f32(0.0))                 # half way between 0 and the least: even
    assert_both_paths(f32(2.0 ** -149), f32(1.5), f32(0), want=f32(2.0 ** -148))         # half way between 1 and 2 least: even
    assert_both_paths(f32(3e-20), f32(-3e-20), f32(1e-39), want=None)
    # an infinite operand
    inf = f32(np.inf)
    with np.errstate(all="ignore"):
        assert_both_paths(inf, f32(2), f32(1), want=inf)
        assert_both_paths(f32(-3), inf, f32(1), want=-inf)
        assert_both_paths(f32(2), f32(2), -inf, want=-inf)
        assert_both_paths(inf, f32(0), f32(1), want=f32(np.nan))
        assert_both_paths(inf, f32(1), -inf, want=f32(np.nan))


def test_camera_direction_gives_the_ray_of_the_oracles_first_bounce(built):
    """Cornell at 16 x 12, iterations 0 and 7, both arithmetics: the triangle pto_trace_path hit accepts the ray made with
    camera_direction at the record's s, t and point, bit for bit (the self-check of guide_cases.Yardstick)."""
    w, h = 16, 12
    from gpu_cases import cached_scene
    sc = cached_scene("cornell", w, h)
    for fused in (False, True):
        y = G.Yardstick(sc, w, h, default_arithmetic=fused)
        hits = 0
        for it in (0, 7):
            for gy in range(h):
                for gx in range(w):
                    s = y.sample(gx, gy, it)
                    if s["hit"]:
                        y.side_by_primary_ray(s["triangle_id"], s["s"], s["t"], s["point"], gx, gy, it)
                        hits += 1
        assert hits > 300
