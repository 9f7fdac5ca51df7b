"""An exact yardstick for the arithmetic of a DTriPre record (csrc/scene_refit_common.h: make_tri_record_pre).

The serial model and the product share that header, so a wrong expression in it would be wrong on both sides of every other
comparison.  Here the record of a triangle is computed a second time in Python with exact rational arithmetic
(fractions.Fraction), every operation of the strict arithmetic rounded ONCE to binary32, round to nearest even: the six edge
subtractions, dot4 as the fma chain the kernels use (a0*b0 rounded, then three single-rounded fmas), uv*uv and uu*vv rounded
separately, their difference rounded, the correctly rounded reciprocal.  Every word of every triangle record of the model's layout
(build_layout, the function the upload runs) must equal it."""
from fractions import Fraction
import math
import struct

import numpy as np
import pytest

from opencl_pathtracer_amd import bvh_create, scenes
import scene_record_cases as R
import scene_update_cases as U

f32 = np.float32
OK = 0


# ---------------------------------------------------------------------------------------------- binary32, exactly

def round_f32(x, zero=0.0):
    """The binary32 nearest to the Fraction `x`, ties to even, as a Python float: subnormal results are exact, what lies beyond
    the largest finite value by half a unit or more is an infinity; `zero` (+0.0 or -0.0) is returned for x == 0."""
    if x == 0:
        return zero
    sign = -1.0 if x < 0 else 1.0
    a = -x if x < 0 else x
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1  # now 2^e <= a < 2^(e+1)
    q = max(e, -126) - 23  # the exponent of the last place
    n = a / Fraction(2) ** q
    m = n.numerator // n.denominator
    rest = n - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m & 1):
        m += 1
    if m * Fraction(2) ** q >= Fraction(2) ** 128:
        return sign * math.inf
    return sign * math.ldexp(float(m), q)  # exact: m <= 2^24, q >= -149


def _neg(a):
    return math.copysign(1.0, a) < 0


def sub(a, b):
    zero = -0.0 if (a == 0 and b == 0 and _neg(a) and not _neg(b)) else 0.0
    return round_f32(Fraction(a) - Fraction(b), zero)


def mul(a, b):
    return round_f32(Fraction(a) * Fraction(b), -0.0 if _neg(a) != _neg(b) else 0.0)


def fma(a, b, c):
    p = Fraction(a) * Fraction(b)
    zero = 0.0
    if p == 0 and c == 0 and (_neg(a) != _neg(b)) and _neg(c):
        zero = -0.0  # (-0) + (-0); every other exact zero of a sum is +0
    return round_f32(p + Fraction(c), zero)


def reciprocal(a):
    if a == 0:
        return math.copysign(math.inf, a)
    return round_f32(1 / Fraction(a), math.copysign(0.0, a))


def dot4(a, b):
    return fma(a[3], b[3], fma(a[2], b[2], fma(a[1], b[1], mul(a[0], b[0]))))


def exact_record(t):
    """The 16 words of the DTriPre record of triangle `t` (a structs.Triangle scalar): n | S1.xyz, dot4(N, S1) | u.xyz, 1 / (uv*uv -
    uu*vv) | v.xyz, S1.w"""
    s1, s2, s3, n = ([float(x) for x in t[k]] for k in ("S1", "S2", "S3", "N"))
    u = [sub(s2[k], s1[k]) for k in range(4)]
    v = [sub(s3[k], s1[k]) for k in range(4)]
    uv, uu, vv = dot4(u, v), dot4(u, u), dot4(v, v)
    den = reciprocal(sub(mul(uv, uv), mul(uu, vv)))
    rec = n + s1[:3] + [dot4(n, s1)] + u[:3] + [den] + v[:3] + [s1[3]]
    return np.frombuffer(struct.pack("<16f", *rec), np.uint32)


# ---------------------------------------------------------------------------------------------- the rounding itself

def test_rounding_is_single_where_a_detour_through_double_is_not():
    """x = 1 + 2^-24 + 2^-60 lies above the midpoint of 1 and 1 + 2^-23: binary32 takes the upper neighbour.  Rounded to double
    first it IS the midpoint, and the tie goes to 1."""
    x = 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert round_f32(x) == 1 + 2.0 ** -23
    assert float(f32(float(x))) == 1.0
    assert round_f32(-x) == -(1 + 2.0 ** -23)
    # the same in the subnormal range: 2^-149 * (1/2 + 2^-60) is nearer to 2^-149 than to 0; its double is exact here, the point
    # is the last place that no longer moves with the exponent
    tiny = Fraction(1, 2 ** 149)
    assert round_f32(tiny * (Fraction(1, 2) + Fraction(1, 2 ** 60))) == 2.0 ** -149
    assert round_f32(tiny / 2) == 0.0 and round_f32(tiny * 3 / 2) == 2.0 ** -148  # ties to even
    assert round_f32(tiny * Fraction(5, 2)) == 2.0 ** -148
    # an fma whose exact value needs more than a double: (1 + 2^-12)^2 + 2^-60 = 1 + 2^-11 + 2^-24 + 2^-60
    a = 1 + 2.0 ** -12
    assert fma(a, a, 2.0 ** -60) == 1 + 2.0 ** -11 + 2.0 ** -23
    assert float(f32(a * a + 2.0 ** -60)) == 1 + 2.0 ** -11


def test_rounding_equals_numpy_on_doubles():
    """numpy rounds a double to binary32 once and correctly: every double is a Fraction, so the two must agree - normal values,
    exact ties, the subnormal range, the overflow threshold, both signs."""
    rs = np.random.default_rng(5)
    values = list(rs.standard_normal(2000) * 2.0 ** rs.integers(-160, 140, 2000))
    for m in rs.integers(1, 2 ** 24, 300):  # ties, and their neighbours in double
        x = (int(m) + 0.5) * 2.0 ** int(rs.integers(-149, 100))
        values += [x, np.nextafter(x, 0), np.nextafter(x, np.inf), -x]
    big = float(np.finfo(f32).max)
    values += [big, big + 2.0 ** 102, np.nextafter(big + 2.0 ** 102, 0), big + 2.0 ** 103, 2.0 ** -150, np.nextafter(2.0 ** -150, 1), 2.0 ** -151]
    with np.errstate(over="ignore", under="ignore"):
        for x in values:
            x = float(x)
            want, got = float(f32(x)), round_f32(Fraction(x), math.copysign(0.0, x))
            assert got == want and _neg(got) == _neg(want), (x, got, want)


def test_signed_zeros_of_the_operations():
    z, nz = 0.0, -0.0
    with np.errstate(all="ignore"):
        for a in (z, nz, 1.5, -1.5):
            for b in (z, nz, 1.5, -1.5):
                assert struct.pack("<f", sub(a, b)) == struct.pack("<f", f32(a) - f32(b)), (a, b)
                assert struct.pack("<f", mul(a, b)) == struct.pack("<f", f32(a) * f32(b)), (a, b)
                for c in (z, nz, 2.25, -2.25):
                    assert struct.pack("<f", fma(a, b, c)) == struct.pack("<f", f32(math.fma(a, b, c) if hasattr(math, "fma") else a * b + c)), (a, b, c)


# ---------------------------------------------------------------------------------------------- the records

@pytest.fixture(scope="module")
def model(built):
    if R.model() is None:
        pytest.fail("oracle/build/libscene_refit_model.so not built (make -C oracle probe)", pytrace=False)
    return R.model()


def scene_of(tris):
    sc = scenes.cornell_box(R.W, R.H)
    sc.triangulation = scenes._concat_tris([tris])
    return bvh_create(sc)


def assert_records_exact(sc):
    lay = R.layout_in_mode(sc, generic=False)
    rows = np.flatnonzero(lay["tri_ids"] != R.NO_TRIANGLE)
    assert len(rows) == len(sc.triangulation) and sorted(lay["tri_ids"][rows]) == list(range(len(rows)))
    bad = []
    for r in rows:
        tid = int(lay["tri_ids"][r])
        want = exact_record(sc.triangulation[tid])
        for w in np.flatnonzero(lay["recs"][r] != want):
            bad.append(f"record {int(r)} (triangle {tid}) word {int(w)}: 0x{int(lay['recs'][r, w]):08x}, exact 0x{int(want[w]):08x}")
    assert not bad, f"{len(bad)} words differ:\n" + "\n".join(bad[:10])
    return len(rows)


def sample_of(name, n, seed):
    sc = R.scene(name)
    pick = np.sort(np.random.default_rng(seed).choice(len(sc.triangulation), n, replace=False))
    return scene_of(sc.triangulation[pick])


@pytest.mark.parametrize("name", ["cornell", "signed_zero-s0"])
def test_every_triangle_record_of_a_scene_is_exact(model, name):
    assert assert_records_exact(R.scene(name)) == len(R.scene(name).triangulation)


def test_a_seeded_2000_of_tris20k_are_exact(model):
    assert assert_records_exact(sample_of("tris20k", 2000, seed=9)) == 2000


def accepted(model, tris):
    """The triangles of `tris` that screen_update accepts, asked one at a time: an update of a one-triangle scene."""
    base = scene_of(scenes.triangle_create(f32([[0, 0, 0]]), f32([[1, 0, 0]]), f32([[0, 1, 0]])))
    keep = []
    for i in range(len(tris)):
        h = model.layout(base)
        rc, _, _ = model.update(h, tris[i:i + 1], 0)
        model.free(h)
        if rc == OK:
            keep.append(i)
    return tris[keep]


def with_normals_from_double(t):
    """N, N1, N2, N3 of the plane through the vertices, the cross product taken in double (triangle_create's, in float, loses
    it below 2^-63 and above 2^63)."""
    e1, e2 = (t["S2"] - t["S1"])[:, :3].astype(np.float64), (t["S3"] - t["S1"])[:, :3].astype(np.float64)
    n = np.cross(e1 / np.linalg.norm(e1, axis=1, keepdims=True), e2 / np.linalg.norm(e2, axis=1, keepdims=True))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    for field in ("N", "N1", "N2", "N3"):
        v = t[field].copy()
        v[:, :3] = n.astype(f32)
        t[field] = v
    return t


def slivers():
    """Near-degenerate triangles, hand-made: v = (1 + eps) u + delta p with p perpendicular to u and |p| = |u|.  The determinant
    uv^2 - uu.vv = -delta^2 |u|^4 is the difference of two numbers that agree in their first -2 log2(delta) bits."""
    rs = np.random.default_rng(12)
    a, b, c = [], [], []
    for delta_exp in range(2, 12):
        for eps in (0.0, 2.0 ** -7, -2.0 ** -3, 0.37):
            for scale in (1.0, 555.0, 2.0 ** -9):
                u = rs.standard_normal(3)
                p = np.cross(u, rs.standard_normal(3))
                p *= np.linalg.norm(u) / np.linalg.norm(p)
                s1 = rs.uniform(-2, 2, 3) * scale
                a.append(s1)
                b.append(s1 + u * scale)
                c.append(s1 + ((1 + eps) * u + 2.0 ** -delta_exp * p) * scale)
    # ... and axis-aligned ones, whose products are exact until the subtraction
    for k in range(2, 12):
        a.append([0, 0, 0])
        b.append([1, 0, 0])
        c.append([1 + 2.0 ** -k, 2.0 ** -k, 0])
    return scenes.triangle_create(f32(a), f32(b), f32(c))


def test_slivers_whose_dot_products_cancel_are_exact(model):
    tris = slivers()
    kept = accepted(model, tris)
    assert len(kept) >= len(tris) // 2, f"screen_update accepts {len(kept)} of {len(tris)}"
    sc = scene_of(kept)
    # the cancellation is there: the determinant of some is below 2^-18 of its terms
    t = sc.triangulation
    u, v = (t["S2"] - t["S1"]).astype(np.float64), (t["S3"] - t["S1"]).astype(np.float64)
    uv, uu, vv = (u * v).sum(1), (u * u).sum(1), (v * v).sum(1)
    assert (np.abs(uv * uv - uu * vv) < 2.0 ** -18 * uu * vv).sum() >= 10
    assert assert_records_exact(sc) == len(kept)


def by_edge_length(w):
    """Triangles with edges from 2^-20 to 2^20 (both edges alike, and one short against one long), vertex w = `w`."""
    rs = np.random.default_rng(21)
    a, b, c = [], [], []
    for ku in range(-20, 21, 2):
        for kv in (ku, -ku, ku // 2):
            u, v = rs.standard_normal(3), rs.standard_normal(3)
            u *= 2.0 ** ku / np.linalg.norm(u)
            v *= 2.0 ** kv / np.linalg.norm(v)
            s1 = rs.uniform(-1, 1, 3) * 2.0 ** min(max(ku, kv), 19)
            a.append(s1)
            b.append(s1 + u)
            c.append(s1 + v)
    with np.errstate(all="ignore"):
        t = with_normals_from_double(scenes.triangle_create(f32(a), f32(b), f32(c)))
    for field in ("S1", "S2", "S3"):
        p = t[field].copy()
        p[:, 3] = w
        t[field] = p
    U.recompute_aabb(t)
    return t


@pytest.mark.parametrize("w", [1.0, 0.0], ids=["w1", "w0"])
def test_edge_lengths_over_forty_binades_are_exact(model, w):
    tris = by_edge_length(w)
    kept = accepted(model, tris)
    assert len(kept) >= len(tris) * 3 // 4, f"screen_update accepts {len(kept)} of {len(tris)}"
    lengths = np.linalg.norm((kept["S2"] - kept["S1"])[:, :3].astype(np.float64), axis=1)
    assert lengths.min() < 2.0 ** -19 and lengths.max() > 2.0 ** 19
    assert (kept["S1"][:, 3] == w).all()
    assert assert_records_exact(scene_of(kept)) == len(kept)
