"""csrc/leaf_cull.h: box_distance2_from_slabs, which the kernel's box tests evaluate on their own slab differences, IS
box_distance2, which the culling's proof speaks of - bit for bit, for every ordered box (lo <= hi) and either order of each axis'
pair (the order follows the sign of the ray's direction).  Then every cull decision is the one box_distance2 would give.

Why it holds: per axis the pair is (lo - o, hi - o).  box_distance2 takes max(lo - o, o - hi, 0), of which at most one difference
is positive; the median of (lo - o, 0, hi - o) is lo - o where that is positive, hi - o where that is negative - o - hi is its exact
negation, and the sign goes in the square - and 0 between.  tests/leaf_cull_slab_model.cpp compiles the header with g++.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import model_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
f32 = np.float32
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    folder = tmp_path_factory.mktemp("leaf_cull_slab_model")
    m = C.CDLL(model_build.library([os.path.join(ROOT, "tests", "leaf_cull_slab_model.cpp")], folder, "libleaf_cull_slab_model.so",
                                   opt="-O2", werror=False, fp_strict=True, includes=[os.path.join(ROOT, "include"), CSRC]))
    m.slab_box_distance2_bits.argtypes = [FP, FP, FP]
    m.slab_box_distance2_bits.restype = C.c_uint32
    m.slab_from_slabs_bits.argtypes = [FP, FP, FP, C.c_int]
    m.slab_from_slabs_bits.restype = C.c_uint32
    m.slab_count_differences.argtypes = [C.c_uint32, FP, FP, FP, C.POINTER(C.c_uint32)]
    m.slab_count_differences.restype = C.c_uint32
    return m


def fp(a):
    return a.ctypes.data_as(FP)


def differences(m, lo, hi, o):
    lo, hi, o = (np.ascontiguousarray(a, f32).reshape(-1, 3) for a in (lo, hi, o))
    assert lo.shape == hi.shape == o.shape and (lo <= hi).all()
    first = C.c_uint32(0)
    n = m.slab_count_differences(len(lo), fp(lo), fp(hi), fp(o), C.byref(first))
    return n, (lo[first.value], hi[first.value], o[first.value]) if n else None


def as_float(bits):
    return float(np.array([bits], np.uint32).view(f32)[0])


def test_random_boxes_and_origins(model):
    """10^5 boxes and origins, magnitudes log-uniform from 1e-3 to 1e4 with either sign; a third of the origins inside their box,
    a third on the box's scale beside it, a third anywhere."""
    rs = np.random.RandomState(2024)
    n = 100_000

    def coords(shape):
        return (rs.choice([-1.0, 1.0], shape) * 10.0 ** rs.uniform(-3, 4, shape)).astype(f32)
    p, q = coords((n, 3)), coords((n, 3))
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    o = coords((n, 3))
    inside = (lo + rs.uniform(0, 1, (n, 3)).astype(f32) * (hi - lo)).astype(f32)
    beside = (lo + rs.uniform(-2, 3, (n, 3)).astype(f32) * (hi - lo)).astype(f32)
    kind = rs.randint(0, 3, n)[:, None]
    o = np.where(kind == 0, inside, np.where(kind == 1, beside, o)).astype(f32)
    differ, where = differences(model, lo, hi, o)
    assert differ == 0, (differ, where)
    # (and the sample does what it says: origins inside, and outside along one, two and three axes)
    outside_axes = ((o < lo) | (o > hi)).sum(axis=1)
    assert all((outside_axes == k).sum() > 1000 for k in range(4))


def directed_cases():
    tiny, least = f32(1e-40), f32(2.0 ** -126)  # a denormal; the least normal number
    below = np.nextafter(least, f32(0))         # least - one denormal step: the difference is the smallest denormal
    cases = []
    unit_lo, unit_hi = [-1, -1, -1], [1, 1, 1]
    cases.append(("origin inside", unit_lo, unit_hi, [0.25, -0.5, 0]))
    for axis in range(3):
        for side in (-1, 1):
            at = [0.3, -0.2, 0.1]
            at[axis] = side
            cases.append((f"on face {axis}{'+' if side > 0 else '-'}", unit_lo, unit_hi, at))
    cases.append(("on an edge", unit_lo, unit_hi, [1, -1, 0.5]))
    for corner in itertools.product((-1, 1), repeat=3):
        cases.append((f"at corner {corner}", unit_lo, unit_hi, list(corner)))
    cases.append(("lo = hi, origin there", [2, 3, 4], [2, 3, 4], [2, 3, 4]))
    cases.append(("lo = hi, origin off", [2, 3, 4], [2, 3, 4], [5, -1, 4]))
    # zeros of either sign in every place (-0 <= +0 and +0 <= -0 both hold): every difference is a zero of some sign
    for zl, zh, zo in itertools.product((0.0, -0.0), repeat=3):
        cases.append((f"zeros {zl} {zh} {zo}", [zl] * 3, [zh] * 3, [zo] * 3))
        cases.append((f"zero slab {zl} {zh}, origin off", [zl, zl, -1], [zh, zh, 1], [zo, 3, zo]))
    # differences that come out as +0 or -0: a coordinate equal to the origin's (x - x = +0 whatever the sign of x)
    cases.append(("lo = o", [1.5, -2.5, 3], [4, 4, 4], [1.5, -2.5, 3]))
    cases.append(("hi = o", [-4, -4, -4], [1.5, -2.5, 3], [1.5, -2.5, 3]))
    cases.append(("hi = o on one axis, outside on another", [-4, -4, -4], [1.5, -2.5, 3], [1.5, 7, -9]))
    # denormal differences (their squares underflow; the sums must still agree)
    cases.append(("denormal lo beyond 0", [tiny, tiny, tiny], [1, 1, 1], [0, 0, 0]))
    cases.append(("denormal hi before 0", [-1, -1, -1], [-tiny, -tiny, -tiny], [0, 0, 0]))
    cases.append(("smallest denormal difference", [least, least, least], [1, 1, 1], [below, below, below]))
    cases.append(("smallest denormal difference and a large one", [least, least, 100], [1, 1, 200], [below, below, 3]))
    cases.append(("denormal box around a denormal origin", [-tiny, -tiny, -tiny], [tiny, tiny, tiny], [tiny / 2, -tiny / 2, 0]))
    # the largest coordinates a certificate admits, seen from the farthest origins the kernel traces from
    big, far = 2.0 ** 20, 2.0 ** 40
    for signs in itertools.product((-1, 1), repeat=3):
        cases.append((f"2^20 box from 2^40 {signs}", [-big] * 3, [big] * 3, [s * far for s in signs]))
    cases.append(("2^20 corner box from 2^40", [big - 1, -big, big - 0.5], [big, -big + 1, big], [far, far, -far]))
    cases.append(("2^20 box, origin inside", [-big] * 3, [big] * 3, [big - 0.0625, 0, -big]))
    return cases


DIRECTED = directed_cases()


@pytest.mark.parametrize("case", DIRECTED, ids=[c[0] for c in DIRECTED])
def test_directed_cases(model, case):
    _, lo, hi, o = case
    differ, where = differences(model, lo, hi, o)
    assert differ == 0, where


def test_the_distance_itself(model):
    """... and what both compute is the distance: 0 inside and on the boundary, the squared gap outside."""
    def both(lo, hi, o):
        lo, hi, o = (np.array(a, f32) for a in (lo, hi, o))
        a = model.slab_box_distance2_bits(fp(lo), fp(hi), fp(o))
        assert all(model.slab_from_slabs_bits(fp(lo), fp(hi), fp(o), order) == a for order in range(8))
        return a
    assert both([-1, -1, -1], [1, 1, 1], [0.25, -0.5, 0]) == 0  # (+0: the bits)
    assert both([-1, -1, -1], [1, 1, 1], [1, -1, 0.5]) == 0
    assert as_float(both([-1, -1, -1], [1, 1, 1], [3, 0, 0])) == 4.0
    assert as_float(both([-1, -1, -1], [1, 1, 1], [3, -4, 0])) == 4.0 + 9.0
    assert as_float(both([-1, -1, -1], [1, 1, 1], [-2, 3, -5])) == 1.0 + 4.0 + 16.0
    assert as_float(both([-2.0 ** 20] * 3, [2.0 ** 20] * 3, [2.0 ** 40, 0, 0])) == float(f32(2.0 ** 40 - 2.0 ** 20) * f32(2.0 ** 40 - 2.0 ** 20))
