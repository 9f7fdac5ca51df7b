"""The node trip of the culling instantiations after its diet ("The node step's diet"; kernel_wavefront.hip:
cull_step): the static instruction counts of the node-trip path - loop header to back edge, as the resource tool's
parsing counts them (through tests/kernel_figures.py) from the assembly hipcc makes (it cross-compiles without a GPU) - stay at
or below what the change reached, the flagship's within the issue's 158 vector / 100 scalar, and the leaf-pass path is not above
what it was.

NODE_TRIP: (vector, scalar) per instantiation, [strict, default].  The parent's figures: plain 170 / 104, general 180 / 104.
The general instantiation of 256 lanes (01000c) keeps the parent's step: under the counting step the allocator spills more of it
than tests/test_path_logic_loads.py pins (default arithmetic 41 registers for 28, strict 62 for 57), so its figures are the
parent's, and pinned as that.

The helpers the step takes from csrc/leaf_cull.h are checked on the CPU: cull_threshold_wide is fmaf(limit, kRelWide, kAbsWide)
bit for bit, and certified_and_beyond_wide is "bit 0 set and box_is_beyond_wide" - at the limits around the wide rule's boundary
(the largest limit at which it fires, -3 .. +3 ulp), at 0.3 .. 0.98 of the squared distance, and at 0, infinity and a NaN.
"""
import ctypes as C
import os

import numpy as np
import pytest

import kernel_figures as K
import model_build

ROOT = K.ROOT

NODE_TRIP = {
    "01010c": [(157, 100), (156, 100)],     # <- the flagship's kernel (default arithmetic)
    "01010b64c": [(156, 100), (156, 100)],
    "01000b64c": [(162, 100), (162, 100)],
    "01000c": [(180, 104), (180, 104)],     # the parent's step, kept (see above)
}
LEAF_PASS = [(151, 108), (146, 108)]  # plain culling instantiations, the parent's figures
FLAGSHIP_BOUND = (158, 100)


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_node_trip_counts_stay_where_the_diet_left_them(arithmetic):
    found = K.trip_loops(arithmetic)
    for key, pinned in sorted(NODE_TRIP.items()):
        vector, scalar = found[key]["node trip"]
        print(key, "node trip", (vector, scalar), "pinned", pinned[arithmetic])
        assert vector <= pinned[arithmetic][0] and scalar <= pinned[arithmetic][1], (key, (vector, scalar), pinned[arithmetic])


@K.needs_hipcc
def test_flagship_is_within_the_issues_bound():
    vector, scalar = K.trip_loops(1)["01010c"]["node trip"]
    assert vector <= FLAGSHIP_BOUND[0] and scalar <= FLAGSHIP_BOUND[1], (vector, scalar)
    assert 170 - vector >= 12 and 104 - scalar >= 4, (vector, scalar)  # (the issue's target, from the parent's 170 / 104)


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_leaf_pass_path_is_not_above_what_it_was(arithmetic):
    found = K.trip_loops(arithmetic)
    for key in ("01010c", "01010b64c"):
        vector, scalar = found[key]["leaf pass"]
        print(key, "leaf pass", (vector, scalar))
        assert vector <= LEAF_PASS[arithmetic][0] and scalar <= LEAF_PASS[arithmetic][1], (key, vector, scalar)


MODEL_SRC = r"""
#include "leaf_cull.h"
extern "C" {
float diet_threshold(float limit) { return ptmi_cull::cull_threshold_wide(limit); }
float diet_fmaf(float limit) { return fmaf(limit, ptmi_cull::kRelWide, ptmi_cull::kAbsWide); }
int diet_beyond(float d2, float limit) { return ptmi_cull::box_is_beyond_wide(d2, limit) ? 1 : 0; }
int diet_key(unsigned certified, float d2, float limit) { return ptmi_cull::certified_and_beyond_wide(certified, d2, -ptmi_cull::cull_threshold_wide(limit)) ? 1 : 0; }
void diet_constants(float* out) { out[0] = ptmi_cull::kRelWide; out[1] = ptmi_cull::kAbsWide; }
}
"""


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """csrc/leaf_cull.h compiled for the host with -ffp-contract=off, as the library is."""
    folder = tmp_path_factory.mktemp("node_step_diet_model")
    src = os.path.join(folder, "diet_model.cpp")
    with open(src, "w") as f:
        f.write(MODEL_SRC)
    m = C.CDLL(model_build.library([src], folder, "libdiet_model.so", opt="-O2", werror=None, extra=["-ffp-contract=off"],
                                   includes=[os.path.join(ROOT, "include"), os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")]))
    m.diet_threshold.restype = m.diet_fmaf.restype = C.c_float
    m.diet_threshold.argtypes = m.diet_fmaf.argtypes = [C.c_float]
    m.diet_beyond.argtypes = [C.c_float, C.c_float]
    m.diet_key.argtypes = [C.c_uint32, C.c_float, C.c_float]
    m.diet_constants.argtypes = [C.POINTER(C.c_float)]
    return m


def limits_and_distances(model):
    """Squared distances as a scene of a few units has them, each with the limits around the wide rule's boundary: the largest
    limit at which the rule fires (bisection over the float bit patterns), -3 .. +3 ulp; 0.3 .. 0.98 of the distance; 0, inf, NaN."""
    f32 = np.float32
    rs = np.random.default_rng(5)
    out = []
    for d2 in np.concatenate([rs.uniform(0.0, 400.0, 200), 10.0 ** rs.uniform(-4, 6, 100), [0.0, 0.05, 0.0500001, 1e30]]).astype(f32):
        limits = [f32(0), f32(np.inf), f32(np.nan), f32(d2), f32(d2 * rs.uniform(0.3, 0.98))]
        a, b = 0, int(f32(d2).view(np.uint32))
        if model.diet_beyond(float(d2), 0.0) and not model.diet_beyond(float(d2), float(d2)):
            while b - a > 1:
                mid = (a + b) // 2
                a, b = (mid, b) if model.diet_beyond(float(d2), float(np.uint32(mid).view(f32))) else (a, mid)
            x = np.uint32(a).view(f32)
            for step in range(-3, 4):
                y = x
                for _ in range(abs(step)):
                    y = np.nextafter(y, f32(np.inf if step > 0 else -np.inf))
                limits.append(max(y, f32(0)))
        out.extend((float(d2), float(l)) for l in limits)
    return out


def test_threshold_is_the_rules_fmaf_bit_for_bit(model):
    f32 = np.float32
    for _, limit in limits_and_distances(model):
        a, b = f32(model.diet_threshold(limit)), f32(model.diet_fmaf(limit))
        assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), (limit, a, b)


def test_one_compare_needs_a_limit_that_is_not_negative(model):
    """The contract's precondition (csrc/leaf_cull.h: certified_and_beyond_wide): the negated threshold is not positive.  Down
    to limit = -0 and the smallest negative limits the threshold stays positive and the function is the conjunction; below
    -kAbsWide / kRelWide it is not - an uncertified child nearer than the (then positive) negated threshold compares true.
    The kernel's limits are squared distances, a linear distance or +inf: never negative."""
    c = (C.c_float * 2)()
    model.diet_constants(c)
    rel, ab = float(c[0]), float(c[1])
    for limit in (-0.0, -1e-30, -0.9 * ab / rel):  # the threshold is still positive
        assert model.diet_threshold(limit) > 0
        for d2 in (0.0, 1e-3, 0.04, 1.0, 100.0):
            want = model.diet_beyond(d2, limit)
            for word in (0, 1, 2, 3):
                assert model.diet_key(word, d2, limit) == (want if word & 1 else 0), (word, d2, limit)
    limit = -2.0 * ab / rel  # the threshold is -kAbsWide: outside the contract
    assert model.diet_threshold(limit) < 0
    assert model.diet_key(0, 0.0, limit) == 1 and model.diet_beyond(0.0, limit) == 1  # (uncertified, and yet "counted")


def test_one_compare_is_certified_and_beyond(model):
    cases = limits_and_distances(model)
    assert any(model.diet_beyond(d2, limit) for d2, limit in cases) and any(not model.diet_beyond(d2, limit) for d2, limit in cases)
    for d2, limit in cases + [(float("nan"), 1.0), (float("inf"), 1.0), (float("inf"), float("inf"))]:
        want = model.diet_beyond(d2, limit)
        for word in (0, 1, 2, 3, 6, 7):  # (bit 0 alone decides; the bits above it are shifted out)
            assert model.diet_key(word, d2, limit) == (want if word & 1 else 0), (word, d2, limit)
