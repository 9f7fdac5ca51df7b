"""Shared by tests/test_leaf_cull_wide_model.py, tests/test_leaf_cull_wide_gpu.py and tools/leaf_cull_potential.py: the model of
tests/leaf_cull_cases.py with tests/leaf_cull_wide_model.cpp compiled into it (the wide tier of csrc/leaf_cull.h), the walk at
the kernel's PTMI_LEAF_CULL levels, and the sliver scene whose leaves only the wide tier certifies."""
import copy
import ctypes as C
import os

import numpy as np

from opencl_pathtracer_amd import scenes
import leaf_cull_cases as K

WIDE_SRC = os.path.join(K.ROOT, "tests", "leaf_cull_wide_model.cpp")
f32 = np.float32
FP = K.FP
# what each tier may grant at most (csrc/leaf_cull.h): the heights below were chosen against these on the CPU
# (tests/test_leaf_cull_wide_model.py asserts what they are chosen for)
THIN_WIDE_ONLY = (0.04, 0.1)  # of the base edge: below what the tight tier certifies at this scene's size, within the wide tier's


def build_model(folder):
    """K.build_model's library plus the wide model's functions."""
    m = K.build_model(folder, extra_sources=[WIDE_SRC])
    m.wide_constants.argtypes = [C.POINTER(C.c_double)]
    m.wide_bits.argtypes = [C.c_void_p]
    m.wide_rule.argtypes = [FP, FP, FP, C.c_float, C.c_float]
    m.wide_triangle_certified.argtypes = [C.c_void_p, FP, FP]
    m.wide_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, FP, FP, C.c_float,
                            C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    m.wide_check_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return m


def bits(m):
    """The record bits, and the record bits a launch looks at for DScene::leaf_cull = 0, 3, 7 and 7 + the tight-only flag."""
    out = np.zeros(11, np.uint32)
    m.wide_bits(out.ctypes.data)
    names = ("child1", "child2", "computed", "wide1", "wide2", "wide_computed", "tight_only", "mask_0", "mask_3", "mask_7", "mask_7_tight_only")
    return dict(zip(names, (int(x) for x in out)))


def walk(lay, lib, origin, direction, limit, shadow, mask, wide):
    """One query of K.Layout `lay` culled by the record bits in `mask` under the wide (or the tight) rule."""
    out = np.zeros(12, np.uint32)
    o, d = np.ascontiguousarray(origin, f32), np.ascontiguousarray(direction, f32)
    lay.m.wide_walk(lay.recs.ctypes.data, lay.tri_ids.ctypes.data, lay.big.ctypes.data, lay.root_ref, lay.tris.ctypes.data,
                    C.cast(lib.pto_bounding_box_intersects, C.c_void_p), C.cast(lib.pto_triangle_intersects, C.c_void_p),
                    K.fp(o), K.fp(d), float(limit), int(shadow), int(mask), int(wide), out.ctypes.data)
    return dict(zip(K.WALK_FIELDS, (int(x) for x in out)))


CHECK_FIELDS = ("inner", "leaves", "tight", "wide", "wide_only", "tight_differs", "wide_differs", "stray_bits", "tight_without_wide")


def check_records(lay):
    """The cull words of K.Layout `lay` against both tiers computed afresh from its records and triangles."""
    out = np.zeros(9, np.uint32)
    lay.m.wide_check_records(lay.recs.ctypes.data, lay.tri_ids.ctypes.data, len(lay.recs), lay.tris.ctypes.data, out.ctypes.data)
    return dict(zip(CHECK_FIELDS, (int(x) for x in out)))


def sliver_scene(n, width, height, thin=THIN_WIDE_ONLY, seed=21):
    """K.random_scene's volume and camera filled with n slivers: a base edge of 0.5 .. 1.2 and the third vertex at `thin` (a range,
    log-uniform) of the edge's length off it."""
    base = scenes.random_triangles(16, width, height)
    rs = np.random.RandomState(seed)
    a = rs.uniform(-5.0, 5.0, (n, 3))
    e = rs.normal(size=(n, 3))
    e *= (rs.uniform(0.5, 1.2, (n, 1)) / np.linalg.norm(e, axis=1)[:, None])
    side = np.cross(e, rs.normal(size=(n, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    h = np.exp(rs.uniform(np.log(thin[0]), np.log(thin[1]), (n, 1))) * np.linalg.norm(e, axis=1)[:, None]
    c = a + e * rs.uniform(0.3, 0.7, (n, 1)) + side * h
    out = copy.copy(base)
    out.triangulation = scenes.triangle_create(a.astype(f32), (a + e).astype(f32), c.astype(f32), mat_pos=0)
    out.bvh = None
    out.name = f"slivers{n}"
    return out
