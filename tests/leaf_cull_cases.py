"""Shared by tests/test_leaf_cull_model.py and tools/leaf_cull_potential.py: tests/leaf_cull_model.cpp built and wrapped, the
rays of a path as the reference shoots them, and one BVH query of the model with the oracle's deciders."""
import ctypes as C
import os

import numpy as np

from opencl_pathtracer_amd import backend, structs as S
from f32_cases import camera_direction, fma as _fma, mad as _mad
import model_build
import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "leaf_cull_model.cpp"), os.path.join(ROOT, "tests", "scene_refit_model.cpp"),
        os.path.join(CSRC, "scene_refit_host.cpp"), os.path.join(CSRC, "scene_layout.cpp")]
f32 = np.float32
FP = C.POINTER(C.c_float)
NONE = 0xFFFFFFFF
WALK_FIELDS = ("hit", "limit_bits", "n_bbx", "n_tri", "direct", "popped", "direct_culled", "direct_culled_tris", "popped_culled",
               "popped_culled_tris", "tested", "direct_uncertified")


def build_model(folder, extra_sources=()):
    m = C.CDLL(model_build.library([*SRCS, *extra_sources], folder, "libleaf_cull_model.so", opt="-O2", werror=False, fp_strict=True,
                                   includes=[os.path.join(ROOT, "include"), CSRC]))
    m.cull_rule.argtypes = [FP, FP, FP, C.c_float, C.c_float]
    m.cull_box_distance2.argtypes = [FP, FP, FP]
    m.cull_box_distance2.restype = C.c_float
    m.cull_triangle_slack.argtypes = [C.c_void_p, FP, FP, C.POINTER(C.c_double)]
    m.cull_triangle_certified.argtypes = [C.c_void_p, FP, FP]
    m.cull_constants.argtypes = [C.POINTER(C.c_double)]
    m.cull_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, FP, FP, C.c_float,
                            C.c_int, C.c_int, C.c_void_p]
    m.cull_layout_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    m.model_layout.restype = C.c_void_p
    m.model_layout.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    m.model_layout_free.argtypes = [C.c_void_p]
    m.model_layout_info.argtypes = [C.c_void_p, C.c_void_p]
    m.model_layout_copy.argtypes = [C.c_void_p] * 5
    m.model_update.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    m.model_error.restype = C.c_char_p
    return m


def fp(a):
    return a.ctypes.data_as(FP)


def config_for(sc, w=64, h=64):
    return backend.Config(C.sizeof(backend.Config), 0, w, h, 4, sc.lightsSize, S.JITTERED, 0, 0)


def layout_bits(m, sc):
    cfg = config_for(sc)
    d, keep = backend.scene_desc(sc)
    out = np.zeros(5, np.uint32)
    rc = m.cull_layout_bits(C.addressof(cfg), C.addressof(d), out.ctypes.data_as(C.c_void_p))
    return rc, dict(zip(("inner", "computed", "leaves", "cullable", "nonzero_pad"), (int(x) for x in out)))


class Layout:
    """build_layout's records of a scene, as arrays the walk reads."""

    def __init__(self, m, sc):
        self.m, self.sc = m, sc
        cfg = config_for(sc)
        d, keep = backend.scene_desc(sc)
        rc = C.c_int(0)
        self.h = m.model_layout(C.addressof(cfg), C.addressof(d), C.byref(rc))
        assert rc.value == 0 and self.h, m.model_error()
        self.tris = np.ascontiguousarray(sc.triangulation)
        self.refresh()

    def refresh(self):
        info = np.zeros(6, np.uint32)
        self.m.model_layout_info(self.h, info.ctypes.data_as(C.c_void_p))
        n_rec, n_tri, n_big = int(info[0]), int(info[1]), int(info[2])
        self.recs, self.tri_ids = np.zeros((n_rec, 16), np.uint32), np.zeros(n_rec, np.uint32)
        shade, self.big = np.zeros((n_tri, 28), np.uint32), np.zeros((max(n_big, 1), 2), np.uint32)
        self.m.model_layout_copy(self.h, *[a.ctypes.data_as(C.c_void_p) for a in (self.recs, self.tri_ids, shade, self.big)])
        self.root_ref = int(info[3])

    def update(self, tris):
        levels = C.c_uint32(0)
        self.tris = np.ascontiguousarray(tris)
        rc = self.m.model_update(self.h, self.tris.ctypes.data_as(C.c_void_p), len(self.tris), 0, C.byref(levels))
        assert rc == 0, self.m.model_error()
        self.refresh()

    def inner(self):
        return self.recs[self.tri_ids == NONE]

    def free(self):
        self.m.model_layout_free(self.h)

    def walk(self, lib, origin, direction, limit, shadow, mode):
        out = np.zeros(12, np.uint32)
        o, d = np.ascontiguousarray(origin, f32), np.ascontiguousarray(direction, f32)
        self.m.cull_walk(self.recs.ctypes.data, self.tri_ids.ctypes.data, self.big.ctypes.data, self.root_ref, self.tris.ctypes.data,
                         C.cast(lib.pto_bounding_box_intersects, C.c_void_p), C.cast(lib.pto_triangle_intersects, C.c_void_p),
                         fp(o), fp(d), float(limit), int(shadow), mode, out.ctypes.data)
        return dict(zip(WALK_FIELDS, (int(x) for x in out)))


def ray_direction(lib, origin, direction):
    """Ray3D_SetDirection of the oracle: the normalised direction (4 components)."""
    lib.pto_ray_create.argtypes = [FP, FP, FP, FP]
    lib.pto_ray_create.restype = None
    out, inv = np.zeros(4, f32), np.zeros(3, f32)
    lib.pto_ray_create(fp(np.ascontiguousarray(origin, f32)), fp(np.ascontiguousarray(direction, f32)), fp(out), fp(inv))
    return out


def _length4(lib, v):
    """length(float4) of the platform library as the oracle restates it: the hardware square root of the fma-chain dot product
    (squared lengths in the normal range, which is all these scenes have)"""
    d = _fma(v[3], v[3], _fma(v[2], v[2], _fma(v[1], v[1], f32(v[0]) * f32(v[0]))))
    assert 2.0 ** -126 <= float(d) < float("inf")
    return float(lib.pto_hardware_sqrt(float(d)))


def path_queries(lib, sc, w, h, depth, x, y, iteration, default_arithmetic):
    """The BVH queries of one path as the reference shoots them, from the oracle's sampler and its per-bounce trace:
    (origin, direction, limit, shadow, oracle's hit triangle or None, bounce the query belongs to).  The camera ray
    (FullKernel.cl:1213, JITTERED sampler); scattered rays start at point + 0.001 out (:880); shadow rays at the point itself
    towards light 0 with the LINEAR distance as their limit (:932-944).  Also returns the bounces (n_bbx, n_tri: the path's
    running totals after each bounce's closest-hit and shadow query)."""
    bounces, _ = O.oracle_trace(sc, w, h, depth, x, y, iteration, default_arithmetic=default_arithmetic)
    bounces = [b for b in bounces if b.n_bbx or b.n_tri]  # (a path that hits nothing comes back as ONE bounce of zeros)
    assert len(sc.lights) <= 1
    light = np.array(sc.lights["position"][0], f32).reshape(4) if len(sc.lights) else None
    seed = C.c_int32(lib.pto_initialize_random_seed(x, y, w, h, iteration))
    sample = (C.c_float * 2)()
    lib.pto_sampler(S.JITTERED, x, y, w, h, iteration, C.byref(seed), sample)
    eye = np.array(sc.cameraPosition, f32).reshape(4)
    shot = camera_direction(sc, sample, default_arithmetic)
    queries = [(eye, ray_direction(lib, eye, shot), float("inf"), False, bounces[0].triangle_id if bounces else None, 0)]
    for k, b in enumerate(bounces):
        point, out = np.array(b.point[:], f32), np.array(b.out_dir[:], f32)
        if light is not None:
            full = (light - point).astype(f32)
            queries.append((point, ray_direction(lib, point, full), _length4(lib, full), True, None, k))
        if k + 1 < depth:
            origin = _mad(out, 0.001, point, default_arithmetic)
            nxt = bounces[k + 1].triangle_id if k + 1 < len(bounces) else None
            queries.append((origin, ray_direction(lib, origin, out), float("inf"), False, nxt, k + 1))
    return queries, bounces


def random_scene(n, width, height, spread=0.6, seed=77):
    """scenes.random_triangles with larger triangles (vertices centre + U[-spread, spread]^3 instead of 0.1): a ray pierces many
    leaf boxes behind its hit, as in the million-triangle scene, and every hit lies beyond unit distance of its ray's origin
    (camera at x = -14, centres in [-5, 5]^3)."""
    import copy
    from opencl_pathtracer_amd import scenes
    base = scenes.random_triangles(16, width, height)
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-5.0, 5.0, (n, 3)).astype(f32)
    v = (centres[:, None, :] + rs.uniform(-spread, spread, (n, 3, 3)).astype(f32)).astype(f32)
    out = copy.copy(base)
    out.triangulation = scenes.triangle_create(v[:, 0], v[:, 1], v[:, 2], mat_pos=0)
    out.bvh = None
    out.name = f"random{n}x{spread}"
    return out
