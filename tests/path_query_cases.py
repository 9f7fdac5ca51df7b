"""The yardstick of ptmi_trace_paths (test_path_query_model.py, test_path_query_gpu.py), and the rays the tests send.  No product
code is involved, and nothing of the integrator is restated: one path is pto_kernel_main of the CPU oracle, unchanged.

An oracle scene whose camera is (position = o, direction = d, right = 0, up = 0) makes Kernel_Main's camera expression
up * sy + (right * sx + d) evaluate to d exactly, in both arithmetics, for every d without an exact-zero x, y or z (a -0 would
come out as +0; the tests send none).  With image_width = index_stride, image_height = 1 and the work-item (gx = index, gy = 0)
the seed is InitializeRandomSeed of index + it * index_stride, the sampler draws what it draws for any work-item, and
Ray3D_Create and the bounce loop are Kernel_Main's own.  The path's radiance is what the work-item adds to the (zeroed) image:
taken from the one pixel whose count is non-zero, wherever the sampler put it (with RANDOM: some other pixel of the row).

A path depends on (o, d, index + it * index_stride mod 2^32) alone - the sampler's values are discarded by the zero basis - so
paths are kept by that key and shared between the batch sizes and iteration counts of a test session.  Sums are np.float32
additions in iteration order, starting at +0; counts are added as integers.
"""
import ctypes as C

import numpy as np

from opencl_pathtracer_amd import structs as S
from f32_cases import camera_direction
import oracle_ffi as O
import ray_query_cases as Q

f32 = np.float32
COUNTS = ("segments", "surface_hits", "shadow_rays", "box_tests", "triangle_tests")


class Yardstick:
    """One scene, depth, sampler, arithmetic and flag set.  sums(rays, ...) -> the structs.PATH_SUM array ptmi_trace_paths must
    return; after it, `sky_ends` and `hits` hold per ray how many of its paths ended on the sky and its surface hits."""

    def __init__(self, scene, depth=4, sampler=S.JITTERED, default_arithmetic=False, russian_roulette=False, source_seed=False):
        self.lib = O.oracle(default_arithmetic)
        self.lib.pto_kernel_main.argtypes = [C.POINTER(O.PtoScene), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(O.PtoBuffers),
                                             C.POINTER(O.PtoTotals)]
        self.osc = O.OracleScene(scene, 1, 1, depth, sampler, russian_roulette=russian_roulette, source_seed=source_seed)
        self.osc.c.camera_right = self.osc.c.camera_up = O.F4(0.0, 0.0, 0.0, 0.0)
        self._paths = {}
        self._stride = 0

    def _image(self, stride):
        if stride != self._stride:
            self._color, self._count = np.zeros((stride, 4), f32), np.zeros(stride, f32)
            self._buf = O.PtoBuffers(self._color.ctypes.data, self._count.ctypes.data, None, None, None, None)
            self._stride = stride
            self.osc.c.image_width, self.osc.c.image_height = stride, 1

    def path(self, origin, direction, index, it, stride):
        """(radiance float32[4], the five counts) of one path: work-item (index, 0) of iteration `it` in an image of stride x 1"""
        o, d = np.asarray(origin, f32), np.asarray(direction, f32)
        assert (d[:3] != 0).all(), "a direction component of exact zero: the zero-basis camera does not reproduce its sign"
        assert index < stride, "the work-item must exist in the oracle's image"
        key = (o.tobytes(), d.tobytes(), (index + it * stride) & 0xFFFFFFFF)
        if key not in self._paths:
            self._image(stride)
            self.osc.c.camera_position, self.osc.c.camera_direction = O._f4(o), O._f4(d)
            tot = O.PtoTotals()
            with np.errstate(all="ignore"):
                traced = self.lib.pto_kernel_main(C.byref(self.osc.c), index, 0, it, C.byref(self._buf), C.byref(tot))
            where = np.flatnonzero(self._count)
            assert traced == 1 and len(where) == 1 and self._count[where[0]] == 1 and tot.paths == 1
            radiance = self._color[where[0]].copy()
            self._color[where[0]], self._count[where[0]] = 0, 0
            self._paths[key] = (radiance, tuple(int(getattr(tot, n)) for n in COUNTS))
        return self._paths[key]

    def refractions(self, scene, origin, direction, index, it, stride):
        """How many bounces of that path left a glass or water surface THROUGH it: the scattered direction points away from the
        shading normal, which faces the arriving ray (pto_trace_path's per-bounce record of the same work-item)."""
        self._image(stride)
        self.osc.c.camera_position, self.osc.c.camera_direction = O._f4(np.asarray(origin, f32)), O._f4(np.asarray(direction, f32))
        bounces, rad = (O.PtoBounce * 64)(), (C.c_float * 4)()
        bounces[0].triangle_id = 0xFFFFFFFF  # (a path without a bounce returns 1 too and writes no record)
        with np.errstate(all="ignore"):
            n = self.lib.pto_trace_path(C.byref(self.osc.c), index, 0, it, bounces, 64, rad)
        types = scene.materiaux["type"]
        return sum(1 for b in bounces[:max(n, 0)] if b.triangle_id != 0xFFFFFFFF and types[b.material_id] in (S.MAT_GLASS, S.MAT_WATER)
                   and float(np.dot(np.array(b.out_dir[:3], np.float64), np.array(b.ns[:3], np.float64))) < 0)

    def sums(self, rays, first_iteration=0, n_iterations=1, first_index=0, index_stride=None):
        stride = len(rays) if index_stride is None else index_stride
        out = np.zeros(len(rays), S.PATH_SUM)
        self.sky_ends, self.hits = np.zeros(len(rays), np.int64), np.zeros(len(rays), np.int64)
        for i, r in enumerate(rays):
            total = np.zeros(4, f32)
            counts = [0] * 5
            for it in range(first_iteration, first_iteration + n_iterations):
                radiance, c = self.path(r["origin"], r["direction"], first_index + i, it, stride)
                with np.errstate(all="ignore"):
                    total = total + radiance
                counts = [a + b for a, b in zip(counts, c)]
                self.sky_ends[i] += c[0] - c[1]  # a path that ends on the sky has one segment more than it has surface hits
            out["radiance"][i] = total
            for name, v in zip(COUNTS, counts):
                out[name][i] = v
            self.hits[i] = counts[1]
        return out


def words(sums):
    """uint32[n, 12] view of a PATH_SUM array: what the tests compare."""
    return np.ascontiguousarray(sums).view(np.uint32).reshape(len(sums), 12)


FIELD_WORDS = dict(radiance=slice(0, 4), segments=4, surface_hits=5, shadow_rays=6, reserved=7, box_tests=slice(8, 10), triangle_tests=slice(10, 12))


def describe_difference(got, want):
    """'' when every word is equal - a radiance word that is a NaN in the yardstick asks for a NaN, of any sign and payload - else
    which fields differ on how many rays and the first such ray."""
    g, w = words(got).copy(), words(want).copy()
    fg, fw = g[:, :4].view(f32), w[:, :4].view(f32)
    both = np.isnan(fg) & np.isnan(fw)
    fg[both], fw[both] = np.nan, np.nan
    if np.array_equal(g, w):
        return ""
    bad = np.nonzero((g != w).any(axis=1))[0]
    fields = [name for name, sl in FIELD_WORDS.items() if (g[:, sl] != w[:, sl]).any()]
    k = int(bad[0])
    return f"{len(bad)} of {len(g)} sums differ in {fields}; first: ray {k}\n  got  {got[k]}\n  want {want[k]}"


# ---------------------------------------------------------------------------------------------- rays

def _nonzero(d):
    d = np.asarray(d, f32)
    assert (d[:, :3] != 0).all(), "a generator produced a direction component of exact zero"
    return d


def camera_rays(scene, width, height, it, sampler=S.JITTERED, default_arithmetic=False):
    """The rays Kernel_Main makes for iteration `it` of a width x height image, ray gy * width + gx for pixel (gx, gy):
    pto_sampler's (sx, sy) and the camera expression of cl:1213 in float32 in the oracle's arithmetic, un-normalised
    (Ray3D_Create normalises).  structs.RAY records; origin and direction carry all four components of the camera's."""
    lib = O.oracle(default_arithmetic)
    d = np.zeros((width * height, 4), f32)
    sample = (C.c_float * 2)()
    for gy in range(height):
        for gx in range(width):
            seed = C.c_int32(lib.pto_initialize_random_seed(gx, gy, width, height, it))
            lib.pto_sampler(sampler, gx, gy, width, height, it, C.byref(seed), sample)
            d[gy * width + gx] = camera_direction(scene, (sample[0], sample[1]), default_arithmetic)
    return Q.make_rays(np.tile(np.asarray(scene.cameraPosition, f32), (len(d), 1)), _nonzero(d))


def interior_rays(scene, n, seed=1):
    """From random points inside the scene's bounds into random directions."""
    rs = np.random.default_rng(seed)
    lo, hi = Q.scene_box(scene)
    o = rs.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), (n, 3)).astype(f32)
    return Q.make_rays(o, _nonzero(rs.normal(size=(n, 3)).astype(f32)))


def surface_rays(scene, n, seed=2):
    """From points ON triangles (the float32 of a barycentric combination: the path starts within rounding of the surface, as a
    bake or a picked point does) into a random direction of the hemisphere of +N or -N."""
    rs = np.random.default_rng(seed)
    t = scene.triangulation
    ok = np.nonzero(np.isfinite(t["N"]).all(axis=1) & np.isfinite(t["S1"]).all(axis=1) & np.isfinite(t["S2"]).all(axis=1) & np.isfinite(t["S3"]).all(axis=1))[0]
    pick = ok[rs.integers(0, len(ok), n)]
    a = rs.uniform(0.05, 0.45, n)[:, None]
    b = rs.uniform(0.05, 0.45, n)[:, None]
    s1, s2, s3, nrm = (t[f][pick][:, :3].astype(np.float64) for f in ("S1", "S2", "S3", "N"))
    p = s1 + a * (s2 - s1) + b * (s3 - s1)
    side = np.where(rs.random(n) < 0.5, 1.0, -1.0)[:, None]
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    along = (d * nrm).sum(axis=1, keepdims=True)
    d = d - along * nrm + np.abs(along) * side * nrm + 0.05 * side * nrm  # mirrored into the chosen side's hemisphere
    return Q.make_rays(p.astype(f32), _nonzero(d.astype(f32)))


def aimed_rays(scene, n, seed=3):
    """From a point just off one triangle towards a point on another: rays that meet geometry in scenes that are mostly sky."""
    a, b = surface_rays(scene, n, seed), surface_rays(scene, n, seed + 1)
    o = (a["origin"][:, :3] + f32(0.01) * a["direction"][:, :3]).astype(f32)
    return Q.make_rays(o, _nonzero((b["origin"][:, :3] - o).astype(f32)))


def degenerate_rays(scene, n, seed=5):
    """From random points of the scene's box towards a vertex of each triangle whose normal is not finite (zero area): the
    records on which the triangle test computes NaNs."""
    t = scene.triangulation
    bad = np.nonzero(~np.isfinite(t["N"]).all(axis=1))[0]
    assert len(bad)
    lo, hi = Q.scene_box(scene)
    o = np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(f32)
    return Q.make_rays(o, _nonzero((t["S1"][bad[np.arange(n) % len(bad)]][:, :3] - o).astype(f32)))


W, H = 64, 48
SCENES = ("one_triangle", "big_leaf", "empty_leaves", "deep_chain", "tris20k", "hostile", "feat_textured", "feat_glass", "feat_water",
          "feat_cubemap", "matmix")
N_CORNELL, N_SCENE = 1000, 257


def scene(name):
    """The scenes of test_ray_query_gpu.py (64 x 48) by its own builder, which also knows every name scenes.build knows."""
    import test_ray_query_gpu as RQ
    return RQ.scene(name)


STRIDE = 4096  # the index_stride of the shared batches: above every batch size, so a ray's indices do not depend on the batch's
_batches = {}


def batch(name, scene, n):
    """The batch of n rays the tests send to scene `name`, chosen once (by the strict JITTERED yardstick at depth 4); the NaN-record
    scene gets 32 rays at its zero-area triangles in place of its last 32."""
    if (name, n) not in _batches:
        with np.errstate(all="ignore"):
            rays = chosen_rays(scene, n, Yardstick(scene), index_stride=STRIDE)
            if name == "hostile":
                rays[-32:] = degenerate_rays(scene, 32)
        _batches[(name, n)] = rays
    return _batches[(name, n)]


def chosen_rays(scene, n, yardstick, first_index=0, index_stride=4096, seed=0, tries=64):
    """n rays out of a pool (the generators in turn), CHOSEN BY THE YARDSTICK so that a pass of the code under test means
    something.  Of every 20 batch positions 13 ask for a path of iteration 0 with two or more surface hits, 3 for one that ends on
    the sky, 4 for nothing; position i takes the next unused candidate whose path UNDER THE INDEX OF POSITION i is of that kind
    (after `tries` candidates: the next unused one, whatever it is - a scene of one triangle has no second hit to offer).
    test_path_query_model.py asserts what came of it."""
    m = 2 * n + 64
    parts = [mixed_rays(scene, m, seed=seed), aimed_rays(scene, m, seed + 5), surface_rays(scene, m, seed + 7)]
    pool = np.zeros(3 * m, S.RAY)
    for k, p in enumerate(parts):
        pool[k::3] = p
    used = np.zeros(len(pool), bool)
    out = np.zeros(n, S.RAY)
    start = 0
    for i in range(n):
        kind = "deep" if i % 20 < 13 else ("sky" if i % 20 < 16 else "any")
        while used[start]:
            start += 1
        pick, tried, k = start, 0, start
        while kind != "any" and tried < tries and k < len(pool):
            if not used[k]:
                _, c = yardstick.path(pool[k]["origin"], pool[k]["direction"], first_index + i, 0, index_stride)
                if (c[1] >= 2) if kind == "deep" else (c[0] > c[1]):
                    pick = k
                    break
                tried += 1
            k += 1
        used[pick] = True
        out[i] = pool[pick]
    return out


def mixed_rays(scene, n, width=64, height=48, seed=0, sampler=S.JITTERED):
    """n rays of the three generators in turn (camera, interior, surface, ...)."""
    m = (n + 2) // 3
    cam = camera_rays(scene, width, height, 0, sampler)
    pix = (np.arange(m) * 1031 + (width // 2) * (height + 1)) % (width * height)
    parts = [cam[pix], interior_rays(scene, m, seed + 1), surface_rays(scene, m, seed + 2)]
    out = np.zeros(3 * m, S.RAY)
    for k, p in enumerate(parts):
        out[k::3] = p
    return out[:n]
