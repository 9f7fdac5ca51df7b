"""The yardstick of ptmi_render_guides (test_guide_buffers_model.py, test_guide_buffers_gpu.py).  No product code is involved.

One sample (gx, gy, it) is pto_trace_path of the CPU oracle with ray_max_depth = 1: Kernel_Main's own seed, sampler, camera
expression, Ray3D_Create and BVH_IntersectRay, in either arithmetic, stopped after the first segment.  The function returns 1
for a miss as well as for one bounce, so the bounce record is pre-filled with triangle_id = 0xFFFFFFFF: a record that still
carries it was not written, which is a miss.

  a hit   triangle_id, material_id, point and ns are the record's.  `front` is the side Triangle_Intersects picked the material
          by: material_id == materialWithPositiveNormalIndex where the triangle's two materials differ, else
          pto_triangle_intersects_side on that triangle with the primary ray, which this module builds from pto_sampler and
          the camera expression of cl:1213 in the oracle's arithmetic (f32_cases.camera_direction).  That second ray checks itself: the triangle must accept it with the record's s, t and point, bit for bit.
          The albedo is the material's simpleColor where isSimpleColor is set; else, for MAT_STANDART, the record's transfer
          (Scene_ComputeRadiance multiplies the initial transfer of 1 by the colour: 1 * c is c exactly).  A hit on a TEXTURED
          material of another type has no bit-exact albedo from this oracle (glass and water scale the texel, varnish may not
          apply it): it is excluded from the albedo comparison, and from that comparison only.
  a miss  the returned radiance is the sky's colour: sky * 1 + 0.

Sums are np.float32 additions in iteration order, starting at +0.  An iteration of a scene is traced once and kept.
"""
import ctypes as C

import numpy as np

from opencl_pathtracer_amd import structs as S
from f32_cases import bits as _bits, c4 as _c4, camera_direction
import oracle_ffi as O

f32 = np.float32
MISS = 0xFFFFFFFF
PLANES = ("albedo", "normal", "position", "hit_count", "ids")
MAX_EXCLUDED = 0.10  # of a scene's hit samples: a condition on the scenes the tests choose, not a measurement


# ---------------------------------------------------------------------------------------------- the primary ray

def _same_words(a, b):
    """bit-equal, a NaN matching any NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------- one scene

class Yardstick:
    """One scene, image size, sampler and arithmetic.  iteration(it) -> the per-pixel records of that iteration;
    planes(first, n) -> the five planes ptmi_render_guides must return, and the mask of pixels without a bit-exact albedo."""

    def __init__(self, scene, width, height, sampler=S.JITTERED, default_arithmetic=False, source_seed=False):
        assert sampler in (S.JITTERED, S.UNIFORM)
        self.scene, self.w, self.h, self.sampler, self.fused, self.source_seed = scene, width, height, sampler, default_arithmetic, source_seed
        self.lib = O.oracle(default_arithmetic)
        self.lib.pto_sample_pixel.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_float]
        self.lib.pto_sample_pixel.restype = C.c_uint32
        self.osc = O.OracleScene(scene, width, height, 1, sampler, source_seed=source_seed)
        self.tris = np.ascontiguousarray(scene.triangulation)
        self.mats = np.ascontiguousarray(scene.materiaux)
        self.mat_pos = self.tris["materialWithPositiveNormalIndex"].tolist()
        self.mat_neg = self.tris["materialWithNegativeNormalIndex"].tolist()
        self.origin = _c4(scene.cameraPosition)
        self._iterations = {}

    def primary_ray(self, gx, gy, it):
        """(sample, un-normalised direction) of Kernel_Main's ray for (gx, gy, it)"""
        seed = C.c_int32(self.lib.pto_initialize_random_seed(gx, gy, self.w, self.h, it))
        if self.source_seed and seed.value == 0:
            seed.value = 1
        sample = (C.c_float * 2)()
        self.lib.pto_sampler(self.sampler, gx, gy, self.w, self.h, it, C.byref(seed), sample)
        return (sample[0], sample[1]), camera_direction(self.scene, sample, self.fused)

    def side_by_primary_ray(self, tri, s, t, point, gx, gy, it):
        """The side of triangle `tri` that this module's own primary ray of (gx, gy, it) meets.  The ray checks itself: the
        triangle must accept it with the hit's s, t and point, bit for bit."""
        _, direction = self.primary_ray(gx, gy, it)
        lim, s_, t_, p, side = C.c_float(np.inf), C.c_float(0), C.c_float(0), (C.c_float * 4)(), C.c_int(0)
        ok = self.lib.pto_triangle_intersects_side(C.c_void_p(self.tris.ctypes.data + 336 * tri), self.origin, _c4(direction),
                                                   C.byref(lim), C.byref(s_), C.byref(t_), p, C.byref(side))
        assert ok and _same_words([s_.value, t_.value], [s, t]) and _same_words(tuple(p), tuple(point)), \
            f"the yardstick's own primary ray does not reproduce the hit of sample ({gx}, {gy}, {it})"
        return 1 if side.value else 0

    def _front(self, b, gx, gy, it):
        tri = b.triangle_id
        if self.mat_pos[tri] != self.mat_neg[tri]:
            return 1 if b.material_id == self.mat_pos[tri] else 0
        return self.side_by_primary_ray(tri, b.s, b.t, b.point, gx, gy, it)

    def sample(self, gx, gy, it):
        """dict(hit, triangle_id, material_id, front, point, ns, s, t, albedo (None: no bit-exact one), sky)"""
        bounce = (O.PtoBounce * 1)()
        bounce[0].triangle_id = MISS
        radiance = (C.c_float * 4)()
        n = self.lib.pto_trace_path(C.byref(self.osc.c), gx, gy, it, bounce, 1, radiance)
        assert n == 1
        b = bounce[0]
        if b.triangle_id == MISS:
            return dict(hit=False, sky=np.array(radiance[:], f32))
        mat = self.mats[b.material_id]
        if mat["isSimpleColor"]:
            albedo = np.array(mat["simpleColor"], f32)
        elif mat["type"] == S.MAT_STANDART:
            albedo = np.array(b.transfer[:], f32)
        else:
            albedo = None
        return dict(hit=True, triangle_id=b.triangle_id, material_id=b.material_id, front=self._front(b, gx, gy, it),
                    point=np.array(b.point[:], f32), ns=np.array(b.ns[:], f32), s=b.s, t=b.t, albedo=albedo,
                    textured=not mat["isSimpleColor"])

    def lands_in_its_own_pixel(self, gx, gy, it):
        (sx, sy), _ = self.primary_ray(gx, gy, it)
        return self.lib.pto_sample_pixel(self.w, self.h, sx, sy) == gy * self.w + gx

    def iteration(self, it):
        if it not in self._iterations:
            h, w = self.h, self.w
            r = dict(hit=np.zeros((h, w), bool), excluded=np.zeros((h, w), bool), textured=np.zeros((h, w), bool),
                     albedo=np.zeros((h, w, 4), f32), normal=np.zeros((h, w, 4), f32), position=np.zeros((h, w, 4), f32),
                     ids=np.zeros((h, w, 4), np.uint32))
            r["ids"][..., 0] = MISS
            with np.errstate(all="ignore"):
                for gy in range(h):
                    for gx in range(w):
                        s = self.sample(gx, gy, it)
                        if not s["hit"]:
                            r["albedo"][gy, gx] = s["sky"]
                            continue
                        r["hit"][gy, gx], r["textured"][gy, gx] = True, s["textured"]
                        r["normal"][gy, gx], r["position"][gy, gx] = s["ns"], s["point"]
                        r["ids"][gy, gx] = (s["triangle_id"], s["material_id"], s["front"], 0)
                        if s["albedo"] is None:
                            r["excluded"][gy, gx] = True
                        else:
                            r["albedo"][gy, gx] = s["albedo"]
            self._iterations[it] = r
        return self._iterations[it]

    def planes(self, first, n):
        """(dict of the five planes, bool[H,W]: pixels whose albedo sum holds a sample without a bit-exact albedo)"""
        h, w = self.h, self.w
        out = dict(albedo=np.zeros((h, w, 4), f32), normal=np.zeros((h, w, 4), f32), position=np.zeros((h, w, 4), f32),
                   hit_count=np.zeros((h, w), f32), ids=self.iteration(first)["ids"].copy() if n else None)
        excluded = np.zeros((h, w), bool)
        with np.errstate(all="ignore"):
            for it in range(first, first + n):
                r = self.iteration(it)
                hit = r["hit"]
                out["albedo"] = (out["albedo"] + r["albedo"]).astype(f32)
                out["normal"] = np.where(hit[..., None], (out["normal"] + r["normal"]).astype(f32), out["normal"])
                out["position"] = np.where(hit[..., None], (out["position"] + r["position"]).astype(f32), out["position"])
                out["hit_count"] = np.where(hit, (out["hit_count"] + f32(1)).astype(f32), out["hit_count"])
                excluded |= r["excluded"]
        return out, excluded

    def census(self, iterations):
        """dict(hits, misses, excluded, textured_hits, fronts) over the samples of `iterations`"""
        rs = [self.iteration(it) for it in iterations]
        hits = sum(int(r["hit"].sum()) for r in rs)
        return dict(hits=hits, misses=sum(int((~r["hit"]).sum()) for r in rs), excluded=sum(int(r["excluded"].sum()) for r in rs),
                    textured_hits=sum(int((r["textured"] & ~r["excluded"]).sum()) for r in rs),
                    fronts=sorted({int(v) for r in rs for v in np.unique(r["ids"][..., 2][r["hit"]])}))


# ---------------------------------------------------------------------------------------------- comparison

def describe_difference(got, want, excluded=None):
    """'' when every plane of `got` equals `want`'s as uint32 words - where the yardstick's word is a NaN the kernel's must be
    a NaN, of any sign and payload; every other word must be equal - else which planes differ, on how many pixels, and the
    first such pixel.  `excluded`: pixels left out of the albedo comparison (and of no other)."""
    lines = []
    for name in PLANES:
        if name not in got:
            continue
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        equal = g.view(np.uint32) == w.view(np.uint32)
        if name != "ids":
            equal |= np.isnan(g) & np.isnan(w)
        if equal.ndim == 3:
            equal = equal.all(axis=2)
        if name == "albedo" and excluded is not None:
            equal |= excluded
        if not equal.all():
            bad = np.argwhere(~equal)
            gy, gx = (int(v) for v in bad[0])
            lines.append(f"{name}: {len(bad)} of {equal.size} pixels differ; first (gx {gx}, gy {gy}): got {g[gy, gx]}, want {w[gy, gx]}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------- the scenes and calls of the tests

W, H = 64, 48
CORNELL_CALLS = ((0, 1), (0, 3), (7, 2))  # (first_iteration, n_iterations): ids follow `first`, sums follow iteration order
SCENE_CALL = (5, 2)                        # what every other scene is asked
SCENES = ("one_triangle", "big_leaf", "empty_leaves", "deep_chain", "feat_textured", "feat_two_sided", "matmix", "mayalike_s",
          "tris20k", "hostile")
_scenes, _yardsticks = {}, {}


def scene(name):
    """The scenes of the GPU tests at W x H, built as test_ray_query_gpu.py builds its own (cached)."""
    import warnings
    from opencl_pathtracer_amd import bvh_create, scenes
    import bvh_stress_cases as stress
    from gpu_cases import cached_scene
    if name not in _scenes:
        if name == "one_triangle":
            sc = scenes.cornell_box(W, H)
            sc.triangulation = scenes._concat_tris([sc.triangulation[5:6]])
            sc = bvh_create(sc)
            assert sc.bvh["isLeaf"][0] and len(sc.bvh) == 1
        elif name == "deep_chain":
            sc = scenes.cornell_box(W, H)
            sc.triangulation = stress.make("deep_chain_27", 0, 56)
            sc = bvh_create(sc)
            assert sc.bvhMaxDepth > 22
        elif name == "hostile":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (the hostile scenes divide 0 by 0 on purpose, as the importer would)
                sc = bvh_create(scenes.add_zero_area_triangles(scenes.build("fuzz5h_l1", W, H), 24))
        elif name == "feat_two_sided_from_behind":
            sc = behind_the_sheet(scene("feat_two_sided"))
        else:
            sc = cached_scene(name, W, H)
        _scenes[name] = sc
    return _scenes[name]


def behind_the_sheet(sc):
    """feat_two_sided with the camera on the far side of its free-standing sheet (scenes.feature_scene: the quad from (-4, -1) to
    (-2, 1), whose normal points to +x -y): from the scene's own camera every primary ray meets a surface from its positive
    side; from here the sheet and the back wall show their negative sides, which carry another material."""
    import copy
    from opencl_pathtracer_amd import scenes
    out = copy.copy(sc)
    span = 0.9
    out.cameraPosition, out.cameraDirection, out.cameraRight, out.cameraUp = scenes.camera(
        (-9.0, 6.0, 2.0), (1.0, -1.0, -0.12), (-0.7 * span, -0.7 * span, 0), (0, 0, span * H / W))
    return out


def yardstick(name, sampler=S.JITTERED, default_arithmetic=False):
    key = (name, sampler, default_arithmetic)
    if key not in _yardsticks:
        _yardsticks[key] = Yardstick(scene(name), W, H, sampler, default_arithmetic)
    return _yardsticks[key]


def calls_of(name):
    return CORNELL_CALLS if name == "cornell" else (SCENE_CALL,)


def iterations_of(name):
    return sorted({it for first, n in calls_of(name) for it in range(first, first + n)})
