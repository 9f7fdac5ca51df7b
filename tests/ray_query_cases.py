"""The yardstick of ptmi_query_rays (test_ray_query_model.py, test_ray_query_gpu.py): a Python walk of the caller's tree in the
reference's layout (scene.bvh, scene.triangulation after bvh_create) in the visit order of BVH_IntersectRay /
BVH_IntersectShadowRay (FullKernel.cl:620-783), and the rays the tests send.  No product code is involved.

The walk has no arithmetic of its own: every box decision is pto_bounding_box_intersects on the son's trianglesAABB, every
triangle decision pto_triangle_intersects, both of the CPU oracle (oracle_ffi.oracle, either arithmetic), which make their ray
with the oracle's ray_create from the caller's origin and direction.  Two things the oracle's entry points do not hand out are
decided here, by rules instead of arithmetic:

  * which son is the near one: the sign of the NORMALISED direction's cutAxis component.  normalize() keeps the sign of every
    component of a finite vector (it multiplies by one positive number) unless the component underflows; `_signs` refuses
    directions where that could happen (a component below 1e-30 of the largest) and applies the library's rules for the rest:
    any NaN component makes every component NaN (no `> 0` holds), an infinite one leaves (+-1, 0 elsewhere).
  * `front` = dot(N, direction) < 0: the triangle test accepts only where that dot product is at least 1e-5 in magnitude or not
    a number, a hundred times the rounding error of a float dot product of unit vectors, so its sign is that of the same sum in
    float64 (`_front` checks the margin and refuses otherwise); a NaN sum compares false.

Counts: the root box is not tested, an inner node counts its two sons' boxes, a tested triangle counts 1.
"""
import ctypes as C

import numpy as np

from opencl_pathtracer_amd import structs as S
from f32_cases import c4 as _c4
import oracle_ffi as O

f32 = np.float32
MISS = 0xFFFFFFFF


def _signs(d):
    """(x > 0, y > 0, z > 0) of normalize(d), by rule (see the module's docstring)."""
    d = np.asarray(d, np.float64)
    if np.isnan(d).any():
        return (False, False, False)
    if np.isinf(d).any():
        return tuple(bool(np.isinf(c) and c > 0) for c in d[:3])
    big = np.abs(d).max()
    for c in d[:3]:
        if c != 0 and abs(c) < 1e-30 * big:
            raise ValueError("a direction component could underflow in normalize(): the yardstick does not decide its sign")
    return tuple(bool(c > 0) for c in d[:3])


def _front(n, d):
    d = np.asarray(d, np.float64)
    if np.isinf(d).any() and not np.isnan(d).any():
        d = np.where(np.isinf(d), np.sign(d), 0.0)
    with np.errstate(all="ignore"):
        nd = float(np.dot(np.asarray(n, np.float64), d))
        norm = float(np.sqrt(np.dot(d, d)))
    if nd != nd or norm != norm:
        return 0
    if not abs(nd) > 1e-6 * norm:
        raise ValueError("an accepted triangle with |dot(N, dir)| below the acceptance threshold: the yardstick does not decide its side")
    return 1 if nd < 0 else 0


class Walker:
    """One scene in one arithmetic.  closest(o, d, limit) / any_hit(o, d, limit) -> a dict with the fields of ptmi_ray_hit."""

    def __init__(self, scene, default_arithmetic=False):
        self.lib = O.oracle(default_arithmetic)
        self.bvh = np.ascontiguousarray(scene.bvh)
        self.tris = np.ascontiguousarray(scene.triangulation)
        assert self.bvh.dtype == S.Node and self.tris.dtype == S.Triangle
        self.box_base, self.tri_base = self.bvh.ctypes.data, self.tris.ctypes.data
        b = self.bvh
        self.leaf = [bool(x) for x in b["isLeaf"]]
        self.start, self.count = b["triangleStartIndex"].tolist(), b["nbTriangles"].tolist()
        self.son1, self.son2, self.axis = b["son1Id"].tolist(), b["son2Id"].tolist(), b["cutAxis"].tolist()
        self.normal = self.tris["N"]

    def _box(self, node, o, d, limit):
        return self.lib.pto_bounding_box_intersects(C.c_void_p(self.box_base + 160 * node), o, d, limit) != 0

    def _tri(self, i, o, d, st):
        """pto_triangle_intersects on triangle i with the running limit st['sqd']; on acceptance st takes the hit."""
        lim, s, t, p = C.c_float(st["sqd"]), C.c_float(0), C.c_float(0), (C.c_float * 4)()
        if not self.lib.pto_triangle_intersects(C.c_void_p(self.tri_base + 336 * i), o, d, C.byref(lim), C.byref(s), C.byref(t), p):
            return False
        st.update(sqd=lim.value, s=s.value, t=t.value, point=tuple(p), id=i)
        return True

    def _result(self, st, found, direction, n_box, n_tri):
        if not found:
            return dict(point=(0.0, 0.0, 0.0, 0.0), squared_distance=0.0, s=0.0, t=0.0, triangle_id=MISS, front=0, box_tests=n_box, triangle_tests=n_tri)
        return dict(point=st["point"], squared_distance=st["sqd"], s=st["s"], t=st["t"], triangle_id=st["id"],
                    front=_front(self.normal[st["id"]], direction), box_tests=n_box, triangle_tests=n_tri)

    def walk(self, origin, direction, limit=np.inf, any_hit=False, on_push=None):
        """on_push: called with the number of pending entries after every push (stack_depth_cases.py reads the stack's
        occupancy off it); it changes nothing of the walk."""
        o, d = _c4(origin), _c4(direction)
        positive = _signs(direction)
        st = dict(sqd=float(f32(limit)))
        found, n_box, n_tri = False, 0, 0
        stack, cur = [], 0
        while True:
            if self.leaf[cur]:
                for i in range(self.start[cur], self.start[cur] + self.count[cur]):
                    n_tri += 1
                    if self._tri(i, o, d, st):
                        found = True
                        if any_hit:
                            return self._result(st, True, direction, n_box, n_tri)
                if not stack:
                    break
                cur = stack.pop()
            else:
                near, far = (self.son1[cur], self.son2[cur]) if positive[self.axis[cur]] else (self.son2[cur], self.son1[cur])
                lim = C.c_float(st["sqd"])
                h_near, h_far = self._box(near, o, d, lim), self._box(far, o, d, lim)
                n_box += 2
                if h_near:
                    if h_far:
                        stack.append(far)
                        if on_push is not None:
                            on_push(len(stack))
                    cur = near
                elif h_far:
                    cur = far
                else:
                    if not stack:
                        break
                    cur = stack.pop()
        return self._result(st, found, direction, n_box, n_tri)

    def brute_force(self, origin, direction, limit=np.inf):
        """Closest hit without a tree: every triangle in index order with a running limit."""
        o, d = _c4(origin), _c4(direction)
        st = dict(sqd=float(f32(limit)))
        found = False
        for i in range(len(self.tris)):
            found |= self._tri(i, o, d, st)
        return self._result(st, found, direction, 0, len(self.tris))

    def at_distance(self, origin, direction, sqd):
        """The triangles that the test accepts under the limit `sqd` at exactly that squared distance (bit-equal): two = a tie."""
        o, d = _c4(origin), _c4(direction)
        out = []
        for i in range(len(self.tris)):
            st = dict(sqd=float(sqd))
            if self._tri(i, o, d, st) and f32(st["sqd"]).view(np.uint32) == f32(sqd).view(np.uint32):
                out.append(i)
        return out


def expected_hits(scene, rays, any_hit=False, default_arithmetic=False, walker=None):
    """The structs.RAY_HIT array ptmi_query_rays must return for `rays` (structs.RAY) on `scene`."""
    w = walker or Walker(scene, default_arithmetic)
    out = np.zeros(len(rays), S.RAY_HIT)
    for k, r in enumerate(rays):
        h = w.walk(r["origin"], r["direction"], r["max_squared_distance"], any_hit)
        for name in ("point", "squared_distance", "s", "t", "triangle_id", "front", "box_tests", "triangle_tests"):
            out[name][k] = h[name]
    return out


def words(hits):
    """uint32[n, 12] view of a RAY_HIT array: what the tests compare."""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(len(hits), 12)


FIELD_WORDS = dict(point=slice(0, 4), squared_distance=4, s=5, t=6, triangle_id=7, front=8, box_tests=9, triangle_tests=10, reserved=11)


def describe_difference(got, want, nan_bits=True):
    """'' when bit-equal, else which fields differ on how many rays and the first such ray.
    nan_bits=False: a float word that is a NaN on both sides counts as equal whatever its sign and payload (for the rays of
    which the walk cannot say WHICH NaN: test_ray_query_gpu.py::test_rays_that_are_not_finite says which and why); a NaN
    against a number, and every other word, still differ."""
    g, w = words(got), words(want)
    if not nan_bits:
        g, w = g.copy(), w.copy()
        fg, fw = g[:, :7].view(f32), w[:, :7].view(f32)  # point, squared_distance, s, t
        both = np.isnan(fg) & np.isnan(fw)
        fg[both], fw[both] = np.nan, np.nan
    if np.array_equal(g, w):
        return ""
    bad = np.nonzero((g != w).any(axis=1))[0]
    fields = [name for name, sl in FIELD_WORDS.items() if (g[:, sl] != w[:, sl]).any()]
    k = int(bad[0])
    return f"{len(bad)} of {len(g)} hits differ in {fields}; first: ray {k}\n  got  {got[k]}\n  want {want[k]}"


# ---------------------------------------------------------------------------------------------- rays

def make_rays(origins, directions, limits=None, origin_w=1.0):
    """structs.RAY records.  An (n,3) origin gets w = `origin_w`: the scenes of this repository carry w = 1 on every point AND on
    the triangles' N (as the reference's importer writes them), and the plane equation of Triangle_Intersects is a 4-wide dot
    product, so a ray means what geometry expects when its origin has w = 1 like the cameras' positions (N.w * S1.w - N.w * o.w
    cancels).  test_ray_query_gpu.py sends origins with w = 0 too: the displaced hits are part of what must be reproduced."""
    o, d = np.asarray(origins, f32), np.asarray(directions, f32)
    rays = np.zeros(len(o), S.RAY)
    rays["origin"][:, 3] = origin_w
    rays["origin"][:, :o.shape[1]] = o
    rays["direction"][:, :d.shape[1]] = d
    rays["max_squared_distance"] = np.inf if limits is None else np.asarray(limits, f32)
    return rays


def scene_box(scene):
    t = scene.triangulation
    p = np.concatenate([t["S1"][:, :3], t["S2"][:, :3], t["S3"][:, :3]])
    p = p[np.isfinite(p).all(axis=1) & (np.abs(p) < 1e9).all(axis=1)]
    return p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)


def pinhole_rays(scene, n, width=64, height=48):
    """Camera rays through the centres of n pixels scattered over a width x height image: direction + right * x + up * y, with x, y
    in [-0.5, 0.5] (FullKernel.cl:1213), origin the camera position."""
    k = np.arange(n)
    pix = (k * 1031 + (width // 2) * (height + 1)) % (width * height)  # (the centre pixel first, then a stride coprime to the usual sizes)
    x = (((pix % width) + 0.5) / width - 0.5).astype(f32)[:, None]
    y = (((pix // width) + 0.5) / height - 0.5).astype(f32)[:, None]
    cd, cr, cu = (np.asarray(v, f32)[None, :] for v in (scene.cameraDirection, scene.cameraRight, scene.cameraUp))
    d = (cd + cr * x + cu * y).astype(f32)
    return make_rays(np.tile(np.asarray(scene.cameraPosition, f32), (n, 1)), d)


def segment_rays(scene, n, seed=1, limited=True):
    """From one random point of the scene's box towards another; every second one limited to the segment (line of sight)."""
    rs = np.random.default_rng(seed)
    lo, hi = scene_box(scene)
    pad = 0.05 * (hi - lo) + 1e-3
    p, q = rs.uniform(lo - pad, hi + pad, (n, 3)).astype(f32), rs.uniform(lo - pad, hi + pad, (n, 3)).astype(f32)
    d = (q - p).astype(f32)
    lim = np.full(n, np.inf, f32)
    if limited:
        lim[1::2] = (d.astype(np.float64) ** 2).sum(axis=1)[1::2]
    return make_rays(p, d, lim)


def grazing_rays(scene, n, seed=2):
    """Rays at the 1e-5 thresholds of Triangle_Intersects: from a point just above a triangle straight down onto it, at heights
    around sqrt(1e-5) (the squared-distance threshold, cl:543), and along the triangle's plane with a normal component around
    1e-5 (the parallelism threshold, cl:533)."""
    rs = np.random.default_rng(seed)
    t = scene.triangulation
    ok = np.nonzero(np.isfinite(t["N"]).all(axis=1) & np.isfinite(t["S1"]).all(axis=1) & np.isfinite(t["S2"]).all(axis=1) & np.isfinite(t["S3"]).all(axis=1))[0]
    pick = ok[rs.integers(0, len(ok), n)]
    a, b = rs.uniform(0.05, 0.45, n)[:, None], rs.uniform(0.05, 0.45, n)[:, None]
    s1, s2, s3, nrm = (t[f][pick][:, :3].astype(np.float64) for f in ("S1", "S2", "S3", "N"))
    p = s1 + a * (s2 - s1) + b * (s3 - s1)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    side = np.where(rs.random(n) < 0.5, 1.0, -1.0)[:, None]
    down = np.arange(n) % 2 == 0
    h = np.sqrt(1e-5) * rs.uniform(0.9, 1.1, n)[:, None]
    o[down] = (p + side * nrm * h)[down]
    d[down] = (-side * nrm)[down]
    edge = s2 - s1
    edge /= np.linalg.norm(edge, axis=1, keepdims=True)
    o[~down] = (p - 0.3 * edge + side * nrm * 3e-6 * rs.uniform(0.5, 2.0, n)[:, None])[~down]
    d[~down] = (edge - side * nrm * 1e-5 * rs.uniform(0.5, 2.0, n)[:, None])[~down]
    return make_rays(o.astype(f32), d.astype(f32))


def axis_rays(scene, n, seed=3):
    """Axis-parallel rays: two direction components are exactly zero, so their reciprocals are infinite and the box test keeps
    its literal form (FullKernel.cl:64-139).  Half of them have those zeros NEGATIVE: the reciprocal is -inf, the slab of such
    an axis spans (-inf, +inf) when the origin lies inside it, and the ray behaves as geometry expects.  The other half have
    them POSITIVE: the reciprocal is +inf, the slab's near end is +inf and its far end -inf, and the reference's test fails
    EVERY box - such a ray misses whatever lies in front of it (`has_positive_zero`).  Both are what the integrator must
    reproduce."""
    rs = np.random.default_rng(seed)
    lo, hi = scene_box(scene)
    o = rs.uniform(lo, hi, (n, 3)).astype(f32)
    k = np.arange(n)
    d = np.where(((k // 6) % 2 == 1)[:, None], f32(-0.0), f32(0.0)) * np.ones((n, 3), f32)
    d[k, k % 3] = np.where((k // 3) % 2 == 0, 1.0, -1.0)
    d[(k // 12) % 2 == 1] *= f32(2.5)  # (not all of unit length)
    return make_rays(o, d.astype(f32))


def has_positive_zero(ray):
    """A direction component that is +0: 1 / +0 = +inf puts that slab's near end at +inf and its far end at -inf, so
    BoundingBox_Intersects returns false for every box (cl:101-102 or :85-86) and the tree walk finds nothing."""
    d = np.asarray(ray["direction"], f32)[:3]
    return bool(((d == 0) & ~np.signbit(d)).any())


def limited_rays(rays, closest):
    """`rays` that hit something (closest = their closest hits), three times over: limited to the squared distance of their own
    closest hit, to one ulp below it, and to 0."""
    hit = closest["triangle_id"] != MISS
    base, sqd = rays[hit], closest["squared_distance"][hit]
    out = []
    for lim in (sqd, np.nextafter(sqd, f32(0)), np.zeros(len(sqd), f32)):
        r = base.copy()
        r["max_squared_distance"] = lim
        out.append(r)
    return np.concatenate(out) if out else rays[:0]


def mixed_rays(scene, n, width=64, height=48, seed=0):
    """n rays of the four generators in turn (pinhole, segment, grazing, axis-parallel, ...)."""
    m = (n + 3) // 4
    parts = [pinhole_rays(scene, m, width, height), segment_rays(scene, m, seed + 1), grazing_rays(scene, m, seed + 2), axis_rays(scene, m, seed + 3)]
    out = np.zeros(4 * m, S.RAY)
    for k, p in enumerate(parts):
        out[k::4] = p
    return out[:n]
