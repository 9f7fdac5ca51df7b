"""The screen of an in-place triangle update (csrc/scene_refit_common.h: screen_triangle), restated in NumPy, and the records it
is tried on: shared by test_update_screen_model.py (the header under g++ and the sanitizers) and
test_update_triangles_device_gpu.py (the screen kernel against the host loop).  Pure NumPy, no files.

A CASE rewrites one or two triangles of any base triangulation: the target becomes a unit right triangle (so that a case says
the same on every base: its materials and texture coordinates stay the base's), then carries the one defect, or the boundary
value, the case is about.  Each case records the code it expects; `verdict` is the restatement the model and the device are
held to.  The codes and their order are the header's: of a triangle with several defects the smallest code is reported, of
several refused triangles the one with the smallest index."""
from fractions import Fraction

import numpy as np

import scene_update_cases as U

f32, f64, u32 = np.float32, np.float64, np.uint32

OK, MATERIAL, TEXCOORD, VERTEX, NORMAL, NO_AREA, UNEQUAL_W, EMPTY_BOX, BAD_BOX = range(9)
ACCEPTED = 0xFFFFFFFF
BAD_SCENE, UNSUPPORTED = -5, -7
STATUS = {MATERIAL: BAD_SCENE, TEXCOORD: BAD_SCENE, VERTEX: UNSUPPORTED, NORMAL: UNSUPPORTED, NO_AREA: UNSUPPORTED,
          UNEQUAL_W: UNSUPPORTED, EMPTY_BOX: UNSUPPORTED, BAD_BOX: UNSUPPORTED}
# the words ptmi_update_triangles has always said, after "triangle <i> "
WORDS = {
    MATERIAL: "references a material out of range",
    TEXCOORD: "has texture coordinates that are not finite (or beyond 2^30)",
    VERTEX: "has a vertex that is not finite (or beyond 2^21)",
    NORMAL: "has a normal that is not finite (a zero-area triangle of the importer: N = 0/0)",
    NO_AREA: "has no area (its barycentric determinant is zero or not finite)",
    UNEQUAL_W: "has vertices of unequal w and the uploaded records are of the precomputed form",
    EMPTY_BOX: "has a bounding box that is marked empty",
    BAD_BOX: "has a bounding box that is not finite with pMin <= pMax",
}
REINITIALISE = ": an update cannot express that, call ptmi_initialize_memory with the new scene"


def message(word, update=True):
    """What follows "ptmi_update_triangles: " for the verdict `word` (update=False: the words alone, as build_layout says them)."""
    index, code = word >> 4, word & 15
    return f"triangle {index} {WORDS[code]}" + (REINITIALISE if update and STATUS[code] == UNSUPPORTED else "")


class Facts:
    """What the screen knows of the uploaded scene: per material whether it is a plain colour, and the record form."""

    def __init__(self, simple, precomputed=True):
        self.simple = np.ascontiguousarray(simple, np.uint8)
        self.precomputed = bool(precomputed)

    @classmethod
    def of(cls, sc, precomputed=True):
        return cls(sc.materiaux["isSimpleColor"] != 0, precomputed)

    def material(self, textured):
        """The first material that is (not) textured, or None"""
        found = np.flatnonzero((self.simple == 0) == textured)
        return int(found[0]) if len(found) else None


# ---------------------------------------------------------------------------------------------- the restatement

def fma32(a, b, c):
    """fmaf on binary32 arrays, rounded once.  The product of two binary32 values is exact in binary64; the sum is rounded to
    binary64 and then to binary32, which differs from one rounding only where the binary64 sum lies exactly half way between two
    binary32 values while the exact sum does not: those elements are redone in rational arithmetic."""
    a, b, c = a.astype(f64), b.astype(f64), c.astype(f64)
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        r = s.astype(f32)
        left = s - r.astype(f64)  # exact
        t = s - p  # TwoSum: the rounding error of s
        e = (p - (s - t)) + (c - t)
        other = np.nextafter(r, np.where(left > 0, f32(np.inf), f32(-np.inf)).astype(f32))  # the binary32 on s's other side
        tie = (r.astype(f64) + other.astype(f64)) / 2 == s  # (adjacent binary32 values: sum and half are exact)
    for k in np.flatnonzero(np.isfinite(s) & np.isfinite(r) & np.isfinite(other) & (left != 0) & (e != 0) & tie):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        if (exact > Fraction(float(s[k]))) == (float(other[k]) > float(r[k])):
            r[k] = other[k]
    return r


def dot4(a, b):
    """dot() of the kernels: fmaf(a3, b3, fmaf(a2, b2, fmaf(a1, b1, a0 * b0)))"""
    r = a[:, 0] * b[:, 0]
    r = fma32(a[:, 1], b[:, 1], r)
    r = fma32(a[:, 2], b[:, 2], r)
    r = fma32(a[:, 3], b[:, 3], r)
    return r


def determinants(t):
    """(strict, fused) of FullKernel.cl:556 per triangle: uv * uv - uu * vv and fmaf(uv, uv, -(uu * vv))"""
    with np.errstate(all="ignore"):
        u = t["S2"] - t["S1"]
        v = t["S3"] - t["S1"]
        uv = dot4(u, v)
        uu = dot4(u, u)
        vv = dot4(v, v)
        uv2 = uv * uv
        uuvv = uu * vv
        strict = uv2 - uuvv
        fused = fma32(uv, uv, -uuvv)
    return strict, fused


def usable(det):
    with np.errstate(all="ignore"):
        inverse = f32(1) / det
        return (det != 0) & np.isfinite(det) & np.isfinite(inverse)


def within(v, bound):
    """every component of every row finite and at most `bound` in magnitude (a NaN fails the <=)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(v.reshape(len(v), -1)) <= f32(bound)).all(axis=1)


def codes(tris, facts):
    """The code of every triangle: the first failing check in the header's order."""
    t = np.ascontiguousarray(tris)
    n, n_mats = len(t), len(facts.simple)
    mp, mn = t["materialWithPositiveNormalIndex"].astype(np.int64), t["materialWithNegativeNormalIndex"].astype(np.int64)
    in_range = (mp < n_mats) & (mn < n_mats)
    simple = np.concatenate([facts.simple, [1]])  # (an index out of range reads the sentinel: decided by in_range already)
    textured = (simple[np.minimum(mp, n_mats)] == 0) | (simple[np.minimum(mn, n_mats)] == 0)
    uv = np.concatenate([t[k] for k in ("UVP1", "UVP2", "UVP3", "UVN1", "UVN2", "UVN3")], axis=1)
    strict, fused = determinants(t)
    box = t["AABB"]
    lo, hi, c = box["pMin"][:, :3], box["pMax"][:, :3], box["centroid"][:, :3]
    with np.errstate(invalid="ignore"):
        equal_w = (t["S1"][:, 3] == t["S2"][:, 3]) & (t["S1"][:, 3] == t["S3"][:, 3]) & np.isfinite(t["S1"][:, 3])
        box_ok = (np.isfinite(lo) & np.isfinite(hi) & np.isfinite(c) & (lo <= hi)).all(axis=1)
    checks = [  # (code, passes)
        (MATERIAL, in_range),
        (TEXCOORD, ~textured | within(uv, 2.0 ** 30)),
        (VERTEX, within(t["S1"], 2.0 ** 21) & within(t["S2"], 2.0 ** 21) & within(t["S3"], 2.0 ** 21)),
        (NORMAL, within(t["N"], 16) & within(t["N1"], 16) & within(t["N2"], 16) & within(t["N3"], 16)),
        (NO_AREA, usable(strict) & usable(fused)),
        (UNEQUAL_W, equal_w | (not facts.precomputed)),
        (EMPTY_BOX, box["isEmpty"] == 0),
        (BAD_BOX, box_ok),
    ]
    out = np.zeros(n, u32)
    for code, passes in reversed(checks):
        out[~passes] = code
    return out


def verdict(tris, facts):
    """The whole array in one word: (index << 4) | code of the first refused triangle, or ACCEPTED."""
    c = codes(tris, facts)
    bad = np.flatnonzero(c)
    return ACCEPTED if len(bad) == 0 else (int(bad[0]) << 4) | int(c[bad[0]])


# ---------------------------------------------------------------------------------------------- the cases

def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def unit_triangle(t, i):
    """Triangle i becomes (0,0,0) (1,0,0) (0,1,0) with its own w, the normal +z on every vertex, its box following."""
    w = t["S1"][i, 3]
    w = f32(1) if not np.isfinite(w) else w
    t["S1"][i], t["S2"][i], t["S3"][i] = [0, 0, 0, w], [1, 0, 0, w], [0, 1, 0, w]
    for k in ("N", "N1", "N2", "N3"):
        t[k][i] = [0, 0, 1, 0]
    follow_box(t, i)


def follow_box(t, i):
    U.recompute_aabb(t[i:i + 1])  # (a view: writes triangle i)
    t["AABB"]["isEmpty"][i] = 0


def set_edges(t, i, u, v):
    w = t["S1"][i, 3]
    t["S2"][i], t["S3"][i] = list(u) + [w], list(v) + [w]
    follow_box(t, i)


def find_sliver(seed=20):
    """Edges (u, v) of a triangle on which the strict determinant is zero and the fused one is not - so that one arithmetic alone
    would let it through: v = u for seeded u, where uv = uu = vv and uu * uu is not exact.  Found by search, not constructed."""
    rs = np.random.default_rng(seed)
    for _ in range(1000):
        u = rs.uniform(0.1, 1.0, 3).astype(f32)
        t = np.zeros(1, U.S.Triangle)
        t["S2"][0, :3] = t["S3"][0, :3] = u
        strict, fused = determinants(t)
        if strict[0] == 0 and usable(fused)[0]:
            return u, u.copy()
    return None


SLIVER = find_sliver()


class Case:
    def __init__(self, name, code, change, pair=None, needs=None, targets=1):
        self.name, self.code, self.change, self.pair, self.needs, self.targets = name, code, change, pair, needs, targets

    def expected(self, facts):
        """The code of the reported triangle on a base with these facts (0: accepted)"""
        if self.needs == "textured" and facts.material(True) is None:
            return OK
        if self.needs == "precomputed" and not facts.precomputed:
            return OK
        return self.code

    def apply(self, tris, at, facts):
        """A byte copy of `tris` with the case at triangle index `at` (a list of `targets` ascending indices)"""
        at = [at] if np.isscalar(at) else list(at)
        assert len(at) == self.targets and at == sorted(at)
        t = U.raw_copy(tris)
        for i in at:
            unit_triangle(t, i)
        self.change(t, at, facts)
        return t

    def word(self, at, facts):
        at = [at] if np.isscalar(at) else list(at)
        code = self.expected(facts)
        return ACCEPTED if code == OK else (at[0] << 4) | code


def _field(name, component, value, box=False):
    def change(t, at, facts):
        t[name][at[0], component] = value
        if box:
            follow_box(t, at[0])
    return change


def _box(corner, component, value):
    def change(t, at, facts):
        t["AABB"][corner][at[0], component] = value
    return change


def _uv(value, textured):
    def change(t, at, facts):
        m = facts.material(textured)
        if m is not None:
            t["materialWithPositiveNormalIndex"][at[0]] = m
            if not textured:
                t["materialWithNegativeNormalIndex"][at[0]] = m
        t["UVN2"][at[0], 1] = value
    return change


def _material(field, value):
    def change(t, at, facts):
        t[field][at[0]] = value(facts)
    return change


def _edges(u, v):
    return lambda t, at, facts: set_edges(t, at[0], u, v)


def _unequal_w(t, at, facts):
    t["S2"][at[0], 3] = t["S2"][at[0], 3] * f32(2) + f32(1)


def _empty(t, at, facts):
    t["AABB"]["isEmpty"][at[0]] = 1


def _pmin_against_pmax(step):
    def change(t, at, facts):
        hi = t["AABB"]["pMax"][at[0], 1]
        t["AABB"]["pMin"][at[0], 1] = up(hi) if step else hi
    return change


def _nan_vertex_and_empty_box(t, at, facts):
    t["S3"][at[0], 0] = np.nan
    _empty(t, at, facts)


def _later_check_first(t, at, facts):
    _empty(t, at[:1], facts)           # the earlier triangle fails a later check
    t["S1"][at[1], 2] = np.nan         # the later triangle an earlier one


P = 2.0 ** -32
CASES = [
    Case("coord_2^21", OK, _field("S2", 0, f32(2.0 ** 21), box=True), pair="coord"),
    Case("coord_above_2^21", VERTEX, _field("S2", 0, up(2.0 ** 21), box=True), pair="coord"),
    Case("coord_minus_2^21", OK, _field("S3", 2, f32(-2.0 ** 21), box=True), pair="coord_negative"),
    Case("coord_below_minus_2^21", VERTEX, _field("S3", 2, -up(2.0 ** 21), box=True), pair="coord_negative"),
    Case("normal_16", OK, _field("N", 0, f32(16)), pair="normal"),
    Case("normal_above_16", NORMAL, _field("N", 0, up(16)), pair="normal"),
    Case("vertex_normal_16", OK, _field("N2", 1, f32(-16)), pair="vertex_normal"),
    Case("vertex_normal_above_16", NORMAL, _field("N2", 1, -up(16)), pair="vertex_normal"),
    Case("nan_w", VERTEX, _field("S2", 3, np.nan)),
    Case("infinite_normal", NORMAL, _field("N3", 2, np.inf)),
    Case("uv_2^30_textured", OK, _uv(f32(2.0 ** 30), True), pair="uv", needs="textured"),
    Case("uv_above_2^30_textured", TEXCOORD, _uv(up(2.0 ** 30), True), pair="uv", needs="textured"),
    Case("uv_nan_textured", TEXCOORD, _uv(np.nan, True), pair="uv_nan", needs="textured"),
    Case("uv_nan_plain", OK, _uv(np.nan, False), pair="uv_nan"),
    Case("material_last", OK, _material("materialWithNegativeNormalIndex", lambda f: len(f.simple) - 1), pair="material"),
    Case("material_count", MATERIAL, _material("materialWithNegativeNormalIndex", lambda f: len(f.simple)), pair="material"),
    Case("material_ffffffff", MATERIAL, _material("materialWithPositiveNormalIndex", lambda f: 0xFFFFFFFF)),
    Case("s3_equals_s2", NO_AREA, _edges((1, 0, 0), (1, 0, 0))),
    Case("determinant_-2^-127", OK, _edges((0, 0, P), (P, P, 0)), pair="determinant"),
    Case("determinant_-2^-128", NO_AREA, _edges((P, 0, 0), (0, P, 0)), pair="determinant"),
    Case("sliver_strict_zero_fused_not", NO_AREA, lambda t, at, facts: set_edges(t, at[0], *SLIVER)),
    Case("unequal_w", UNEQUAL_W, _unequal_w, needs="precomputed"),
    Case("is_empty", EMPTY_BOX, _empty),
    Case("pmin_equals_pmax", OK, _pmin_against_pmax(False), pair="box_order"),
    Case("pmin_above_pmax", BAD_BOX, _pmin_against_pmax(True), pair="box_order"),
    Case("infinite_centroid", BAD_BOX, _box("centroid", 2, np.inf)),
    Case("nan_pmin", BAD_BOX, _box("pMin", 0, np.nan)),
    Case("nan_vertex_and_empty_box", VERTEX, _nan_vertex_and_empty_box),
    Case("later_triangle_earlier_check", EMPTY_BOX, _later_check_first, targets=2),
]
BY_NAME = {c.name: c for c in CASES}


def check_the_list():
    """What the list promises of itself: every code occurs, every boundary pair has one accepted and one refused member, the
    sliver was found and is what it is called."""
    assert len(BY_NAME) == len(CASES)
    assert {c.code for c in CASES} == set(range(9)), sorted({c.code for c in CASES})
    pairs = {}
    for c in CASES:
        if c.pair:
            pairs.setdefault(c.pair, []).append(c.code)
    for name, members in pairs.items():
        assert len(members) == 2 and sorted(x != OK for x in members) == [False, True], (name, members)
    assert SLIVER is not None
    t = np.zeros(1, U.S.Triangle)
    t["S2"][0, :3], t["S3"][0, :3] = SLIVER
    strict, fused = determinants(t)
    assert strict[0] == 0 and fused[0] != 0 and usable(fused)[0] and not usable(strict)[0]
