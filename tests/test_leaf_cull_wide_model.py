"""The wide tier of csrc/leaf_cull.h on the CPU: its two inequalities, its claim, whole walks at the kernel's levels, the tight
tier left bit for bit what it was, and both tiers' life through an update.

The kernel culls a leaf that carries the tight OR the wide bit under ONE rule, the wide one (kernel_wavefront.hip: node_step).
THE CLAIM for that: the wide rule fired on a wide-certified leaf => pto_triangle_intersects, the oracle's float restatement of
Triangle_Intersects, rejects - on the cases of tests/test_leaf_cull_model.py (random, grazing, slivers, vertex-on-face, grown
boxes, scales 1e-3 .. 1e4), with limits within +-3 ulp of the WIDE rule's own boundary and at 0.3 .. 0.98 of D^2.  A tight
certificate implies the wide one and the wide rule the tight one (both asserted per case): a tight leaf under the wide rule is
covered twice.
THE WALK: tests/leaf_cull_wide_model.cpp walks build_layout's records as node_step does at every level of PTMI_LEAF_CULL; each
must equal the plain walk in hit record, limit bits, box tests and triangle tests.
"""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import bvh_create, scenes
import leaf_cull_cases as K
import leaf_cull_wide_cases as KW
import oracle_ffi as O
import scene_update_cases as U
import test_leaf_cull_model as M

f32 = np.float32
W = H = 64
DEPTH = 6


@pytest.fixture(scope="module")
def model(tmp_path_factory, built):
    return KW.build_model(tmp_path_factory.mktemp("leaf_cull_wide_model"))


def wide_constants(model):
    c = (C.c_double * 4)()
    model.wide_constants(c)
    return dict(rel=c[0], abs=c[1], kappa_max=c[2], eps_abs_max=c[3])


def test_wide_constants_satisfy_the_proofs_two_inequalities(model):
    """with eta = (kRelWide - 1) / 2, (1 - kappa)^2 (1 - eta) kRelWide >= 1 + 40u and eps_abs^2 / eta <= 0.99 kAbsWide."""
    c = wide_constants(model)
    eta, u = (c["rel"] - 1) / 2, 2.0 ** -24
    assert (1 - c["kappa_max"]) ** 2 * (1 - eta) * c["rel"] >= 1 + 40 * u
    assert c["eps_abs_max"] ** 2 / eta <= 0.99 * c["abs"]


def test_the_tight_tier_implies_the_wide_one_and_the_bits_are_apart(model):
    c, t = wide_constants(model), M.constants(model)
    assert (t["rel"], t["abs"], t["kappa_max"], t["eps_abs_max"]) == (float(f32(1.001)), float(f32(0.01)), 2.0 ** -13, 2.0e-3)
    assert c["rel"] >= t["rel"] and c["abs"] >= t["abs"] and c["kappa_max"] >= t["kappa_max"] and c["eps_abs_max"] >= t["eps_abs_max"]
    b = KW.bits(model)
    assert (b["child1"], b["child2"], b["computed"]) == (1, 2, 4)
    six = [b[k] for k in ("child1", "child2", "computed", "wide1", "wide2", "wide_computed")]
    assert all(x and not x & (x - 1) for x in six + [b["tight_only"]]) and len(set(six + [b["tight_only"]])) == 7
    # DScene::leaf_cull -> the record bits a launch looks at: the wide tier's (a leaf of the tight tier carries them too), or,
    # with the flag, the tight tier's
    assert b["mask_0"] == 0
    assert b["mask_3"] == b["wide1"] | b["wide2"]
    assert b["mask_7"] == b["mask_3"] | b["wide_computed"]
    assert b["mask_7_tight_only"] == 7


# ------------------------------------------------------------------------------------------------------------------ the claim

def limits_around_the_wide_rule(model, rs, tris, origins, boxes=None):
    """M.limits_around_the_rule for the wide rule: the largest limit at which it still fires (searched by bisection over
    the float bit patterns, and held against what its constants give), stepped by -3 .. +3 ulp; for every other case 0.3 .. 0.98 of the squared box distance."""
    c = wide_constants(model)
    n = len(tris)
    out = np.zeros(n, f32)
    los, his = boxes if boxes is not None else (tris["AABB"]["pMin"][:, :3], tris["AABB"]["pMax"][:, :3])
    for i in range(n):
        lo, hi = np.ascontiguousarray(los[i], f32), np.ascontiguousarray(his[i], f32)
        o = np.ascontiguousarray(origins[i], f32)
        d2 = model.cull_box_distance2(K.fp(lo), K.fp(hi), K.fp(o))
        if i % 2:
            out[i] = f32(d2 * rs.uniform(0.3, 0.98))
            continue
        fires = lambda bits: bool(model.wide_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, float(np.uint32(bits).view(f32))))
        # the rule is monotone in the limit and does not fire at limit = D^2: bisect the bit patterns of [0, D^2]
        a, b = 0, int(f32(d2).view(np.uint32))
        assert not fires(b)
        if not fires(a):  # (a box nearer than sqrt(kAbsWide) never fires: no boundary)
            out[i] = f32(0)
            continue
        while b - a > 1:
            mid = (a + b) // 2
            a, b = (mid, b) if fires(mid) else (a, mid)
        x = np.uint32(a).view(f32)
        assert abs(float(x) - (d2 - c["abs"]) / c["rel"]) <= 1e-5 * d2  # (what the wide constants say)
        steps = int(rs.integers(-3, 4))
        for _ in range(abs(steps)):
            x = np.nextafter(x, f32(np.inf if steps > 0 else -np.inf))
        out[i] = max(x, f32(0))
    return out


def check_wide_claim(model, lib, tris, origins, directions, limits, boxes=None):
    """-> (cases on which the wide rule fired on a wide-certified leaf, of them certified by the wide tier ONLY, wide-certified
    leaves, tight-certified leaves).  Asserts the oracle rejects on every fired case."""
    fired = fired_wide_only = certified = tight = 0
    los, his = boxes if boxes is not None else (tris["AABB"]["pMin"][:, :3], tris["AABB"]["pMax"][:, :3])
    for i in range(len(tris)):
        lo, hi = np.ascontiguousarray(los[i], f32), np.ascontiguousarray(his[i], f32)
        t = tris[i:i + 1]
        is_tight = bool(model.cull_triangle_certified(t.ctypes.data, K.fp(lo), K.fp(hi)))
        is_wide = bool(model.wide_triangle_certified(t.ctypes.data, K.fp(lo), K.fp(hi)))
        assert is_wide or not is_tight, f"case {i}: certified by the tight tier and not by the wide one"
        tight += is_tight
        if not is_wide:
            continue
        certified += 1
        o = np.ascontiguousarray(origins[i], f32)
        if not model.wide_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, float(limits[i])):
            continue
        assert model.cull_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, float(limits[i])), f"case {i}: the wide rule fired and the tight one did not"
        fired += 1
        fired_wide_only += not is_tight
        d = K.ray_direction(lib, o, directions[i])
        dist, s, tt, point = C.c_float(float(limits[i])), C.c_float(0), C.c_float(0), np.zeros(4, f32)
        hit = lib.pto_triangle_intersects(t.ctypes.data, K.fp(o), K.fp(d), C.byref(dist), C.byref(s), C.byref(tt), K.fp(point))
        assert hit == 0, f"case {i}: the wide rule fired at limit {limits[i]!r} and the oracle accepted with nsd {dist.value!r} (origin {o}, direction {d})"
    return fired, fired_wide_only, certified, tight


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_wide_rule_on_a_wide_certified_leaf_means_the_oracle_rejects(model, da):
    lib = O.oracle(da)
    rs = np.random.default_rng(12)
    kinds = []
    for scale in (1e-3, 0.1, 1.0, 10.0, 300.0, 1e4):
        kinds.append((f"random@{scale}", M.leaf_cases(rs, 300, scale), None))
        kinds.append((f"grazing@{scale}", M.leaf_cases(rs, 200, scale), 10.0 ** rs.uniform(-6.5, -3.5, 200)))
        # slivers across BOTH thresholds: heights from 1e-4 to 0.3 of the base edge (the tight tier starts refusing near 0.1,
        # the wide one near 0.03)
        kinds.append((f"slivers@{scale}", M.leaf_cases(rs, 300, scale, thin=10.0 ** rs.uniform(-4, -0.5, 300)), None))
        kinds.append((f"vertex@{scale}", M.leaf_cases(rs, 300, scale), "vertex"))
        kinds.append((f"grown@{scale}", M.leaf_cases(rs, 200, scale), "grown"))
    per_kind = {}
    fired = total = 0
    for name, tris, grazing in kinds:
        scale = float(name.split("@")[1])
        boxes = M.grown_boxes(rs, tris, scale) if isinstance(grazing, str) and grazing == "grown" else None
        if isinstance(grazing, str):
            origins, directions = M.vertex_rays(rs, tris, scale)
        else:
            origins, directions = M.aimed_rays(rs, tris, scale, grazing)
        limits = limits_around_the_wide_rule(model, rs, tris, origins, boxes)
        per_kind[name] = (*check_wide_claim(model, lib, tris, origins, directions, limits, boxes), len(tris))
        fired += per_kind[name][0]
        total += len(tris)
    print(per_kind)
    assert fired * 3 >= total, (fired, total, per_kind)
    # among the slivers some are certified by the wide tier ONLY and fire; and the slivers cross the wide threshold too
    f, wide_only, c, t, n = per_kind["slivers@1.0"]
    assert wide_only > 0 and t < c < n, per_kind["slivers@1.0"]
    assert sum(v[1] for k, v in per_kind.items() if k.startswith("slivers")) >= 20, per_kind


def test_directed_origins_never_cull_under_the_wide_rule(model):
    lo, hi = np.array([-0.0, 1.0, -2.0], f32), np.array([0.0, 2.0, -1.0], f32)
    inf, nan = f32(np.inf), f32(np.nan)
    for o in ([0.0, 1.5, -1.5], [-0.0, 1.0, -2.0], [inf, 1.5, -1.5], [nan, 1.5, -1.5], [5.0, nan, 0.0], [nan, nan, nan], [3e38, 0, 0]):
        o = np.array(o + [1.0], f32)
        for limit in (0.0, 1e-6, 1.0, float("inf")):
            assert not model.wide_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, limit), (o, limit)
    away = np.array([3.0, 1.5, -1.5, 1.0], f32)
    assert model.wide_rule(K.fp(lo), K.fp(hi), K.fp(away), 0.0, 1.0)
    assert not model.wide_rule(K.fp(lo), K.fp(hi), K.fp(away), 0.0, float("nan"))
    for o_w, d_w in ((0.0, 0.0), (1.0, 1e-30), (float("nan"), 0.0), (1.0, float("nan")), (2.0, 0.0)):
        o = away.copy()
        o[3] = o_w
        assert not model.wide_rule(K.fp(lo), K.fp(hi), K.fp(o), d_w, 1.0)


# ------------------------------------------------------------------------------------------------------------------- the walk

_scenes = {}


def walk_scene(name):
    if name not in _scenes:
        _scenes[name] = bvh_create(K.random_scene(4096, W, H) if name == "rand4096" else KW.sliver_scene(4096, W, H))
    return _scenes[name]


PIXELS = [(x, y) for y in range(3, H, 10) for x in range(2, W, 9)][:40]


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("name", ["rand4096", "slivers4096"])
def test_walk_culled_by_both_tiers_is_the_plain_walk(model, name, da):
    """The kernel's levels: unset / 2 (both tiers, direct and pushed), 1 (both tiers, direct), 3 (the tight bits alone) - all
    under the wide rule - and the walk of the commit before (tight bits, tight rule)."""
    lib = O.oracle(da)
    b = KW.bits(model)
    levels = {"2": (b["mask_7"], True), "1": (b["mask_3"], True), "3": (b["mask_7_tight_only"], True), "before": (b["mask_7_tight_only"], False)}
    lay = K.Layout(model, walk_scene(name))
    try:
        assert len(PIXELS) == 40
        queries = 0
        culled = dict.fromkeys(levels, 0)
        for x, y in PIXELS:
            path, bounces = K.path_queries(lib, walk_scene(name), W, H, DEPTH, x, y, 0, da)
            for origin, direction, limit, shadow, want_hit, bounce in path:
                plain = KW.walk(lay, lib, origin, direction, limit, shadow, 0, True)
                assert plain["direct_culled"] == plain["popped_culled"] == 0 and plain["tested"] == plain["n_tri"]
                old_plain = lay.walk(lib, origin, direction, limit, shadow, 0)  # (the model of tests/leaf_cull_model.cpp)
                for key in ("hit", "limit_bits", "n_bbx", "n_tri"):
                    assert plain[key] == old_plain[key], (x, y, key, plain, old_plain)
                if want_hit is not None:
                    assert plain["hit"] != K.NONE and int(lay.tri_ids[plain["hit"]]) == want_hit, (x, y, plain, want_hit)
                for level, (mask, wide) in levels.items():
                    got = KW.walk(lay, lib, origin, direction, limit, shadow, mask, wide)
                    for key in ("hit", "limit_bits", "n_bbx", "n_tri"):
                        assert got[key] == plain[key], (x, y, level, key, got, plain)
                    if shadow or level == "1":
                        assert got["popped_culled"] == 0
                    culled[level] += got["direct_culled_tris"] + got["popped_culled_tris"]
                queries += 1
        print(f"{name}: {queries} queries; triangle tests skipped per level: {culled}")
        assert queries >= len(PIXELS)
        # conditions: the wide tier culls more than the tight one did, the pushed rule adds to the direct one; in the sliver
        # scene the tight tier certifies nothing
        assert culled["2"] > culled["before"] and culled["2"] > culled["1"] > 0
        if name == "slivers4096":
            assert culled["3"] == culled["before"] == 0
    finally:
        lay.free()


# ----------------------------------------------------------------------------------------------------------- the certificate

# cull_layout_bits of the commit before the wide tier, on K.random_scene(4096, 64, 64): inner records, of them computed, leaf
# children, of them cullable (the tight tier), records whose cull word is not zero
PARENT_LAYOUT_BITS = {"rand4096": dict(inner=1351, computed=1351, leaves=1352, cullable=1117, nonzero_pad=1351)}


@pytest.mark.parametrize("name", ["rand4096", "slivers4096", "cornell"])
def test_the_tight_bits_are_what_they_were(model, name):
    """`cull & 7` of every inner record is kCullComputed + leaf_is_cullable of its children, which this change leaves alone
    (tests/test_leaf_cull_model.py pins it on cases); the wide bits are leaf_is_cullable_wide; no other bit is set."""
    sc = bvh_create(scenes.cornell_box(W, H)) if name == "cornell" else walk_scene(name)
    lay = K.Layout(model, sc)
    try:
        got = KW.check_records(lay)
        assert got["inner"] > 0 and got["tight_differs"] == got["wide_differs"] == got["stray_bits"] == got["tight_without_wide"] == 0, got
        rc, old = K.layout_bits(model, sc)
        assert rc == 0 and old == dict(inner=got["inner"], computed=got["inner"], leaves=got["leaves"], cullable=got["tight"], nonzero_pad=got["inner"])
        if name in PARENT_LAYOUT_BITS:
            assert old == PARENT_LAYOUT_BITS[name]
        if name == "slivers4096":  # what the GPU tests need of this scene: the upload's gate opens on wide-only leaves
            assert got["tight"] == 0 and got["wide_only"] >= 1024, got
        if name == "rand4096":
            assert got["wide_only"] > 0
    finally:
        lay.free()


def test_refit_recomputes_both_tiers(model):
    """A third of the triangles move - half of those become slivers of the wide-only range, the others slivers below both tiers:
    the refit's words equal a fresh layout's, tier by tier."""
    sc = walk_scene("rand4096")
    lay = K.Layout(model, sc)
    try:
        before = lay.inner()[:, 15].copy()
        tris = U.raw_copy(sc.triangulation)
        pick = np.arange(0, len(tris), 3)
        rs = np.random.default_rng(8)
        s1, s2 = tris["S1"][pick][:, :3].astype(np.float64), tris["S2"][pick][:, :3].astype(np.float64)
        side = np.cross(s2 - s1, rs.normal(size=(len(pick), 3)))
        side /= np.linalg.norm(side, axis=1)[:, None]
        thin = np.where(np.arange(len(pick)) % 2 == 0, 0.06, 1e-3)[:, None]
        s3 = tris["S3"].copy()
        s3[pick, :3] = (0.5 * (s1 + s2) + side * np.linalg.norm(s2 - s1, axis=1)[:, None] * thin).astype(f32)
        tris["S3"] = s3
        tris = U.displaced(tris, seed=9, amplitude=0.0)  # (normals and boxes of the new vertices)
        lay.update(tris)
        fresh = K.Layout(model, U.moved_scene(sc, tris))
        try:
            assert np.array_equal(lay.recs, fresh.recs)
            got = KW.check_records(lay)
            assert got["tight_differs"] == got["wide_differs"] == got["stray_bits"] == got["tight_without_wide"] == 0, got
            after = lay.inner()[:, 15]
            assert ((after & 3) != (before & 3)).any() and ((after & 24) != (before & 24)).any() and (after & 36 == 36).all()
            assert 0 < got["tight"] < got["wide"] < got["leaves"]
        finally:
            fresh.free()
    finally:
        lay.free()
