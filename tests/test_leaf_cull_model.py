"""csrc/leaf_cull.h on the CPU: the claim, a whole walk, and the certificate's life through an update.

THE CLAIM: where the rule fires on a certified leaf, the oracle's own Triangle_Intersects (pto_triangle_intersects) rejects every
triangle of that leaf at that limit - in both arithmetics, on random and on directed cases.  The generators are chosen so that
the rule fires on more than a third of the cases (asserted): a test that never culls proves nothing.

THE WALK: tests/leaf_cull_model.cpp walks build_layout's records in the kernel's visit order with the oracle's box and triangle
deciders, on the queries of real paths (camera, shadow and scattered rays restated from pto_trace_path's bounces); with the
culling on (direct leaves, and direct + pushed) it must yield the ORACLE's hit, box-test count and triangle-test count per bounce.
"""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import bvh_create, scenes
import leaf_cull_cases as K
import oracle_ffi as O
import scene_update_cases as U

f32 = np.float32


@pytest.fixture(scope="module")
def model(tmp_path_factory, built):
    return K.build_model(tmp_path_factory.mktemp("leaf_cull_model"))


def constants(model):
    c = (C.c_double * 4)()
    model.cull_constants(c)
    return dict(rel=c[0], abs=c[1], kappa_max=c[2], eps_abs_max=c[3])


def test_constants_satisfy_the_proofs_two_inequalities(model):
    """with eta = (kRel - 1) / 2, (1 - kappa)^2 (1 - eta) kRel >= 1 + 40u and eps_abs^2 / eta <= 0.99 kAbs."""
    c = constants(model)
    eta, u = (c["rel"] - 1) / 2, 2.0 ** -24
    assert (1 - c["kappa_max"]) ** 2 * (1 - eta) * c["rel"] >= 1 + 40 * u
    assert c["eps_abs_max"] ** 2 / eta <= 0.99 * c["abs"]


# ------------------------------------------------------------------------------------------------------------------ the claim

def leaf_cases(rs, n, scale, thin=None):
    """n leaves of one triangle each: vertices around a centre of magnitude `scale`, box = the triangle's own AABB.  thin: the
    third vertex lies at that fraction of the base edge's length off the edge (slivers)."""
    centre = (rs.uniform(-1, 1, (n, 3)) * scale).astype(f32)
    size = f32(scale * 0.05)
    a = (centre + rs.uniform(-1, 1, (n, 3)).astype(f32) * size).astype(f32)
    b = (centre + rs.uniform(-1, 1, (n, 3)).astype(f32) * size).astype(f32)
    if thin is None:
        c = (centre + rs.uniform(-1, 1, (n, 3)).astype(f32) * size).astype(f32)
    else:
        side = np.cross(b - a, rs.uniform(-1, 1, (n, 3)))
        side /= np.linalg.norm(side, axis=1)[:, None]
        c = (a + (b - a) * rs.uniform(0.2, 0.8, (n, 1)) + side * np.linalg.norm(b - a, axis=1)[:, None] * np.asarray(thin).reshape(-1, 1)).astype(f32)
    with np.errstate(all="ignore"):
        return scenes.triangle_create(a, b, c, mat_pos=0)


def check_claim(model, lib, tris, origins, directions, limits, boxes=None):
    """-> (cases on which the rule fired on a certified leaf, certified leaves).  Asserts the oracle rejects on every such case."""
    fired = certified = 0
    los, his = boxes if boxes is not None else (tris["AABB"]["pMin"][:, :3], tris["AABB"]["pMax"][:, :3])
    for i in range(len(tris)):
        lo, hi = np.ascontiguousarray(los[i], f32), np.ascontiguousarray(his[i], f32)
        t = tris[i:i + 1]
        if not model.cull_triangle_certified(t.ctypes.data, K.fp(lo), K.fp(hi)):
            continue
        certified += 1
        o = np.ascontiguousarray(origins[i], f32)
        if not model.cull_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, float(limits[i])):
            continue
        fired += 1
        d = K.ray_direction(lib, o, directions[i])
        dist, s, tt, point = C.c_float(float(limits[i])), C.c_float(0), C.c_float(0), np.zeros(4, f32)
        hit = lib.pto_triangle_intersects(t.ctypes.data, K.fp(o), K.fp(d), C.byref(dist), C.byref(s), C.byref(tt), K.fp(point))
        assert hit == 0, f"case {i}: the rule fired at limit {limits[i]!r} and the oracle accepted with nsd {dist.value!r} (origin {o}, direction {d})"
    return fired, certified


def aimed_rays(rs, tris, scale, grazing=None):
    """Origins at 0.2 .. 30 box sizes from the triangle, directions at a random point of it (so that the computed distance is
    about the true one); grazing: the direction lies in the triangle's plane up to that much of the normal (|N.dir| ~ grazing)."""
    n = len(tris)
    s1, s2, s3 = tris["S1"][:, :3], tris["S2"][:, :3], tris["S3"][:, :3]
    bary = rs.dirichlet((1, 1, 1), n).astype(f32)
    target = s1 * bary[:, :1] + s2 * bary[:, 1:2] + s3 * bary[:, 2:]
    away = rs.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1)[:, None]
    if grazing is not None:
        nrm = tris["N"][:, :3].astype(np.float64)
        away = away - nrm * (away * nrm).sum(1)[:, None]
        away /= np.linalg.norm(away, axis=1)[:, None]
        away = away + nrm * np.asarray(grazing).reshape(-1, 1)
    dist = scale * 0.05 * rs.uniform(0.2, 30, (n, 1)) + 0.2
    origins = np.concatenate([(target + away * dist).astype(f32), np.ones((n, 1), f32)], axis=1)
    directions = np.concatenate([(target - origins[:, :3]).astype(f32), np.zeros((n, 1), f32)], axis=1)
    return origins, directions


def vertex_rays(rs, tris, scale):
    """No geometric slack: the origin lies straight out of a box face along one axis, from a vertex that lies ON that face, so
    the vertex is the box's nearest point and the box distance is the distance to the triangle itself; the ray is aimed at the
    vertex, or a hair inside / outside the triangle next to it.  Only the rule's margins stand between nsd and the limit."""
    n = len(tris)
    verts = np.stack([tris["S1"][:, :3], tris["S2"][:, :3], tris["S3"][:, :3]], axis=1).astype(np.float64)  # n, 3 vertices, 3 axes
    axis = rs.integers(0, 3, n)
    high = rs.integers(0, 2, n).astype(bool)
    coord = verts[np.arange(n), :, axis]
    which = np.where(high, coord.argmax(1), coord.argmin(1))
    v = verts[np.arange(n), which]
    step = np.zeros((n, 3))
    step[np.arange(n), axis] = np.where(high, 1.0, -1.0)
    dist = scale * 0.05 * rs.uniform(0.2, 30, (n, 1)) + 0.2
    origins = np.concatenate([(v + step * dist).astype(f32), np.ones((n, 1), f32)], axis=1)
    centre = verts.mean(1)
    hair = (centre - v) * rs.choice([0.0, 1e-6, -1e-6, 1e-3, -1e-3], (n, 1))  # towards the inside / away from it
    directions = np.concatenate([((v + hair) - origins[:, :3].astype(np.float64)).astype(f32), np.zeros((n, 1), f32)], axis=1)
    return origins, directions


def grown_boxes(rs, tris, scale):
    """The boxes of leaves that hold more than this triangle: the tight box grown on random sides by up to two triangle sizes."""
    box = tris["AABB"]
    lo = (box["pMin"][:, :3] - rs.uniform(0, 1, (len(tris), 3)) * rs.integers(0, 2, (len(tris), 3)) * scale * 0.1).astype(f32)
    hi = (box["pMax"][:, :3] + rs.uniform(0, 1, (len(tris), 3)) * rs.integers(0, 2, (len(tris), 3)) * scale * 0.1).astype(f32)
    return lo, hi


def limits_around_the_rule(model, rs, tris, origins, boxes=None):
    """Per case a limit near the rule's boundary: the largest limit at which the rule still fires, stepped by -3 .. +3 ulp - and
    for half of the cases a limit well inside (0.3 .. 0.98 of the squared box distance)."""
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
        x = f32(max((d2 - 0.01) / 1.001, 0.0))
        for _ in range(64):  # the boundary in ulp steps (the estimate is within a few ulp of it)
            if model.cull_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, float(x)):
                nxt = np.nextafter(x, f32(np.inf))
                if not model.cull_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, float(nxt)):
                    break
                x = nxt
            else:
                x = np.nextafter(x, f32(-np.inf))
        steps = int(rs.integers(-3, 4))
        for _ in range(abs(steps)):
            x = np.nextafter(x, f32(np.inf if steps > 0 else -np.inf))
        out[i] = max(x, f32(0))
    return out


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_rule_on_a_certified_leaf_means_the_oracle_rejects(model, da):
    lib = O.oracle(da)
    rs = np.random.default_rng(11)
    fired = total = 0
    kinds = []
    for scale in (1e-3, 0.1, 1.0, 10.0, 300.0, 1e4):
        kinds.append((f"random@{scale}", leaf_cases(rs, 300, scale), None))
        kinds.append((f"grazing@{scale}", leaf_cases(rs, 200, scale), 10.0 ** rs.uniform(-6.5, -3.5, 200)))
        # slivers across the certification threshold: heights from 1e-4 to 0.3 of the base edge
        kinds.append((f"slivers@{scale}", leaf_cases(rs, 300, scale, thin=10.0 ** rs.uniform(-4, -0.5, 300)), None))
        kinds.append((f"vertex@{scale}", leaf_cases(rs, 300, scale), "vertex"))
        kinds.append((f"grown@{scale}", leaf_cases(rs, 200, scale), "grown"))
    per_kind = {}
    for name, tris, grazing in kinds:
        scale = float(name.split("@")[1])
        boxes = grown_boxes(rs, tris, scale) if isinstance(grazing, str) and grazing == "grown" else None
        if isinstance(grazing, str):
            origins, directions = vertex_rays(rs, tris, scale)  # (against a grown box the vertex is still the target)
        else:
            origins, directions = aimed_rays(rs, tris, scale, grazing)
        limits = limits_around_the_rule(model, rs, tris, origins, boxes)
        f, c = check_claim(model, lib, tris, origins, directions, limits, boxes)
        per_kind[name] = (f, c, len(tris))
        fired += f
        total += len(tris)
    print(per_kind)
    assert fired * 3 >= total, (fired, total, per_kind)
    # the slivers do cross the threshold: some certified, some not, at the scales where anything is certified
    f, c, n = per_kind["slivers@1.0"]
    assert 0 < c < n


def test_directed_origins_never_cull(model):
    """On and inside the box's faces (distance 0), signed zeros, infinite and NaN origins."""
    lo, hi = np.array([-0.0, 1.0, -2.0], f32), np.array([0.0, 2.0, -1.0], f32)
    inf, nan = f32(np.inf), f32(np.nan)
    for o in ([0.0, 1.5, -1.5], [-0.0, 1.0, -2.0], [0.0, 2.0, -1.0], [-0.0, 1.5, -1.0], [inf, 1.5, -1.5], [-inf, 0, 0], [nan, 1.5, -1.5],
              [5.0, nan, 0.0], [5.0, 5.0, nan], [nan, nan, nan], [inf, inf, inf], [3e38, 0, 0]):
        o = np.array(o + [1.0], f32)
        for limit in (0.0, 1e-6, 1.0, float("inf")):
            assert not model.cull_rule(K.fp(lo), K.fp(hi), K.fp(o), 0.0, limit), (o, limit)
    # ... and a finite origin away from the box does, with either zero for the shared face
    away = np.array([3.0, 1.5, -1.5, 1.0], f32)
    for o in (away, away * f32([-1, 1, 1, 1])):
        assert model.cull_rule(K.fp(lo), K.fp(hi), K.fp(np.ascontiguousarray(o)), 0.0, 1.0)
    assert not model.cull_rule(K.fp(lo), K.fp(hi), K.fp(away), 0.0, float("nan"))
    # a ray whose fourth components are not a point's and a direction's (behind a GLASS / WATER reflection) never culls
    for o_w, d_w in ((0.0, 0.0), (1.0, 1e-30), (float("nan"), 0.0), (1.0, float("nan")), (2.0, 0.0)):
        o = away.copy()
        o[3] = o_w
        assert not model.cull_rule(K.fp(lo), K.fp(hi), K.fp(o), d_w, 1.0)


def test_what_the_certificate_refuses(model):
    rs = np.random.default_rng(5)
    tris = leaf_cases(rs, 1, 1.0)
    lo, hi = np.ascontiguousarray(tris["AABB"]["pMin"][0][:3], f32), np.ascontiguousarray(tris["AABB"]["pMax"][0][:3], f32)
    assert model.cull_triangle_certified(tris.ctypes.data, K.fp(lo), K.fp(hi))

    def refused(change, lo=lo, hi=hi):
        t = U.raw_copy(tris)
        change(t)
        return not model.cull_triangle_certified(t.ctypes.data, K.fp(lo), K.fp(hi))

    def set_field(name, value):
        def change(t):
            v = t[name].copy()
            v[0] = value
            t[name] = v
        return change

    n = tris["N"][0].copy()
    assert not refused(set_field("N", [n[0], n[1], n[2], 0.0]))             # (w = 0 or the importers' w = 1: both certified)
    assert refused(set_field("N", [n[0], n[1], n[2], 8.0]))                 # a normal with a large w component
    assert refused(set_field("N", [n[1], n[2], n[0], 0.0]))                 # a normal that is not the plane's
    assert refused(set_field("N", [np.nan, 0, 0, 0]))
    assert refused(set_field("S3", tris["S2"][0]))                          # no area
    s1 = tris["S1"][0].copy()
    assert refused(set_field("S1", [s1[0], s1[1], s1[2], 2.0]))             # unequal w
    assert refused(lambda t: [set_field(k, list(t[k][0][:3]) + [2.0])(t) for k in ("S1", "S2", "S3")])  # w = 2 under N.w = 1
    assert refused(lambda t: None, hi=(hi - f32(0.5) * (hi - lo)).astype(f32))  # a box that does not hold the vertices
    assert refused(lambda t: None, lo=np.array([np.nan, lo[1], lo[2]], f32))


# ------------------------------------------------------------------------------------------------------------------- the walk

W = H = 64
DEPTH = 6


def walk_scene(name):
    if name == "rand4096":
        return bvh_create(K.random_scene(4096, W, H))  # seen from x = -14: hits beyond unit distance
    return bvh_create(scenes.cornell_box(W, H))


# measured by this test on rand4096 (strict and default arithmetic alike): 1143 of the 6444 leaf visits of the 935 sampled queries
# are culled as direct leaves, 0.177 (the Cornell box: none - what a ray hits there is the farthest thing along it); the floor
# is that less a margin
CULLED_SHARE_FLOOR = {"rand4096": 0.15}


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("name", ["rand4096", "cornell"])
def test_walk_with_culling_is_the_walk_without(model, name, da):
    lib = O.oracle(da)
    sc = walk_scene(name)
    lay = K.Layout(model, sc)
    try:
        visits = culled = queries = bounces_checked = 0
        for y in range(2, H, 5):
            for x in range(1, W, 5):
                path, bounces = K.path_queries(lib, sc, W, H, DEPTH, x, y, 0, da)
                per_bounce = {mode: [[0, 0] for _ in bounces] for mode in (0, 1, 2)}
                for origin, direction, limit, shadow, want_hit, bounce in path:
                    plain = lay.walk(lib, origin, direction, limit, shadow, 0)
                    for mode in (0, 1, 2):
                        got = plain if mode == 0 else lay.walk(lib, origin, direction, limit, shadow, mode)
                        for key in ("hit", "limit_bits", "n_bbx", "n_tri"):
                            assert got[key] == plain[key], (x, y, mode, key, got, plain)
                        if bounce < len(bounces):
                            per_bounce[mode][bounce][0] += got["n_bbx"]
                            per_bounce[mode][bounce][1] += got["n_tri"]
                    if want_hit is not None:  # the oracle's next bounce
                        assert plain["hit"] != K.NONE and int(lay.tri_ids[plain["hit"]]) == want_hit, (x, y, plain, want_hit)
                    direct = lay.walk(lib, origin, direction, limit, shadow, 1)
                    visits += direct["direct"] + direct["popped"]
                    culled += direct["direct_culled"]
                    queries += 1
                # the oracle's own counts per bounce (pto_trace_path keeps the path's running totals after each bounce's
                # closest-hit and shadow query): the culled walks must yield exactly them
                before = (0, 0)
                for k, b in enumerate(bounces):
                    want = [b.n_bbx - before[0], b.n_tri - before[1]]
                    before = (b.n_bbx, b.n_tri)
                    for mode in (0, 1, 2):
                        assert per_bounce[mode][k] == want, (x, y, k, mode, per_bounce[mode][k], want)
                    bounces_checked += 1
        assert bounces_checked > 100
        assert queries > 100
        print(f"{name}: {queries} queries, {visits} leaf visits, {culled} culled ({culled / max(visits, 1):.3f})")
        if name in CULLED_SHARE_FLOOR:
            assert culled / visits > CULLED_SHARE_FLOOR[name], (culled, visits)
    finally:
        lay.free()


# ----------------------------------------------------------------------------------------------------------- the certificate

def bits_of(lay):
    return lay.inner()[:, 15].copy()


def test_refit_keeps_recomputes_and_never_leaves_stale_bits(model):
    sc = walk_scene("rand4096")
    lay = K.Layout(model, sc)
    try:
        before_recs, before = lay.recs.copy(), bits_of(lay)
        assert (before & 4).all() and (before & 3).any()
        lay.update(sc.triangulation)  # unchanged triangles: no byte changes
        assert np.array_equal(lay.recs, before_recs)
        # a tenth of the triangles become slivers (uncertifiable): exactly the bits a fresh layout computes, and none stale
        tris = U.raw_copy(sc.triangulation)
        pick = np.arange(0, len(tris), 10)
        s3 = tris["S3"].copy()
        s3[pick] = (tris["S1"][pick] * f32(0.5) + tris["S2"][pick] * f32(0.5) + f32([1e-3, -7e-4, 5e-4, 0])).astype(f32)
        tris["S3"] = s3
        tris = U.displaced(tris, seed=9, amplitude=0.0)  # (normals and boxes of the new vertices)
        lay.update(tris)
        fresh = K.Layout(model, U.moved_scene(sc, tris))
        try:
            assert np.array_equal(lay.recs, fresh.recs)
            after = bits_of(lay)
            assert (after & 4).all() and (after != before).any() and ((after & 3) <= (before & 3)).all()
        finally:
            fresh.free()
    finally:
        lay.free()


def test_scene_of_nan_records_and_generic_records_get_no_bits(model, monkeypatch):
    base = scenes.random_triangles(512, W, H)
    rc, bits = K.layout_bits(model, bvh_create(base))
    assert rc == 0 and bits["computed"] == bits["inner"] > 0 and bits["cullable"] > 0
    rc, bits = K.layout_bits(model, bvh_create(scenes.add_zero_area_triangles(base, 8)))
    assert rc == 0 and bits["inner"] > 0 and bits["nonzero_pad"] == 0
    monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    rc, bits = K.layout_bits(model, bvh_create(base))
    assert rc == 0 and bits["inner"] > 0 and bits["nonzero_pad"] == 0
