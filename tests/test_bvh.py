"""The product BVH builder (ptmi_bvh_create) against the reference's own BVH_Create.

* where oracle/_ref/libref_bvh.so exists (the reference's PathTracer_BVH.cpp compiled UNMODIFIED) every
  field the reference writes must be equal, and the triangle array must be reordered identically;
* elsewhere the same fields, hashed, against the digests of the reference builder's own trees
  (tests/golden/bvh_reference_trees.json);
* everywhere: committed digests of trees that were checked against the reference when they were made
  (tests/golden/bvh_digests.json).  Generator of both: this file run as a script where libref_bvh.so exists.

The small cases of bvh_stress_cases.py (ties, lattices, duplicates, sorted input, clusters, chains) go through all three:
the device builder is compared with this builder, so this builder is compared with the reference's on the same geometry.
One of them is a tree of 300 levels.  The reference's builder knows no depth limit and builds it; the product's refuses
trees deeper than 8 x PTMI_BVH_MAX_DEPTH.  bvh_reference_trees.json records such a case as {"refused": <the product's
error code>, "reference_max_depth": <the depth of the reference's tree>} instead of a digest.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import bvh_stress_cases as stress
import oracle_ffi as O
from opencl_pathtracer_amd import scenes, bvh_create, structs as S, PtmiError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bvh_digests.json")
REF_TREES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bvh_reference_trees.json")
NODE_FIELDS = ["cutAxis", "triangleStartIndex", "nbTriangles", "son1Id", "son2Id", "isLeaf"]
CASES = [("cornell", 64, 48), ("matmix", 96, 96), ("tris20k", 96, 64), ("tris1m", 160, 90)]


def digest(sc):
    h = hashlib.sha256()
    for f in NODE_FIELDS:
        h.update(np.ascontiguousarray(sc.bvh[f]).tobytes())
    for bb in ("trianglesAABB", "centroidsAABB"):
        for f in ("pMin", "pMax", "centroid", "isEmpty"):
            h.update(np.ascontiguousarray(sc.bvh[bb][f]).tobytes())
    leaf = sc.bvh["isLeaf"] != 0
    h.update(np.ascontiguousarray(sc.bvh["comments"][leaf]).tobytes())
    h.update(np.ascontiguousarray(sc.triangulation["id"]).tobytes())
    return {"nodes": int(len(sc.bvh)), "max_depth": int(sc.bvhMaxDepth), "leaves": int(leaf.sum()),
            "sha256": h.hexdigest()}


def assert_same_tree(ref_nodes, ref_tris, ref_depth, sc):
    assert len(ref_nodes) == len(sc.bvh) and ref_depth == sc.bvhMaxDepth
    for f in NODE_FIELDS:
        assert np.array_equal(ref_nodes[f], sc.bvh[f]), f
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else x  # (a zero-area triangle's N is NaN)
    for bb in ("trianglesAABB", "centroidsAABB"):
        for f in ("pMin", "pMax", "centroid", "isEmpty"):  # (bit for bit: a NaN w reaches the boxes, and -0 is not +0)
            assert np.array_equal(bits(ref_nodes[bb][f]), bits(sc.bvh[bb][f])), (bb, f)
    leaf = ref_nodes["isLeaf"] != 0
    assert np.array_equal(ref_nodes["comments"][leaf], sc.bvh["comments"][leaf])
    for f in S.Triangle.names:  # field-wise: the reference's member-wise swap does not move padding bytes
        a, b = ref_tris[f], sc.triangulation[f]
        if a.dtype.names:
            for g in a.dtype.names:
                assert np.array_equal(bits(a[g]), bits(b[g])), (f, g)
        else:
            assert np.array_equal(bits(a), bits(b)), f


def tree_digest(nodes, tris, depth):
    """SHA-256 over everything assert_same_tree compares, field by field (a record's padding bytes are left out)."""
    h = hashlib.sha256()
    h.update(np.array([len(nodes), depth], np.int64).tobytes())
    for f in NODE_FIELDS:
        h.update(np.ascontiguousarray(nodes[f]).tobytes())
    for bb in ("trianglesAABB", "centroidsAABB"):
        for f in ("pMin", "pMax", "centroid", "isEmpty"):
            h.update(np.ascontiguousarray(nodes[bb][f]).tobytes())
    h.update(np.ascontiguousarray(nodes["comments"][nodes["isLeaf"] != 0]).tobytes())
    for f in S.Triangle.names:
        a = tris[f]
        for g in a.dtype.names or (None,):
            h.update(np.ascontiguousarray(a if g is None else a[g]).tobytes())
    return h.hexdigest()


def reference_tree(key, triangulation):
    """The reference's BVH_Create on `triangulation` (call it before the product's builder reorders the triangles): its tree
    where oracle/_ref/libref_bvh.so exists, elsewhere the digest of that tree stored in tests/golden/bvh_reference_trees.json."""
    if O.have_ref_bvh():
        return O.ref_bvh_create(triangulation)
    return json.load(open(REF_TREES))[key]


def assert_same_as_reference(ref, sc):
    if isinstance(ref, str):
        assert tree_digest(sc.bvh, sc.triangulation, sc.bvhMaxDepth) == ref
    else:
        assert_same_tree(*ref, sc)


@pytest.mark.parametrize("name,w,h", CASES)
def test_matches_reference_builder(name, w, h, built):
    if name == "tris1m" and os.environ.get("PTMI_SKIP_SLOW"):
        pytest.skip("slow")
    sc = scenes.build(name, w, h)
    ref = reference_tree(f"{name}_{w}x{h}", sc.triangulation)
    bvh_create(sc)
    assert_same_as_reference(ref, sc)


@pytest.mark.parametrize("name,w,h", CASES)
def test_matches_committed_digest(name, w, h, built):
    golden = json.load(open(GOLDEN))
    sc = bvh_create(scenes.build(name, w, h))
    assert digest(sc) == golden[name]


def _random_soup(n, seed, spread=1.0):
    rs = np.random.RandomState(seed)
    c = rs.uniform(-spread, spread, (n, 1, 3))
    v = (c + rs.uniform(-0.2, 0.2, (n, 3, 3))).astype(np.float32)
    return scenes.triangle_create(v[:, 0], v[:, 1], v[:, 2])


@pytest.mark.parametrize("n", [1, 2, 4, 5, 9, 33, 257])
def test_small_and_ragged_sizes(n, built):
    tris = _random_soup(n, 100 + n)
    sc = scenes.cornell_box(8, 8)
    sc.triangulation = tris
    ref = reference_tree(f"soup{n}", tris)
    bvh_create(sc)
    assert sc.bvh["isLeaf"][0] == (1 if n <= 4 else 0) or n > 4
    leaves = sc.bvh[sc.bvh["isLeaf"] != 0]
    assert leaves["nbTriangles"].sum() == n  # every triangle in exactly one leaf
    covered = np.zeros(n, bool)
    for l in leaves:
        covered[l["triangleStartIndex"]:l["triangleStartIndex"] + l["nbTriangles"]] = True
    assert covered.all() and sorted(sc.triangulation["id"].tolist()) == list(range(n))
    assert_same_as_reference(ref, sc)


def _coincident_stack():
    rs = np.random.RandomState(7)
    base = rs.uniform(-0.2, 0.2, (1, 3, 3)).astype(np.float32)
    v = np.repeat(base, 40, axis=0)
    return scenes.triangle_create(v[:, 0], v[:, 1], v[:, 2])


def test_coincident_centroids_stop_on_min_diagonal(built):
    """All centroids (nearly) equal: the reference stops with NODE_LEAF_MIN_DIAG and a big leaf (BVH.cpp:142-149)."""
    tris = _coincident_stack()
    sc = scenes.cornell_box(8, 8)
    sc.triangulation = tris
    ref = reference_tree("coincident40", tris)
    bvh_create(sc)
    assert len(sc.bvh) == 1 and sc.bvh["isLeaf"][0] and sc.bvh["nbTriangles"][0] == 40
    assert sc.bvh["comments"][0] == S.NODE_LEAF_MIN_DIAG
    assert_same_as_reference(ref, sc)


@pytest.mark.parametrize("seed", range(0, 60, 3))
def test_fuzzed_scenes_match_reference_builder(seed, built):
    """scenes.fuzz_scene (soup at mixed scales, coincident stacks of up to 40 triangles, flat boxes, clusters of thousands)
    with and without the hostile records (zero-area triangles, 1e6-unit coordinates, a 1e-6-unit triangle) and the corrupted
    ones (w components that are not 1 enter the boxes' fourth component): the same tree as the reference's own builder,
    field for field, and the same triangle order."""
    import warnings
    for suffix in ("", "h", "r", "hr"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sc = scenes.build(f"fuzz{seed}{suffix}_l1", 64, 64)
        ref = reference_tree(f"fuzz{seed}{suffix}_l1", sc.triangulation)
        bvh_create(sc)
        assert_same_as_reference(ref, sc)


def stress_key(case):
    return "stress_" + stress.case_id(case)


def _stress_scene(case):
    sc = scenes.cornell_box(8, 8)
    sc.triangulation = stress.make(*case)
    return sc


@pytest.mark.parametrize("case", [c for c in stress.SMALL if c[0] != stress.REFUSED], ids=stress.case_id)
def test_stress_cases_match_reference_builder(case, built):
    """Tied and structured geometry: the reference builder's tree (or its digest), and the committed digest."""
    sc = _stress_scene(case)
    ref = reference_tree(stress_key(case), sc.triangulation)
    bvh_create(sc)
    assert_same_as_reference(ref, sc)
    assert digest(sc) == json.load(open(GOLDEN))[stress_key(case)]


@pytest.mark.parametrize("case", [c for c in stress.SMALL if c[0] == stress.REFUSED], ids=stress.case_id)
def test_stress_case_deeper_than_the_limit_is_refused(case, built):
    """A chain of 300 levels: the reference builds it, that deep; the product refuses it with PTMI_ERR_BAD_SCENE."""
    sc = _stress_scene(case)
    recorded = json.load(open(REF_TREES))[stress_key(case)]
    assert recorded["refused"] == -5 and recorded["reference_max_depth"] == 300
    if O.have_ref_bvh():
        assert O.ref_bvh_create(sc.triangulation)[2] == recorded["reference_max_depth"]
    with pytest.raises(PtmiError, match="too large to build a tree from") as e:
        bvh_create(sc)
    assert e.value.code == recorded["refused"]


# cloud + wall scenes (test_bvh_device_model.cloud_wall) in which the SAH picks an axis that was skipped at its node, and
# which the host builder builds: it splits there with k1 and the scans an earlier node left behind (BVH.cpp:154-161).
STALE_AXIS_SEEDS = (4, 7, 14, 27, 30, 36)


@pytest.fixture(scope="module")
def device_model(tmp_path_factory):
    import test_bvh_device_model as M  # (it imports this module: not at the top)
    return M.build_model(tmp_path_factory.mktemp("bvh_model"))


def _build_and_compare(key, tris):
    sc = scenes.cornell_box(8, 8)
    sc.triangulation = tris
    ref = reference_tree(key, tris)
    bvh_create(sc)
    assert_same_as_reference(ref, sc)
    return sc


@pytest.mark.parametrize("seed", STALE_AXIS_SEEDS)
def test_stale_axis_splits_match_reference_builder(seed, built, device_model):
    """Only the host builder implements the split on a skipped axis (the device and the model hand such scenes to it): the
    reference builder's tree, field for field.  The model must flag the scene, so that the case cannot stop taking that path."""
    import test_bvh_device_model as M
    tris = M.cloud_wall(seed)
    assert device_model(np.ascontiguousarray(tris))[0] == M.MODEL_STALE
    _build_and_compare(f"cloud_wall{seed}", tris)


def _empty_twins():
    """150 triangles, and the first 40 again with their boxes marked empty: a twin falls into its original's bin at every
    node, so no side of any split holds empty boxes alone."""
    t = _random_soup(150, 901)
    twins = t[:40].copy()
    twins["AABB"]["isEmpty"] = 1
    return scenes._concat_tris([t, twins])


def _nan_w():
    t = _random_soup(300, 903)
    rs = np.random.RandomState(4)
    for f in ("pMin", "pMax", "centroid"):
        t["AABB"][f][rs.choice(300, 25, replace=False), 3] = np.nan
    return t


def _empty_third():
    t = _random_soup(300, 902)
    t["AABB"]["isEmpty"][np.random.RandomState(3).rand(300) < 0.3] = 1
    return t


RECORD_CASES = {"records_empty_twins": _empty_twins, "records_nan_w": _nan_w}


@pytest.mark.parametrize("key", sorted(RECORD_CASES))
def test_records_the_device_refuses_match_reference_builder(key, built, device_model):
    """Boxes marked empty (counted in their bin, never united) and NaN w components (they stop a min / max fold where it
    stands): the device builder hands both to the host builder, whose tree must be the reference builder's."""
    import test_bvh_device_model as M
    tris = RECORD_CASES[key]()
    assert device_model(np.ascontiguousarray(tris))[0] == M.MODEL_RECORDS
    sc = _build_and_compare(key, tris)
    if key == "records_nan_w":
        assert np.isnan(sc.bvh["trianglesAABB"]["pMin"][:, 3]).any() and np.isnan(sc.bvh["centroidsAABB"]["pMax"][:, 3]).any()
    else:
        assert (sc.bvh["trianglesAABB"]["isEmpty"] == 0).all()


def test_child_of_empty_boxes_alone_keeps_its_bytes(built):
    """Three boxes in ten marked empty: some splits leave a side that holds such boxes alone.  Its node box is marked empty,
    and its corners are whatever the bin after (or before) the split plane held the last time a box was united into it - at an
    earlier node.  In the reference's builder those arrays are function-level statics that outlive a call, so its bytes there
    depend on the builds the process made before; the product's scratch starts at zero in every call.  Pinned here: the
    product's own tree, as the builder wrote it before it was moved onto bvh_build_common.h."""
    sc = scenes.cornell_box(8, 8)
    sc.triangulation = _empty_third()
    bvh_create(sc)
    assert (sc.bvh["trianglesAABB"]["isEmpty"] != 0).sum() == 4 and len(sc.bvh) == 193
    assert tree_digest(sc.bvh, sc.triangulation, sc.bvhMaxDepth) == "3bc3f3abde81d8b80b05d1631a64dc6a5150beb94b1ad47eceddfa57d228a094"


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 3e38])
def test_boxes_that_are_not_numbers_are_an_error_not_a_fault(value, built):
    """The reference's builder ASSERTs on them (BVH.cpp:199: a bin index out of range; without assertions it writes out of
    bounds).  The product's refuses non-finite boxes outright; with finite but overflowing ones (3e38) it either builds a tree
    (a usable one: every triangle in one leaf) or refuses - it never faults."""
    import warnings
    for seed in range(1, 7):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sc = scenes.build(f"fuzz{seed}_l1", 64, 64)
        rs = np.random.RandomState(seed)
        t = sc.triangulation
        for i in rs.choice(len(t), max(1, len(t) // 20), replace=False):
            t["AABB"][rs.choice(["pMin", "pMax", "centroid"])][i][int(rs.randint(0, 3))] = value
        if np.isfinite(value):
            try:
                bvh_create(sc)
            except PtmiError as e:
                assert e.code == -5 and "overflow" in str(e)
                continue
            leaves = sc.bvh[sc.bvh["isLeaf"] != 0]
            assert leaves["nbTriangles"].sum() == len(t) and sorted(sc.triangulation["id"].tolist()) == list(range(len(t)))
        else:
            with pytest.raises(PtmiError, match="not finite") as e:
                bvh_create(sc)
            assert e.value.code == -5


def test_builder_under_sanitizers(tmp_path):
    """csrc/bvh_build.cpp compiled with g++ -fsanitize=address,undefined and run on the fuzzed scenes (valid, hostile, corrupted
    records) and on boxes that are not numbers: no out-of-bounds access, no undefined behaviour.  (It found the node array
    overrun of a split that leaves one side empty - boxes whose extents overflow - which is an error code now.)"""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not installed")
    asan = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    ubsan = subprocess.run([gxx, "-print-file-name=libubsan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(asan) and os.path.exists(asan) and os.path.isabs(ubsan) and os.path.exists(ubsan)):
        pytest.skip("libasan / libubsan not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = tmp_path / "stub.cpp"
    stub.write_text('#include <string>\nnamespace ptmi_internal { void set_global_error(const std::string&) {} }\n')
    so = tmp_path / "libbvh_asan.so"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "opencl_pathtracer_amd", "csrc"),
                        os.path.join(root, "opencl_pathtracer_amd", "csrc", "bvh_build.cpp"), str(stub), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = {**os.environ, "LD_PRELOAD": asan + ":" + ubsan, "ASAN_OPTIONS": "detect_leaks=0"}
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "sanitize", "bvh_builder_asan.py"), str(so)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


def test_empty_triangulation_is_an_error(built):
    sc = scenes.cornell_box(8, 8)
    sc.triangulation = np.zeros(0, S.Triangle)
    with pytest.raises(PtmiError):
        bvh_create(sc)


def test_tree_invariants_1m(built):
    """Properties the traversal relies on, at the BASELINE size: pre-order numbering (son1 = parent+1),
    children boxes inside the parent box, depth below the 30-entry stack."""
    sc = bvh_create(scenes.build("tris1m", 160, 90))
    b = sc.bvh
    inner = np.flatnonzero(b["isLeaf"] == 0)
    assert np.array_equal(b["son1Id"][inner], inner + 1)
    assert (b["son2Id"][inner] > b["son1Id"][inner]).all() and b["son2Id"].max() < len(b)
    assert sc.bvhMaxDepth < S.BVH_MAX_DEPTH and len(b) == 665533 and sc.bvhMaxDepth == 22
    for son in ("son1Id", "son2Id"):
        child = b["trianglesAABB"][b[son][inner]]
        parent = b["trianglesAABB"][inner]
        assert (child["pMin"][:, :3] >= parent["pMin"][:, :3]).all() and (child["pMax"][:, :3] <= parent["pMax"][:, :3]).all()
    leaves = b[b["isLeaf"] != 0]
    assert leaves["nbTriangles"].sum() == 1000000 and leaves["nbTriangles"].max() <= 4


if __name__ == "__main__":  # regenerate the digests (only meaningful where the reference builder agrees)
    out = {}
    for name, w, h in CASES:
        sc = scenes.build(name, w, h)
        if O.have_ref_bvh():
            ref = O.ref_bvh_create(sc.triangulation)
        bvh_create(sc)
        if O.have_ref_bvh():
            assert_same_tree(*ref, sc)
        out[name] = digest(sc)
        print(name, out[name])
    for case in stress.SMALL:
        if case[0] != stress.REFUSED:
            sc = _stress_scene(case)
            if O.have_ref_bvh():
                ref = O.ref_bvh_create(sc.triangulation)
            bvh_create(sc)
            if O.have_ref_bvh():
                assert_same_tree(*ref, sc)
            out[stress_key(case)] = digest(sc)
    json.dump(out, open(GOLDEN, "w"), indent=1, sort_keys=True)
    if O.have_ref_bvh():  # the reference builder's own trees, hashed (each one checked against the product's first)
        import warnings
        inputs = [(f"{name}_{w}x{h}", lambda name=name, w=w, h=h: scenes.build(name, w, h).triangulation) for name, w, h in CASES]
        inputs += [(f"soup{n}", lambda n=n: _random_soup(n, 100 + n)) for n in (1, 2, 4, 5, 9, 33, 257)]
        inputs += [("coincident40", _coincident_stack)]
        inputs += [(f"fuzz{s}{x}_l1", lambda s=s, x=x: scenes.build(f"fuzz{s}{x}_l1", 64, 64).triangulation)
                   for s in range(0, 60, 3) for x in ("", "h", "r", "hr")]
        inputs += [(stress_key(case), lambda case=case: stress.make(*case)) for case in stress.SMALL if case[0] != stress.REFUSED]
        import test_bvh_device_model as M
        inputs += [(f"cloud_wall{seed}", lambda seed=seed: M.cloud_wall(seed)) for seed in STALE_AXIS_SEEDS]
        inputs += sorted(RECORD_CASES.items())
        trees = {}
        for key, make in inputs:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                tris = make()
            ref = O.ref_bvh_create(tris)
            sc = scenes.cornell_box(8, 8)
            sc.triangulation = tris
            bvh_create(sc)
            assert_same_tree(*ref, sc)
            trees[key] = tree_digest(*ref)
            assert tree_digest(sc.bvh, sc.triangulation, sc.bvhMaxDepth) == trees[key], key
        for case in stress.SMALL:
            if case[0] == stress.REFUSED:  # the reference builds it; the product refuses trees that deep
                sc = _stress_scene(case)
                depth = O.ref_bvh_create(sc.triangulation)[2]
                with pytest.raises(PtmiError) as e:
                    bvh_create(sc)
                trees[stress_key(case)] = {"refused": e.value.code, "reference_max_depth": int(depth)}
        json.dump(trees, open(REF_TREES, "w"), indent=1, sort_keys=True)
