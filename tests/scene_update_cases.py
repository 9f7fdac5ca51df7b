"""Moved geometry for the scene-update tests (test_scene_refit_model.py, test_scene_update_gpu.py): seeded displacements of a
triangulation with the derived fields recomputed as scenes.triangle_create computes them, the host refit through the C ABI,
a numpy refit to hold it against, and the hand-made trees the product builder never emits.  Pure numpy, no files."""
import copy
import ctypes as C

import numpy as np

from opencl_pathtracer_amd import backend, scenes, structs as S

f32 = np.float32


def raw_copy(a):
    """A byte-level copy of a struct array (numpy's .copy() of a padded dtype leaves the padding bytes undefined)."""
    return np.frombuffer(bytearray(np.ascontiguousarray(a).tobytes()), dtype=a.dtype)


def displaced(tris, seed, amplitude=0.02):
    """Every vertex of every triangle moved by a seeded offset of at most `amplitude` per axis; N follows the new plane on the
    side it was on, and the AABB is BoundingBox_Create of the new vertices (all four components), as in triangle_create."""
    rs = np.random.default_rng(seed)
    t = raw_copy(tris)
    n = len(t)
    for name in ("S1", "S2", "S3"):
        v = t[name].copy()
        v[:, :3] += rs.uniform(-amplitude, amplitude, (n, 3)).astype(f32)
        t[name] = v
    follow_vertices(t)
    return t


def follow_vertices(t):
    """The derived fields of triangles whose vertices were moved in place: N is the unit normal of the new plane on the side it
    was on, AABB is recompute_aabb's."""
    s1, s2, s3 = t["S1"][:, :3], t["S2"][:, :3], t["S3"][:, :3]
    c = scenes._cross3(s2 - s1, s3 - s1)
    nrm = (c / np.sqrt(scenes._dot3(c, c)).astype(f32)[:, None]).astype(f32)
    flip = scenes._dot3(nrm, t["N"][:, :3]) < 0
    nrm[flip] = -nrm[flip]
    N = t["N"].copy()
    N[:, :3] = nrm
    t["N"] = N
    recompute_aabb(t)


def moved_triangles(sc, name, seed=7):
    """The motion of the GPU update tests for scene `name`: every vertex displaced (0.01 on tris20k, else 0.02), and on
    feat_textured all twelve texture coordinates and the three shading normals as well."""
    tris = displaced(sc.triangulation, seed, amplitude=0.01 if name == "tris20k" else 0.02)
    if name == "feat_textured":
        rs = np.random.default_rng(seed)
        for field in ("UVP1", "UVP2", "UVP3", "UVN1", "UVN2", "UVN3"):
            tris[field] = (tris[field] + rs.uniform(-0.3, 0.3, tris[field].shape)).astype(np.float32)
        for field in ("N1", "N2", "N3"):
            v = tris[field].copy()
            v[:, :3] += rs.uniform(-0.2, 0.2, (len(v), 3)).astype(np.float32)
            v[:, :3] /= np.linalg.norm(v[:, :3], axis=1, keepdims=True).astype(np.float32)
            tris[field] = v
    return tris


def recompute_aabb(t):
    p = np.stack([t["S1"], t["S2"], t["S3"]], axis=1)
    pmin = np.minimum(np.minimum(p[:, 0], p[:, 1]), p[:, 2])
    pmax = np.maximum(np.maximum(p[:, 0], p[:, 1]), p[:, 2])
    box = t["AABB"].copy()
    box["pMin"], box["pMax"], box["centroid"] = pmin, pmax, (pmin + pmax) / f32(2)
    t["AABB"] = box


def moved_camera(sc, step=1):
    """`sc` seen from a little to the side, the view tilted about the camera's right axis (the frame stays orthonormal)."""
    out = copy.copy(sc)
    a = np.float32(0.07 * step)
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    d, u = np.asarray(sc.cameraDirection, np.float32), np.asarray(sc.cameraUp, np.float32)
    out.cameraPosition = (np.asarray(sc.cameraPosition, np.float32) + np.float32([0.11 * step, -0.05 * step, 0.02, 0])).astype(np.float32)
    out.cameraDirection = (c * d + s * u).astype(np.float32)
    out.cameraUp = (c * u - s * d).astype(np.float32)
    return out


BAD_TRIANGLES = ("zero_area", "nan_vertex", "unequal_w", "empty_aabb", "wrong_count")  # (the last: INVALID_ARGUMENT, the others: UNSUPPORTED)


def bad_triangles(sc, kind):
    """`sc`'s triangles with one defect that ptmi_update_triangles refuses."""
    t = raw_copy(sc.triangulation)
    if kind == "zero_area":
        t["S3"][5] = t["S2"][5]
        recompute_aabb(t)
    elif kind == "nan_vertex":
        t["S1"][2] = [np.nan, 0, 0, 1]
    elif kind == "unequal_w":
        t["S2"][7] = t["S2"][7] * np.float32([1, 1, 1, 2])
    elif kind == "empty_aabb":
        box = t["AABB"].copy()
        box["isEmpty"][1] = 1
        t["AABB"] = box
    elif kind == "wrong_count":
        t = t[:-1]
    return t


def bvh_refit(tris, bvh):
    """ptmi_bvh_refit on a byte copy of `bvh`: (status, message, the tree)."""
    lib = backend.load_library()
    lib.ptmi_bvh_refit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    out = raw_copy(bvh)
    tris = np.ascontiguousarray(tris)
    rc = lib.ptmi_bvh_refit(tris.ctypes.data_as(C.c_void_p), len(tris), out.ctypes.data_as(C.c_void_p), len(out))
    return rc, (lib.ptmi_last_error(None).decode() if rc else ""), out


def moved_scene(scene, tris):
    """`scene` with the triangles `tris` and ptmi_bvh_refit's tree for them: what a fresh context is given as the yardstick."""
    rc, msg, bvh = bvh_refit(tris, scene.bvh)
    assert rc == 0, msg
    sc = copy.copy(scene)
    sc.triangulation, sc.bvh = tris, bvh
    return sc


def numpy_refit(tris, bvh):
    """(pMin, pMax) float32[n_nodes, 4] of every node's trianglesAABB: min / max over the node's triangle range, nodes in
    reverse index order (the builders number a node before its subtree)."""
    n = len(bvh)
    lo, hi = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    box = tris["AABB"]
    for i in range(n - 1, -1, -1):
        if bvh["isLeaf"][i]:
            a, k = int(bvh["triangleStartIndex"][i]), int(bvh["nbTriangles"][i])
            lo[i], hi[i] = box["pMin"][a:a + k].min(axis=0), box["pMax"][a:a + k].max(axis=0)
        else:
            s1, s2 = int(bvh["son1Id"][i]), int(bvh["son2Id"][i])
            lo[i], hi[i] = np.minimum(lo[s1], lo[s2]), np.maximum(hi[s1], hi[s2])
    return lo, hi


def big_leaf_scene(width, height, n=9):
    """The Cornell box plus `n` coincident triangles: they end as one leaf of more than 6 triangles (a big leaf)."""
    sc = scenes.cornell_box(width, height)
    a = np.tile(np.array([[0.1, 0.2, 0.05]], f32), (n, 1))
    stack = scenes.triangle_create(a, a + f32([0.3, 0, 0]), a + f32([0, 0.3, 0]))
    sc.triangulation = scenes._concat_tris([sc.triangulation, stack])
    return sc


def with_empty_leaves(base):
    """tests/test_parity_gpu.py: test_leaf_without_triangles_next_to_a_leaf's tree - every inner node both of whose children
    are leaves gets its second child replaced by a new inner node (an empty leaf E not flagged isEmpty, the old leaf B)."""
    sc = copy.copy(base)
    bvh = base.bvh
    leaf = bvh["isLeaf"] != 0
    parents = [i for i in range(len(bvh)) if not leaf[i] and leaf[bvh["son1Id"][i]] and leaf[bvh["son2Id"][i]]]
    assert parents
    extra = np.zeros(2 * len(parents), dtype=S.Node)
    new = np.frombuffer(bytearray(bvh.tobytes() + extra.tobytes()), dtype=S.Node)
    for j, p in enumerate(parents):
        y, e = len(bvh) + 2 * j, len(bvh) + 2 * j + 1
        b = int(new["son2Id"][p])
        new[y] = new[b]
        new["isLeaf"][y] = 0
        new["nbTriangles"][y] = 0
        new["cutAxis"][y] = (int(new["cutAxis"][p]) + 1) % 3
        new["son1Id"][y], new["son2Id"][y] = (e, b) if j % 2 == 0 else (b, e)
        new[e] = new[b]
        new["nbTriangles"][e] = 0
        new["trianglesAABB"]["isEmpty"][e] = 0
        new["son2Id"][p] = y
    sc.bvh = new
    sc.bvhMaxDepth = base.bvhMaxDepth + 1
    return sc
