"""What the tests of the device scene records share (test_scene_refit_model.py, test_tri_record_exact.py on the CPU,
test_scene_records_gpu.py on the GPU): the scenes, the serial model of the record arrays (tests/scene_refit_model.cpp, built by
`make -C oracle probe` into oracle/build/libscene_refit_model.so: build_layout, and the device side of ptmi_update_triangles
lane by lane), the motions the update tests apply, the reader of a context's device records (oracle/scene_record_probe.cpp) and
the word-for-word comparison of two sets of record arrays.  No product code is changed by any of it."""
import copy
import ctypes as C
import os

import numpy as np

from opencl_pathtracer_amd import backend, bvh_create, scenes, structs as S
import bvh_stress_cases as stress
import gpu_cases
import scene_update_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_LIB = os.path.join(ROOT, "oracle", "build", "libscene_refit_model.so")
PROBE_LIB = os.path.join(ROOT, "oracle", "build", "libscene_record_probe.so")
W, H = 64, 48
OK = 0
f32, u32 = np.float32, np.uint32
NO_TRIANGLE = 0xFFFFFFFF  # tri_ids[] of a node record
REF_EMPTY = 0x40000000
ARRAYS = ("recs", "tri_ids", "shade", "big_leaves")
U_DEN_W = 11  # the word of a DTriPre record that holds u_den[3]: n[4], s1d[4], u_den[4], v_s1w[4]

# the scenes of the model tests (test_scene_refit_model.py)
MODEL_SCENES = ["cornell", "tris20k", "fuzz3_l1", "fuzz7_l1", "fuzz12_l1", "big_leaf", "signed_zero-s0", "signed_zero-s1"]

# its triangles span 2^27 units: the one-path-per-lane kernel renders it (ptmi_literal_kernel_reason), ptmi_update_triangles refuses it
NOT_UPDATABLE = ("deep_chain_27",)

_scenes = {}


def scene(name):
    """`big_leaf`, `empty_leaves` (of cornell), `textured`, `signed_zero-s<seed>` (4096 triangles), `deep_chain_27`, `chain_26`
    (cornell under a hand-made chain), `cornell*2^<k>` (cornell and its tree scaled by a power of two), or a name scenes.build
    knows - with its tree, at W x H, built once."""
    if name not in _scenes:
        if name.startswith("signed_zero"):
            sc = scenes.cornell_box(W, H)
            sc.triangulation = stress.make("signed_zero_lattice", int(name[-1]), 16 ** 3)
            sc = bvh_create(sc)
        elif name == "deep_chain_27":
            sc = scenes.cornell_box(W, H)
            sc.triangulation = stress.make("deep_chain_27", 0, 56)
            sc = bvh_create(sc)
            assert sc.bvhMaxDepth > 22
        elif name == "textured":
            sc = bvh_create(scenes.feature_scene("textured", W, H))
        elif name == "chain_26":
            sc = chain_scene(scene("cornell"), 26)
        elif name.startswith("cornell*2^"):
            sc = scaled(scene("cornell"), int(name[len("cornell*2^"):]))
        else:
            sc = gpu_cases.cached_scene(name, W, H)
        _scenes[name] = sc
    return _scenes[name]


# ---------------------------------------------------------------------------------------------- motions

def scaled(sc, k):
    """`sc` with its tree, scaled uniformly by 2^k about the origin: vertices, every box of the triangles and of the tree, the
    camera position and the lights' positions.  Every product is exact, so this is the same scene, and the same tree, in another
    exponent range."""
    out = copy.copy(sc)
    m = np.array([2.0 ** k] * 3 + [1.0], f32)
    t = U.raw_copy(sc.triangulation)
    for field in ("S1", "S2", "S3"):
        t[field] = t[field] * m
    bvh = U.raw_copy(sc.bvh)
    for boxes in (t["AABB"], bvh["trianglesAABB"], bvh["centroidsAABB"]):  # (views: the arrays own their bytes)
        for corner in ("pMin", "pMax", "centroid"):
            boxes[corner] = boxes[corner] * m
    out.triangulation, out.bvh = t, bvh
    out.cameraPosition = (np.asarray(sc.cameraPosition, f32) * m).astype(f32)
    lights = U.raw_copy(sc.lights)
    lights["position"] = lights["position"] * m
    out.lights = lights
    return out


def chain_scene(base, inner):
    """`base`'s triangles under a hand-made chain, the shape of deep_chain's trees inside the coordinate range an update accepts:
    inner node k (index 2k) has the leaf of triangle k as its first child and inner node k + 1 as its second, the last one a
    leaf with the remaining triangles.  One inner node per level, `inner` levels.  The boxes are ptmi_bvh_refit's."""
    tris = base.triangulation
    n = len(tris)
    assert 0 < n - inner <= 6
    bvh = np.frombuffer(bytearray(2 * inner + 1) * S.Node.itemsize, dtype=S.Node)
    for k in range(inner):
        bvh["triangleStartIndex"][2 * k], bvh["nbTriangles"][2 * k] = k, n - k
        bvh["son1Id"][2 * k], bvh["son2Id"][2 * k] = 2 * k + 1, 2 * k + 2
        bvh["triangleStartIndex"][2 * k + 1], bvh["nbTriangles"][2 * k + 1], bvh["isLeaf"][2 * k + 1] = k, 1, 1
    bvh["triangleStartIndex"][2 * inner], bvh["nbTriangles"][2 * inner], bvh["isLeaf"][2 * inner] = inner, n - inner, 1
    rc, msg, bvh = U.bvh_refit(tris, bvh)
    assert rc == OK, msg
    out = copy.copy(base)
    out.bvh, out.bvhMaxDepth = bvh, inner
    return out


def snapped_to_signed_zero(tris, seed, amplitude=0.02):
    """U.displaced(tris, seed, amplitude), then a seeded tenth of the vertex coordinates that lie within `amplitude` of 0 set to
    -0.0 or +0.0 (seeded), the derived fields following: new corners that tie with held zeros of the other sign."""
    t = U.displaced(tris, seed, amplitude)
    rs = np.random.default_rng(1000 + seed)
    snapped = 0
    for field in ("S1", "S2", "S3"):
        v = t[field].copy()
        near = np.abs(v[:, :3]) <= f32(amplitude)
        pick = near & (rs.random(near.shape) < 0.1)
        zero = np.where(rs.random(near.shape) < 0.5, f32(-0.0), f32(0.0)).astype(f32)
        v[:, :3] = np.where(pick, zero, v[:, :3])
        t[field] = v
        snapped += int(pick.sum())
    assert snapped > 0
    U.follow_vertices(t)
    return t


def shrunk(tris, fraction=0.02):
    """Every vertex pulled `fraction` of the way towards its triangle's centroid (computed in double, rounded once: a coordinate
    stays between the triangle's least and greatest, so no aabb grows); N keeps its side, the aabb follows."""
    t = U.raw_copy(tris)
    p = np.stack([t["S1"], t["S2"], t["S3"]], axis=1).astype(np.float64)
    c = p.sum(axis=1, keepdims=True) / 3.0
    q = (p + (c - p) * fraction).astype(f32)
    q[:, :, 3] = np.stack([t["S1"], t["S2"], t["S3"]], axis=1)[:, :, 3]
    t["S1"], t["S2"], t["S3"] = q[:, 0], q[:, 1], q[:, 2]
    U.follow_vertices(t)
    return t


# ---------------------------------------------------------------------------------------------- the model

class Model:
    def __init__(self, so):
        m = C.CDLL(so)
        m.model_layout.restype = C.c_void_p
        m.model_layout.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        m.model_layout_uploaded.restype = C.c_void_p
        m.model_layout_uploaded.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        m.model_layout_free.argtypes = [C.c_void_p]
        m.model_layout_info.argtypes = [C.c_void_p, C.c_void_p]
        m.model_layout_copy.argtypes = [C.c_void_p] * 5
        m.model_update.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        m.model_error.restype = C.c_char_p
        self.m = m

    def layout(self, sc, for_update=True):
        """for_update: a scene ptmi_update_triangles would refuse as a whole (its ptmi_literal_kernel_reason) is refused here"""
        cfg = backend.Config(C.sizeof(backend.Config), 0, W, H, 4, sc.lightsSize, S.JITTERED, 0, 0)
        d, keep = backend.scene_desc(sc)
        rc = C.c_int(0)
        h = (self.m.model_layout if for_update else self.m.model_layout_uploaded)(C.addressof(cfg), C.addressof(d), C.byref(rc))
        assert rc.value == OK and h, self.m.model_error()
        return h

    def arrays(self, h):
        """info: n_records, n_triangles, n_big_leaves, root_ref, tris_precomputed, max_depth"""
        info = np.zeros(6, np.uint32)
        self.m.model_layout_info(h, info.ctypes.data_as(C.c_void_p))
        n_rec, n_tri, n_big = int(info[0]), int(info[1]), int(info[2])
        recs, ids = np.zeros((n_rec, 16), np.uint32), np.zeros(n_rec, np.uint32)
        shade, big = np.zeros((n_tri, 28), np.uint32), np.zeros((max(n_big, 1), 2), np.uint32)
        self.m.model_layout_copy(h, *[a.ctypes.data_as(C.c_void_p) for a in (recs, ids, shade, big)])
        return dict(recs=recs, tri_ids=ids, shade=shade, big_leaves=big[:n_big], info=info)

    def update(self, h, tris, order_seed):
        levels = C.c_uint32(0)
        tris = np.ascontiguousarray(tris)
        rc = self.m.model_update(h, tris.ctypes.data_as(C.c_void_p), len(tris), order_seed, C.byref(levels))
        return rc, self.m.model_error().decode(), levels.value

    def free(self, h):
        self.m.model_layout_free(h)

    def layout_arrays(self, sc, for_update=True):
        """build_layout's arrays for `sc` under the environment as it is (PTMI_GENERIC_TRIANGLES)."""
        h = self.layout(sc, for_update)
        try:
            return self.arrays(h)
        finally:
            self.free(h)


_model = []


def model():
    """The built model library (loaded once), or None where `make -C oracle probe` has not built it."""
    if not _model:
        _model.append(Model(MODEL_LIB) if os.path.exists(MODEL_LIB) else None)
    return _model[0]


_layouts = {}


def cached_layout(name, generic):
    """model().layout_arrays(scene(name)) with the generic / precomputed triangle records, computed once; read-only."""
    key = (name, bool(generic))
    if key not in _layouts:
        _layouts[key] = layout_in_mode(scene(name), generic, for_update=name not in NOT_UPDATABLE)
    return _layouts[key]


def layout_in_mode(sc, generic, for_update=True):
    """model().layout_arrays(sc) with PTMI_GENERIC_TRIANGLES set (generic) or unset, whatever the environment says."""
    old = os.environ.pop("PTMI_GENERIC_TRIANGLES", None)
    try:
        if generic:
            os.environ["PTMI_GENERIC_TRIANGLES"] = "1"
        lay = model().layout_arrays(sc, for_update)
    finally:
        os.environ.pop("PTMI_GENERIC_TRIANGLES", None)
        if old is not None:
            os.environ["PTMI_GENERIC_TRIANGLES"] = old
    assert int(lay["info"][4]) == (0 if generic else 1)
    for a in ARRAYS:
        lay[a].setflags(write=False)
    return lay


def with_default_arithmetic_denominators(lay, tris):
    """`lay` as a context in the default arithmetic holds it: u_den[3] of every DTriPre record is what the default-arithmetic
    oracle computes for FullKernel.cl:556 from that record's triangle (pto_triangle_inverse_determinant); every other word,
    and every word of generic records, is the layout's."""
    if not int(lay["info"][4]):
        return lay
    import oracle_ffi as O
    lib = O.oracle(True)
    lib.pto_triangle_inverse_determinant.argtypes = [C.c_void_p]
    lib.pto_triangle_inverse_determinant.restype = C.c_float
    tris = np.ascontiguousarray(tris)
    base, step = tris.ctypes.data, tris.dtype.itemsize
    den = np.array([lib.pto_triangle_inverse_determinant(base + i * step) for i in range(len(tris))], f32).view(u32)
    out = dict(lay)
    recs = lay["recs"].copy()
    rows = np.flatnonzero(lay["tri_ids"] != NO_TRIANGLE)
    recs[rows, U_DEN_W] = den[lay["tri_ids"][rows]]
    recs.setflags(write=False)
    out["recs"] = recs
    return out


# ---------------------------------------------------------------------------------------------- comparison

def describe_difference(got, want, what=""):
    """"" where the four arrays are equal word for word, else: per array the number of entries that differ and, for the first
    few, the entry, the triangle behind it (records: through tri_ids; `node` for a node record), the word and both values."""
    lines = []
    for key in ARRAYS:
        g, w = got[key], want[key]
        if g.shape != w.shape:
            lines.append(f"{key}: shape {g.shape}, expected {w.shape}")
            continue
        if len(w) == 0:
            continue
        g2, w2 = g.reshape(len(w), -1), w.reshape(len(w), -1)
        bad = np.flatnonzero((g2 != w2).any(axis=1))
        if len(bad) == 0:
            continue
        lines.append(f"{key}: {len(bad)} of {len(w)} entries differ")
        for r in bad[:6]:
            if key in ("recs", "tri_ids"):
                tid = int(want["tri_ids"][r])
                who = "node record" if tid == NO_TRIANGLE else f"triangle {tid}"
            elif key == "shade":
                who = f"triangle {int(r)}"
            else:
                who = "big leaf"
            for word in np.flatnonzero(g2[r] != w2[r])[:4]:
                lines.append(f"    {key}[{int(r)}] ({who}) word {int(word)}: 0x{int(g2[r, word]):08x}, expected 0x{int(w2[r, word]):08x}")
    return (what + "\n" if lines and what else "") + "\n".join(lines)


def same_arrays(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ARRAYS)


# ---------------------------------------------------------------------------------------------- the reader

_probe = []


def probe():
    """oracle/build/libscene_record_probe.so (loaded once), or None where it has not been built."""
    if not _probe:
        lib = None
        if os.path.exists(PROBE_LIB):
            backend.load_library()  # (the library the probe asks ptmi_synchronize of: the process's one copy)
            lib = C.CDLL(PROBE_LIB)
            lib.probe_record_sizes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            lib.probe_read_records.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
        _probe.append(lib)
    return _probe[0]


def record_sizes(be, device_index=0):
    """(status, [n_records, triangles, n_big_leaves, tris_precomputed, root_ref, listed devices]) of backend context `be`"""
    out = np.zeros(6, u32)
    rc = probe().probe_record_sizes(be._ctx, device_index, out.ctypes.data_as(C.c_void_p))
    return rc, out


def read_records(be, want, device_index=0):
    """The four record arrays listed device `device_index` of `be` holds, as uint32 words.  `want`: a layout of the model; the
    sizes the context reports must be that layout's BEFORE anything is copied."""
    rc, sizes = record_sizes(be, device_index)
    assert rc == OK, f"probe_record_sizes: {rc}"
    info = want["info"]
    assert [int(x) for x in sizes[:5]] == [int(info[0]), int(info[1]), int(info[2]), int(info[4]), int(info[3])], \
        f"the context reports {sizes[:5]} (records, triangles, big leaves, precomputed, root), the model {info}"
    n_rec, n_tri, n_big = int(sizes[0]), int(sizes[1]), int(sizes[2])
    recs, ids = np.zeros((n_rec, 16), u32), np.zeros(n_rec, u32)
    shade, big = np.zeros((n_tri, 28), u32), np.zeros((max(n_big, 1), 2), u32)
    rc = probe().probe_read_records(be._ctx, device_index, *[a.ctypes.data_as(C.c_void_p) for a in (recs, ids, shade, big)])
    assert rc == OK, f"probe_read_records: {rc}"
    return dict(recs=recs, tri_ids=ids, shade=shade, big_leaves=big[:n_big], n_devices=int(sizes[5]))
