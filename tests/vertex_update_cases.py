"""What the tests of ptmi_update_vertices share (test_mesh_assemble_model.py on the CPU, test_update_vertices_gpu.py on the GPU):
a NumPy restatement of the record include/ptmi.h promises (steps 1-6 of its comment on ptmi_update_vertices), one binary32
operation per line, the unit meshes that put each branch of it to the test, and the derived meshes of the test scenes at rest
and moved.  Pure numpy; of the product only scenes.mesh_from_triangulation is called, to derive those meshes."""
import types

import numpy as np

from opencl_pathtracer_amd import scenes, structs as S

f32, u32 = np.float32, np.uint32
NAN = f32(np.nan)
OUTCOMES = 6  # of the Vector_LexLessThan cascade (MayaImporter.cpp:961-1020), numbered in the order they are written there
# per outcome: which corner of the face becomes S1, S2, S3
PLACED = np.array([[0, 1, 2], [0, 2, 1], [2, 0, 1], [1, 0, 2], [1, 2, 0], [2, 1, 0]])


def mesh(positions, indices, normals=None, uvp=None, uvn=None, mat_pos=None, mat_neg=None, ids=None):
    indices = np.asarray(indices, u32).reshape(-1, 3)
    return types.SimpleNamespace(positions=np.asarray(positions, f32).reshape(-1, 3),
                                 normals=None if normals is None else np.asarray(normals, f32).reshape(-1, 3), indices=indices,
                                 uvp=None if uvp is None else np.asarray(uvp, f32).reshape(-1, 3, 2),
                                 uvn=None if uvn is None else np.asarray(uvn, f32).reshape(-1, 3, 2),
                                 mat_pos=np.zeros(len(indices), u32) if mat_pos is None else np.asarray(mat_pos, u32),
                                 mat_neg=None if mat_neg is None else np.asarray(mat_neg, u32),
                                 ids=None if ids is None else np.asarray(ids, u32))


KEEP = object()  # with_buffers(normals=...): the mesh's normals as they are (None there means a flat mesh)


def with_buffers(m, positions=None, normals=KEEP):
    """`m` with other vertex buffers (normals None: flat)"""
    out = types.SimpleNamespace(**vars(m))
    if positions is not None:
        out.positions = np.asarray(positions, f32).reshape(-1, 3)
    if normals is not KEEP:
        out.normals = None if normals is None else np.asarray(normals, f32).reshape(-1, 3)
    return out


def padded(a, stride):
    """The (V, 3) array `a` as a view of rows `stride` bytes apart, NaN in every word between them"""
    a = np.asarray(a, f32).reshape(-1, 3)
    buf = np.full((len(a), stride // 4), NAN, f32)
    buf[:, :3] = a
    return buf[:, :3]


_meshes = {}


def derived(name):
    """scenes.mesh_from_triangulation of scene `name` (scene_record_cases.scene), once; read-only"""
    if name not in _meshes:
        import scene_record_cases as R
        _meshes[name] = scenes.mesh_from_triangulation(R.scene(name).triangulation)
    return _meshes[name]


def moved(name, seed=7, perturb_normals=False):
    """The derived mesh with every VERTEX displaced by the seeded offset of scene_update_cases.displaced (uniform, at most 0.01
    per axis on tris20k, 0.02 elsewhere): the topology stays, as in an update.  perturb_normals: every vertex normal offset by
    at most 0.2 per axis as well, and left at whatever length that gives."""
    m = derived(name)
    amplitude = 0.01 if name == "tris20k" else 0.02
    rs = np.random.default_rng(seed)
    out = with_buffers(m, positions=m.positions + rs.uniform(-amplitude, amplitude, m.positions.shape).astype(f32))
    if perturb_normals:
        out.normals = (m.normals + np.random.default_rng(seed + 1).uniform(-0.2, 0.2, m.normals.shape).astype(f32)).astype(f32)
    return out


# ---------------------------------------------------------------------------------------------- the restatement

def _min(a, b):
    return np.where(b < a, b, a)  # std::min: a tie keeps the first (np.minimum does not promise that)


def _max(a, b):
    return np.where(a < b, b, a)


def _dot3(a, b):
    xx = a[..., 0] * b[..., 0]
    yy = a[..., 1] * b[..., 1]
    zz = a[..., 2] * b[..., 2]
    s = xx + yy
    return s + zz


def _lex_less(a, b):
    ex, ey = a[:, 0] == b[:, 0], a[:, 1] == b[:, 1]
    return (a[:, 0] < b[:, 0]) | (ex & (a[:, 1] < b[:, 1])) | (ex & ey & (a[:, 2] < b[:, 2]))


def _point4(xyz, w):
    out = np.empty(xyz.shape[:-1] + (4,), f32)
    out[..., :3] = xyz
    out[..., 3] = w
    return out


def restate(m):
    """(the structs.Triangle records of mesh `m`, the cascade's outcome per face, which of the 3 x F shading normals fell back to N)"""
    idx = np.asarray(m.indices, np.int64).reshape(-1, 3)
    n = len(idx)
    pos = np.asarray(m.positions, f32)[:, :3]
    with np.errstate(all="ignore"):
        # 1. corners, in the face's own winding
        p = _point4(pos[idx], 1.0)  # (n, 3, 4)
        # 2. box
        lo = _min(_min(p[:, 0], p[:, 1]), p[:, 2])
        hi = _max(_max(p[:, 0], p[:, 1]), p[:, 2])
        both = lo + hi
        centroid = both / f32(2)
        # 3. normal
        e1 = p[:, 1, :3] - p[:, 0, :3]
        e2 = p[:, 2, :3] - p[:, 0, :3]
        a = e1[:, 1] * e2[:, 2]
        b = e1[:, 2] * e2[:, 1]
        cx = a - b
        a = e1[:, 2] * e2[:, 0]
        b = e1[:, 0] * e2[:, 2]
        cy = a - b
        a = e1[:, 0] * e2[:, 1]
        b = e1[:, 1] * e2[:, 0]
        cz = a - b
        c = np.stack([cx, cy, cz], axis=-1)
        ll = _dot3(c, c)
        l = np.sqrt(ll)
        N = np.ones((n, 4), f32)
        N[:, 0] = cx / l
        N[:, 1] = cy / l
        N[:, 2] = cz / l
        if m.normals is None:
            mm = _point4(np.repeat(N[:, None, :3], 3, axis=1), 0.0)
        else:
            mm = _point4(np.asarray(m.normals, f32)[:, :3][idx], 0.0)
        # 4. order: the cascade, written out
        l01, l12, l02 = _lex_less(p[:, 0], p[:, 1]), _lex_less(p[:, 1], p[:, 2]), _lex_less(p[:, 0], p[:, 2])
        outcome = np.where(l01, np.where(l12, 0, np.where(l02, 1, 2)), np.where(l02, 3, np.where(l12, 4, 5)))
        order = PLACED[outcome]
        rows = np.arange(n)[:, None]
        uvp = np.zeros((n, 3, 2), f32) if m.uvp is None else np.asarray(m.uvp, f32).reshape(n, 3, 2)
        uvn = uvp if m.uvn is None else np.asarray(m.uvn, f32).reshape(n, 3, 2)
        p, mm, uvp, uvn = p[rows, order], mm[rows, order], uvp[rows, order], uvn[rows, order]
        # 5. shading normals
        lk2 = _dot3(mm, mm)
        lk = np.sqrt(lk2)
        fallback = lk < f32(0.5)
        divided = mm / lk[..., None]
        shading = np.where(fallback[..., None], N[:, None, :], divided).astype(f32)
    # 6. the rest: a record of zero bytes, then the fields
    t = np.frombuffer(bytearray(max(n, 1) * S.Triangle.itemsize), dtype=S.Triangle)[:n]
    for k, name in enumerate(("S1", "S2", "S3")):
        t[name] = p[:, k]
    for k, name in enumerate(("N1", "N2", "N3")):
        t[name] = shading[:, k]
    for k, name in enumerate(("UVP1", "UVP2", "UVP3")):
        t[name] = uvp[:, k]
    for k, name in enumerate(("UVN1", "UVN2", "UVN3")):
        t[name] = uvn[:, k]
    t["N"] = N
    box = t["AABB"]  # (a view: the array owns its bytes)
    box["pMin"], box["pMax"], box["centroid"] = lo, hi, centroid
    t["materialWithPositiveNormalIndex"] = m.mat_pos
    t["materialWithNegativeNormalIndex"] = m.mat_pos if m.mat_neg is None else m.mat_neg
    t["id"] = np.arange(n, dtype=u32) if m.ids is None else m.ids
    return t, outcome, fallback


def words(tris):
    """(n, 84) uint32: a record array word for word"""
    return np.frombuffer(np.ascontiguousarray(tris).tobytes(), u32).reshape(len(tris), 84)


def describe_difference(got, want, what=""):
    """"" where two record arrays agree word for word, else the first few words that differ"""
    g, w = words(got), words(want)
    if g.shape != w.shape:
        return f"{what}: {g.shape[0]} records, expected {w.shape[0]}"
    bad = np.argwhere(g != w)
    if len(bad) == 0:
        return ""
    lines = [f"{what}: {len(np.unique(bad[:, 0]))} of {len(w)} records differ"]
    for i, k in bad[:8]:
        lines.append(f"    record {int(i)} word {int(k)} (byte {4 * int(k)}): 0x{int(g[i, k]):08x}, expected 0x{int(w[i, k]):08x}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------- unit meshes

A, B, C3 = [0.25, 0.5, 0.75], [1.0, -2.0, 3.0], [4.0, 0.125, -1.0]  # A < B < C3 lexicographically, in x already
UV = np.arange(1, 13, dtype=f32).reshape(1, 6, 2) / f32(16)  # twelve distinct coordinates: uvp of the three corners, then uvn
PERMUTATIONS = [(0, 1, 2), (0, 2, 1), (1, 2, 0), (1, 0, 2), (2, 0, 1), (2, 1, 0)]  # face k of `six_outcomes` has outcome k


def _six(points, normals=None):
    uv = np.repeat(UV, 6, axis=0)
    return mesh(points, PERMUTATIONS, normals=normals, uvp=uv[:, :3], uvn=uv[:, 3:], mat_pos=np.arange(6), mat_neg=np.arange(6)[::-1],
                ids=100 + np.arange(6))


def _without(m, *fields):
    for f in fields:
        setattr(m, f, None)
    return m


def _lengths():
    below = np.nextafter(f32(0.5), f32(0))
    normals = [[0, 0, 0], [below, 0, 0], [0, 0.5, 0], [0, 0, 3], [0.3, 0.3, 0.3], [-0.0, 0, 0]]
    pts = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 0, 1], [0, 2, 1]]
    return mesh(pts, [[0, 1, 2], [3, 4, 5], [1, 3, 5], [0, 2, 4]], normals=normals)


def _fan(k=40):
    ang = np.linspace(0, 2 * np.pi, k, endpoint=False)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], axis=1)
    pts = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(f32)
    faces = [[0, 1 + i, 1 + (i + 1) % k] for i in range(k)]
    nrm = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    return mesh(pts, faces, normals=nrm.astype(f32))


BIG = f32(2.0 ** 21)
UNIT_CASES = {
    # each of the six outcomes, in order; with smooth normals of length 2 that travel with their corners
    "six_outcomes": _six([A, B, C3], normals=[[2, 0, 0], [0, 2, 0], [0, 0, 2]]),
    "six_outcomes_flat": _six([A, B, C3]),
    # each default of the topology on its own: uvp NULL = zeros while uvn is given, uvn NULL = uvp, mat_neg NULL = mat_pos, ids NULL = i
    "uvn_only": _without(_six([A, B, C3]), "uvp"),
    "uvp_only": _without(_six([A, B, C3]), "uvn"),
    "no_mat_neg": _without(_six([A, B, C3]), "mat_neg"),
    "no_ids": _without(_six([A, B, C3]), "ids"),
    # equal x: y decides; equal x and y: z decides
    "ties_in_x": _six([[1, 0, 5], [1, 2, -5], [1, 3, 0]]),
    "ties_in_x_and_y": _six([[1, 2, -1], [1, 2, 0], [1, 2, 7]]),
    # -0.0 == +0.0, so y decides
    "signed_zero_x": _six([[0.0, 1, 0], [-0.0, 2, 0], [0.0, 3, 1]]),
    # +-0 ties in the box: which zero pMin and pMax keep depends on the corner order
    "signed_zero_box": _six([[0.0, -0.0, 0.0], [-0.0, 0.0, 1.0], [1.0, -0.0, -0.0]]),
    "normal_lengths": _lengths(),
    "nan_normal": mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], normals=[[0, 0, 1], [np.nan, 0, 0], [0, 1, 0]]),
    "index_twice": mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 1], [2, 2, 2], [0, 1, 2]], normals=[[0, 0, 1]] * 3),
    "two_to_the_21": mesh([[BIG, 0, 0], [np.nextafter(BIG, f32(np.inf)), 1, 0], [0, BIG, 1], [0, 0, -BIG]], [[0, 1, 2], [1, 2, 3], [3, 0, 1]]),
    "shared_index": _fan(),
}
STRIDES = (12, 16, 32)


def check_the_list():
    """The promises of the list: face k of the permuted meshes has outcome k; the fallback to N is taken and not taken; the box
    of `signed_zero_box` holds zeros of both signs."""
    for name in ("six_outcomes", "six_outcomes_flat", "ties_in_x", "ties_in_x_and_y", "signed_zero_x"):
        _, outcome, _ = restate(UNIT_CASES[name])
        assert list(outcome) == list(range(OUTCOMES)), (name, outcome)
    t, _, fallback = restate(UNIT_CASES["normal_lengths"])
    assert fallback.any() and not fallback.all()
    # per vertex: 0 and the value below one half fall back, one half and 3 do not
    m = UNIT_CASES["normal_lengths"]
    assert np.array_equal(t["N1"][0], t["N"][0]) and t["N1"][0][3] == 1  # vertex 0 (length 0) is the least corner of face 0
    lo = words(restate(UNIT_CASES["signed_zero_box"])[0])[:, 64:68]
    assert len({int(x) for x in lo[:, 0]}) == 2, "pMin.x is +0 in some corner orders and -0 in others"
    t, _, _ = restate(UNIT_CASES["index_twice"])
    assert np.isnan(t["N"][0][:3]).all() and np.isnan(t["N"][1][:3]).all() and not np.isnan(t["N"][2]).any()
    assert m.normals is not None
    t = restate(UNIT_CASES["uvn_only"])[0]
    assert not t["UVP1"].any() and t["UVN1"].all() and t["UVN3"].all()  # zeros for uvp, the caller's uvn
    t = restate(UNIT_CASES["uvp_only"])[0]
    assert t["UVP2"].all() and np.array_equal(t["UVP2"], t["UVN2"])
