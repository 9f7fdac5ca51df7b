"""What the tests of the in-place scene edits share (ptmi_update_materials, ptmi_update_lights, ptmi_set_sky):
test_scene_edit_model.py on the CPU, test_scene_edit_gpu.py on the GPU.  Pure NumPy, no files.

Two things.  The screen a material update runs on the DShade records a context holds, restated on the caller's triangles -
its verdict must be build_layout's for the edited scene - with the boundary triangles it is tried on.  And the edited scenes
themselves: copies of a scene with other materials, lights or sky, which a second context is given through
ptmi_initialize_memory as the yardstick."""
import copy

import numpy as np

from opencl_pathtracer_amd import structs as S
import scene_update_cases as U

f32, u32 = np.float32, np.uint32

OK, MATERIAL, TEXCOORD = 0, 1, 2  # csrc/scene_refit_common.h: ScreenCode
ACCEPTED = 0xFFFFFFFF
INVALID_ARGUMENT, BAD_SCENE, STATE, UNSUPPORTED = -1, -5, -6, -7
WORDS = {MATERIAL: "references a material out of range", TEXCOORD: "has texture coordinates that are not finite (or beyond 2^30)"}
UV_FIELDS = ("UVP1", "UVP2", "UVP3", "UVN1", "UVN2", "UVN3")
UV_SLOTS = [(field, k) for field in UV_FIELDS for k in (0, 1)]  # the twelve coordinates of a triangle
TEXCOORD_BOUND = f32(2.0 ** 30)


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


# ---------------------------------------------------------------------------------------------- the restatement

def codes(tris, simple):
    """Per triangle what build_layout says of its materials under the table `simple` (one byte per material: plain colour?):
    an index out of range, else - one of its two materials textured - a coordinate that is not finite or beyond 2^30."""
    t = np.ascontiguousarray(tris)
    simple = np.asarray(simple, np.uint8)
    n = len(simple)
    mp, mn = t["materialWithPositiveNormalIndex"].astype(np.int64), t["materialWithNegativeNormalIndex"].astype(np.int64)
    in_range = (mp < n) & (mn < n)
    table = np.concatenate([simple, [1]])
    textured = (table[np.minimum(mp, n)] == 0) | (table[np.minimum(mn, n)] == 0)
    uv = np.concatenate([t[k] for k in UV_FIELDS], axis=1)
    with np.errstate(invalid="ignore"):
        within = (np.abs(uv) <= TEXCOORD_BOUND).all(axis=1)  # (a NaN fails the <=)
    out = np.zeros(len(t), u32)
    out[textured & ~within] = TEXCOORD
    out[~in_range] = MATERIAL
    return out


def verdict(tris, simple):
    """The whole array in one word: (index << 4) | code of the first refused triangle, or ACCEPTED."""
    c = codes(tris, simple)
    bad = np.flatnonzero(c)
    return ACCEPTED if len(bad) == 0 else (int(bad[0]) << 4) | int(c[bad[0]])


def message(word):
    """build_layout's words for the verdict `word`"""
    return f"triangle {word >> 4} {WORDS[word & 15]}"


# ---------------------------------------------------------------------------------------------- boundary triangles

PLAIN, TEXTURED = 0, 1  # the materials of the model's blocks: the table is [1, 0]
TABLE = np.array([1, 0], np.uint8)


def base_triangles(n=5):
    """n unit right triangles side by side, both materials PLAIN, texture coordinates inside [0, 1]."""
    t = np.frombuffer(bytearray(n * S.Triangle.itemsize), dtype=S.Triangle)
    for i in range(n):
        t["S1"][i], t["S2"][i], t["S3"][i] = [2 * i, 0, 0, 1], [2 * i + 1, 0, 0, 1], [2 * i, 1, 0, 1]
        for k in ("N", "N1", "N2", "N3"):
            t[k][i] = [0, 0, 1, 0]
        for j, field in enumerate(UV_FIELDS):
            t[field][i] = [0.125 * j, 0.25 + 0.0625 * i]
        t["id"][i] = i
    U.recompute_aabb(t)
    return t


def boundary_blocks():
    """[(name, triangles, expected word)]: every case of the list the issue of ptmi_update_materials sets, on five triangles
    under the table [plain, textured]."""
    out = []

    def block(name, word, *edits):
        t = base_triangles()
        for i, pos, neg, slot, value in edits:
            t["materialWithPositiveNormalIndex"][i], t["materialWithNegativeNormalIndex"][i] = pos, neg
            if slot is not None:
                t[slot[0]][i, slot[1]] = value
        out.append((name, t, word))

    tex = (TEXCOORD, )
    block("all_plain", ACCEPTED)
    block("textured_and_sound", ACCEPTED, (1, TEXTURED, TEXTURED, None, 0), (4, PLAIN, TEXTURED, None, 0))
    for sign in (1, -1):
        block(f"2^30_sign{sign}", ACCEPTED, (2, TEXTURED, TEXTURED, ("UVN2", 1), f32(sign) * TEXCOORD_BOUND))
        block(f"above_2^30_sign{sign}", (2 << 4) | TEXCOORD, (2, TEXTURED, TEXTURED, ("UVN2", 1), f32(sign) * up(TEXCOORD_BOUND)))
    for k, slot in enumerate(UV_SLOTS):
        for label, value in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
            i = k % 5
            block(f"{label}_in_{slot[0]}.{slot[1]}", (i << 4) | TEXCOORD, (i, TEXTURED, TEXTURED, slot, value))
    block("defect_under_plain", ACCEPTED, (3, PLAIN, PLAIN, ("UVP2", 0), np.nan), (0, TEXTURED, TEXTURED, None, 0))
    block("defect_under_mat_neg_only", (3 << 4) | TEXCOORD, (3, PLAIN, TEXTURED, ("UVP3", 1), np.inf))
    block("defect_under_mat_pos_only", (0 << 4) | TEXCOORD, (0, TEXTURED, PLAIN, ("UVN1", 0), up(TEXCOORD_BOUND)))
    block("two_defects_first_wins", (1 << 4) | TEXCOORD, (1, TEXTURED, TEXTURED, ("UVP1", 0), np.inf), (4, TEXTURED, TEXTURED, ("UVN3", 1), np.nan))
    block("material_out_of_range", (1 << 4) | MATERIAL, (1, PLAIN, 2, None, 0), (3, TEXTURED, TEXTURED, ("UVP1", 1), np.nan))
    assert all(word == ACCEPTED or word & 15 in tex + (MATERIAL, ) for _, _, word in out)
    return out


# ---------------------------------------------------------------------------------------------- edited scenes

def edited(sc, **fields):
    """A copy of scene `sc` with the given arrays replaced (materiaux, lights, sky, textures, texturesData, triangulation)."""
    out = copy.copy(sc)
    for k, v in fields.items():
        assert hasattr(out, k), k
        setattr(out, k, v)
    return out


def all_plain(materiaux):
    """The materials as plain-colour MAT_STANDART ones of their own simpleColor (a textured one gets a grey)"""
    m = U.raw_copy(materiaux)
    m["type"] = S.MAT_STANDART
    grey = m["isSimpleColor"] == 0
    m["simpleColor"][grey] = f32([0.5, 0.5, 0.5, 0])
    m["isSimpleColor"] = 1
    m["textureId"] = 0  # (as scenes.material_create leaves it)
    return m


def with_one_texture(sc, material=0):
    """`sc` with a 2x2 texture appended to its texels (all materials still plain), and the material record that uses it."""
    texels = np.concatenate([np.ascontiguousarray(sc.texturesData).reshape(-1, 4),
                             np.array([[230, 40, 40, 0], [40, 230, 40, 0], [40, 40, 230, 0], [230, 230, 40, 0]], np.uint8)])
    textures = np.concatenate([np.ascontiguousarray(sc.textures), np.array([(2, 2, len(texels) - 4)], dtype=S.Texture)])
    out = edited(sc, texturesData=texels, textures=textures)
    textured = U.raw_copy(sc.materiaux[material:material + 1])
    textured["isSimpleColor"] = 0
    textured["textureId"] = len(textures) - 1
    return out, textured


def with_bad_coordinate(tris, at, value, slot=("UVN2", 1)):
    t = U.raw_copy(tris)
    for i in np.atleast_1d(at):
        t[slot[0]][i, slot[1]] = value
    return t
