"""ptmi_update_materials, ptmi_update_lights, ptmi_set_sky: what can be checked without a GPU.

The three entry points are declared, exported and bound; the info struct has the layout the header promises; a NULL context is
refused.  tests/material_screen_model.cpp - a program of its own, compiled here with g++ -fsanitize=address,undefined together
with the host files around it - holds the verdict the screen kernel of ptmi_update_materials computes from a DShade record to
build_layout's verdict on the triangle the record was made from and to the NumPy restatement of scene_edit_cases.py, on the
boundary triangles; and the one function that decides DScene::plain_shading to what build_layout reports, over every small
combination of materials, lights and the PTMI_GENERIC_SHADING switch.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from opencl_pathtracer_amd import backend, structs as S
import abi_cases
import model_build
import scene_edit_cases as E

ROOT = abi_cases.ROOT
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "material_screen_model.cpp"), os.path.join(CSRC, "scene_refit_host.cpp"), os.path.join(CSRC, "scene_layout.cpp")]
NAMES = ["ptmi_update_materials", "ptmi_update_lights", "ptmi_set_sky"]


# ---------------------------------------------------------------------------------------------- the ABI

def test_the_three_calls_are_declared_exported_and_bound():
    declared, exported = abi_cases.declared_symbols(), abi_cases.exported_symbols()
    for name in NAMES:
        assert name in declared and name in exported and name in backend.ABI_SYMBOLS, name


def test_the_info_struct_is_32_bytes_and_the_abi_version_stays_4():
    v = abi_cases.header_values(["SIZE(ptmi_material_update_info);", "OFFSET(ptmi_material_update_info, struct_size);",
                                 "OFFSET(ptmi_material_update_info, screened_triangles);", "OFFSET(ptmi_material_update_info, plain_before);",
                                 "OFFSET(ptmi_material_update_info, plain_after);", "OFFSET(ptmi_material_update_info, validate_ms);",
                                 "OFFSET(ptmi_material_update_info, total_ms);", 'VALUE("abi", PTMI_ABI_VERSION);'])
    assert v == {"ptmi_material_update_info": 32, "ptmi_material_update_info.struct_size": 0,
                 "ptmi_material_update_info.screened_triangles": 4, "ptmi_material_update_info.plain_before": 8,
                 "ptmi_material_update_info.plain_after": 12, "ptmi_material_update_info.validate_ms": 16,
                 "ptmi_material_update_info.total_ms": 24, "abi": 4}
    assert C.sizeof(backend.MaterialUpdateInfo) == 32
    for name, _ in backend.MaterialUpdateInfo._fields_:
        assert getattr(backend.MaterialUpdateInfo, name).offset == v["ptmi_material_update_info." + name], name
    assert backend.load_library().ptmi_abi_version() == 4


def test_a_null_context_is_an_invalid_argument(built):
    lib = backend.load_library()
    mats, lights, sky = np.zeros(1, S.Material), np.zeros(1, S.Light), np.zeros(1, S.Sky)
    info = backend.MaterialUpdateInfo()
    assert lib.ptmi_update_materials(None, 0, mats.ctypes.data_as(C.c_void_p), 1, C.byref(info)) == E.INVALID_ARGUMENT
    assert info.struct_size == 32  # (set before anything is looked at, as ptmi_update_triangles does)
    assert lib.ptmi_update_materials(None, 0, mats.ctypes.data_as(C.c_void_p), 1, None) == E.INVALID_ARGUMENT
    assert lib.ptmi_update_lights(None, lights.ctypes.data_as(C.c_void_p), 1) == E.INVALID_ARGUMENT
    assert lib.ptmi_set_sky(None, sky.ctypes.data_as(C.c_void_p)) == E.INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- the model program

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    model_build.sanitizer_runtimes_or_skip()
    tmp = tmp_path_factory.mktemp("material_screen")
    exe = model_build.program(SOURCES, tmp, "material_screen_model", opt=["-O1", "-g"], werror=False, fp_strict=True,
                              sanitize=model_build.SANITIZE, includes=[os.path.join(ROOT, "include"), CSRC])

    def run(*args):
        env = {k: v for k, v in os.environ.items() if k != "PTMI_GENERIC_SHADING"}
        r = subprocess.run([exe, *args], capture_output=True, text=True, env={**env, "ASAN_OPTIONS": "detect_leaks=1"})
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        return r.stdout.splitlines()

    def screen(blocks):
        """blocks: (triangles, table) -> per block (word, status, message, codes)"""
        path = str(tmp / "records.bin")
        with open(path, "wb") as f:
            for tris, simple in blocks:
                tris = np.ascontiguousarray(tris)
                assert tris.dtype == S.Triangle
                f.write(np.array([len(tris), len(simple), 0, 0], np.uint32).tobytes())
                f.write(np.asarray(simple, np.uint8).tobytes().ljust((len(simple) + 15) // 16 * 16, b"\0"))
                f.write(tris.tobytes())
        lines = run("screen", path)
        assert len(lines) == 2 * len(blocks)
        out = []
        for head, digits in zip(lines[0::2], lines[1::2]):
            word, status, text = (head + " ").split(" ", 2)
            out.append((int(word, 16), int(status), text.strip(), [int(c) for c in digits]))
        return out
    run.screen = screen
    return run


def test_the_shade_record_verdict_is_the_triangles_on_the_boundary_cases(program):
    blocks = E.boundary_blocks()
    names = [b[0] for b in blocks]
    assert len(set(names)) == len(names)
    for label in ("nan", "inf", "-inf"):  # each of the twelve slots, each of the three values
        assert sum(n.startswith(label + "_in_") for n in names) == 12
    for need in ("2^30_sign1", "above_2^30_sign1", "defect_under_plain", "defect_under_mat_neg_only", "two_defects_first_wins"):
        assert need in names
    got = program.screen([(tris, E.TABLE) for _, tris, _ in blocks])
    for (name, tris, want), (word, status, text, digits) in zip(blocks, got):
        assert E.verdict(tris, E.TABLE) == want, (name, hex(want))
        assert word == want, (name, hex(word), hex(want))
        assert digits == [int(c) for c in E.codes(tris, E.TABLE)], name
        if want == E.ACCEPTED:
            assert (status, text) == (0, ""), (name, status, text)
        else:
            assert (status, text) == (E.BAD_SCENE, E.message(want)), (name, status, text)


def test_under_a_table_of_plain_colours_every_defect_is_accepted(program):
    blocks = [b for b in E.boundary_blocks() if "material_out_of_range" not in b[0]]
    got = program.screen([(tris, [1, 1]) for _, tris, _ in blocks])
    assert all(g == (E.ACCEPTED, 0, "", [0] * 5) for g in got)
    assert all(E.verdict(tris, [1, 1]) == E.ACCEPTED for _, tris, _ in blocks)


def test_an_empty_array_and_no_materials(program):
    t = E.base_triangles(3)
    got = program.screen([(t[:0], E.TABLE), (t, [])])
    assert got[0] == (E.ACCEPTED, 0, "", [])
    assert got[1] == ((0 << 4) | E.MATERIAL, E.BAD_SCENE, E.message(E.MATERIAL), [1, 1, 1])


def test_plain_shading_is_one_rule_for_the_upload_and_the_edits(program):
    """Every combination of 0..2 materials (type, plain colour), 0..2 lights (type) and the switch: kernel_choice.h:
    scene_plain_shading agrees with build_layout's Relayout::plain_shading (the program fails otherwise) and with the rule as
    the documents state it."""
    lines = program("plain")
    seen = set()
    for line in lines:
        left, right = line.split(" : ")
        n_mats, t0, s0, t1, s1, n_lights, l0, l1, generic = [int(x) for x in left.split()]
        layout, function = [int(x) for x in right.split()]
        mats = [(t0, s0), (t1, s1)][:n_mats]
        lights = [l0, l1][:n_lights]
        want = int(not generic and all(t == S.MAT_STANDART and s for t, s in mats) and all(l == S.LIGHT_POINT for l in lights))
        assert layout == function == want, line
        seen.add((n_mats, n_lights, tuple(mats), tuple(lights), generic))
    assert len(seen) == len(lines) == sum(2 ** (2 * m + l + 1) for m in range(3) for l in range(3))
    assert {k[4] for k in seen} == {0, 1} and any(l == S.LIGHT_SPOT for k in seen for l in k[3]) and any(l == S.LIGHT_DIRECTIONNAL for k in seen for l in k[3])


def test_validate_scene_answers_as_before_on_the_edited_scenes(built):
    """ptmi_validate_scene is the yardstick of the GPU tests: a textured material with a texture id out of range, a coordinate
    beyond 2^30 under a textured material and a sky face outside the texels are refused with the words the edits repeat."""
    from opencl_pathtracer_amd import PtmiError, bvh_create, scenes
    sc = bvh_create(scenes.build("feat_textured", 64, 48))
    backend.validate_scene(sc, 64, 48, 4)
    mats = sc.materiaux.copy()
    mats["textureId"][2] = len(sc.textures)
    sky = sc.sky.copy()
    sky["skyTextures"][3] = (2, 2, len(sc.texturesData) - 3)
    floor = int(np.flatnonzero(sc.triangulation["materialWithPositiveNormalIndex"] == 0)[1])
    for bad, words in ((E.edited(sc, materiaux=mats), "material 2 has an invalid textureId"),
                       (E.edited(sc, sky=sky), "sky texture 3 outside textures_data"),
                       (E.edited(sc, triangulation=E.with_bad_coordinate(sc.triangulation, floor, E.up(2.0 ** 30))),
                        E.message((floor << 4) | E.TEXCOORD))):
        with pytest.raises(PtmiError) as e:
            backend.validate_scene(bad, 64, 48, 4)
        assert e.value.code == E.BAD_SCENE and str(e.value).endswith(": " + words), str(e.value)
    backend.validate_scene(E.edited(sc, materiaux=E.all_plain(sc.materiaux),
                                    triangulation=E.with_bad_coordinate(sc.triangulation, floor, np.nan)), 64, 48, 4)
