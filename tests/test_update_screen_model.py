"""The screen of an in-place triangle update, checked on the host.

csrc/scene_refit_common.h holds ONE classification of a new triangle - a small refusal code - which the host loops
(ptmi_update_triangles, ptmi_initialize_memory, ptmi_validate_scene) and the screen kernel of ptmi_update_triangles_device
share.  tests/update_screen_model.cpp runs it as a program of its own, compiled here with g++ -ffp-contract=off
-fsanitize=address,undefined together with the host files around it, over files of records and facts; what it prints is held,
string for string, to the NumPy restatement of update_screen_cases.py and to the words ptmi_update_triangles has always said.
The scenes' own triangulations are accepted whole.  ptmi_validate_scene and build_layout (through the serial model of
scene_record_cases.py) still say what they said on the cases that reach them.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from opencl_pathtracer_amd import PtmiError, backend, structs as S
import model_build
import scene_record_cases as R
import update_screen_cases as X

ROOT = R.ROOT
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "update_screen_model.cpp"), os.path.join(CSRC, "scene_refit_host.cpp"), os.path.join(CSRC, "scene_layout.cpp")]
BASES = ["cornell", "feat_textured"]
WHOLE = ["cornell", "feat_textured", "signed_zero-s0", "tris20k"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    model_build.sanitizer_runtimes_or_skip()
    tmp = tmp_path_factory.mktemp("update_screen")
    exe = model_build.program(SOURCES, tmp, "update_screen_model", opt=["-O1", "-g"], werror=False, fp_strict=True,
                              sanitize=model_build.SANITIZE, includes=[os.path.join(ROOT, "include"), CSRC])

    def run(blocks):
        """blocks: (triangles, facts) -> per block (word, status, message)"""
        path = str(tmp / "records.bin")
        with open(path, "wb") as f:
            for tris, facts in blocks:
                tris = np.ascontiguousarray(tris)
                assert tris.dtype == S.Triangle
                f.write(np.array([len(tris), len(facts.simple), int(facts.precomputed), 0], np.uint32).tobytes())
                f.write(facts.simple.tobytes().ljust((len(facts.simple) + 15) // 16 * 16, b"\0"))
                f.write(tris.tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        out = []
        for line in r.stdout.splitlines():
            word, status, text = (line + " ").split(" ", 2)
            out.append((int(word, 16), int(status), text.strip()))
        assert len(out) == len(blocks)
        return out
    return run


def placements(n, targets):
    """Where a case goes: the first and the last triangle (and for two targets a pair in between)"""
    return [[0], [n // 2], [n - 1]] if targets == 1 else [[0, n - 1], [n // 3, n // 2]]


def test_the_case_list_keeps_its_promises():
    X.check_the_list()


@pytest.mark.parametrize("precomputed", [True, False], ids=["precomputed", "generic"])
@pytest.mark.parametrize("base", BASES)
def test_every_case_gets_the_restatements_verdict_and_the_old_words(program, base, precomputed):
    sc = R.scene(base)
    facts = X.Facts.of(sc, precomputed)
    if base == "feat_textured":
        assert facts.material(True) is not None and facts.material(False) is not None
    blocks, want = [], []
    for case in X.CASES:
        for at in placements(len(sc.triangulation), case.targets):
            tris = case.apply(sc.triangulation, at, facts)
            word = X.verdict(tris, facts)
            assert word == case.word(at, facts), (case.name, at, hex(word), hex(case.word(at, facts)))
            blocks.append((tris, facts))
            want.append((case.name, at, word))
    seen = set()
    for (name, at, word), (got, status, text) in zip(want, program(blocks)):
        assert got == word, (name, at, hex(got), hex(word))
        if word == X.ACCEPTED:
            assert (status, text) == (0, ""), (name, at, status, text)
        else:
            assert status == X.STATUS[word & 15] and text == X.message(word), (name, at, status, text)
            seen.add(word & 15)
    assert seen == set(range(1, 9)) - (set() if precomputed else {X.UNEQUAL_W}) - (set() if facts.material(True) is not None else {X.TEXCOORD})


@pytest.mark.parametrize("name", WHOLE)
def test_the_scenes_own_triangles_are_accepted(program, name):
    sc = R.scene(name)
    facts = X.Facts.of(sc)
    assert X.verdict(sc.triangulation, facts) == X.ACCEPTED
    assert program([(sc.triangulation, facts)]) == [(X.ACCEPTED, 0, "")]


def test_an_empty_array_and_a_scene_without_materials(program):
    sc = R.scene("cornell")
    none = X.Facts(np.zeros(0, np.uint8))
    got = program([(sc.triangulation[:0], X.Facts.of(sc)), (sc.triangulation[:3], none)])
    assert got[0] == (X.ACCEPTED, 0, "")
    assert got[1] == ((0 << 4) | X.MATERIAL, X.BAD_SCENE, X.message(X.MATERIAL))
    assert X.verdict(sc.triangulation[:3], none) == X.MATERIAL


# ---------------------------------------------------------------------------------------------- the other callers of the classification

def with_triangles(sc, tris):
    import copy
    out = copy.copy(sc)
    out.triangulation = tris
    return out


@pytest.mark.parametrize("base", BASES)
def test_validate_scene_and_build_layout_say_what_they_said(built, base):
    """Codes 1 and 2 are build_layout's refusals (ptmi_validate_scene: BAD_SCENE, the words alone); codes 3 to 5 are the scene's
    ptmi_literal_kernel_reason, which the serial model reports for a layout that is to be updated (UNSUPPORTED, the words alone);
    what only an update refuses passes both."""
    model = R.model()
    if model is None:
        pytest.fail("oracle/build/libscene_refit_model.so not built (make -C oracle probe)", pytrace=False)
    sc = R.scene(base)
    facts = X.Facts.of(sc)
    at = [len(sc.triangulation) // 2]
    reached = set()
    for case in X.CASES:
        if case.targets != 1:
            continue
        code = case.expected(facts)
        moved = with_triangles(sc, case.apply(sc.triangulation, at, facts))
        words = f"triangle {at[0]} {X.WORDS[code]}" if code else ""
        if code in (X.MATERIAL, X.TEXCOORD):
            with pytest.raises(PtmiError) as e:
                backend.validate_scene(moved, R.W, R.H, 4)
            assert e.value.code == X.BAD_SCENE and str(e.value).endswith(words) and words in str(e.value), str(e.value)
        else:
            backend.validate_scene(moved, R.W, R.H, 4)
        cfg = backend.Config(C.sizeof(backend.Config), 0, R.W, R.H, 4, sc.lightsSize, S.JITTERED, 0, 0)
        d, keep = backend.scene_desc(moved)
        rc = C.c_int(0)
        h = model.m.model_layout(C.addressof(cfg), C.addressof(d), C.byref(rc))
        if h:
            model.free(h)
        if code in (X.MATERIAL, X.TEXCOORD):
            assert (rc.value, model.m.model_error().decode()) == (X.BAD_SCENE, words), case.name
        elif code in (X.VERTEX, X.NORMAL, X.NO_AREA):
            assert (rc.value, model.m.model_error().decode()) == (X.UNSUPPORTED, words), case.name
        else:
            assert rc.value == 0 and h, (case.name, model.m.model_error())
        reached.add(code)
    assert reached >= {X.MATERIAL, X.VERTEX, X.NORMAL, X.NO_AREA} | ({X.TEXCOORD} if base == "feat_textured" else set())
