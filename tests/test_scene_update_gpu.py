"""Updating a loaded scene in place: ptmi_set_camera and ptmi_update_triangles against a fresh upload.

The yardstick is always a SECOND context that was given the new scene through ptmi_initialize_memory - the new camera, or the new
triangles with ptmi_bvh_refit's tree - which is code that existed before the update calls did.  What the two contexts render must
be bit-equal: image, sample counts, the three histograms and ptmi_counters.  Refused updates must leave the old scene rendering
as before.
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, structs as S
from gpu_cases import assert_same_state as assert_same, cached_scene, state
import gpu_cases
import scene_update_cases as U

pytestmark = pytest.mark.gpu
W, H = 64, 48
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, BAD_SCENE, STATE, UNSUPPORTED = -1, -5, -6, -7


def scene(name):
    return cached_scene(name, W, H)


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, **kw)


moved_camera, _bad_triangles = U.moved_camera, U.bad_triangles  # (shared with the random call sequences: api_fuzz_cases.py)


def set_camera(be, sc):
    be.set_camera(sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp)


def rendered(sc, n=4, first=0, **kw):
    be = context(sc, **kw)
    try:
        be.render(first, n)
        return state(be, variance=kw.get("super_sampling", False))
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- camera

@pytest.mark.parametrize("sampler", [S.JITTERED, S.UNIFORM], ids=["jittered", "uniform"])
@pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])
@pytest.mark.parametrize("name", ["cornell", "matmix"])
def test_set_camera_equals_a_fresh_upload(name, flags, sampler):
    sc = scene(name)
    cam = moved_camera(sc)
    be = context(sc, flags=flags, sampler=sampler)
    try:
        be.render(0, 2)
        set_camera(be, cam)
        be.clear()
        be.render(0, 4)
        got = state(be)
    finally:
        be.release()
    want = rendered(cam, flags=flags, sampler=sampler)
    assert_same(got, want)
    assert not np.array_equal(want["color"], rendered(sc, flags=flags, sampler=sampler)["color"])  # (the camera did move)


@pytest.mark.parametrize("kw", [dict(flags=backend.FLAG_MEGAKERNEL), dict(super_sampling=True)], ids=["megakernel", "super_sampling"])
def test_set_camera_with_the_other_kernel_and_with_adaptive_sampling(kw):
    sc = scene("cornell")
    cam = moved_camera(sc)
    be = context(sc, **kw)
    try:
        be.render(0, 2)
        set_camera(be, cam)
        be.clear()
        be.render(0, 6)
        got = state(be, variance="super_sampling" in kw)
    finally:
        be.release()
    assert_same(got, rendered(cam, n=6, **kw))


# ---------------------------------------------------------------------------------------------- triangles

def moved_triangles(name, seed=7):
    sc = scene(name)
    return sc, U.moved_triangles(sc, name, seed)


UPDATE_CASES = {
    "cornell-strict": ("cornell", 0, 4, False),
    "cornell-default": ("cornell", DA, 4, False),
    "tris20k-precomputed": ("tris20k", 0, 5, False),
    "tris20k-precomputed-default": ("tris20k", DA, 5, False),
    "tris20k-generic": ("tris20k", 0, 5, True),
    "textured": ("feat_textured", 0, 4, False),
    "textured-default": ("feat_textured", DA, 4, False),
    "big_leaf": ("big_leaf", 0, 4, False),
    "empty_leaves": ("empty_leaves", 0, 4, False),
}


@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_update_triangles_equals_a_fresh_upload_of_the_refit_tree(case, monkeypatch):
    name, flags, depth, generic = UPDATE_CASES[case]
    if generic:
        monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    sc, tris = moved_triangles(name)
    be = context(sc, depth=depth, flags=flags)
    try:
        be.render(0, 2)
        info = be.update_triangles(tris)
        be.clear()
        be.render(0, 4)
        got = state(be)
    finally:
        be.release()
    want = rendered(U.moved_scene(sc, tris), depth=depth, flags=flags)
    assert_same(got, want)
    assert info["struct_size"] == 40 and info["levels"] == sc.bvhMaxDepth and info["total_ms"] > 0
    if name == "tris20k":
        assert 12 <= info["levels"] <= 20
    assert not np.array_equal(want["color"], rendered(sc, depth=depth, flags=flags)["color"])  # (the triangles did move)


def test_two_successive_updates_reuse_the_schedule():
    sc, tris1 = moved_triangles("tris20k", seed=1)
    tris2 = U.displaced(tris1, seed=2, amplitude=0.01)
    be = context(sc, depth=5)
    try:
        first = be.update_triangles(tris1)
        second = be.update_triangles(tris2)
        be.render(0, 4)
        got = state(be)
    finally:
        be.release()
    assert first["levels"] == second["levels"] > 0
    once = U.moved_scene(sc, tris1)
    assert_same(got, rendered(U.moved_scene(once, tris2), depth=5))


def test_update_with_unchanged_triangles_changes_nothing():
    sc = scene("cornell")
    be = context(sc)
    try:
        be.update_triangles(sc.triangulation)
        be.render(0, 4)
        got = state(be)
    finally:
        be.release()
    assert_same(got, rendered(sc))


def test_an_update_keeps_what_has_been_rendered():
    """4 iterations, update, 4 more WITHOUT a clear: accumulation over the motion."""
    sc, tris = moved_triangles("cornell")
    be = context(sc)
    try:
        be.render(0, 4)
        before = state(be)
        be.update_triangles(tris)
        assert_same(state(be), before)  # the update itself touched nothing that was rendered
        be.render(4, 4)
        got = state(be)
    finally:
        be.release()
    yard = context(U.moved_scene(sc, tris))
    try:
        yard.write_image(before["color"].view(np.float32), before["count"])
        yard.render(4, 4)
        want = state(yard)
    finally:
        yard.release()
    assert np.array_equal(got["color"], want["color"]) and np.array_equal(got["count"], want["count"])
    assert got["counters"] == {k: before["counters"][k] + want["counters"][k] for k in want["counters"]}
    for g, b, w in zip(got["stats"], before["stats"], want["stats"]):
        assert np.array_equal(g, b + w)


def test_set_camera_under_render_ahead(monkeypatch):
    """The blocking one-iteration-per-call caller that is rendered ahead of: what ran ahead for the old camera is dropped."""
    sc = scene("cornell")
    cam = moved_camera(sc)

    def play(ahead):
        monkeypatch.setenv("PTMI_RENDER_AHEAD", str(ahead))
        be = context(sc)
        try:
            for k in range(6):
                be.render(k, 1)
                be.synchronize()
            set_camera(be, cam)
            for k in range(6, 12):
                be.render(k, 1)
                be.synchronize()
            return state(be)
        finally:
            be.release()

    assert_same(play(2), play(0))


def test_update_triangles_under_render_ahead(monkeypatch):
    sc, tris = moved_triangles("cornell")

    def play(ahead):
        monkeypatch.setenv("PTMI_RENDER_AHEAD", str(ahead))
        be = context(sc)
        try:
            for k in range(6):
                be.render(k, 1)
                be.synchronize()
            be.update_triangles(tris)
            for k in range(6, 12):
                be.render(k, 1)
                be.synchronize()
            return state(be)
        finally:
            be.release()

    assert_same(play(2), play(0))


def test_two_listed_devices():
    sc, tris = moved_triangles("cornell")
    cam = moved_camera(sc)
    be = context(sc, devices=[0, 0])
    try:
        be.render(0, 3)
        set_camera(be, cam)
        be.clear()
        be.render(0, 5)
        got_camera = state(be)
        be.update_triangles(tris)
        be.clear()
        be.render(0, 5)
        got_both = state(be)
    finally:
        be.release()
    assert_same(got_camera, rendered(cam, n=5, devices=[0, 0]))
    assert_same(got_both, rendered(U.moved_scene(cam, tris), n=5, devices=[0, 0]))


# ---------------------------------------------------------------------------------------------- refusals

def test_refused_updates_leave_the_old_scene_rendering():
    sc = scene("cornell")
    be = context(sc)
    try:
        be.render(0, 3)
        baseline = state(be)

        def refused(call, code):
            with pytest.raises(PtmiError) as e:
                call()
            assert e.value.code == code, str(e.value)
            assert len(str(e.value).split(": ", 1)[1]) > 0
            be.clear()
            be.render(0, 3)
            assert_same(state(be), baseline)

        for kind, code in (("zero_area", UNSUPPORTED), ("nan_vertex", UNSUPPORTED), ("unequal_w", UNSUPPORTED), ("empty_aabb", UNSUPPORTED),
                           ("wrong_count", INVALID_ARGUMENT)):
            refused(lambda: be.update_triangles(_bad_triangles(sc, kind)), code)
        bad = moved_camera(sc)
        bad.cameraPosition = np.float32([np.inf, 0, 0, 1])
        refused(lambda: set_camera(be, bad), UNSUPPORTED)
        bad = moved_camera(sc)
        bad.cameraUp = np.float32([0, np.nan, 0, 0])
        refused(lambda: set_camera(be, bad), UNSUPPORTED)
        # ... and a good update still works after the refused ones
        _, tris = moved_triangles("cornell")
        be.update_triangles(tris)
        be.clear()
        be.render(0, 3)
        assert_same(state(be), rendered(U.moved_scene(sc, tris), n=3))
    finally:
        be.release()


def test_update_before_initialize_memory_is_a_state_error():
    sc = scene("cornell")
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        for call in (lambda: be.update_triangles(sc.triangulation), lambda: set_camera(be, sc)):
            with pytest.raises(PtmiError) as e:
                call()
            assert e.value.code == STATE and "before ptmi_initialize_memory" in str(e.value)
    finally:
        be.release()
