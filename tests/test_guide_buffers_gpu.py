"""ptmi_render_guides / ptmi_render_guides_device against the yardstick of guide_cases.py: every word of every plane equal
(compared as uint32; where the yardstick's word is a NaN the kernel's must be a NaN), in both arithmetics and for both samplers,
on the image shapes and scenes that take each path of the kernel; and what the feature promises around the kernel - guide calls
change nothing that was rendered, they follow ptmi_set_camera and ptmi_update_triangles, errors leave the context rendering as
before.  An iteration of a (scene, sampler, arithmetic) is traced once by the yardstick and shared."""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, bvh_create, scenes, structs as S
from gpu_cases import assert_same_state, state
import gpu_cases
import guide_cases as G
import scene_update_cases as U

pytestmark = pytest.mark.gpu
W, H = G.W, G.H
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
ARITHMETICS = pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])
SAMPLERS = pytest.mark.parametrize("sampler", [S.JITTERED, S.UNIFORM], ids=["jittered", "uniform"])


def context(sc, width=W, height=H, **kw):
    return gpu_cases.context(sc, width, height, **kw)


def assert_equal(got, want, excluded=None):
    msg = G.describe_difference(got, want, excluded)
    assert not msg, msg


def check_calls(be, y, calls, planes=G.PLANES):
    for first, n in calls:
        want, excluded = y.planes(first, n)
        got = be.render_guides(first, n, planes=planes)
        assert set(got) == set(planes)
        assert_equal(got, want, excluded)


# ---------------------------------------------------------------------------------------------- the kernel against the yardstick

@ARITHMETICS
@SAMPLERS
def test_iteration_ranges_on_cornell(flags, sampler):
    """(0, 1), (0, 3), (7, 2): the ids are those of the call's first iteration, the sums add in iteration order."""
    y = G.yardstick("cornell", sampler, flags == DA)
    ids0, ids7 = y.iteration(0)["ids"], y.iteration(7)["ids"]
    three, _ = y.planes(0, 3)
    assert sampler == S.UNIFORM or not np.array_equal(ids0, ids7)  # (the two first iterations do see other triangles)
    assert three["hit_count"].max() == 3 and three["hit_count"].min() == 0 and not np.array_equal(three["albedo"], y.planes(0, 1)[0]["albedo"])
    be = context(G.scene("cornell"), flags=flags, sampler=sampler)
    try:
        check_calls(be, y, G.CORNELL_CALLS)
    finally:
        be.release()


_shaped = {}


@pytest.mark.parametrize("shape", [(1, 1), (8, 8), (9, 7), (37, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_shapes(shape):
    """One pixel, one full wave, and tails in both axes with a partial workgroup."""
    w, h = shape
    if shape not in _shaped:
        sc = bvh_create(scenes.cornell_box(w, h))
        _shaped[shape] = (sc, G.Yardstick(sc, w, h))
    sc, y = _shaped[shape]
    be = context(sc, width=w, height=h)
    try:
        want, excluded = y.planes(3, 2)
        got = be.render_guides(3, 2)
        assert got["albedo"].shape == (h, w, 4) and got["hit_count"].shape == (h, w) and got["ids"].dtype == np.uint32
        assert_equal(got, want, excluded)
        assert want["hit_count"].sum() > 0
    finally:
        be.release()


@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_stride_loop(blocks, monkeypatch):
    """48 tiles on one and on two workgroups of four waves."""
    monkeypatch.setenv("PTMI_GUIDE_MAX_BLOCKS", str(blocks))
    be = context(G.scene("cornell"))
    try:
        check_calls(be, G.yardstick("cornell"), [(0, 3)])
    finally:
        be.release()


@ARITHMETICS
@pytest.mark.parametrize("name", G.SCENES)
def test_scenes(name, flags):
    """A single leaf, a big leaf, empty leaves, a stack deeper than 22 levels, textures, two-sided triangles, every material,
    and records that yield NaN distances.  (strict with the JITTERED sampler, default with the UNIFORM one)"""
    sampler = S.UNIFORM if flags == DA else S.JITTERED
    y = G.yardstick(name, sampler, flags == DA)
    be = context(G.scene(name), flags=flags, sampler=sampler)
    try:
        if name == "hostile":
            assert be.literal_kernel_reason()
        check_calls(be, y, G.calls_of(name))
    finally:
        be.release()


@ARITHMETICS
def test_records_that_are_not_precomputed(flags, monkeypatch):
    """PTMI_GENERIC_TRIANGLES uploads the plain DTri records: the other instantiation of the kernel."""
    monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    be = context(G.scene("tris20k"), flags=flags)
    try:
        check_calls(be, G.yardstick("tris20k", S.JITTERED, flags == DA), G.calls_of("tris20k"))
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- planes

def test_a_subset_of_planes():
    be = context(G.scene("cornell"))
    try:
        y = G.yardstick("cornell")
        check_calls(be, y, [(7, 2)], planes=("ids",))
        check_calls(be, y, [(0, 3)], planes=("albedo", "hit_count"))  # (a larger request: the scratch grows)
        check_calls(be, y, [(7, 2)], planes=("position",))
        check_calls(be, y, [(0, 1)])
        # a plane that is not asked for is not written
        tensors = device_planes()
        be.render_guides_device(0, 3, albedo=tensors["albedo"].data_ptr(), hit_count=tensors["hit_count"].data_ptr())
        be.synchronize()
        got = from_device(tensors)
        want, excluded = y.planes(0, 3)
        assert_equal({k: got[k] for k in ("albedo", "hit_count")}, want, excluded)
        for name in ("normal", "position", "ids"):
            assert sentinel_intact(got[name]), name
    finally:
        be.release()


def device_planes(w=W, h=H):
    """torch tensors of the five planes, filled with a sentinel (-1.0; ids: 0xFFFFFFFF)"""
    import torch
    t = {name: torch.full((h, w) if name == "hit_count" else (h, w, 4), -1, dtype=torch.int32 if name == "ids" else torch.float32, device="cuda")
         for name in G.PLANES}
    torch.cuda.synchronize()
    return t


def from_device(tensors):
    return {name: (t.cpu().numpy().view(np.uint32) if name == "ids" else t.cpu().numpy()) for name, t in tensors.items()}


def sentinel_intact(a):
    return bool((a == (0xFFFFFFFF if a.dtype == np.uint32 else -1.0)).all())


def pointers(tensors):
    return {name: t.data_ptr() for name, t in tensors.items()}


def test_device_pointers_equal_host_planes():
    import torch
    be = context(G.scene("cornell"))
    try:
        want, excluded = G.yardstick("cornell").planes(0, 3)
        host = be.render_guides(0, 3)
        assert_equal(host, want, excluded)
        tensors = device_planes()
        be.render_guides_device(0, 3, **pointers(tensors))  # the context's own stream
        be.synchronize()
        assert_equal(from_device(tensors), host)
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        be.set_stream(stream.cuda_stream)
        again = device_planes()
        be.render_guides_device(0, 3, **pointers(again))
        with torch.cuda.stream(stream):
            on_stream = {name: t.clone() for name, t in again.items()}  # torch ops ordered behind the call on the caller's stream
        stream.synchronize()
        assert_equal(from_device(on_stream), host)
        assert_equal(be.render_guides(0, 3), host)  # host planes on the caller's stream
        be.set_stream(None)
    finally:
        be.release()


def test_a_page_locked_plane_is_filled_in_place():
    be = context(G.scene("cornell"))
    try:
        want, excluded = G.yardstick("cornell").planes(7, 2)
        out = {"normal": np.full((H, W, 4), -1.0, np.float32), "ids": np.full((H, W, 4), 7, np.uint32)}
        be.pin_host_buffer(out["normal"])  # (one plane page-locked, the other through the context's landing buffer)
        got = be.render_guides(7, 2, planes=("normal", "ids"), out=out)
        assert got["normal"] is out["normal"] and got["ids"] is out["ids"]
        assert_equal(out, want, excluded)
        be.unpin_host_buffer(out["normal"])
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- guides and renders

def test_guides_are_invisible_to_renders():
    sc, y = G.scene("cornell"), G.yardstick("cornell")

    def play(with_guides):
        be = context(sc)
        try:
            be.render(0, 2)
            if with_guides:
                check_calls(be, y, [(0, 3)])
            be.render(2, 2)
            if with_guides:
                check_calls(be, y, [(7, 2)], planes=("ids", "hit_count"))
            for k in range(4, 12):  # one-iteration calls of a caller that waits: rendered ahead of
                be.render(k, 1)
                be.synchronize()
                if with_guides:
                    check_calls(be, y, [(0, 1)], planes=("albedo",))
            return state(be)
        finally:
            be.release()

    assert_same_state(play(True), play(False))


def test_guides_leave_the_scheduler_statistics():
    be = context(G.scene("cornell"), flags=backend.FLAG_SCHEDULER_STATS)
    try:
        be.render(0, 2)
        before, checks = be.scheduler_stats(), be.invariant_checks()
        assert before["trips_node"] > 0
        check_calls(be, G.yardstick("cornell"), [(0, 3)])
        assert be.scheduler_stats() == before and be.invariant_checks() == checks
    finally:
        be.release()


def test_guides_follow_set_camera():
    """... to the far side of feat_two_sided's sheet, where the negative sides and their materials show."""
    moved = G.scene("feat_two_sided_from_behind")
    first, n = G.SCENE_CALL
    be = context(G.scene("feat_two_sided"))
    try:
        check_calls(be, G.yardstick("feat_two_sided"), [(first, n)])
        be.render(0, 2)
        be.set_camera(moved.cameraPosition, moved.cameraDirection, moved.cameraRight, moved.cameraUp)
        want, excluded = G.yardstick("feat_two_sided_from_behind").planes(first, n)
        assert set(np.unique(want["ids"][..., 2])) == {0, 1}
        assert_equal(be.render_guides(first, n), want, excluded)
    finally:
        be.release()


def test_guides_follow_update_triangles():
    sc = G.scene("cornell")
    tris = U.displaced(sc.triangulation, 7)
    moved = U.moved_scene(sc, tris)
    y, y_moved = G.yardstick("cornell"), G.Yardstick(moved, W, H)
    want, _ = y.planes(0, 1)
    want_moved, excluded = y_moved.planes(0, 1)
    assert not np.array_equal(want["position"], want_moved["position"])  # (the triangles did move)
    be = context(sc)
    try:
        before, after = device_planes(), device_planes()
        be.render_guides_device(0, 1, **pointers(before))  # not waited for: the update must
        be.update_triangles(tris)
        be.render_guides_device(0, 1, **pointers(after))
        be.synchronize()
        assert_equal(from_device(before), want)
        assert_equal(from_device(after), want_moved, excluded)  # triangle_id still indexes the array the caller uploaded
        assert_equal(be.render_guides(0, 1), want_moved, excluded)
    finally:
        be.release()


def test_two_listed_devices_answer_like_one():
    be = context(G.scene("cornell"), devices=[0, 0])
    try:
        be.render(0, 3)
        check_calls(be, G.yardstick("cornell"), [(0, 3), (7, 2)])
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- errors

def test_errors_leave_the_context_rendering():
    sc = G.scene("cornell")
    lib = backend.load_library()
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        with pytest.raises(PtmiError) as e:
            be.render_guides(0, 1)
        assert e.value.code == STATE and "before ptmi_initialize_memory" in str(e.value)
        with pytest.raises(PtmiError) as e:
            be.render_guides_device(0, 1, albedo=256)
        assert e.value.code == STATE
        be.initialize_memory(sc)
        be.render(0, 3)
        baseline = state(be)

        def refused(rc):
            assert rc == INVALID_ARGUMENT and len(lib.ptmi_last_error(be._ctx)) > 0
            be.clear()
            be.render(0, 3)
            assert_same_state(state(be), baseline)

        tensors = device_planes()
        good = backend.Guides(C.sizeof(backend.Guides), 0, **pointers(tensors))
        wrong_size = backend.Guides(C.sizeof(backend.Guides) + 8, 0, **pointers(tensors))
        misaligned = backend.Guides(C.sizeof(backend.Guides), 0, **dict(pointers(tensors), hit_count=tensors["hit_count"].data_ptr() + 4))
        host = {name: be.guide_plane(name) for name in G.PLANES}
        host_wrong_size = backend.Guides(4, 0, **{name: a.ctypes.data for name, a in host.items()})
        refused(lib.ptmi_render_guides(be._ctx, 0, 1, None))
        refused(lib.ptmi_render_guides_device(be._ctx, 0, 1, None))
        refused(lib.ptmi_render_guides(be._ctx, 0, 1, C.byref(host_wrong_size)))
        refused(lib.ptmi_render_guides_device(be._ctx, 0, 1, C.byref(wrong_size)))
        refused(lib.ptmi_render_guides_device(be._ctx, 0, 1, C.byref(misaligned)))
        assert all(sentinel_intact(a) for a in from_device(tensors).values())  # nothing was launched
        nothing = backend.Guides(C.sizeof(backend.Guides), 0)
        assert lib.ptmi_render_guides_device(be._ctx, 0, 0, C.byref(good)) == 0 and lib.ptmi_render_guides(be._ctx, 5, 0, C.byref(nothing)) == 0
        assert lib.ptmi_render_guides_device(be._ctx, 0, 4, C.byref(nothing)) == 0 and lib.ptmi_render_guides(be._ctx, 0, 4, C.byref(nothing)) == 0
        be.synchronize()
        assert all(sentinel_intact(a) for a in from_device(tensors).values())
        check_calls(be, G.yardstick("cornell"), [(0, 1)])  # ... and a good call still works
        be.clear()
        be.render(0, 3)
        assert_same_state(state(be), baseline)
    finally:
        be.release()


def test_the_random_sampler_is_refused():
    sc = G.scene("cornell")
    be = context(sc, sampler=S.RANDOM)
    try:
        be.render(0, 2)
        baseline = state(be)
        with pytest.raises(PtmiError) as e:
            be.render_guides(0, 1)
        assert e.value.code == UNSUPPORTED and "RANDOM" in str(e.value)
        tensors = device_planes()
        with pytest.raises(PtmiError) as e:
            be.render_guides_device(0, 1, **pointers(tensors))
        assert e.value.code == UNSUPPORTED
        assert all(sentinel_intact(a) for a in from_device(tensors).values())
        assert_same_state(state(be), baseline)
    finally:
        be.release()
