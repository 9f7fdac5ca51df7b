"""ptmi_reproject_device / ptmi_set_camera_reprojected against the yardstick of reproject_cases.py, every word of both result
planes equal: synthetic planes on the image sizes that take each edge of the kernel's tiles and its grid-stride loop, under
every previous camera of the list; the host form on rendered scenes against a twin context that makes the separate calls; and
what the feature promises around the kernel - only the camera and the accumulators change, the device form changes nothing, it
is ordered on the context's stream, refusals leave the context as it was - and that carrying the image along beats clearing it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, scenes, structs as S
from gpu_cases import assert_same_state, state
import gpu_cases
import guide_cases as G
import reproject_cases as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = G.W, G.H
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
PLANES = ("normal", "position", "hit_count")
PARAMS = dict(position_tolerance=0.03, normal_tolerance=0.4, max_history=6.0)  # (a cap below the counts the tests carry)


def assert_equal(got, want):
    msg = R.describe_difference(got, want)
    assert not msg, msg


to_device = gpu_cases.tensor_on_device


def empty_result(w, h):
    import torch
    out = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda"), torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return out


def device_guides(be, first, n, w=W, h=H):
    """the three planes the reprojection reads, rendered into tensors by ptmi_render_guides_device (not waited for)"""
    import torch
    t = {name: torch.empty((h, w) if name == "hit_count" else (h, w, 4), dtype=torch.float32, device="cuda") for name in PLANES}
    torch.cuda.synchronize()
    be.render_guides_device(first, n, **{name: x.data_ptr() for name, x in t.items()})
    return t


def pointers(tensors):
    return {name: tensors[name].data_ptr() for name in PLANES}


def camera_of(sc):
    return tuple(np.asarray(v, np.float32) for v in (sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp))


def orbited(sc, degrees=R.ORBIT_DEGREES, distance=None):
    """the scene's camera turned about the Cornell box's centre, or about the point `distance` ahead of it"""
    cam = camera_of(sc)
    d = cam[1][:3].astype(np.float64)
    centre = np.full(3, 277.5) if distance is None else cam[0][:3] + d / np.linalg.norm(d) * distance
    return scenes.orbit_camera(cam, centre, degrees)


def results(tensors):
    return tensors[0].cpu().numpy(), tensors[1].cpu().numpy()


# ---------------------------------------------------------------------------------------------- the kernel against the yardstick

SIZES = [(1, 1), (5, 3), (33, 9), (70, 37), (130, 66)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_cases(size):
    """One pixel; less than a tile; a ragged row of tiles; several tiles each way with ragged edges; more than one workgroup's
    four tiles per row.  Every previous camera of the list; by contract no word of the result is a NaN."""
    w, h = size
    be = gpu_cases.context(G.scene("one_triangle"), w, h)
    try:
        for name in R.CAMERAS:
            prev_cam, previous, current = R.case(w, h, name)
            want = R.reproject(prev_cam, previous, current, **R.synthetic_params(w, h))
            p, c = {k: to_device(a) for k, a in previous.items()}, {k: to_device(a) for k, a in current.items()}
            out = empty_result(w, h)
            be.reproject_device(out[0].data_ptr(), out[1].data_ptr(), prev_cam, pointers(p), p["color"].data_ptr(), p["ray_nb"].data_ptr(),
                                pointers(c), **R.synthetic_params(w, h))
            be.synchronize()
            got = results(out)
            assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
            assert_equal(got, want)
            if w * h >= 15:
                assert (want[1] > 0).any() == (name != "behind")
    finally:
        be.release()


def test_more_tiles_than_the_grid_holds():
    """1000 x 530 is 125 x 67 = 8375 tiles, more than the 8192 waves of the largest grid: the grid-stride loop comes round."""
    w, h = 1000, 530
    be = gpu_cases.context(G.scene("one_triangle"), w, h)
    try:
        prev_cam, previous, current = R.case(w, h, "pan_fraction")
        params = R.synthetic_params(w, h)
        want = R.reproject(prev_cam, previous, current, **params)
        p, c = {k: to_device(a) for k, a in previous.items()}, {k: to_device(a) for k, a in current.items()}
        out = empty_result(w, h)
        be.reproject_device(out[0].data_ptr(), out[1].data_ptr(), prev_cam, pointers(p), p["color"].data_ptr(), p["ray_nb"].data_ptr(), pointers(c), **params)
        be.synchronize()
        assert (want[1] > 0).mean() > 0.5
        assert_equal(results(out), want)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- the host form against a twin

def separate_calls(twin, new_camera, first, n, **params):
    """What ptmi_set_camera_reprojected does, by the calls a caller has without it; the yardstick in place of the kernel.  Leaves
    the twin under the new camera with its image untouched."""
    old_camera = twin.camera
    color, count = twin.read_image()
    previous = twin.render_guides(first, n, planes=PLANES)
    twin.set_camera(*new_camera)
    twin.camera = new_camera
    current = twin.render_guides(first, n, planes=PLANES)
    return R.reproject(old_camera, dict(previous, color=color, ray_nb=count), current, **params)


def context_at(sc, camera=None, **kw):
    be = gpu_cases.context(sc, W, H, **kw)
    be.camera = camera_of(sc)
    if camera is not None:
        be.set_camera(*camera)
        be.camera = camera
    return be


@pytest.mark.parametrize("sampler", [S.JITTERED, S.UNIFORM], ids=["jittered", "uniform"])
@pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])
@pytest.mark.parametrize("name", ["cornell", "feat_textured"])
def test_host_form_equals_the_separate_calls(name, flags, sampler):
    sc = G.scene(name)
    moved = orbited(sc) if name == "cornell" else orbited(sc, 3.0, 8.0)
    be, twin = context_at(sc, flags=flags, sampler=sampler), context_at(sc, flags=flags, sampler=sampler)
    try:
        for b in (be, twin):
            b.render(0, 9)
        before = state(be)
        want = separate_calls(twin, moved, 2, 3, **PARAMS)
        assert (want[1] > 0).mean() > 0.3 and (want[1] == 0).any() and want[1].max() == PARAMS["max_history"]
        be.set_camera_reprojected(*moved, guide_first_iteration=2, guide_iterations=3, **PARAMS)
        after = state(be)
        assert_equal(be.read_image(), want)
        assert after["counters"] == before["counters"] and all(np.array_equal(x, y) for x, y in zip(after["stats"], before["stats"]))
        # a render adds on top exactly as after set_camera + write_image
        twin.write_image(*want)
        for b in (be, twin):
            b.render(9, 2)
        assert_same_state(state(be), state(twin))
        # ... and a second move, from scratch that exists now, with every default
        home = camera_of(sc)
        want = separate_calls(twin, home, 0, 1, **backend.REPROJECT_DEFAULTS)
        be.set_camera_reprojected(*home)
        assert_equal(be.read_image(), want)
    finally:
        be.release()
        twin.release()


@pytest.mark.parametrize("size", [(5, 3), (33, 9), (31, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_form_at_pixel_counts_that_are_no_multiple_of_four(size):
    """15, 297 and 217 pixels (1, 3 and 1 over a multiple of 4): the planes of the host form's scratch lie behind one another and
    each must start 16-byte aligned all the same.  Held against the twin's separate calls, as at 64 x 48, twice (the second move
    from scratch that exists)."""
    w, h = size
    sc = gpu_cases.cached_scene("cornell", w, h)
    cam = camera_of(sc)
    moved = scenes.orbit_camera(cam, np.full(3, 277.5), R.ORBIT_DEGREES)
    params = dict(position_tolerance=0.5, normal_tolerance=0.4, max_history=6.0)  # (a pixel is a fifth of the distance wide at 5 x 3)
    be, twin = gpu_cases.context(sc, w, h), gpu_cases.context(sc, w, h)
    try:
        be.camera = twin.camera = cam
        for b in (be, twin):
            b.render(0, 9)
        for camera in (moved, cam):
            want = separate_calls(twin, camera, 1, 2, **params)
            assert (want[1] > 0).any()
            be.set_camera_reprojected(*camera, guide_first_iteration=1, guide_iterations=2, **params)
            assert_equal(be.read_image(), want)
            twin.write_image(*want)
            for b in (be, twin):
                b.render(9, 1)
            assert_same_state(state(be), state(twin))
    finally:
        be.release()
        twin.release()


def test_host_form_leaves_scheduler_statistics_and_snapshots():
    sc = G.scene("cornell")
    be = context_at(sc, flags=backend.FLAG_SCHEDULER_STATS)
    try:
        be.render(0, 3)
        be.snapshot(5)
        be.render(3, 1)
        kept = [a.view(np.uint32).copy() for a in be.read_snapshot(5)]
        stats, checks, counters = be.scheduler_stats(), be.invariant_checks(), be.counters()
        assert stats["trips_node"] > 0
        be.set_camera_reprojected(*orbited(sc), **PARAMS)
        assert be.scheduler_stats() == stats and be.invariant_checks() == checks and be.counters() == counters
        assert all(np.array_equal(x, y.view(np.uint32)) for x, y in zip(kept, be.read_snapshot(5)))
    finally:
        be.release()


def test_two_listed_devices():
    """The shares are summed before the move; afterwards devices[0] holds the result and the second device's share is zero: the
    image read back - the sum of both - is the yardstick's, counts included, and what a single-device context makes of the same
    image.  A share by itself cannot be read through the public API (ptmi_device_accumulators and ptmi_bind_accumulators refuse
    a multi-device context, every readback sums), so WHICH device holds the result is not observable here, nor to any caller:
    x + 0 and 0 + x are the same words.  What is held is that the shares together are the result - a share left as it was would
    show in the counts, which were 8 before the call - now and after four more iterations on both devices."""
    sc = G.scene("cornell")
    moved = orbited(sc)
    be, twin = context_at(sc, devices=[0, 0]), context_at(sc, devices=[0, 0])
    single = context_at(sc)
    try:
        for b in (be, twin):
            b.render(0, 8)
        single.write_image(*twin.read_image())  # (the sum of the shares, which a single device's own 8 iterations equal to rounding only)
        want = separate_calls(twin, moved, 0, 2, **PARAMS)
        be.set_camera_reprojected(*moved, guide_iterations=2, **PARAMS)
        single.set_camera_reprojected(*moved, guide_iterations=2, **PARAMS)
        assert_equal(be.read_image(), want)
        assert_equal(single.read_image(), want)
        twin.write_image(*want)
        for b in (be, twin):
            b.render(8, 4)
        assert_same_state(state(be), state(twin))
    finally:
        be.release()
        twin.release()
        single.release()


def test_bound_accumulators_are_written_in_place():
    import torch
    sc = G.scene("cornell")
    moved = orbited(sc)
    be, twin = context_at(sc), context_at(sc)
    try:
        color = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        count = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        be.bind_accumulators(color.data_ptr(), count.data_ptr())
        for b in (be, twin):
            b.render(0, 7)
        want = separate_calls(twin, moved, 0, 1, **PARAMS)
        be.set_camera_reprojected(*moved, **PARAMS)
        assert_equal((color.cpu().numpy(), count.cpu().numpy()), want)
        assert_equal(be.read_image(), want)
    finally:
        be.release()
        twin.release()


# ---------------------------------------------------------------------------------------------- the device form and renders

def test_device_form_is_invisible_to_renders():
    sc = G.scene("cornell")

    def play(with_reprojection):
        be = context_at(sc)
        try:
            be.render(0, 2)
            be.snapshot(5)
            guides, out = device_guides(be, 0, 2), empty_result(W, H)
            image = [to_device(a) for a in be.read_image()]
            be.render(2, 2)
            for k in range(4, 12):  # one-iteration calls of a caller that waits: rendered ahead of
                be.render(k, 1)
                be.synchronize()
                if with_reprojection:
                    be.reproject_device(out[0].data_ptr(), out[1].data_ptr(), be.camera, pointers(guides), image[0].data_ptr(),
                                        image[1].data_ptr(), pointers(guides), **PARAMS)
            kept = be.read_snapshot(5)
            return state(be), [a.view(np.uint32).copy() for a in kept]
        finally:
            be.release()

    (a, kept_a), (b, kept_b) = play(True), play(False)
    assert_same_state(a, b)
    assert all(np.array_equal(x, y) for x, y in zip(kept_a, kept_b)) and kept_a[1].view(np.float32).max() == 2


def test_a_call_in_flight_is_ordered_before_set_camera():
    """Guides of the old camera and a reprojection from them, not waited for; ptmi_set_camera; guides of the new one and the
    reprojection between the two.  The reprojection reads no scene record, so its own order against ptmi_set_camera cannot be
    seen from outside: what this holds is the guide launch in flight, which must see the old camera, and that the reprojection
    queued behind it on the same stream reads the planes that launch wrote."""
    sc = G.scene("cornell")
    moved = orbited(sc)
    be = context_at(sc)
    try:
        be.render(0, 5)
        color, count = be.read_image()
        image = [to_device(color), to_device(count)]
        old = be.render_guides(5, 2, planes=PLANES)
        want_old = R.reproject(be.camera, dict(old, color=color, ray_nb=count), old, **PARAMS)
        out_old, out_new = empty_result(W, H), empty_result(W, H)
        guides_old = device_guides(be, 5, 2)
        be.reproject_device(out_old[0].data_ptr(), out_old[1].data_ptr(), be.camera, pointers(guides_old), image[0].data_ptr(),
                            image[1].data_ptr(), pointers(guides_old), **PARAMS)  # not waited for: set_camera must
        be.set_camera(*moved)
        guides_new = device_guides(be, 5, 2)
        be.reproject_device(out_new[0].data_ptr(), out_new[1].data_ptr(), be.camera, pointers(guides_old), image[0].data_ptr(),
                            image[1].data_ptr(), pointers(guides_new), **PARAMS)
        be.synchronize()
        new = be.render_guides(5, 2, planes=PLANES)
        want_new = R.reproject(be.camera, dict(old, color=color, ray_nb=count), new, **PARAMS)
        assert not np.array_equal(want_old[1], want_new[1])
        assert_equal(results(out_old), want_old)
        assert_equal(results(out_new), want_new)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- errors

def test_refusals_leave_camera_and_accumulators():
    sc = G.scene("cornell")
    moved = orbited(sc)
    lib = backend.load_library()
    vp = C.c_void_p
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    twin = context_at(sc)
    try:
        with pytest.raises(PtmiError) as e:
            be.set_camera_reprojected(*moved)
        assert e.value.code == STATE and "before ptmi_initialize_memory" in str(e.value)
        with pytest.raises(PtmiError) as e:
            be.reproject_device(256, 256, moved, dict(normal=256, position=256, hit_count=256), 256, 256, dict(normal=256, position=256, hit_count=256))
        assert e.value.code == STATE
        be.initialize_memory(sc)
        be.camera = camera_of(sc)
        for b in (be, twin):
            b.render(0, 3)
        guides, out = device_guides(be, 0, 1), empty_result(W, H)
        be.synchronize()
        image = [to_device(a) for a in be.read_image()]

        def params(**changes):
            p = backend.Backend.reproject_params(**PARAMS)
            for k, v in changes.items():
                setattr(p, k, v)
            return p

        bad_params = [None, params(struct_size=28), params(struct_size=36), params(flags=1), params(flags=0x80000000), params(reserved=1)]
        for name in ("position_tolerance", "normal_tolerance"):
            bad_params += [params(**{name: v}) for v in (0.0, -1.0, float("inf"), float("nan"))]
        bad_params += [params(max_history=v) for v in (float("nan"), 0.5, 0.0, -2.0, float("-inf"))]
        cam = (backend.Float4 * 4)(*[backend._f4(v) for v in be.camera])
        new = [backend._f4(v) for v in moved]
        good_guides = backend.Guides(C.sizeof(backend.Guides), 0, **pointers(guides))

        def device_call(p=None, camera=cam, previous=good_guides, color=None, count=None, current=good_guides, out_color=None, out_count=None):
            p = params() if p is None else p
            byref = lambda x: None if x is None else C.byref(x)  # noqa: E731
            return lib.ptmi_reproject_device(be._ctx, byref(p), byref(camera), byref(previous), vp(image[0].data_ptr() if color is None else color),
                                             vp(image[1].data_ptr() if count is None else count), byref(current),
                                             vp(out[0].data_ptr() if out_color is None else out_color),
                                             vp(out[1].data_ptr() if out_count is None else out_count))

        def host_call(p, camera=new):
            return lib.ptmi_set_camera_reprojected(be._ctx, *[None if x is None else C.byref(x) for x in camera], None if p is None else C.byref(p))

        attempts = []
        for p in bad_params:
            attempts.append(lambda p=p: host_call(p))
            attempts.append(lambda p=p: lib.ptmi_reproject_device(be._ctx, None if p is None else C.byref(p), C.byref(cam), C.byref(good_guides),
                                                                  vp(image[0].data_ptr()), vp(image[1].data_ptr()), C.byref(good_guides),
                                                                  vp(out[0].data_ptr()), vp(out[1].data_ptr())))
        attempts += [lambda v=v: host_call(params(guide_iterations=v)) for v in (0, 1 << 24)]
        attempts += [lambda i=i: host_call(params(), [None if k == i else x for k, x in enumerate(new)]) for i in range(4)]
        # the guides structs, their planes, the image planes and the result's: missing, misaligned
        wrong_size = backend.Guides(C.sizeof(backend.Guides) + 8, 0, **pointers(guides))
        for which in ("previous", "current"):
            attempts.append(lambda which=which: device_call(**{which: wrong_size}))
            for name in PLANES:
                without = backend.Guides(C.sizeof(backend.Guides), 0, **dict(pointers(guides), **{name: None}))
                shifted = backend.Guides(C.sizeof(backend.Guides), 0, **dict(pointers(guides), **{name: guides[name].data_ptr() + 4}))
                attempts.append(lambda which=which, g=without: device_call(**{which: g}))
                attempts.append(lambda which=which, g=shifted: device_call(**{which: g}))
        attempts.append(lambda: lib.ptmi_reproject_device(be._ctx, C.byref(params()), C.byref(cam), None, vp(image[0].data_ptr()), vp(image[1].data_ptr()),
                                                          C.byref(good_guides), vp(out[0].data_ptr()), vp(out[1].data_ptr())))
        attempts.append(lambda: lib.ptmi_reproject_device(be._ctx, C.byref(params()), None, C.byref(good_guides), vp(image[0].data_ptr()),
                                                          vp(image[1].data_ptr()), C.byref(good_guides), vp(out[0].data_ptr()), vp(out[1].data_ptr())))
        for key, tensor in (("color", image[0]), ("count", image[1]), ("out_color", out[0]), ("out_count", out[1])):
            attempts.append(lambda key=key, tensor=tensor: device_call(**{key: tensor.data_ptr() + 4}))
            attempts.append(lambda key=key: device_call(**{key: 0}))  # (NULL)
        # a previous camera that is not finite, or that spans no volume
        def camera_with(i, c, value):
            v = [np.array(x, np.float32) for x in be.camera]
            v[i][c] = value
            return (backend.Float4 * 4)(*[backend._f4(x) for x in v])

        for i in range(4):
            attempts.append(lambda i=i: device_call(camera=camera_with(i, i % 3, float("nan"))))
            attempts.append(lambda i=i: device_call(camera=camera_with(i, (i + 1) % 3, float("inf"))))
        flat = [np.array(x, np.float32) for x in be.camera]
        flat[3] = flat[2]  # up = right: det = 0
        attempts.append(lambda: device_call(camera=(backend.Float4 * 4)(*[backend._f4(x) for x in flat])))
        for attempt in attempts:
            assert attempt() == INVALID_ARGUMENT and len(lib.ptmi_last_error(be._ctx)) > 0
        # what ptmi_set_camera refuses
        far_away = [backend._f4(v) for v in moved]
        far_away[0].x = 1e30
        assert host_call(params(), far_away) == UNSUPPORTED and lib.ptmi_set_camera(be._ctx, *[C.byref(x) for x in far_away]) == UNSUPPORTED
        be.synchronize()
        assert bool((out[0] == -1).all()) and bool((out[1] == -1).all())  # nothing was launched
        for b in (be, twin):
            b.render(3, 1)
        assert_same_state(state(be), state(twin))
        # the w components of the previous camera, albedo and ids are ignored, and a good call still works
        with_more = backend.Guides(C.sizeof(backend.Guides), 0, **dict(pointers(guides), albedo=12, ids=12))
        assert device_call(camera=camera_with(0, 3, float("nan")), previous=with_more, current=with_more) == 0
        be.synchronize()
        color, count = be.read_image()
        planes = be.render_guides(0, 1, planes=PLANES)
        assert (count == 4).all()  # (the image the tensors hold is of 3 iterations)
        assert_equal(results(out), R.reproject(be.camera, dict(planes, color=image[0].cpu().numpy(), ray_nb=image[1].cpu().numpy()), planes, **PARAMS))
    finally:
        be.release()
        twin.release()


@pytest.mark.parametrize("kind", ["random", "super_sampling"])
def test_contexts_the_host_form_cannot_serve(kind):
    """(Two RANDOM contexts agree to rounding only - their samples land on other work-items' pixels, in any order - so there the
    refusal is held against the context's own state before it, and the camera against the twin's guides.)"""
    sc = G.scene("cornell")
    kw = dict(sampler=S.RANDOM) if kind == "random" else dict(super_sampling=True)
    be, twin = context_at(sc, **kw), context_at(sc, **kw)
    try:
        for b in (be, twin):
            b.render(0, 2)
        before = state(be, variance=kind != "random")
        with pytest.raises(PtmiError) as e:
            be.set_camera_reprojected(*orbited(sc))
        assert e.value.code == UNSUPPORTED and ("RANDOM" if kind == "random" else "super_sampling") in str(e.value)
        assert_same_state(state(be, variance=kind != "random"), before)
        for b in (be, twin):
            b.render(2, 1)
        a, b = state(be, variance=kind != "random"), state(twin, variance=kind != "random")
        if kind == "random":  # the camera is the old one: the same paths, hit for hit
            assert a["counters"] == b["counters"] and all(np.array_equal(x, y) for x, y in zip(a["stats"], b["stats"]))
            assert np.array_equal(a["count"], b["count"])
            assert np.allclose(a["color"].view(np.float32), b["color"].view(np.float32), rtol=1e-5, atol=1e-6)
        else:
            assert_same_state(a, b)
    finally:
        be.release()
        twin.release()


# ---------------------------------------------------------------------------------------------- it helps

BEFORE, AFTER, TRUTH_SPP = 16, 4, 1024
_quality = {}


def json_safe(x):
    """the record with an infinite cap written as the string "inf": strict JSON has no infinity"""
    if isinstance(x, dict):
        return {k: json_safe(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [json_safe(v) for v in x]
    return "inf" if isinstance(x, float) and x == float("inf") else x


def quality():
    """Cornell at 64 x 48: 16 iterations at camera A, then camera B = A orbited by R.ORBIT_DEGREES about the box's centre.  (i)
    clear + 4 iterations; (ii) set_camera_reprojected + the same 4 iterations, at every point of the committed grid and with the
    shipped defaults; both against 1024 further iterations at B.  Computed once, printed, and written to
    profiles/reproject_quality_cornell.json."""
    if _quality:
        return _quality
    sc = G.scene("cornell")
    a, b = camera_of(sc), orbited(sc)
    be = context_at(sc, camera=b)
    try:
        first = BEFORE + AFTER
        be.render(first, TRUTH_SPP)
        color, count = be.read_image()
        truth = color[..., :3] / count[..., None]
        be.clear()
        be.render(BEFORE, AFTER)
        color, count = be.read_image()
        cleared = color[..., :3] / count[..., None]
        be.set_camera(*a)
        be.clear()
        be.render(0, BEFORE)
        image_a = be.read_image()

        def carried(**params):
            be.set_camera(*a)
            be.write_image(*image_a)
            be.set_camera_reprojected(*b, guide_first_iteration=0, guide_iterations=AFTER, **params)
            kept = float((be.read_image()[1] > 0).mean())
            be.render(BEFORE, AFTER)
            color, count = be.read_image()
            return R.rmse(color[..., :3] / count[..., None], truth), kept

        grid = []
        for tp in R.GRID_POSITION_TOLERANCE:
            for tn in R.GRID_NORMAL_TOLERANCE:
                for cap in R.GRID_MAX_HISTORY:
                    rmse, kept = carried(position_tolerance=tp, normal_tolerance=tn, max_history=cap)
                    grid.append(dict(position_tolerance=tp, normal_tolerance=tn, max_history=cap, rmse=rmse, kept=kept))
        shipped, kept = carried()
    finally:
        be.release()
    _quality.update(scene="cornell", width=W, height=H, iterations_before=BEFORE, iterations_after=AFTER, truth_spp=TRUTH_SPP,
                    orbit_degrees=R.ORBIT_DEGREES, rmse_cleared=R.rmse(cleared, truth), rmse_reprojected=shipped,
                    ratio=shipped / R.rmse(cleared, truth), pixels_with_history=kept, defaults=backend.REPROJECT_DEFAULTS, grid=grid)
    print(json.dumps({k: v for k, v in _quality.items() if k != "grid"}))
    print("grid minimum:", min(grid, key=lambda r: r["rmse"]))
    with open(os.path.join(ROOT, "profiles", "reproject_quality_cornell.json"), "w") as f:
        json.dump(json_safe(_quality), f, indent=1, allow_nan=False)
        f.write("\n")
    return _quality


def test_it_beats_clearing():
    """After the move, 4 iterations on top of the reprojected image are closer to the truth than 4 iterations on a cleared one:
    what the caller had before this call existed."""
    q = quality()
    assert q["rmse_reprojected"] < q["rmse_cleared"], q


def test_defaults_are_the_grids_minimum():
    """... and the minimum is interior on every axis that has room to be: the grid is wide enough to have found it.  Measured on
    the MI355X (profiles/reproject_quality_cornell.json): RMSE 0.0850 cleared, 0.0325 reprojected.  Two axes SATURATE, and the
    test says so instead of calling their minimum interior: from some value on the test rejects nothing more, every looser grid
    point gives the same image (equal RMSE, equal share of pixels with history), and there is no room above.  That holds for the
    history cap from 16 on (there were 16 iterations to carry) and, in this box, for the position tolerance from 0.64 on.  The
    shipped value is the tightest point of the plateau; the point below it must be strictly worse, or the plateau would be the
    grid's fault."""
    q = quality()
    grid = q["grid"]
    best = min(grid, key=lambda r: r["rmse"])
    assert best["rmse"] < q["rmse_cleared"], (best, q["rmse_cleared"])
    assert q["rmse_reprojected"] == best["rmse"], (backend.REPROJECT_DEFAULTS, best)
    assert {k: best[k] for k in backend.REPROJECT_DEFAULTS} == backend.REPROJECT_DEFAULTS  # the tightest of equal minima, not any of them

    def along(axis):
        """the grid's points on the line through the minimum along `axis`, in the axis's order"""
        others = [k for k in backend.REPROJECT_DEFAULTS if k != axis]
        return [r for r in grid if all(r[k] == best[k] for k in others)]

    values = R.GRID_NORMAL_TOLERANCE
    assert values[0] < best["normal_tolerance"] < values[-1], best  # interior
    for axis, values in (("position_tolerance", R.GRID_POSITION_TOLERANCE), ("max_history", R.GRID_MAX_HISTORY)):
        line = along(axis)
        assert [r[axis] for r in line] == list(values)
        i = list(values).index(best[axis])
        assert 0 < i < len(values) - 1, (axis, best)  # (a plateau of one point would be an edge)
        assert all((r["rmse"], r["kept"]) == (best["rmse"], best["kept"]) for r in line[i:]), (axis, line[i:])  # saturated from here on
        assert line[i - 1]["rmse"] > best["rmse"], (axis, line[i - 1], best)
