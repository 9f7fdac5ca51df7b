"""ptmi_render_region / ptmi_read_region on the GPU: a region call is ptmi_render with fewer work-items.

The yardsticks are code that existed before the region calls did: ptmi_render on a second context; the per-iteration planes
R_it of a fresh context (clear; render(it, 1); read_image), folded with numpy float32 adds; and ptmi_trace_paths along the
built-in camera's rays for per-path counts.  Image 43 x 29 (neither side a multiple of the 8 x 8 job tile), depth 4.

Where a scene's image holds NaNs (the zero-area triangles) the numpy fold asks for a NaN, of any sign and payload, where it
has one: which NaN an addition keeps is the adder's, not the renderer's.  Every comparison between two contexts is word for
word (gpu_cases.assert_same_state).
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, bvh_create, scenes, structs as S
from gpu_cases import assert_same_state, cached_scene, state
import gpu_cases
import path_query_cases as P
import scene_update_cases as U

pytestmark = pytest.mark.gpu
W, H, DEPTH = 43, 29, 4
DA = backend.FLAG_DEFAULT_ARITHMETIC
ARITHMETICS = [pytest.param(0, id="strict"), pytest.param(DA, id="default")]
WHOLE = (0, 0, W, H)
INNER = (13, 7, 17, 11)
REGIONS = [WHOLE, (0, 0, 1, 1), (42, 28, 1, 1), (5, 3, 8, 8), (8, 8, 16, 8), (37, 0, 6, 29), (0, 27, 43, 2), (3, 0, 1, 29), INNER]
QUARTERS = [(19, 11, 24, 18), (0, 0, 19, 11), (19, 0, 24, 11), (0, 11, 19, 18)]  # the image cut at (19, 11), scrambled
STRIPS = [(0, y, W, 1) for y in np.random.RandomState(3).permutation(H)]        # the 29 rows, scrambled
ERR_INVALID_ARGUMENT, ERR_STATE = -1, -6


def scene(name):
    if name == "cornell_za":  # records that yield NaN distances: the NANSAFE instantiation and redo_poisoned_kernel
        key = (name, W, H)
        if key not in gpu_cases._scenes:
            gpu_cases._scenes[key] = bvh_create(scenes.add_zero_area_triangles(scenes.build("cornell", W, H), 12))
        return gpu_cases._scenes[key]
    return cached_scene(name, W, H)


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, depth=DEPTH, **kw)


def rows(r):
    x, y, w, h = r
    return (slice(y, y + h), slice(x, x + w))


_planes = {}


def planes(name, flags, n):
    """R_0 .. R_{n-1} of scene `name`: what one iteration adds to a cleared image, float32[H, W, 4] each.  Computed once, read-only."""
    have = _planes.setdefault((name, flags), [])
    if len(have) < n:
        be = context(scene(name), flags=flags)
        try:
            for it in range(len(have), n):
                be.clear()
                be.render(it, 1)
                color, count = be.read_image()
                assert (count == 1).all()
                have.append(color.copy())
        finally:
            be.release()
    return have[:n]


def fold(color, count, planes_in_order, r):
    """color, count with the planes added inside region r, in order, in float32: what the calls must leave"""
    color, count = color.copy(), count.copy()
    with np.errstate(all="ignore"):
        for plane in planes_in_order:
            color[rows(r)] = color[rows(r)] + plane[rows(r)]
            count[rows(r)] = count[rows(r)] + np.float32(1)
    return color, count


def same_words(got, want):
    """word for word, except that a NaN of the yardstick asks for a NaN of any sign and payload"""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    both = np.isnan(g) & np.isnan(w)
    return np.array_equal(np.where(both, 0, g.view(np.uint32)), np.where(both, 0, w.view(np.uint32)))


def pattern():
    """finite, distinct per pixel and channel; counts distinct per pixel"""
    idx = np.arange(W * H, dtype=np.float32).reshape(H, W)
    color = np.stack([idx * 0.25 + 1, idx * 0.5 + 2, 3 - idx * 0.125, idx + 0.0625], axis=-1).astype(np.float32)
    return color, (idx + 1).astype(np.float32)


# ---- 1. inside equal, outside untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ARITHMETICS)
def test_inside_gains_the_iterations_and_outside_keeps_every_word(flags):
    """n = 1, 3: short launches on a stage set of their own; 5: one launch on the main stream; 33: two launches across the cap."""
    p_color, p_count = pattern()
    R = planes("cornell", flags, 33)
    be = context(scene("cornell"), flags=flags)
    try:
        for r in REGIONS:
            for n in (1, 3, 5, 33):
                be.write_image(p_color, p_count)
                be.render_region(*r, 0, n)
                color, count = be.read_image()
                want_color, want_count = fold(p_color, p_count, R[:n], r)
                outside = np.ones((H, W), bool)
                outside[rows(r)] = False
                assert np.array_equal(color.view(np.uint32)[outside], p_color.view(np.uint32)[outside]), (r, n, "colour outside")
                assert np.array_equal(count.view(np.uint32)[outside], p_count.view(np.uint32)[outside]), (r, n, "count outside")
                bad = int((color.view(np.uint32) != want_color.view(np.uint32)).any(axis=-1).sum())
                assert bad == 0, (r, n, f"{bad} pixels differ from the fold")
                assert np.array_equal(count, want_count), (r, n)
    finally:
        be.release()


# ---- 2. / 3. a partition is the frame; the whole image as a region is ptmi_render --------------------------------------------
def _modes():
    yield "plain_strict", "cornell", {}
    yield "plain_default", "cornell", dict(flags=DA)
    yield "general", "feat_textured", dict(flags=DA)
    yield "nansafe", "cornell_za", dict(flags=DA)
    yield "nansafe_strict", "cornell_za", {}
    yield "megakernel", "cornell", dict(flags=DA | backend.FLAG_MEGAKERNEL)
    yield "two_devices", "cornell", dict(flags=DA, devices=[0, 0])
    yield "uniform", "cornell", dict(flags=DA, sampler=S.UNIFORM)
    yield "russian_roulette_source_seed", "cornell", dict(flags=DA | backend.FLAG_RUSSIAN_ROULETTE | backend.FLAG_SOURCE_SEED)
    yield "super_sampling", "cornell", dict(flags=DA, super_sampling=True)
    yield "statistics", "cornell", dict(flags=DA | backend.FLAG_SCHEDULER_STATS)


MODES = [pytest.param(name, kw, id=mode) for mode, name, kw in _modes()]
_frames = {}


def frame(mode_id, name, kw, n):
    """what ptmi_render(0, n) leaves in a fresh context; computed once, read-only"""
    key = (mode_id, n)
    if key not in _frames:
        be = context(scene(name), **kw)
        try:
            be.render(0, n)
            _frames[key] = state(be, variance=kw.get("super_sampling", False))
        finally:
            be.release()
    return _frames[key]


def iterations_of(kw):
    return 10 if kw.get("super_sampling") else 6  # (the stop criterion starts to skip paths from iteration 6 on)


@pytest.mark.parametrize("name, kw", MODES)
def test_a_partition_is_the_frame(name, kw, request):
    n, ss = iterations_of(kw), kw.get("super_sampling", False)
    want = frame(request.node.callspec.id, name, kw, n)
    be = context(scene(name), **kw)
    try:
        if name == "cornell_za":
            assert kw.get("flags", 0) & backend.FLAG_MEGAKERNEL == 0 and be.literal_kernel_reason()
        for parts in (QUARTERS, STRIPS):
            be.clear()
            for r in parts:
                be.render_region(*r, 0, n)
            assert_same_state(state(be, variance=ss), want)
    finally:
        be.release()


@pytest.mark.parametrize("name, kw", MODES)
def test_the_whole_image_as_a_region_is_ptmi_render(name, kw, request):
    n, ss = iterations_of(kw), kw.get("super_sampling", False)
    want = frame(request.node.callspec.id, name, kw, n)
    be = context(scene(name), **kw)
    try:
        be.render_region(*WHOLE, 0, n)
        assert_same_state(state(be, variance=ss), want)
    finally:
        be.release()


@pytest.mark.parametrize("flags", ARITHMETICS)
def test_the_whole_image_as_a_region_after_scene_updates(flags):
    """... also after ptmi_update_triangles and ptmi_set_camera: both contexts get the same edits."""
    sc = scene("cornell")
    moved, cam = U.moved_triangles(sc, "cornell"), U.moved_camera(sc)
    a, b = context(sc, flags=flags), context(sc, flags=flags)
    try:
        for be in (a, b):
            be.update_triangles(moved)
            be.set_camera(cam.cameraPosition, cam.cameraDirection, cam.cameraRight, cam.cameraUp)
        a.render(0, 6)
        b.render_region(*WHOLE, 0, 6)
        assert_same_state(state(a), state(b))
        assert not np.array_equal(state(a)["color"], frame("plain_default" if flags else "plain_strict", "cornell", dict(flags=flags) if flags else {}, 6)["color"])  # (the edits did change the image)
    finally:
        a.release()
        b.release()


# ---- 4. the per-path yardstick -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "cornell_za"])
def test_counters_and_histograms_gain_what_the_paths_predict(name):
    """Region (13, 7, 17, 11), iterations [2, 5): ptmi_trace_paths along the camera's rays, with the work-items' own seed indices
    (gx + gy * W + it * W * H), gives each of the 187 x 3 paths' radiance and counts."""
    sc, (x, y, w, h) = scene(name), INNER
    be = context(sc, flags=DA)
    try:
        inside = np.array([gy * W + gx for gy in range(y, y + h) for gx in range(x, x + w)])
        sums = []
        for it in range(2, 5):
            rays = P.camera_rays(sc, W, H, it, default_arithmetic=True)[inside]
            # ray i of a batch gets seed index first_index + i + it * index_stride: one call per row of the region
            per_row = [be.trace_paths(rays[k * w:(k + 1) * w]["origin"], rays[k * w:(k + 1) * w]["direction"], first_iteration=it, n_iterations=1,
                                      first_index=(y + k) * W + x, index_stride=W * H) for k in range(h)]
            sums.append(np.concatenate(per_row))
        before = state(be)
        be.render_region(x, y, w, h, 2, 3)
        after = state(be)
        allsums = np.concatenate(sums)
        assert len(allsums) == 187 * 3
        gained = {k: after["counters"][k] - before["counters"][k] for k in after["counters"]}
        want = dict(paths=len(allsums), segments=int(allsums["segments"].sum()), surface_hits=int(allsums["surface_hits"].sum()),
                    shadow_rays=int(allsums["shadow_rays"].sum()), box_tests=int(allsums["box_tests"].sum()),
                    triangle_tests=int(allsums["triangle_tests"].sum()))
        assert gained == want
        dep, bbx, tri = (a.astype(np.int64) - b.astype(np.int64) for a, b in zip(after["stats"], before["stats"]))
        assert np.array_equal(dep, np.bincount(allsums["surface_hits"], minlength=len(dep)))
        limit = S.MAX_INTERSETCION_NUMBER
        assert np.array_equal(bbx, np.bincount(allsums["box_tests"][allsums["box_tests"] < limit].astype(np.int64), minlength=limit))
        assert np.array_equal(tri, np.bincount(allsums["triangle_tests"][allsums["triangle_tests"] < limit].astype(np.int64), minlength=limit))
        color = np.zeros((h, w, 4), np.float32)
        with np.errstate(all="ignore"):
            for s in sums:
                color = color + s["radiance"].reshape(h, w, 4)
        got_color, got_count = be.read_region(x, y, w, h)
        assert same_words(got_color, color) and (got_count == 3).all()
        assert int(after["count"].sum()) == 187 * 3
    finally:
        be.release()


# ---- 5. the RANDOM sampler -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "cornell_za"])
def test_random_sampler_partition(name):
    """The region selects work-items; their samples land anywhere, atomically.  Counts, histograms and counters exactly; colours
    as the other RANDOM tests compare two renders (tests/test_render_ahead_gpu.py: the float sums are atomic)."""
    kw = dict(flags=DA, sampler=S.RANDOM)
    want = frame("random_" + name, name, kw, 6)
    be = context(scene(name), **kw)
    try:
        for parts in (QUARTERS, STRIPS):
            be.clear()
            for r in parts:
                be.render_region(*r, 0, 6)
            got = state(be)
            assert got["counters"] == want["counters"]
            for a, b in zip(got["stats"], want["stats"]):
                assert np.array_equal(a, b)
            assert got["count"].sum() == want["count"].sum() == W * H * 6 and np.array_equal(got["count"], want["count"])
            g, w_ = got["color"].view(np.float32), want["color"].view(np.float32)
            assert np.array_equal(np.isnan(g), np.isnan(w_)) and np.allclose(np.nan_to_num(g), np.nan_to_num(w_), rtol=1e-4, atol=1e-5)
    finally:
        be.release()


# ---- 6. seeded random sequences of calls ----------------------------------------------------------------------------------------
def _sequence(rs):
    """25 calls: full calls, region calls over overlapping rectangles, repeated and out-of-order ids, read_region and clear, and
    runs of short in-order full calls that leave launches ahead in flight when a region call arrives"""
    calls, nxt = [], 0
    while len(calls) < 25:
        kind = rs.randint(6)
        if kind == 0:  # a run of short in-order full calls, each waited for: the pattern that is rendered ahead of
            n = int(rs.randint(1, 4))
            for _ in range(int(rs.randint(3, 6))):
                calls.append(("render", nxt, n))
                nxt += n
        elif kind in (1, 2, 3):
            x, y = int(rs.randint(0, W)), int(rs.randint(0, H))
            r = (x, y, int(rs.randint(1, W - x + 1)), int(rs.randint(1, H - y + 1)))
            first = nxt if rs.randint(2) else int(rs.randint(0, 12))
            calls.append(("region", r, first, int(rs.choice([1, 2, 3, 5, 7]))))
        elif kind == 4:
            x, y = int(rs.randint(0, W)), int(rs.randint(0, H))
            calls.append(("read", (x, y, int(rs.randint(1, W - x + 1)), int(rs.randint(1, H - y + 1)))))
        else:
            calls.append(("clear",) if rs.randint(3) == 0 else ("render", int(rs.randint(0, 12)), int(rs.randint(1, 6))))
    return calls[:25]


@pytest.mark.parametrize("name", ["cornell", "cornell_za"])
@pytest.mark.parametrize("seed", range(20))
def test_seeded_sequences_of_calls(name, seed):
    calls = _sequence(np.random.RandomState(1000 + seed))
    top = max([c[1] + c[2] for c in calls if c[0] == "render"] + [c[2] + c[3] for c in calls if c[0] == "region"] + [1])
    R = planes(name, DA, top)
    be = context(scene(name), flags=DA)
    try:
        color, count, paths = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32), 0
        for c in calls:
            if c[0] == "render":
                be.render(c[1], c[2])
                be.synchronize()  # (a caller that waits: what launches ahead want to see)
                color, count = fold(color, count, R[c[1]:c[1] + c[2]], WHOLE)
                paths += W * H * c[2]
            elif c[0] == "region":
                be.render_region(*c[1], c[2], c[3])
                color, count = fold(color, count, R[c[2]:c[2] + c[3]], c[1])
                paths += c[1][2] * c[1][3] * c[3]
            elif c[0] == "clear":
                be.clear()
                color[:], count[:], paths = 0, 0, 0
            else:
                r_color, r_count = be.read_region(*c[1])
                i_color, i_count = be.read_image()
                assert np.array_equal(r_color.view(np.uint32), i_color.view(np.uint32)[rows(c[1])]), (c, "read_region colour")
                assert np.array_equal(r_count.view(np.uint32), i_count.view(np.uint32)[rows(c[1])]), (c, "read_region count")
            got_color, got_count = be.read_image()
            assert same_words(got_color, color), (seed, c)
            assert np.array_equal(got_count, count), (seed, c)
            assert be.counters()["paths"] == paths, (seed, c)
    finally:
        be.release()


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_device", "device_listed_twice"])
def test_read_region_is_the_slice_of_read_image(devices):
    """... word for word, into pageable and into page-locked destinations, either pointer NULL."""
    be = context(scene("cornell"), flags=DA, devices=devices)
    pinned = (np.full((H, W, 4), -1, np.float32), np.full((H, W), -1, np.float32))
    try:
        be.render(0, 3)
        be.render_region(*INNER, 3, 2)
        color, count = be.read_image()
        be.pin_host_buffer(pinned[0])
        be.pin_host_buffer(pinned[1])
        for r in REGIONS:
            x, y, w, h = r
            for out in (None, (pinned[0].reshape(-1)[:w * h * 4].reshape(h, w, 4), pinned[1].reshape(-1)[:w * h].reshape(h, w))):
                r_color, r_count = be.read_region(*r, out=out)
                assert np.array_equal(r_color.view(np.uint32), color.view(np.uint32)[rows(r)]), r
                assert np.array_equal(r_count.view(np.uint32), count.view(np.uint32)[rows(r)]), r
            only_color, none = be.read_region(*r, out=(np.empty((h, w, 4), np.float32), None))
            assert none is None and np.array_equal(only_color.view(np.uint32), color.view(np.uint32)[rows(r)])
            none, only_count = be.read_region(*r, out=(None, np.empty((h, w), np.float32)))
            assert none is None and np.array_equal(only_count, count[rows(r)])
        assert (pinned[0].reshape(-1)[W * H * 4 - 4:] != -1).all()  # (the whole image was the first region read into it)
    finally:
        be.unpin_host_buffer(pinned[0])
        be.unpin_host_buffer(pinned[1])
        be.release()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    sc = scene("cornell")
    early = Backend().setup_context(W, H, DEPTH, sc.lightsSize, flags=DA)
    try:
        for call in (lambda: early.render_region(0, 0, 1, 1, 0, 1), lambda: early.read_region(0, 0, 1, 1)):
            with pytest.raises(PtmiError) as e:
                call()
            assert e.value.code == ERR_STATE and "before ptmi_initialize_memory" in str(e.value)
    finally:
        early.release()
    be = context(sc, flags=DA)
    try:
        be.render(0, 2)
        before = state(be)
        be.kernel_time()
        lib, ctx = be._lib, be._ctx
        bad = [(W - 3, 0, 4, 1), (0, H - 1, 1, 2), (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2), (W, 0, 1, 1), (0, 0, W + 1, H)]
        for entry, call in (("ptmi_render_region", lambda r: be.render_region(*r, 0, 1)), ("ptmi_read_region", lambda r: be.read_region(*r))):
            for r in bad:
                with pytest.raises(PtmiError) as e:
                    call(r)
                assert e.value.code == ERR_INVALID_ARGUMENT and entry in str(e.value), (entry, r, str(e.value))
                assert_same_state(state(be), before)
        assert lib.ptmi_render_region(ctx, None, 0, 1) == ERR_INVALID_ARGUMENT and b"ptmi_render_region" in lib.ptmi_last_error(ctx)
        assert lib.ptmi_read_region(ctx, None, None, None) == ERR_INVALID_ARGUMENT and b"ptmi_read_region" in lib.ptmi_last_error(ctx)
        with pytest.raises(PtmiError) as e:
            be.render_region(0, 0, 1, 1, 0xFFFFFFFF, 2)
        assert e.value.code == ERR_INVALID_ARGUMENT and "ptmi_render_region" in str(e.value) and "32 bits" in str(e.value)
        assert_same_state(state(be), before)
        # empty regions and n = 0 are PTMI_OK and launch nothing
        assert be.kernel_time()[1] == 0
        for r, n in (((5, 5, 0, 3), 4), ((5, 5, 3, 0), 4), ((W, H, 0, 0), 4), ((5, 5, 3, 3), 0)):
            be.render_region(*r, 0, n)
        be.synchronize()
        assert be.kernel_time()[1] == 0
        color, count = be.read_region(5, 5, 0, 3)
        assert color.size == 0 and count.size == 0
        assert_same_state(state(be), before)
        # ... and the context renders as before
        be.render_region(*INNER, 2, 1)
        be.synchronize()
        assert be.kernel_time()[1] == 1
        be.render(2, 1)
        want = context(sc, flags=DA)
        try:
            want.render(0, 3)
            want.render_region(*INNER, 2, 1)
            assert_same_state(state(be), state(want))
        finally:
            want.release()
    finally:
        be.release()
