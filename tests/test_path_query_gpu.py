"""ptmi_trace_paths / ptmi_trace_paths_device against the yardstick of path_query_cases.py (the CPU oracle's Kernel_Main on a
zero-basis camera): every field of every sum bit-equal, compared as uint32 words (a NaN where the yardstick has a NaN), in both
arithmetics and under all three samplers, on the scenes that take each path of the kernel; the built-in camera's rays against
ptmi_render itself; and what the feature promises around the kernel - calls change nothing that was rendered, they follow
ptmi_update_triangles, errors leave the context rendering as before.  test_path_query_model.py asserts what the shared batches
reach.  A yardstick is computed once per (scene, configuration) and shared."""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, structs as S
from gpu_cases import assert_same_state, state
import gpu_cases
import path_query_cases as P
import scene_update_cases as U

pytestmark = pytest.mark.gpu
W, H, STRIDE = P.W, P.H, P.STRIDE
DA, RR, SOURCE_SEED = backend.FLAG_DEFAULT_ARITHMETIC, backend.FLAG_RUSSIAN_ROULETTE, backend.FLAG_SOURCE_SEED
INVALID_ARGUMENT, STATE = -1, -6
ARITHMETICS = pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])
SAMPLERS = pytest.mark.parametrize("sampler", [S.JITTERED, S.RANDOM, S.UNIFORM], ids=["jittered", "random", "uniform"])
_yardsticks = {}


def yardstick(name, flags=0, sampler=S.JITTERED, depth=4, sc=None):
    key = (name, flags, sampler, depth)
    if key not in _yardsticks:
        _yardsticks[key] = P.Yardstick(sc or P.scene(name), depth, sampler, default_arithmetic=bool(flags & DA),
                                       russian_roulette=bool(flags & RR), source_seed=bool(flags & SOURCE_SEED))
    return _yardsticks[key]


def wanted(name, rays, flags=0, sampler=S.JITTERED, depth=4, **kw):
    with np.errstate(all="ignore"):
        return yardstick(name, flags, sampler, depth).sums(rays, **kw)


def cornell(n=P.N_CORNELL):
    return P.batch("cornell", P.scene("cornell"), P.N_CORNELL)[:n]


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, **kw)


def trace(be, rays, out=None, **kw):
    kw.setdefault("index_stride", STRIDE)
    return be.trace_paths(rays["origin"], rays["direction"], out=out, **kw)


def assert_equal(got, want):
    msg = P.describe_difference(got, want)
    assert not msg, msg


# ---------------------------------------------------------------------------------------------- the kernel against the yardstick

@ARITHMETICS
@SAMPLERS
def test_batch_sizes_on_cornell(flags, sampler, monkeypatch):
    """Wave and workgroup tails (1, 63, 64, 65, 257, 1000 rays) for one and for three iterations, and the grid-stride loop (257
    and 1000 rays on ONE and on two workgroups).  A ray keeps its index whatever the batch, so the sizes share one yardstick."""
    rays = cornell()
    be = context(P.scene("cornell"), flags=flags, sampler=sampler)
    try:
        for n_it in (1, 3):
            want = wanted("cornell", rays, flags, sampler, n_iterations=n_it, index_stride=STRIDE)
            for n in (1, 63, 64, 65, 257, 1000):
                assert_equal(trace(be, rays[:n], n_iterations=n_it), want[:n])
            for blocks, n in ((1, 257), (1, 1000), (2, 1000)):
                monkeypatch.setenv("PTMI_QUERY_MAX_BLOCKS", str(blocks))
                assert_equal(trace(be, rays[:n], n_iterations=n_it), want[:n])
            monkeypatch.delenv("PTMI_QUERY_MAX_BLOCKS")
        # a middle slice is its own batch: the same rays under the indices of their new positions, from a later iteration on
        want = wanted("cornell", rays[100:165], flags, sampler, first_iteration=2, n_iterations=2, first_index=7, index_stride=STRIDE)
        assert_equal(trace(be, rays[100:165], first_iteration=2, n_iterations=2, first_index=7), want)
    finally:
        be.release()


@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page_locked"])
def test_the_scratch_grows_and_is_reused(page_locked):
    """257 rays, then 1100 - past the 1024-ray floor of the context's buffers, which are freed and regrown - then 257 again, into
    an ordinary array and into one the caller has page-locked."""
    rays = np.concatenate([cornell(), cornell(100)])
    want = wanted("cornell", rays, DA, n_iterations=2, index_stride=STRIDE)
    out = np.zeros(1100, S.PATH_SUM)
    be = context(P.scene("cornell"), flags=DA)
    try:
        if page_locked:
            be.pin_host_buffer(out)
        for n in (257, 1100, 257):
            out[:] = np.zeros(1, S.PATH_SUM)
            got = trace(be, rays[:n], out=out[:n], n_iterations=2)
            assert got.ctypes.data == out.ctypes.data
            assert_equal(got, want[:n])
        if page_locked:
            be.unpin_host_buffer(out)
    finally:
        be.release()


@ARITHMETICS
@pytest.mark.parametrize("name", P.SCENES)
def test_scenes(name, flags):
    """A one-triangle tree, big and empty leaves, a tree deeper than 22 levels, 20 000 triangles, the NaN-record scene (served by
    the literal kernel's loops), textures, glass, water, a cube-map sky, and three lights over mixed materials."""
    sc = P.scene(name)
    rays = P.batch(name, sc, P.N_SCENE)
    want = wanted(name, rays, flags, n_iterations=2, index_stride=STRIDE)
    be = context(sc, flags=flags)
    try:
        if name == "hostile":
            assert be.literal_kernel_reason()
        assert_equal(trace(be, rays, n_iterations=2), want)
    finally:
        be.release()


@ARITHMETICS
def test_records_that_are_not_precomputed(flags, monkeypatch):
    """PTMI_GENERIC_TRIANGLES uploads the plain DTri records: the other instantiation of the kernel."""
    monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    sc = P.scene("tris20k")
    rays = P.batch("tris20k", sc, P.N_SCENE)
    be = context(sc, flags=flags)
    try:
        assert_equal(trace(be, rays, n_iterations=2), wanted("tris20k", rays, flags, n_iterations=2, index_stride=STRIDE))
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- the built-in camera

@pytest.mark.parametrize("sampler", [S.JITTERED, S.UNIFORM], ids=["jittered", "uniform"])
def test_the_cameras_own_rays_give_the_rendered_image(sampler):
    """Strict arithmetic, 64 x 48: the camera's rays of iteration `it`, built here in float32 from pto_sampler's sample and
    up * sy + (right * sx + dir) without contraction, first_index = 0 and index_stride = W * H: ray gy * W + gx gets the words
    ptmi_render(it, 1) leaves in that pixel of a fresh context, the counts add up to its ptmi_counters, and a new camera on the
    context does not move a result."""
    sc = P.scene("cornell")
    for it in (0, 5):
        rays = P.camera_rays(sc, W, H, it, sampler)
        be = context(sc, sampler=sampler)
        try:
            sums = trace(be, rays, first_iteration=it, first_index=0, index_stride=W * H)
            be.set_camera(np.asarray(sc.cameraPosition, np.float32) + np.float32([10, -5, 20, 0]), sc.cameraDirection, sc.cameraRight, sc.cameraUp)
            assert_equal(trace(be, rays, first_iteration=it, first_index=0, index_stride=W * H), sums)
        finally:
            be.release()
        fresh = context(sc, sampler=sampler)
        try:
            fresh.render(it, 1)
            color, count = fresh.read_image()
            counters = fresh.counters()
        finally:
            fresh.release()
        assert (count == 1).all()
        differ = int((sums["radiance"].view(np.uint32) != color.reshape(-1, 4).view(np.uint32)).any(axis=1).sum())
        assert differ == 0, f"iteration {it}: {differ} of {W * H} rays differ from the rendered pixel"
        assert {n: int(sums[n].sum()) for n in P.COUNTS} == {n: counters[n] for n in P.COUNTS} and counters["paths"] == W * H


# ---------------------------------------------------------------------------------------------- flags

@ARITHMETICS
def test_russian_roulette_at_depth_12(flags):
    rays = cornell(257)
    want = wanted("cornell", rays, flags | RR, depth=12, n_iterations=2, index_stride=STRIDE)
    plain = wanted("cornell", rays, flags, depth=12, n_iterations=2, index_stride=STRIDE)
    assert P.describe_difference(want, plain) and want["surface_hits"].max() > 2 * 6  # (the block past reflection 5 was reached)
    be = context(P.scene("cornell"), depth=12, flags=flags | RR)
    try:
        assert_equal(trace(be, rays, n_iterations=2), want)
    finally:
        be.release()


@pytest.mark.parametrize("flags", [0, SOURCE_SEED, DA | SOURCE_SEED], ids=["compiled_rule", "source_rule", "source_rule_default"])
def test_the_seed_rule_at_a_multiple_of_65536(flags):
    """64 rays whose indices run from 65504 to 65567: position 32 has index 2^16, whose squared seed wraps to 0 - the compiled
    reference keeps 0 (every random number of that path is 0), PTMI_FLAG_SOURCE_SEED makes it 1."""
    rays, first, stride = cornell(64), 65536 - 32, 70000
    want = wanted("cornell", rays, flags, n_iterations=2, first_index=first, index_stride=stride)
    other = wanted("cornell", rays, flags ^ SOURCE_SEED, n_iterations=2, first_index=first, index_stride=stride)
    differ = np.nonzero((P.words(want) != P.words(other)).any(axis=1))[0]
    assert differ.tolist() == [32]  # (the two rules part on that path, and on no other)
    be = context(P.scene("cornell"), flags=flags)
    try:
        assert_equal(trace(be, rays, n_iterations=2, first_index=first, index_stride=stride), want)
    finally:
        be.release()


def test_super_sampling_is_ignored():
    """A SUPER_SAMPLING context from iteration 6 on, where Kernel_Main draws for its stop criterion: no draw is made here."""
    rays = cornell(257)
    want = wanted("cornell", rays, first_iteration=6, n_iterations=2, index_stride=STRIDE)
    be = context(P.scene("cornell"), super_sampling=True)
    try:
        be.render(0, 8)
        assert_equal(trace(be, rays, first_iteration=6, n_iterations=2), want)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- device pointers

def _tensors(rays):
    import torch
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(len(rays), 12).copy()).cuda()
    d_sums = torch.full((len(rays), 12), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return d_rays, d_sums


def _sums(d_sums):
    return np.ascontiguousarray(d_sums.cpu().numpy()).view(S.PATH_SUM).reshape(-1)


def test_device_pointers_equal_host_arrays():
    import torch
    rays = cornell(257)
    want = wanted("cornell", rays, n_iterations=3, index_stride=STRIDE)
    be = context(P.scene("cornell"))
    try:
        d_rays, d_sums = _tensors(rays)
        be.trace_paths_device(d_rays.data_ptr(), len(rays), d_sums.data_ptr(), n_iterations=3, index_stride=STRIDE)  # the context's own stream
        be.synchronize()
        assert_equal(_sums(d_sums), want)
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        be.set_stream(stream.cuda_stream)
        d_sums2 = torch.full_like(d_sums, -1.0)
        torch.cuda.synchronize()
        be.trace_paths_device(d_rays.data_ptr(), len(rays), d_sums2.data_ptr(), n_iterations=3, index_stride=STRIDE)
        with torch.cuda.stream(stream):
            on_stream = d_sums2.clone()  # a torch op ordered behind the call on the caller's stream
        stream.synchronize()
        assert_equal(_sums(on_stream), want)
        assert_equal(trace(be, rays, n_iterations=3), want)  # host arrays on the caller's stream
        be.set_stream(None)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- calls and renders

def test_calls_are_invisible_to_renders():
    sc, rays = P.scene("cornell"), cornell(257)
    want = wanted("cornell", rays, n_iterations=2, index_stride=STRIDE)

    def play(with_calls):
        be = context(sc)
        try:
            be.render(0, 2)
            if with_calls:
                assert_equal(trace(be, rays, n_iterations=2), want)
            be.render(2, 2)
            if with_calls:
                assert_equal(trace(be, rays[:65], n_iterations=2), want[:65])
            for k in range(4, 12):  # one-iteration calls of a caller that waits: rendered ahead of, then adopted
                be.render(k, 1)
                be.synchronize()
                if with_calls:
                    assert_equal(trace(be, rays[:65], n_iterations=2), want[:65])
            return state(be)
        finally:
            be.release()

    assert_same_state(play(True), play(False))


def test_calls_leave_the_scheduler_statistics():
    rays = cornell(257)
    be = context(P.scene("cornell"), flags=backend.FLAG_SCHEDULER_STATS)
    try:
        be.render(0, 2)
        before, checks = be.scheduler_stats(), be.invariant_checks()
        assert before["trips_node"] > 0
        assert_equal(trace(be, rays), wanted("cornell", rays, index_stride=STRIDE))
        assert be.scheduler_stats() == before and be.invariant_checks() == checks
    finally:
        be.release()


def test_calls_follow_update_triangles():
    import torch
    sc = P.scene("cornell")
    tris = U.displaced(sc.triangulation, 7)
    moved = U.moved_scene(sc, tris)
    rays = cornell(257)
    want = wanted("cornell", rays, n_iterations=2, index_stride=STRIDE)
    with np.errstate(all="ignore"):
        want_moved = P.Yardstick(moved).sums(rays, n_iterations=2, index_stride=STRIDE)
    assert P.describe_difference(want_moved, want)  # (the triangles did move)
    be = context(sc)
    try:
        d_rays, before = _tensors(rays)
        after = torch.full_like(before, -1.0)
        torch.cuda.synchronize()
        be.trace_paths_device(d_rays.data_ptr(), len(rays), before.data_ptr(), n_iterations=2, index_stride=STRIDE)  # not waited for: the update must
        be.update_triangles(tris)
        be.trace_paths_device(d_rays.data_ptr(), len(rays), after.data_ptr(), n_iterations=2, index_stride=STRIDE)
        be.synchronize()
        assert_equal(_sums(before), want)
        assert_equal(_sums(after), want_moved)
        assert_equal(trace(be, rays, n_iterations=2), want_moved)
    finally:
        be.release()


def test_a_context_that_lists_one_device_twice():
    rays = cornell(257)
    be = context(P.scene("cornell"), devices=[0, 0])
    try:
        be.render(0, 3)
        assert_equal(trace(be, rays, n_iterations=2), wanted("cornell", rays, n_iterations=2, index_stride=STRIDE))
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- errors

def test_status_codes_and_errors_leave_the_context_rendering():
    sc, rays = P.scene("cornell"), np.ascontiguousarray(cornell(64))
    lib = backend.load_library()
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        poison = np.frombuffer(b"\xA5" * (64 * 48), S.PATH_SUM).copy()
        sums = poison.copy()
        good = backend.PathParams(C.sizeof(backend.PathParams), 0, 2, 0, STRIDE)
        p_rays, p_sums = rays.ctypes.data, sums.ctypes.data
        assert lib.ptmi_trace_paths(be._ctx, C.byref(good), p_rays, 64, p_sums) == STATE
        assert b"before ptmi_initialize_memory" in lib.ptmi_last_error(be._ctx)
        assert lib.ptmi_trace_paths_device(be._ctx, C.byref(good), 256, 1, 512) == STATE
        be.initialize_memory(sc)
        be.render(0, 3)
        baseline = state(be)

        def refused(rc):
            assert rc == INVALID_ARGUMENT and len(lib.ptmi_last_error(be._ctx)) > 0
            be.clear()
            be.render(0, 3)
            assert_same_state(state(be), baseline)

        def params(**kw):
            p = backend.PathParams(C.sizeof(backend.PathParams), 0, 2, 0, STRIDE)
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        reserved = params()
        reserved.reserved[2] = 1
        d_rays, d_sums = _tensors(rays)
        for form, r, s in ((lib.ptmi_trace_paths, p_rays, p_sums), (lib.ptmi_trace_paths_device, d_rays.data_ptr(), d_sums.data_ptr())):
            refused(form(be._ctx, None, r, 64, s))
            refused(form(be._ctx, C.byref(params(struct_size=28)), r, 64, s))
            refused(form(be._ctx, C.byref(reserved), r, 64, s))
            refused(form(be._ctx, C.byref(params(n_iterations=4097)), r, 64, s))
            refused(form(be._ctx, C.byref(params(n_iterations=4097)), None, 0, None))  # (the cap holds whatever the count)
            refused(form(be._ctx, C.byref(good), None, 64, s))
            refused(form(be._ctx, C.byref(good), r, 64, None))
        refused(lib.ptmi_trace_paths_device(be._ctx, C.byref(good), d_rays.data_ptr() + 4, 63, d_sums.data_ptr()))
        refused(lib.ptmi_trace_paths_device(be._ctx, C.byref(good), d_rays.data_ptr(), 63, d_sums.data_ptr() + 8))
        # no work: PTMI_OK, nothing launched, nothing written - not even with NULL arrays
        for form, r, s in ((lib.ptmi_trace_paths, p_rays, p_sums), (lib.ptmi_trace_paths_device, d_rays.data_ptr(), d_sums.data_ptr())):
            assert form(be._ctx, C.byref(good), r, 0, s) == 0 and form(be._ctx, C.byref(params(n_iterations=0)), r, 64, s) == 0
            assert form(be._ctx, C.byref(good), None, 0, None) == 0 and form(be._ctx, C.byref(params(n_iterations=0)), None, 64, None) == 0
        be.synchronize()
        assert (d_sums.cpu().numpy() == -1).all() and sums.tobytes() == poison.tobytes()
        be.clear()
        be.render(0, 3)
        assert_same_state(state(be), baseline)
        assert_equal(trace(be, rays, n_iterations=2), wanted("cornell", rays, n_iterations=2, index_stride=STRIDE))  # a good call still works
        with pytest.raises(PtmiError):
            be.trace_paths(rays["origin"], rays["direction"], out=np.zeros(3, S.PATH_SUM))
    finally:
        be.release()
