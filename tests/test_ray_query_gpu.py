"""ptmi_query_rays / ptmi_query_rays_device against the walk of ray_query_cases.py: every field of every hit bit-equal (compared as
uint32 words), in both arithmetics and for both kinds, on the scenes that take each path of the kernel; and what the feature
promises around the kernel - queries change nothing that was rendered, they follow ptmi_update_triangles, errors leave the
context rendering as before.  The walk of a (scene, arithmetic, kind) is computed once and shared."""
import warnings

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, bvh_create, scenes, structs as S
import bvh_stress_cases as stress
from gpu_cases import assert_same_state, cached_scene, state
import gpu_cases
import ray_query_cases as Q
import scene_update_cases as U

pytestmark = pytest.mark.gpu
W, H = 64, 48
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE = -1, -6
ARITHMETICS = pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])
KINDS = pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
_scenes, _rays, _want = {}, {}, {}


def scene(name):
    if name not in _scenes:
        if name == "one_triangle":
            sc = scenes.cornell_box(W, H)
            sc.triangulation = scenes._concat_tris([sc.triangulation[5:6]])
            sc = bvh_create(sc)
            assert sc.bvh["isLeaf"][0] and len(sc.bvh) == 1
        elif name == "deep_chain":
            sc = scenes.cornell_box(W, H)
            sc.triangulation = stress.make("deep_chain_27", 0, 56)
            sc = bvh_create(sc)
            assert sc.bvhMaxDepth > 22
        elif name == "hostile":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (the hostile scenes divide 0 by 0 on purpose, as the importer would)
                sc = bvh_create(scenes.add_zero_area_triangles(scenes.build("fuzz5h_l1", W, H), 24))
        else:
            sc = cached_scene(name, W, H)
        _scenes[name] = sc
    return _scenes[name]


def rays_of(name):
    """The rays a scene is asked: the four generators in turn, then the distance-limited ones of the first rays' closest hits."""
    if name not in _rays:
        sc = scene(name)
        n = 1000 if name == "cornell" else 257
        with np.errstate(all="ignore"):
            rays = Q.mixed_rays(sc, n - 48, W, H)
            head = Q.expected_hits(sc, rays[:64])
            limited = Q.limited_rays(rays[:64], head)[:48]
            more = Q.mixed_rays(sc, 48 - len(limited), W, H, seed=11)
        _rays[name] = np.concatenate([rays, limited, more])
        assert len(_rays[name]) == n
    return _rays[name]


def wanted(name, flags, any_hit, sc=None, rays=None):
    key = (name, flags, any_hit)
    if key not in _want:
        with np.errstate(all="ignore"):
            _want[key] = Q.expected_hits(sc or scene(name), rays_of(name) if rays is None else rays, any_hit, default_arithmetic=flags == DA)
    return _want[key]


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, **kw)


def query(be, rays, any_hit=False, out=None):
    return be.query_rays(rays["origin"], rays["direction"], rays["max_squared_distance"], any_hit=any_hit, out=out)


def assert_equal(got, want, nan_bits=True):
    msg = Q.describe_difference(got, want, nan_bits)
    assert not msg, msg


# ---------------------------------------------------------------------------------------------- the kernel against the walk

@ARITHMETICS
@KINDS
def test_batch_sizes_on_cornell(flags, any_hit, monkeypatch):
    """Wave and workgroup tails (1, 63, 64, 65, 257) and the grid-stride loop (257 and 1000 rays on ONE and on two workgroups)."""
    rays, want = rays_of("cornell"), wanted("cornell", flags, any_hit)
    assert (want["triangle_id"] != Q.MISS).sum() > 300 and (want["triangle_id"] == Q.MISS).sum() > 50
    be = context(scene("cornell"), flags=flags)
    try:
        for n in (1, 63, 64, 65, 257, 1000):
            assert_equal(query(be, rays[:n], any_hit), want[:n])
        for blocks, n in ((1, 257), (1, 1000), (2, 1000)):
            monkeypatch.setenv("PTMI_QUERY_MAX_BLOCKS", str(blocks))
            assert_equal(query(be, rays[:n], any_hit), want[:n])
        monkeypatch.delenv("PTMI_QUERY_MAX_BLOCKS")
        # a later, smaller batch reuses the scratch; a middle slice is its own batch
        assert_equal(query(be, rays[100:165], any_hit), want[100:165])
    finally:
        be.release()


@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page_locked"])
def test_the_scratch_grows_and_is_reused(page_locked):
    """257 rays, then 1100 - the cached 1000 and their first 100 again, past the 1024-ray floor of the context's buffers, which
    are freed and regrown - then 257 again, into an ordinary array and into one the caller has page-locked."""
    rays, want = rays_of("cornell"), wanted("cornell", DA, False)
    rays, want = np.concatenate([rays, rays[:100]]), np.concatenate([want, want[:100]])
    out = np.zeros(1100, S.RAY_HIT)
    be = context(scene("cornell"), flags=DA)
    try:
        if page_locked:
            be.pin_host_buffer(out)
        for n in (257, 1100, 257):
            out[:] = np.zeros(1, S.RAY_HIT)
            assert_equal(query(be, rays[:n], out=out[:n]), want[:n])
        if page_locked:
            be.unpin_host_buffer(out)
    finally:
        be.release()


@ARITHMETICS
@pytest.mark.parametrize("name", ["one_triangle", "big_leaf", "empty_leaves", "feat_textured", "deep_chain", "tris20k", "hostile"])
def test_scenes(name, flags):
    sc, rays = scene(name), rays_of(name)
    be = context(sc, flags=flags)
    try:
        if name == "hostile":
            assert be.literal_kernel_reason()  # NaN distances are accepted and the last passer wins: the walk says which
        for any_hit in (False, True):
            want = wanted(name, flags, any_hit)
            assert_equal(query(be, rays, any_hit), want)
            if name not in ("hostile",):
                assert (want["triangle_id"] != Q.MISS).any()
    finally:
        be.release()


@ARITHMETICS
def test_records_that_are_not_precomputed(flags, monkeypatch):
    """PTMI_GENERIC_TRIANGLES uploads the plain DTri records: the other two instantiations of the kernel."""
    monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    be = context(scene("tris20k"), flags=flags)
    try:
        for any_hit in (False, True):
            assert_equal(query(be, rays_of("tris20k"), any_hit), wanted("tris20k", flags, any_hit))
    finally:
        be.release()


def odd_rays():
    """Rays that are not finite, and the other inputs nothing validates: an origin with w = 0 in a scene whose points carry
    w = 1 (the hits are displaced), a negative and a NaN distance limit."""
    sc = scene("cornell")
    base = Q.pinhole_rays(sc, 8, W, H)
    out = []
    for k, (field, value) in enumerate([("direction", [np.nan] * 4), ("direction", [np.nan, 1, 0.25, 0]), ("direction", [0.1, np.nan, 0.3, 0]),
                                        ("origin", [np.inf, 0, 0, 1]), ("origin", [278, -np.inf, 273, 1]), ("direction", [np.inf, 1, 1, 0]),
                                        ("direction", [0, 0, 0, 0]), ("origin", [np.nan, 0, 0, 1])]):
        r = base[k:k + 1].copy()
        r[field] = np.float32(value)
        out.append(r)
    w0 = Q.segment_rays(sc, 8, seed=21)
    w0["origin"][:, 3] = 0
    neg = base.copy()
    neg["max_squared_distance"] = np.float32([-1, -0.0, -np.inf, np.nan, -1e-30, -1, np.nan, -5])
    return np.concatenate(out + [w0, neg])


@ARITHMETICS
@KINDS
def test_rays_that_are_not_finite(flags, any_hit):
    """Every word equals the walk's, NaN words included - except WHICH NaN a ray with a NaN ORIGIN gets.  Such an origin is the
    one input of these tests that puts a NaN on the right of a subtraction (d - dot(N, origin), cl:538) and two NaNs of
    different descent into one operation (direction * t + origin).  IEEE 754 (6.3) leaves the sign and the payload of a NaN
    result open, OpenCL C adds nothing, and the walk's are those of the host's instructions (x86 `subss` hands the NaN operand
    on as it is, and of two NaNs the first): not the reference's, which has none.  On the MI355X the four float fields of
    this ray came out as NaNs of other bits than the host's 0x7FC00000, with every other word equal.  For
    those rays a float word must be a NaN where the walk's is; the triangle, the side, both counts and every word that is a
    number are compared as everywhere else."""
    rays = odd_rays()
    nan_origin = np.isnan(rays["origin"]).any(axis=1)
    with np.errstate(all="ignore"):
        want = Q.expected_hits(scene("cornell"), rays, any_hit, default_arithmetic=flags == DA)
    assert nan_origin.sum() == 1 and np.isnan(want["squared_distance"][nan_origin]).all()  # (accepted, at a NaN distance)
    be = context(scene("cornell"), flags=flags)
    try:
        got = query(be, rays, any_hit)
    finally:
        be.release()
    assert_equal(got[~nan_origin], want[~nan_origin])
    assert_equal(got[nan_origin], want[nan_origin], nan_bits=False)
    if not any_hit:
        n_tris, n_inner = len(scene("cornell").triangulation), int((scene("cornell").bvh["isLeaf"] == 0).sum())
        # the all-NaN direction walks the whole tree and keeps its last triangle
        assert (want["box_tests"][0], want["triangle_tests"][0]) == (2 * n_inner, n_tris) and want["triangle_id"][0] != Q.MISS


# ---------------------------------------------------------------------------------------------- device pointers

def _tensors(rays):
    import torch
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(len(rays), 12).copy()).cuda()
    d_hits = torch.full((len(rays), 12), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return d_rays, d_hits


def _hits(d_hits):
    return np.ascontiguousarray(d_hits.cpu().numpy()).view(S.RAY_HIT).reshape(-1)


@KINDS
def test_device_pointers_equal_host_arrays(any_hit):
    import torch
    rays = rays_of("cornell")[:257]
    be = context(scene("cornell"))
    try:
        host = query(be, rays, any_hit)
        assert_equal(host, wanted("cornell", 0, any_hit)[:257])
        d_rays, d_hits = _tensors(rays)
        be.query_rays_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), any_hit=any_hit)  # the context's own stream
        be.synchronize()
        assert_equal(_hits(d_hits), host)
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        be.set_stream(stream.cuda_stream)
        d_hits2 = torch.full_like(d_hits, -1.0)
        torch.cuda.synchronize()
        be.query_rays_device(d_rays.data_ptr(), len(rays), d_hits2.data_ptr(), any_hit=any_hit)
        with torch.cuda.stream(stream):
            on_stream = d_hits2.clone()  # a torch op ordered behind the query on the caller's stream
        stream.synchronize()
        assert_equal(_hits(on_stream), host)
        assert_equal(query(be, rays, any_hit), host)  # host arrays on the caller's stream
        be.set_stream(None)
    finally:
        be.release()


def test_a_page_locked_destination_is_filled_in_place():
    rays = rays_of("cornell")[:65]
    be = context(scene("cornell"))
    try:
        out = np.zeros(65, S.RAY_HIT)
        be.pin_host_buffer(out)
        assert query(be, rays, out=out) is out
        assert_equal(out, wanted("cornell", 0, False)[:65])
        be.unpin_host_buffer(out)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- queries and renders

def test_queries_are_invisible_to_renders():
    flags = 0
    sc, rays = scene("cornell"), rays_of("cornell")[:257]
    want = wanted("cornell", 0, False)[:257]

    def play(with_queries):
        be = context(sc, flags=flags)
        try:
            be.render(0, 2)
            if with_queries:
                assert_equal(query(be, rays), want)
            be.render(2, 2)
            if with_queries:
                assert_equal(query(be, rays, any_hit=True), wanted("cornell", 0, True)[:257])
            for k in range(4, 12):  # one-iteration calls of a caller that waits: rendered ahead of
                be.render(k, 1)
                be.synchronize()
                if with_queries:
                    assert_equal(query(be, rays[:65]), want[:65])
            return state(be)
        finally:
            be.release()

    assert_same_state(play(True), play(False))


def test_queries_leave_the_scheduler_statistics():
    be = context(scene("cornell"), flags=backend.FLAG_SCHEDULER_STATS)
    try:
        be.render(0, 2)
        before, checks = be.scheduler_stats(), be.invariant_checks()
        assert before["trips_node"] > 0
        assert_equal(query(be, rays_of("cornell")[:257]), wanted("cornell", 0, False)[:257])
        assert be.scheduler_stats() == before and be.invariant_checks() == checks
    finally:
        be.release()


def test_queries_follow_update_triangles():
    import torch
    sc = scene("cornell")
    tris = U.displaced(sc.triangulation, 7)
    moved = U.moved_scene(sc, tris)
    rays = rays_of("cornell")[:257]
    want_moved = Q.expected_hits(moved, rays)
    assert not np.array_equal(Q.words(want_moved), Q.words(wanted("cornell", 0, False)[:257]))  # (the triangles did move)
    be = context(sc)
    try:
        d_rays, before = _tensors(rays)
        after = torch.full_like(before, -1.0)
        torch.cuda.synchronize()
        be.query_rays_device(d_rays.data_ptr(), len(rays), before.data_ptr())  # not waited for: the update must
        be.update_triangles(tris)
        be.query_rays_device(d_rays.data_ptr(), len(rays), after.data_ptr())
        be.synchronize()
        assert_equal(_hits(before), wanted("cornell", 0, False)[:257])
        assert_equal(_hits(after), want_moved)  # triangle_id still indexes the array the caller uploaded
        assert_equal(query(be, rays, any_hit=True), Q.expected_hits(moved, rays, any_hit=True))
    finally:
        be.release()


def test_two_listed_devices_answer_like_one():
    rays = rays_of("cornell")[:257]
    be = context(scene("cornell"), devices=[0, 0])
    try:
        be.render(0, 3)
        for any_hit in (False, True):
            assert_equal(query(be, rays, any_hit), wanted("cornell", 0, any_hit)[:257])
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- errors

def test_errors_leave_the_context_rendering():
    sc, rays = scene("cornell"), rays_of("cornell")[:64]
    lib = backend.load_library()
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        hits = np.zeros(64, S.RAY_HIT)
        with pytest.raises(PtmiError) as e:
            query(be, rays)
        assert e.value.code == STATE and "before ptmi_initialize_memory" in str(e.value)
        with pytest.raises(PtmiError) as e:
            be.query_rays_device(256, 1, 512)
        assert e.value.code == STATE
        be.initialize_memory(sc)
        be.render(0, 3)
        baseline = state(be)

        def refused(rc):
            assert rc == INVALID_ARGUMENT and len(lib.ptmi_last_error(be._ctx)) > 0
            be.clear()
            be.render(0, 3)
            assert_same_state(state(be), baseline)

        p_rays, p_hits = rays.ctypes.data, hits.ctypes.data
        refused(lib.ptmi_query_rays(be._ctx, 2, p_rays, 64, p_hits))
        refused(lib.ptmi_query_rays(be._ctx, 0, p_rays, 64, None))
        refused(lib.ptmi_query_rays(be._ctx, 0, None, 64, p_hits))
        refused(lib.ptmi_query_rays_device(be._ctx, 2, p_rays, 64, p_hits))
        refused(lib.ptmi_query_rays_device(be._ctx, 0, None, 64, p_hits))
        d_rays, d_hits = _tensors(rays)
        refused(lib.ptmi_query_rays_device(be._ctx, 0, d_rays.data_ptr() + 4, 63, d_hits.data_ptr()))
        refused(lib.ptmi_query_rays_device(be._ctx, 1, d_rays.data_ptr(), 63, d_hits.data_ptr() + 8))
        assert (d_hits.cpu().numpy() == -1).all()  # nothing was launched
        assert lib.ptmi_query_rays(be._ctx, 0, None, 0, None) == 0 and lib.ptmi_query_rays_device(be._ctx, 1, None, 0, None) == 0
        assert lib.ptmi_query_rays(be._ctx, 7, None, 0, None) == INVALID_ARGUMENT  # (a bad kind is refused whatever the count)
        assert_equal(query(be, rays), wanted("cornell", 0, False)[:64])  # ... and a good query still works
    finally:
        be.release()
