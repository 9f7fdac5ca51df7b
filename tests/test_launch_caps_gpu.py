"""Calls cut into launches of 1, 2 or 3 iterations (GPU).

ptmi_setup_context caps the iterations of one launch so that its staging stays within 4 GiB: 32 up to about 6.7 M pixels,
3 or fewer from about 53.7 M pixels on (8192 x 8192: 3, 16384 x 8192: 1).  Below a cap of four every launch of a call is
SHORT - on a stream and a stage set of its own - which is where the stage sets used to be left unallocated
(csrc/stage_sets.h, csrc/launch_schedule.h, tests/test_launch_schedule_model.py).  PTMI_ITERATIONS_PER_LAUNCH lowers the cap of a small image to reach
those plans cheaply; the last two tests render at the sizes that take them without it.

Every iteration's paths are deterministic and staged results are added in iteration order, so image bits, counts, histograms
and counters do not depend on how a call is cut into launches, on the stage set a launch takes, or on whether it ran ahead:
they must equal the per-iteration oracle model of tests/test_api_fuzz_gpu.py, or the run at the full cap of 32."""
import numpy as np
import pytest

import cases
import oracle_ffi as O
from opencl_pathtracer_amd import Backend, backend, structs as S
from test_api_fuzz_gpu import D, H, N_IDS, W, Model, per_iteration  # noqa: F401  (per_iteration: the fixture)
from test_render_ahead_gpu import SEQUENCES, _play, _same

pytestmark = pytest.mark.gpu
DA = backend.FLAG_DEFAULT_ARITHMETIC
LOW_CAPS = [1, 2, 3]


def _cap(monkeypatch, cap):
    """The cap of the contexts set up from here on (None: the one setup computes)."""
    if cap is None:
        monkeypatch.delenv("PTMI_ITERATIONS_PER_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("PTMI_ITERATIONS_PER_LAUNCH", str(cap))


def _check(be, m, what):
    color, count = be.read_image()
    assert np.array_equal(count, m.count), f"sample counts: {what}"
    assert np.array_equal(color.view(np.uint32), m.color.view(np.uint32)), f"image bits: {what}"
    got = be.read_statistics()
    assert all(np.array_equal(a.astype(np.int64), b) for a, b in zip(got, m.stats)), f"histograms: {what}"
    assert be.counters() == m.totals, f"counters: {what}"


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("scene", ["cornell", "fuzz5h_l1"])  # (fuzz5h_l1: NaN-distance records, the NANSAFE instantiation)
@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5, 32])
def test_single_calls_equal_the_oracle(cap, scene, da, per_iteration, monkeypatch):
    """Calls of whole multiples of the cap one after the other (which continue: launches ahead of them at the lowest caps),
    then every n in 1 .. 2 cap + 1 at a few first ids, each call alone: bit for bit the per-iteration model.  Fresh contexts
    where a call must not find stage sets that an earlier call of another shape has allocated."""
    sc, per_it = per_iteration[scene, da]
    _cap(monkeypatch, cap)

    def fresh():
        be = Backend().setup_context(W, H, D, sc.lightsSize, S.JITTERED, flags=DA if da else 0)
        try:
            be.initialize_memory(sc)
        except Exception:
            be.release()
            raise
        return be

    for mult in (1, 2):
        step = mult * cap
        be = fresh()
        try:
            m = Model(per_it)
            for c in range(min(6, N_IDS // step)):
                be.render(c * step, step)
                be.synchronize()
                for k in range(c * step, (c + 1) * step):
                    m.add(k)
                _check(be, m, f"call {c} of {step} at cap {cap}")
        finally:
            be.release()
    shared = None
    try:
        for first in ((0, 7, 19) if cap < 32 else (0,)):
            for n in range(1, min(2 * cap + 1, N_IDS - first) + 1):
                be = fresh() if first == 0 else (shared := shared or fresh())
                try:
                    be.clear()
                    be.render(first, n)
                    m = Model(per_it)
                    for k in range(first, first + n):
                        m.add(k)
                    _check(be, m, f"render({first}, {n}) at cap {cap}")
                finally:
                    if be is not shared:
                        be.release()
    finally:
        if shared is not None:
            shared.release()


@pytest.mark.parametrize("flags, depth", [(DA | backend.FLAG_NO_HISTOGRAMS, 4), (DA | backend.FLAG_SCHEDULER_STATS, 4), (DA, 64)],
                         ids=["no_histograms", "scheduler_stats", "depth64"])
def test_statistics_paths_at_low_caps(flags, depth, scene_factory, monkeypatch):
    """Where a launch stages no statistics words (stats_of() is null) and nothing renders ahead: the same as at cap 32."""
    w, h = 64, 48
    sc = scene_factory("cornell", w, h)
    calls = SEQUENCES["jumps"] + SEQUENCES["pairs_then_triples"]
    _cap(monkeypatch, 32)
    want = _play(sc, w, h, depth, calls, flags, monkeypatch, ahead=2)
    for cap in LOW_CAPS:
        _cap(monkeypatch, cap)
        _same(_play(sc, w, h, depth, calls, flags, monkeypatch, ahead=2), want)


@pytest.mark.parametrize("devices", [None, [0, 0], [0, 0, 0]], ids=["one", "two", "three"])
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_render_ahead_sequences_at_low_caps(name, devices, scene_factory, monkeypatch):
    """Every sequence of tests/test_render_ahead_gpu.py at caps 1 - 3, with and without launches ahead: every read, the counters
    after every call and the final state equal the cap-32 run without them, bit for bit, on the same device list."""
    scene, _, w, h, d = cases.CASES["cornell_64x48_d4"]
    sc = scene_factory(scene, w, h)
    _cap(monkeypatch, 32)
    want = _play(sc, w, h, d, SEQUENCES[name], DA, monkeypatch, ahead=0, devices=devices)
    for cap in LOW_CAPS:
        _cap(monkeypatch, cap)
        for ahead in (0, 2):
            _same(_play(sc, w, h, d, SEQUENCES[name], DA, monkeypatch, ahead=ahead, devices=devices), want)


@pytest.mark.parametrize("scene", ["cornell", "fuzz5h_l1"])
@pytest.mark.parametrize("cap", LOW_CAPS)
def test_bursts_at_low_caps(cap, scene, per_iteration, monkeypatch):
    """ptmi_render_snapshots: every slot holds the image after its iteration, bit for bit."""
    sc, per_it = per_iteration[scene, True]
    _cap(monkeypatch, cap)
    be = Backend().setup_context(W, H, D, sc.lightsSize, S.JITTERED, flags=DA)
    ring = backend.USER_SNAPSHOT_SLOTS
    try:
        be.initialize_memory(sc)
        m = Model(per_it)
        for first, n, slot in ((0, 1, 0), (1, 2 * cap, 3), (1 + 2 * cap, 7, ring - 2), (20, 3 * cap + 1, 10)):
            be.render_snapshots(first, n, slot)
            want = []
            for k in range(n):
                m.add(first + k)
                want.append(((slot + k) % ring, m.color.copy(), m.count.copy()))
            for s, color, count in want:
                got_color, got_count = be.read_snapshot(s)
                assert np.array_equal(got_count, count), (cap, first, n, s)
                assert np.array_equal(got_color.view(np.uint32), color.view(np.uint32)), (cap, first, n, s)
        _check(be, m, f"after the bursts at cap {cap}")
    finally:
        be.release()


@pytest.mark.parametrize("per_launch", ["one", "cap"])
@pytest.mark.parametrize("cap", LOW_CAPS)
def test_run_kernel_at_low_caps(cap, per_launch, per_iteration, monkeypatch):
    """The reference's loop (one image per call, or the cap's worth), which the library renders ahead of."""
    sc, per_it = per_iteration["cornell", True]
    _cap(monkeypatch, cap)
    monkeypatch.delenv("PTMI_RENDER_AHEAD", raising=False)
    be = Backend().setup_context(W, H, D, sc.lightsSize, S.JITTERED, flags=DA)
    be.initialize_memory(sc)
    images = 11
    color, count, stats, _ = be.run_kernel(num_images_to_render=images, images_per_launch=1 if per_launch == "one" else cap)
    m = Model(per_it)
    for k in range(images):
        m.add(k)
    assert np.array_equal(count, m.count) and np.array_equal(color.view(np.uint32), m.color.view(np.uint32))
    assert all(np.array_equal(a.astype(np.int64), b) for a, b in zip(stats, m.stats))


@pytest.mark.parametrize("cap", LOW_CAPS)
def test_samplers_and_super_sampling_at_low_caps(cap, scene_factory, monkeypatch):
    """RANDOM (nothing staged; its colour sums are atomic: counts and counters exactly, colours closely) and SUPER_SAMPLING
    (one iteration per launch whatever the cap; bit for bit): unchanged from cap 32."""
    scene, _, w, h, d = cases.CASES["cornell_64x48_d4"]
    sc = scene_factory(scene, w, h)
    calls = SEQUENCES["jumps"]
    _cap(monkeypatch, 32)
    b = _play(sc, w, h, d, calls, DA, monkeypatch, ahead=2, sampler=S.RANDOM)
    _cap(monkeypatch, cap)
    a = _play(sc, w, h, d, calls, DA, monkeypatch, ahead=2, sampler=S.RANDOM)
    assert np.array_equal(a[2], b[2]) and a[4] == b[4] and np.allclose(a[1], b[1], rtol=1e-4, atol=1e-5)

    def super_sampled():
        be = Backend().setup_context(w, h, d, sc.lightsSize, S.JITTERED, super_sampling=True, flags=DA)
        try:
            be.initialize_memory(sc)
            for first, n in ((0, 1), (1, 1), (2, 5), (7, 2 * cap), (7 + 2 * cap, 1)):
                be.render(first, n)
                be.synchronize()
            return be.read_image(), be.read_variance(), be.read_statistics(), be.counters()
        finally:
            be.release()

    _cap(monkeypatch, 32)
    want = super_sampled()
    _cap(monkeypatch, cap)
    got = super_sampled()
    assert np.array_equal(got[0][0].view(np.uint32), want[0][0].view(np.uint32)) and np.array_equal(got[0][1], want[0][1])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert all(np.array_equal(x, y) for x, y in zip(got[2], want[2])) and got[3] == want[3]


def _setup_cap(w, h):
    """ptmi_setup_context's cap for a JITTERED image of w x h."""
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    return max(1, min(32, 0xFFFFFFF0 // (tiles * 64), (4 << 30) // (w * h * 20)))


@pytest.mark.parametrize("w, h, cap, calls", [
    (8192, 8192, 3, [(0, 3), (3, 3), (6, 1), (7, 1), (8, 1), (9, 2)]),
    (16384, 8192, 1, [(0, 1), (1, 1), (2, 1), (3, 1)]),
], ids=["8192x8192_cap3", "16384x8192_cap1"])
def test_real_sizes_with_low_caps(w, h, cap, calls, monkeypatch):
    """No override: the sizes whose own cap is 3 and 1, in call patterns that used to stage into unallocated sets.  Size-
    independent properties over the whole image, and a seeded sample of pixels (the corners, the last row and column among
    them) bit for bit against the oracle's paths summed in iteration order."""
    import torch
    import warnings
    from opencl_pathtracer_amd import scenes, bvh_create
    assert _setup_cap(w, h) == cap
    _cap(monkeypatch, None)
    d, npix = 2, w * h
    # four stage sets of `cap` iterations, the accumulators, the snapshot-free readback; and room to spare
    need = 4 * cap * npix * 20 + npix * 20 + (1 << 30)
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        pytest.skip(f"{free / 2**30:.1f} GiB free on the device, the test needs {need / 2**30:.1f} GiB")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sc = bvh_create(scenes.cornell_box(w, h))
    be = Backend().setup_context(w, h, d, sc.lightsSize, S.JITTERED, flags=DA)
    try:
        be.initialize_memory(sc)
        for first, n in calls:
            be.render(first, n)
            be.synchronize()
        color, count = be.read_image()
        dep, bbx, tri = be.read_statistics()
        c = be.counters()
    finally:
        be.release()
    iters = sum(n for _, n in calls)
    ids = [first + k for first, n in calls for k in range(n)]
    assert ids == list(range(iters))
    assert (count == iters).all()
    paths = npix * iters
    assert dep.sum() == paths == c["paths"] and bbx.sum() <= paths and tri.sum() <= paths
    k = np.arange(d + 1, dtype=np.int64)
    assert (dep.astype(np.int64) * k).sum() == c["surface_hits"] == c["shadow_rays"]  # one light: one shadow ray per hit
    assert c["surface_hits"] <= c["segments"] <= c["surface_hits"] + paths
    k5 = np.arange(len(bbx), dtype=np.int64)
    assert (bbx.astype(np.int64) * k5).sum() <= c["box_tests"] and c["box_tests"] % 2 == 0  # two box tests per node visit
    assert np.isfinite(color).all() and (color >= 0).all()

    rs = np.random.RandomState(w ^ h)
    xs = list(rs.randint(0, w, 480)) + [0, w - 1, 0, w - 1] + [w - 1] * 8 + list(rs.randint(0, w, 8))
    ys = list(rs.randint(0, h, 480)) + [0, 0, h - 1, h - 1] + list(rs.randint(0, h, 8)) + [h - 1] * 8
    lib = O.oracle(True)
    osc = O.OracleScene(sc, w, h, d)
    import ctypes as C
    bounces, rad = (O.PtoBounce * 64)(), (C.c_float * 4)()
    for x, y in zip(xs, ys):
        acc = np.zeros(4, np.float32)
        for it in ids:
            lib.pto_trace_path(C.byref(osc.c), int(x), int(y), it, bounces, 64, rad)
            acc = acc + np.array(rad[:], np.float32)  # float32 adds in iteration order: what the accumulation does
        assert np.array_equal(color[y, x].view(np.uint32), acc.view(np.uint32)), (x, y, color[y, x], acc)
