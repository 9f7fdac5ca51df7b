"""ptmi_bvh_create_device on the MI355X against ptmi_bvh_create: the same status, message, nodes, depth and reordered
triangles, compared as bytes (a float compared as a number would take -0 for +0)."""
import ctypes as C
import os

import numpy as np
import pytest

from opencl_pathtracer_amd import backend, scenes, structs as S, bvh_create
import bvh_stress_cases as stress
from test_bvh_device_model import (FUZZ_NAMES, WALL_SEEDS, MODEL_STALE, MODEL_BUILT, cloud_wall, signed_zero_tris, small_tris,
                                   coincident_stack, host_build, assert_case_hits_its_target, model)  # noqa: F401  (model: a fixture)

pytestmark = pytest.mark.gpu
DEVICE = 0


def device_build(tris, device=DEVICE):
    lib = backend.load_library()
    t = np.frombuffer(bytearray(np.ascontiguousarray(tris).tobytes()), dtype=S.Triangle)
    n = len(t)
    nodes = np.zeros(max(2 * n - 1, 1), dtype=S.Node)
    size, depth = C.c_uint32(0), C.c_uint32(0)
    info = backend.BvhBuildInfo()
    rc = lib.ptmi_bvh_create_device(device, t.ctypes.data_as(C.c_void_p), n, nodes.ctypes.data_as(C.c_void_p),
                                    C.byref(size), C.byref(depth), C.byref(info))
    msg = lib.ptmi_last_error(None).decode() if rc else ""
    return rc, msg, nodes[:size.value], t, depth.value, info


def assert_same(tris, what, on_device=True, host=None):
    """`host`: host_build(tris), where the caller has it already"""
    rc, msg, nodes, t, depth, info = device_build(tris)
    hrc, hmsg, hnodes, ht, hdepth = host or host_build(tris)
    assert (rc, msg) == (hrc, hmsg), what
    if on_device:
        assert info.built_on_device == 1 and info.fallback == backend.BVH_FALLBACK_NONE, (what, info.as_dict())
    if rc == 0:
        assert len(nodes) == len(hnodes) and depth == hdepth, what
        assert nodes.tobytes() == hnodes.tobytes(), what
        assert t.tobytes() == ht.tobytes(), what
    return info


NAMED = [("cornell", 64, 48), ("matmix", 96, 96), ("tris20k", 96, 64), ("mayalike_s", 64, 64)] + \
        [("feat_" + f, 64, 64) for f in scenes.FEATURES] + [("tris1m", 160, 90), ("mayalike", 160, 90), ("tris4m", 160, 90)]


@pytest.mark.parametrize("name,w,h", NAMED)
def test_device_tree_equals_host_tree(name, w, h):
    assert_same(scenes.build(name, w, h).triangulation, name)


def test_device_tree_equals_host_tree_fuzzed():
    for name in FUZZ_NAMES:
        assert_same(scenes.build(name, 64, 64).triangulation, name)


def test_device_tree_equals_host_tree_small_and_signed_zeros():
    t = signed_zero_tris()
    assert_same(t, "signed zeros")
    assert_same(t[::-1].copy(), "signed zeros, reversed")
    for n in range(1, 10):
        assert_same(small_tris(n), f"n={n}")
    assert_same(coincident_stack(), "coincident stack")


def test_cloud_and_wall_fall_back_exactly_where_the_model_flags(model):
    stale = []
    for seed in WALL_SEEDS:
        t = cloud_wall(seed)
        info = assert_same(t, f"cloud+wall {seed}", on_device=False)
        flagged = model(np.ascontiguousarray(t))[0] == MODEL_STALE
        assert (info.fallback == backend.BVH_FALLBACK_STALE_AXIS) == flagged, (seed, info.as_dict())
        assert (info.built_on_device == 1) == (info.fallback == backend.BVH_FALLBACK_NONE), seed
        stale.append(flagged)
    assert any(stale)


STRESS_BUILT = [c for c in stress.SMALL + stress.MID + stress.BIG if c[0] != stress.REFUSED]
STRESS_REFUSED = [c for c in stress.SMALL + stress.MID + stress.BIG if c[0] == stress.REFUSED]


def test_stress_table_has_a_device_built_case_in_every_row():
    """Every case of STRESS_BUILT must be built on the device (the test below): a fallback would compare the host builder
    with itself.  So no row of the family table may be missing from it."""
    assert {stress.ROWS[c[0]] for c in STRESS_BUILT} == set(stress.ROWS.values())
    for sizes in (stress.SMALL, stress.MID, stress.BIG):
        assert {c[0] for c in sizes} == set(stress.FAMILIES)


@pytest.mark.parametrize("case", STRESS_BUILT, ids=stress.case_id)
def test_device_tree_equals_host_tree_on_stress_cases(case, model):
    """Tied, structured and lopsided geometry at three sizes: built on the device with no fallback, the host's bytes, one
    launch per level of the tree - and, at the small size, as many levels as the model takes."""
    tris = stress.make(*case)
    host = host_build(tris)
    assert host[0] == 0, (case, host[1])
    assert_case_hits_its_target(case, host[2], host[4])
    info = assert_same(tris, case, host=host)
    assert info.levels == host[4] + 1, (case, info.as_dict())
    if case in stress.SMALL:
        rc, nodes, perm, depth, levels = model(np.ascontiguousarray(tris), with_levels=True)
        assert rc == MODEL_BUILT and info.levels == levels, (case, rc, levels, info.as_dict())


@pytest.mark.parametrize("case", STRESS_REFUSED, ids=stress.case_id)
def test_device_and_host_refuse_a_chain_deeper_than_the_limit(case):
    """300 levels: the kernel flags the node past 8 x PTMI_BVH_MAX_DEPTH, the call hands the scene to the host builder, and the
    caller gets the host builder's status and message."""
    tris = stress.make(*case)
    host = host_build(tris)
    assert host[0] == -5 and "too large to build a tree from" in host[1], host[:2]
    info = assert_same(tris, case, on_device=False, host=host)
    assert info.built_on_device == 0 and info.fallback == backend.BVH_FALLBACK_HOST_ERROR, info.as_dict()


@pytest.mark.parametrize("case", stress.STALE, ids=stress.case_id)
def test_wide_flat_lattices_fall_back_exactly_where_the_model_flags(case, model):
    """The two stress cases the device cannot build (bvh_stress_cases.STALE): the stale-axis fallback, as the model
    flags it, and the host builder's status and message."""
    tris = stress.make(*case)
    info = assert_same(tris, case, on_device=False)
    assert model(np.ascontiguousarray(tris))[0] == MODEL_STALE
    assert info.built_on_device == 0 and info.fallback == backend.BVH_FALLBACK_STALE_AXIS, info.as_dict()


def _repeat_cases():
    return [("lattice", lambda: stress.make("grid3d", 1, 28 ** 3)), ("clusters", lambda: stress.make("clusters_exp", 0, 24000)),
            ("random 300000", lambda: scenes.random_triangles(300000, 32, 32).triangulation)]


@pytest.mark.parametrize("what,make", _repeat_cases(), ids=[w for w, _ in _repeat_cases()])
def test_repeated_device_builds_give_the_same_bytes(what, make):
    """The child slots of a level go to whichever workgroup asks first, so two builds of one scene lay their workspace out
    differently.  Five builds in a row, and one more while a render is in flight on the same device: the same nodes, depth
    and triangle order every time (and the host's)."""
    tris = make()
    host = host_build(tris)
    assert host[0] == 0

    def build():
        rc, msg, nodes, t, depth, info = device_build(tris)
        assert rc == 0 and info.built_on_device == 1 and info.fallback == backend.BVH_FALLBACK_NONE, (what, msg, info.as_dict())
        return nodes.tobytes(), t.tobytes(), depth, info.levels

    first = build()
    assert first[:3] == (host[2].tobytes(), host[3].tobytes(), host[4]), what
    for k in range(4):
        assert build() == first, (what, k)
    w, h = 96, 64
    sc = bvh_create(scenes.build("matmix", w, h))
    be = backend.Backend().setup_context(w, h, 6, len(sc.lights), device=DEVICE)
    try:
        be.initialize_memory(sc)
        be.render(0, 8)
        during = build()
        be.synchronize()
    finally:
        be.release()
    assert during == first, what


def _before_the_largest_cluster(tris):
    """four radii in front of the last (largest, radius 2^20) cluster of clusters_exp in construction order"""
    return tris["AABB"]["centroid"][-(len(tris) // 41):, :3].astype(np.float64).mean(0) - [4 * 2.0 ** 20, 0, 0]


@pytest.mark.parametrize("family,seed,n,eye", [("grid3d", 1, 28 ** 3, lambda tris: (-30.0, 13.5, 13.5)),
                                               ("clusters_exp", 0, 24000, _before_the_largest_cluster)],
                         ids=["grid3d", "clusters_exp"])
def test_image_of_a_device_built_stress_scene_is_the_host_built_one(family, seed, n, eye):
    """4 spp at 96 x 64 of a lattice and of the clusters, once with the device-built tree and once with the host-built one:
    image, sample counts, histograms and counters are the same bytes."""
    w, h, d, spp = 96, 64, 6, 4

    def scene():
        sc = scenes.random_triangles(16, w, h)  # its material, light and sky
        sc.triangulation = stress.make(family, seed, n)
        sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp = scenes.camera(eye(sc.triangulation), (1, 0, 0), (0, 1, 0), (0, 0, h / w))
        return sc

    on_host, on_device = bvh_create(scene()), bvh_create(scene(), device=DEVICE)
    assert on_device.bvh_build_info.built_on_device == 1 and on_device.bvh_build_info.fallback == backend.BVH_FALLBACK_NONE
    assert on_host.bvhMaxDepth < S.BVH_MAX_DEPTH  # (a tree the integrator takes)
    a = backend.render_scene(on_host, w, h, d, spp, device=DEVICE)
    b = backend.render_scene(on_device, w, h, d, spp, device=DEVICE)
    assert a[3]["surface_hits"] > 100  # (an image of the geometry, not of the sky)
    for x, y in zip(a[:2] + tuple(a[2]), b[:2] + tuple(b[2])):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert a[3] == b[3]


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 3e38, -3e38])
def test_boxes_that_are_not_numbers_or_overflow(value):
    t = scenes.build("tris20k", 32, 32).triangulation.copy()
    for k, field in enumerate(("pMin", "pMax", "centroid")):
        t["AABB"][field][1000 + 7 * k, k] = value
    assert_same(t, f"box value {value}", on_device=False)


def test_build_during_a_render_leaves_it_alone():
    """A context renders on the same device while the tree of another scene is built: the image equals one rendered
    without the build, and the calling thread's current device is unchanged."""
    import torch
    w, h = 96, 64
    sc = bvh_create(scenes.build("matmix", w, h))

    def render(with_build):
        be = backend.Backend().setup_context(w, h, 6, len(sc.lights), device=DEVICE)
        be.initialize_memory(sc)
        be.render(0, 8)
        if with_build:
            before = torch.cuda.current_device()
            assert_same(scenes.build("tris20k", 32, 32).triangulation, "during a render")
            assert torch.cuda.current_device() == before
        be.synchronize()
        img = be.read_image()
        be.release()
        return img

    a, b = render(False), render(True)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_python_binding_reports_the_device_build():
    sc = bvh_create(scenes.build("tris20k", 32, 32), device=DEVICE)
    ref = bvh_create(scenes.build("tris20k", 32, 32))
    assert sc.bvh_build_info.built_on_device == 1 and sc.bvh_build_info.levels > 0
    assert sc.bvh.tobytes() == ref.bvh.tobytes() and sc.triangulation.tobytes() == ref.triangulation.tobytes()
    assert sc.bvhMaxDepth == ref.bvhMaxDepth


def test_shim_builds_on_the_device_above_its_threshold(tmp_path):
    """PathTracer_Main through the shim on a scene above the shim's threshold: its log names the device builder, and the
    tree, image and statistics are those of the host-built scene."""
    import subprocess
    import oracle_ffi as O
    from test_shim import DRIVER, dump_scene, read_result
    name, w, h, d, n = "tris20k", 64, 48, 4, 2
    sc = scenes.build(name, w, h)
    scene_file, out_file = str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
    dump_scene(scene_file, sc, w, h, d, S.JITTERED, n)
    r = subprocess.run([DRIVER, scene_file, out_file], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PTMI_LOG": "1", "PTMI_DEVICE": str(DEVICE)})
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"20000 triangles, device builder on device {DEVICE}" in r.stderr, r.stderr[-2000:]
    (callbacks, bvh_size, bvh_depth), color, count, dep, bbx, tri = read_result(out_file, w, h, d)
    ref = bvh_create(scenes.build(name, w, h))
    assert callbacks == n and bvh_size == len(ref.bvh) and bvh_depth == ref.bvhMaxDepth
    o_color, o_count, (o_dep, o_bbx, o_tri), _ = O.oracle_render(ref, w, h, d, n, sampler=S.JITTERED, default_arithmetic=True)
    assert np.array_equal(color.view(np.uint32), o_color.view(np.uint32)) and np.array_equal(count, o_count)
    assert np.array_equal(dep, o_dep) and np.array_equal(bbx, o_bbx) and np.array_equal(tri, o_tri)
