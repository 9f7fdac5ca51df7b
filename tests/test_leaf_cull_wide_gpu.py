"""The wavefront kernel culls the leaves of BOTH tiers of the certificate under the wide rule (csrc/leaf_cull.h, kernel_wavefront.hip:
node_step), and nothing else changes: image, sample counts, the three histograms and the counters equal the CPU oracle's word
for word, in both arithmetics, plain and general shading, with PTMI_LEAF_CULL unset (both tiers), =3 (the level that masks the
wide bits out) and =0 (the instantiations without culling code).

Scenes: the random scene of tests/test_leaf_cull_gpu.py (its oracle renders are shared), a scene of 4096 slivers none of whose
leaves the tight tier certifies and more than 1024 of whose leaves the wide tier does (tests/test_leaf_cull_wide_model.py asserts
both on the CPU) - so that the upload's gate opens on wide-only leaves - and, for the workgroups of 64 lanes, the deep tree of
tests/test_node_step_waits_gpu.py.  That the wide tier does anything is read off the scheduler statistics.
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, bvh_create
import leaf_cull_wide_cases as KW
import oracle_ffi as O
import test_leaf_cull_gpu as G
import test_leaf_cull_pushed_gpu as P
import test_node_step_waits_gpu as D

pytestmark = pytest.mark.gpu
W, H, DEPTH, SPP = G.W, G.H, G.DEPTH, G.SPP
DA, STATS = G.DA, G.STATS
LEVELS = (None, "3", "0")  # unset: both tiers; 3: the tight bits alone; 0: never
_slivers = {}


def sliver_scene():
    if "scene" not in _slivers:
        _slivers["scene"] = bvh_create(KW.sliver_scene(4096, W, H))
    return _slivers["scene"]


def sliver_oracle(da):
    """One oracle render per arithmetic, shared by the tests and left unchanged."""
    if da not in _slivers:
        color, count, hists, totals = O.oracle_render(sliver_scene(), W, H, DEPTH, SPP, default_arithmetic=da)
        _slivers[da] = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals)
    return _slivers[da]


def scene_and_oracle(name, da):
    return (sliver_scene(), sliver_oracle(da)) if name == "slivers4096" else (G.scene(name), G.oracle(name, da))


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("generic", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("name", ["rand4096", "slivers4096"])
def test_every_level_renders_the_oracle(name, generic, da, monkeypatch):
    sc, want = scene_and_oracle(name, da)
    for level in LEVELS:
        got = P.render(sc, monkeypatch, level, flags=DA if da else 0, generic=generic)
        G.assert_same(got, want)
        assert got["counters"] == want["counters"], (level, got["counters"], want["counters"])


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_deep_tree_in_workgroups_of_64_lanes_renders_the_oracle_at_every_level(da, monkeypatch):
    sc, want = D.deep_scene(), D.deep_oracle(da)
    monkeypatch.delenv("PTMI_GENERIC_SHADING", raising=False)
    for level in LEVELS:
        if level is None:
            monkeypatch.delenv("PTMI_LEAF_CULL", raising=False)
        else:
            monkeypatch.setenv("PTMI_LEAF_CULL", level)
        be = Backend().setup_context(W, H, DEPTH, sc.lightsSize, flags=DA if da else 0)
        try:
            be.initialize_memory(sc)
            be.render(0, SPP)
            color, count = be.read_image()
            got = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[s.copy() for s in be.read_statistics()], counters=be.counters())
            grid = be.scheduler_stats()
        finally:
            be.release()
        assert grid["workgroup_lanes"] == 64, (level, grid)
        G.assert_same(got, want)


@pytest.fixture(scope="module")
def sliver_scheduler_by_level():
    """The sliver scene with scheduler statistics at every level (one render each)."""
    mp = pytest.MonkeyPatch()
    try:
        return {level: P.render(sliver_scene(), mp, level, flags=STATS | DA) for level in LEVELS}
    finally:
        mp.undo()


def test_the_wide_tier_saves_leaf_passes_where_the_tight_one_certifies_nothing(sliver_scheduler_by_level):
    st = sliver_scheduler_by_level
    trips = {level: st[level]["scheduler"]["trips_triangle"] for level in LEVELS}
    print("sliver scene, trips_triangle at PTMI_LEAF_CULL = unset / 3 / 0:", [trips[level] for level in LEVELS])
    print("sliver scene, lanes_triangle at PTMI_LEAF_CULL = unset / 3 / 0:", [st[level]["scheduler"]["lanes_triangle"] for level in LEVELS])
    for level in LEVELS:
        G.assert_same(st[level], sliver_oracle(True))
        assert st[level]["scheduler"]["leaf_item_violations"] == 0
        assert st[level]["counters"]["triangle_tests"] <= st[level]["scheduler"]["lanes_triangle"]
    assert trips[None] < trips["3"]
    assert trips["3"] <= trips["0"]


def test_the_gate_opens_on_leaves_of_the_wide_tier_alone(monkeypatch):
    """Unset, the upload's gate (1024 cullable leaves, of either tier) lets the sliver scene cull: fewer leaf passes than at 0,
    as forced to 2 - read off the statistics build, which masks the records' bits with DScene::leaf_cull."""
    got = {level: P.render(sliver_scene(), monkeypatch, level, flags=STATS | DA)["scheduler"]["trips_triangle"] for level in (None, "2", "0")}
    assert got[None] < got["0"] and got["2"] < got["0"], got
