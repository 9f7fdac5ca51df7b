"""Leaves beyond the limit that a node step would PUSH are counted where they would be pushed (kernel_wavefront.hip: node_step,
closest-hit queries only), the box distances come from the box tests' own slab differences (csrc/leaf_cull.h:
box_distance2_from_slabs), and nothing else changes: PTMI_LEAF_CULL=2 (direct and pushed leaves, forced) and the switch left
unset (the upload's gate; where it culls, it culls both) give the oracle's image, counts, histograms and counters bit for bit,
in both arithmetics and both shadings, and the counters of =0 (never cull) and =1 (direct leaves only).

What would catch a pushed leaf counted early in a SHADOW query: these small scenes do cull in shadow queries (72 direct leaves
in a 1-in-49 pixel sample of the random scene, CPU model), a shadow query ends at its first accepted triangle with the leaves on
its stack uncounted, so a count taken at the push would raise `triangle_tests` above the oracle's in every scene below whose
shadow rays are ever blocked - the comparison of `shadow_rays` and `triangle_tests` with the oracle is that check.

Scenes, shapes and the oracle renders are tests/test_leaf_cull_gpu.py's (one oracle render per scene and arithmetic, shared).
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, backend
import test_leaf_cull_gpu as G

pytestmark = pytest.mark.gpu
W, H, DEPTH, SPP = G.W, G.H, G.DEPTH, G.SPP
DA, STATS = G.DA, G.STATS
LEVELS = ("2", None, "1", "0")  # None: unset


def render(sc, monkeypatch, setting, flags=0, generic=False, update_from=None):
    """G.render with the switch at any of its settings.  update_from: upload that scene first and reach `sc` through
    ptmi_update_triangles."""
    if setting is None:
        monkeypatch.delenv("PTMI_LEAF_CULL", raising=False)
    else:
        monkeypatch.setenv("PTMI_LEAF_CULL", setting)
    if generic:
        monkeypatch.setenv("PTMI_GENERIC_SHADING", "1")
    else:
        monkeypatch.delenv("PTMI_GENERIC_SHADING", raising=False)
    be = Backend().setup_context(W, H, DEPTH, sc.lightsSize, flags=flags)
    try:
        be.initialize_memory(sc if update_from is None else update_from)
        if update_from is not None:
            be.render(0, 1)
            be.update_triangles(sc.triangulation)
            be.clear()
        be.render(0, SPP)
        color, count = be.read_image()
        out = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[s.copy() for s in be.read_statistics()], counters=be.counters())
        if flags & STATS:
            out["scheduler"] = be.scheduler_stats()
            out["reason"] = be.literal_kernel_reason()
        return out
    finally:
        be.release()


CASES = [(name, generic) for name in ("rand4096", "slivers", "big_leaf", "nan_records") for generic in (False, True)]


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("name,generic", CASES, ids=[f"{n}-{'general' if g else 'plain'}" for n, g in CASES])
def test_every_level_renders_the_oracle(name, generic, da, monkeypatch):
    """Forced to 2 and unset: the oracle's results; and the counters of =1 and =0 (see the module's text on shadow queries)."""
    flags = DA if da else 0
    got = {level: render(G.scene(name), monkeypatch, level, flags=flags, generic=generic) for level in LEVELS}
    for level in ("2", None):
        G.assert_same(got[level], G.oracle(name, da))
    for level in LEVELS:
        assert got[level]["counters"] == got["0"]["counters"], (level, got[level]["counters"], got["0"]["counters"])


@pytest.mark.parametrize("generic", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_every_level_after_update_triangles(da, generic, monkeypatch):
    """`moved`, reached through ptmi_update_triangles: the refit's bits serve the rule at the push as they serve the direct one."""
    flags = DA if da else 0
    got = {level: render(G.scene("moved"), monkeypatch, level, flags=flags, generic=generic, update_from=G.scene("rand4096")) for level in LEVELS}
    for level in ("2", None):
        G.assert_same(got[level], G.oracle("moved", da))
    for level in LEVELS:
        assert got[level]["counters"] == got["0"]["counters"], (level, got[level]["counters"], got["0"]["counters"])


@pytest.fixture(scope="module")
def scheduler_by_level():
    """The random scene with scheduler statistics at every setting of the switch (one render each for the tests below)."""
    mp = pytest.MonkeyPatch()
    try:
        return {level: render(G.scene("rand4096"), mp, level, flags=STATS | DA) for level in LEVELS}
    finally:
        mp.undo()


def test_pushed_leaves_save_leaf_passes(scheduler_by_level):
    """Strictly fewer leaf passes with each level.  The CPU model on this scene (a 1-in-49 pixel sample, default arithmetic): 348
    of 1177 popped closest-hit leaves satisfy the rule when they are pushed and carry 1066 of 15532 triangle tests, beside the
    3216 of the direct leaves - a third again of what the direct rule saves, not a margin."""
    st = scheduler_by_level
    trips = {level: st[level]["scheduler"]["trips_triangle"] for level in LEVELS}
    print("trips_triangle at PTMI_LEAF_CULL = 2 / unset / 1 / 0:", [trips[level] for level in LEVELS])
    print("lanes_triangle at PTMI_LEAF_CULL = 2 / unset / 1 / 0:", [st[level]["scheduler"]["lanes_triangle"] for level in LEVELS])
    for level in LEVELS:
        G.assert_same(st[level], G.oracle("rand4096", True))
        assert st[level]["scheduler"]["leaf_item_violations"] == 0
        # every counted triangle test is still accounted for as a lane of triangle work (a counted leaf's triangles are added)
        assert st[level]["counters"]["triangle_tests"] <= st[level]["scheduler"]["lanes_triangle"] <= 1.2 * st[level]["counters"]["triangle_tests"]
    assert trips["2"] < trips["1"] < trips["0"]
    assert trips[None] < trips["1"]  # unset: the gate lets this scene cull, and then it culls both


def test_scene_of_nan_records_deals_out_the_same_at_level_2(monkeypatch):
    on = render(G.scene("nan_records"), monkeypatch, "2", flags=STATS | DA)
    off = render(G.scene("nan_records"), monkeypatch, "0", flags=STATS | DA)
    assert on["reason"]  # (the scene does run the NaN-safe code, whose records carry no bits)
    assert on["scheduler"]["lanes_triangle"] == off["scheduler"]["lanes_triangle"]


def test_big_leaf_counters_at_every_level(monkeypatch):
    got = [render(G.scene("big_leaf"), monkeypatch, level, flags=STATS | DA)["counters"] for level in LEVELS]
    assert got[0] == got[1] == got[2] == got[3]
