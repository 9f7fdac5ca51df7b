"""The wavefront kernel reads the scene's rare fields - sky, camera, histogram and counter pointers - through the global address
space, so that the node step's waits follow its four record loads one by one (tests/test_node_step_waits.py pins the waits on
the CPU).  Nothing in the results may move: image, sample counts, the three histograms and the totals equal the oracle's bit for
bit, in both arithmetics, plain and general shading, with the culling instantiations (PTMI_LEAF_CULL unset) and the ones
without culling code (=0) - eight of the twelve production instantiations between them on the random scene, and the workgroups
of 64 lanes on a deep tree.

Scenes, shapes and the oracle renders of the random scene are tests/test_leaf_cull_gpu.py's (one oracle render per scene and
arithmetic, shared with its tests).

The deep tree: the launch takes workgroups of 64 lanes from 23 levels on, and only in the instantiations without the NaN
check.  The trees of that depth among tests/bvh_stress_cases.py (deep_chain's 27 and 200 levels, clusters_exp's 24 at 300 000
triangles) are made of coordinates beyond 2^21, which the upload answers with the NaN-safe kernel in wide workgroups - they
cannot reach the narrow ones.  So the deep scene is the one tests/test_reference_default_gpu.py already uses for them: the
configs[4] stand-in (23 levels), at this module's image size.  Its materials are textured: general shading, whatever the
switch says.  (Chains that do reach the narrow workgroups, with every level of their stack in use: the hand-made decks of
tests/test_stack_depth_gpu.py, whose coordinates stay small.)
"""
import os

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, bvh_create, scenes
import oracle_ffi as O
import test_leaf_cull_gpu as G
import test_leaf_cull_pushed_gpu as P

pytestmark = pytest.mark.gpu
W, H, DEPTH, SPP = G.W, G.H, G.DEPTH, G.SPP
DA = G.DA
CULL = (None, "0")  # unset: the upload's gate (these scenes cull); 0: the instantiations without culling code
_deep = {}


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("generic", [False, True], ids=["plain", "general"])
def test_random_scene_renders_the_oracle(generic, da, monkeypatch):
    want = G.oracle("rand4096", da)
    for setting in CULL:
        got = P.render(G.scene("rand4096"), monkeypatch, setting, flags=DA if da else 0, generic=generic)
        G.assert_same(got, want)


def deep_scene():
    if "scene" not in _deep:
        _deep["scene"] = bvh_create(scenes.build("mayalike", W, H))
        assert _deep["scene"].bvhMaxDepth >= 23
    return _deep["scene"]


def deep_oracle(da):
    if da not in _deep:
        color, count, hists, totals = O.oracle_render(deep_scene(), W, H, DEPTH, SPP, default_arithmetic=da)
        _deep[da] = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals)
    return _deep[da]


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_deep_tree_in_workgroups_of_64_lanes_renders_the_oracle(da, monkeypatch):
    if os.environ.get("PTMI_GENERIC_TRIANGLES"):
        pytest.skip("workgroups of 64 lanes exist for the two production instantiations only (precomputed triangle records)")
    sc, want = deep_scene(), deep_oracle(da)
    monkeypatch.delenv("PTMI_GENERIC_SHADING", raising=False)
    for setting in CULL:
        if setting is None:
            monkeypatch.delenv("PTMI_LEAF_CULL", raising=False)
        else:
            monkeypatch.setenv("PTMI_LEAF_CULL", setting)
        be = Backend().setup_context(W, H, DEPTH, sc.lightsSize, flags=DA if da else 0)
        try:
            be.initialize_memory(sc)
            be.render(0, SPP)
            color, count = be.read_image()
            got = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[s.copy() for s in be.read_statistics()], counters=be.counters())
            grid = be.scheduler_stats()
        finally:
            be.release()
        assert grid["workgroup_lanes"] == 64, (setting, grid)
        G.assert_same(got, want)
