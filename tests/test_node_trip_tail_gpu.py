"""The shorter trip choice of the wavefront kernel's traversal loop (csrc/trip_choice.h) changes no result: image, sample counts,
the three histograms and the counters equal the CPU oracle's word for word, in both arithmetics - on the smallest scenes at
which a node trip's tail (push, pop, leaf after leaf) and the choice behind it can go wrong.

PTMI_LEAF_CULL=2 forces the culling instantiations (cull_step), =0 the ones without culling code (node_step);
PTMI_GENERIC_SHADING=1 the general instantiations, which hold the top of the stack in a register.  Scenes:
  one_leaf      the root is a leaf: no node step at all;
  two_leaves    a root with two leaf children: every pop meets the sentinel, and the stack holds 0 or 1 entries;
  chain         a lopsided chain of 22 levels (tests/bvh_stress_cases.py: deep_chain), as deep as five wide workgroups per CU
                allow.  Seen from +x every node's near child is the rest of the chain and its far child a leaf: a push on every
                level, then pops that land on leaf after leaf - each one the second pop of the step or pass before.  Seen from
                -x the near child is the leaf: no stack at all, a leaf child and the sentinel in every step;
                (the chain's coordinates reach 2^27: its records can yield distances that are no numbers, so it runs the
                NANSAFE instantiation);
  big_leaf      a leaf of REF_COUNT_BIG or more triangles, whose range comes from the big leaves' table, inside the closed
                Cornell box: paths scatter to depth 6 and meet it from every side - as the child a step chooses and as the
                one it pushed and pops;
  big_stacks    six such leaves among four hundred random triangles, in the open;
  rand400       four hundred random triangles;
  deep          the deep textured tree of tests/test_node_step_waits_gpu.py: workgroups of 64 lanes, where a level is 256
                bytes and not 1024 (general shading);
  plain_deep    the same tree with plain materials and one point light (tests/test_node_step_diet_gpu.py): the plain
                instantiations of 64 lanes;
  nan_records   zero-area triangles (the NANSAFE instantiation), also in the statistics build.
"""
import copy

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, bvh_create, scenes
import bvh_stress_cases as B
import leaf_cull_cases as K
import oracle_ffi as O
import test_leaf_cull_gpu as G
import test_node_step_diet_gpu as T
import test_node_step_waits_gpu as D

pytestmark = pytest.mark.gpu
W, H, DEPTH, SPP = G.W, G.H, G.DEPTH, G.SPP  # 96 x 96, depth 6, 2 iterations: the shape whose oracle renders the neighbouring files share
DA, STATS = G.DA, G.STATS
LEVELS = ("2", "0")  # forced on: cull_step in the plain instantiations; off: node_step
FROM_PLUS_X = ([14.0, 0.3, 0.2, 1.0], [-1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.0], [0.0, 0.5, 0.0, 0.0])
_scenes, _oracle = {}, {}


def _with(tris, camera=None):
    sc = copy.copy(scenes.random_triangles(16, W, H))
    sc.triangulation = tris
    sc.bvh = None
    if camera is not None:
        sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp = (np.array(v, np.float32) for v in camera)
    return sc


def scene(name):
    if name in _scenes:
        return _scenes[name]
    large = lambda n: K.random_scene(n, W, H, spread=4.0).triangulation  # (triangles that fill the view)
    if name == "one_leaf":
        sc = bvh_create(_with(large(2)))
        assert len(sc.bvh) == 1 and sc.bvh["isLeaf"][0]
    elif name == "two_leaves":
        sc = next(s for s in (bvh_create(_with(large(n))) for n in range(3, 9)) if len(s.bvh) == 3)
        assert not sc.bvh["isLeaf"][0] and int((sc.bvh["isLeaf"] != 0).sum()) == 2
    elif name.startswith("chain"):
        stacks = 21
        sc = bvh_create(_with(B.deep_chain(stacks, 0, 3 * (stacks + 1)), FROM_PLUS_X if name.endswith("+x") else None))
        assert len(sc.bvh) == 2 * stacks + 1 and int((sc.bvh["isLeaf"] != 0).sum()) == stacks + 1  # one level per stack
    elif name == "big_leaf":
        sc = G.scene("big_leaf")
        assert sc.bvh["nbTriangles"][sc.bvh["isLeaf"] != 0].max() >= 7  # REF_COUNT_BIG
    elif name == "big_stacks":
        rs = np.random.RandomState(5)
        parts = [K.random_scene(400, W, H).triangulation]
        for k in range(6):  # 7 to 12 coincident triangles each: one leaf
            a = np.tile(rs.uniform(-4.0, 4.0, (1, 3)).astype(np.float32), (7 + k, 1))
            parts.append(scenes.triangle_create(a, a + np.float32([0, 1.5, 0]), a + np.float32([0, 0, 1.5])))
        sc = bvh_create(_with(scenes._concat_tris(parts)))
        assert int((sc.bvh["nbTriangles"][sc.bvh["isLeaf"] != 0] >= 7).sum()) >= 6
    elif name == "rand400":
        sc = bvh_create(K.random_scene(400, W, H))
    elif name == "deep":
        sc = D.deep_scene()
    elif name == "plain_deep":
        sc = T.plain_deep_scene()
    elif name == "nan_records":
        sc = G.scene("nan_records")
    _scenes[name] = sc
    return sc


def oracle(name, da):
    """One oracle render per (scene, arithmetic), shared by the tests and left unchanged."""
    if name in ("big_leaf", "nan_records"):
        return G.oracle(name, da)
    if name == "deep":
        return D.deep_oracle(da)
    if name == "plain_deep":  # (shared with tests/test_node_step_diet_gpu.py, whichever file runs first)
        if ("plain_deep", da) not in T._flat:
            color, count, hists, totals = O.oracle_render(scene(name), W, H, DEPTH, SPP, default_arithmetic=da)
            T._flat["plain_deep", da] = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals)
        return T._flat["plain_deep", da]
    if (name, da) not in _oracle:
        color, count, hists, totals = O.oracle_render(scene(name), W, H, DEPTH, SPP, default_arithmetic=da)
        _oracle[name, da] = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals)
    return _oracle[name, da]


def render(sc, monkeypatch, level, flags=0, generic=False):
    monkeypatch.setenv("PTMI_LEAF_CULL", level)
    if generic:
        monkeypatch.setenv("PTMI_GENERIC_SHADING", "1")
    else:
        monkeypatch.delenv("PTMI_GENERIC_SHADING", raising=False)
    be = Backend().setup_context(W, H, DEPTH, sc.lightsSize, flags=flags)
    try:
        be.initialize_memory(sc)
        be.render(0, SPP)
        color, count = be.read_image()
        return dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[s.copy() for s in be.read_statistics()], counters=be.counters(),
                    scheduler=be.scheduler_stats(), reason=be.literal_kernel_reason())
    finally:
        be.release()


def test_shape_is_within_the_issues():
    assert 64 <= W <= 96 and 64 <= H <= 96 and DEPTH <= 6 and SPP <= 8


WIDE = ["one_leaf", "two_leaves", "chain", "chain+x", "big_leaf", "big_stacks", "rand400", "nan_records"]
NARROW = ["deep", "plain_deep"]


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("generic", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("name", WIDE + NARROW)
def test_renders_the_oracle_with_culling_forced_on_and_off(name, generic, da, monkeypatch):
    sc, want = scene(name), oracle(name, da)
    for level in LEVELS:
        got = render(sc, monkeypatch, level, flags=DA if da else 0, generic=generic)
        assert got["scheduler"]["workgroup_lanes"] == (64 if name in NARROW else 256), (level, got["scheduler"])
        G.assert_same(got, want)
        assert got["counters"] == want["counters"], (level, got["counters"], want["counters"])


def test_the_scenes_are_what_they_are_for():
    """Read off the oracle: the chain seen from +x tests about twice the boxes of the chain seen from -x (it walks down the
    chain pushing, where the other side finds its hit in the first leaf and the boxes behind it fail against the limit), every
    scene's rays reach surfaces, and the one-leaf scene tests no box at all."""
    assert oracle("one_leaf", True)["counters"]["box_tests"] == 0 and oracle("one_leaf", True)["counters"]["triangle_tests"] > 0
    assert oracle("chain+x", True)["counters"]["box_tests"] > 1.5 * oracle("chain", True)["counters"]["box_tests"]
    for name in WIDE + NARROW:
        assert oracle(name, True)["counters"]["surface_hits"] > 0, name


@pytest.mark.parametrize("name", ["nan_records", "rand400", "chain+x"])
def test_statistics_build_keeps_the_item_protocol(name, monkeypatch):
    """As tests/test_parity_gpu.py: every item a lane read was written in its pass, and - in a scene none of whose paths is
    given up and traced again by the literal loops, which deal out no items - every counted triangle test was one item of one
    pass or one triangle of a counted leaf."""
    sc, want = scene(name), oracle(name, True)
    got = render(sc, monkeypatch, "2", flags=DA | STATS)
    G.assert_same(got, want)
    st = got["scheduler"]
    assert st["leaf_item_violations"] == 0
    assert (got["reason"] is not None) == (name != "rand400"), got["reason"]  # (records that can yield NaN distances: the NANSAFE path)
    if got["reason"] is None:
        assert got["counters"]["triangle_tests"] <= st["lanes_triangle"]
    assert st["trips_node"] > 0
