"""The counting node step of the culling instantiations (kernel_wavefront.hip: cull_step - one count update per step, the
counted children treated as missed, "certified and beyond" as one compare per child) changes no result: image, sample counts,
the three histograms and the counters equal the CPU oracle's word for word, in both arithmetics, plain and general shading, with
PTMI_LEAF_CULL unset (both tiers), =3 (the tight tier's bits alone) and =0 (the instantiations without culling code).

Scenes (the pattern and helpers of tests/test_leaf_cull_wide_gpu.py, whose oracle renders are shared): the random scene of 4096
triangles; the 4096 slivers whose leaves the wide tier alone certifies; the deep tree that runs in workgroups of 64 lanes -
as it is (textured: the general instantiation, whatever the switch says) and with plain materials and one point light (the
plain instantiation of 64 lanes, which the textured tree never reaches); and
the random scene seen by a camera whose right and up vectors both lie along z, so that EVERY camera ray has a zero y component
(+0 or -0): those rays need the literal box test, their waves take the step's other branch, and the waves of the scattered rays
behind them - ordinary directions - mix both.
"""
import copy

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, bvh_create, structs as S
import leaf_cull_cases as K
import oracle_ffi as O
import test_leaf_cull_gpu as G
import test_leaf_cull_pushed_gpu as P
import test_leaf_cull_wide_gpu as WG
import test_node_step_waits_gpu as D

pytestmark = pytest.mark.gpu
W, H, DEPTH, SPP = G.W, G.H, G.DEPTH, G.SPP
DA = G.DA
LEVELS = WG.LEVELS
_flat = {}


def flat_camera_scene():
    if "scene" not in _flat:
        sc = copy.copy(K.random_scene(4096, W, H))
        sc.cameraPosition = np.array([-14.0, 0.0, 0.0, 1.0], np.float32)
        sc.cameraDirection = np.array([1.0, -0.0, 0.0, 0.0], np.float32)
        sc.cameraRight = np.array([0.0, 0.0, 0.5, 0.0], np.float32)
        sc.cameraUp = np.array([0.0, 0.0, 0.3, 0.0], np.float32)
        _flat["scene"] = bvh_create(sc)
    return _flat["scene"]


def flat_camera_oracle(da):
    """One oracle render per arithmetic, shared by the tests and left unchanged."""
    if da not in _flat:
        color, count, hists, totals = O.oracle_render(flat_camera_scene(), W, H, DEPTH, SPP, default_arithmetic=da)
        _flat[da] = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals)
    return _flat[da]


def scene_and_oracle(name, da):
    return (flat_camera_scene(), flat_camera_oracle(da)) if name == "flat_camera" else WG.scene_and_oracle(name, da)


def test_shape_is_the_issues():
    assert (W, H, DEPTH, SPP) == (96, 96, 6, 2)


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("generic", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("name", ["rand4096", "slivers4096", "flat_camera"])
def test_every_level_renders_the_oracle(name, generic, da, monkeypatch):
    sc, want = scene_and_oracle(name, da)
    for level in LEVELS:
        got = P.render(sc, monkeypatch, level, flags=DA if da else 0, generic=generic)
        G.assert_same(got, want)
        assert got["counters"] == want["counters"], (level, got["counters"], want["counters"])


def test_flat_camera_rays_need_the_literal_box_test_and_hit_the_scene():
    """What the scene is for.  Every camera ray is direction + x * right + y * up, and the y components of all three are zero:
    the rays' d.y is +0 or -0, their reciprocal is infinite, and a ray with an infinite reciprocal is marked for the literal
    box test where its query starts (kernel_wavefront.hip: start_query, ray_slabs_are_ordered) - a wave that holds one takes the
    step's literal branch (wave_exact).  Every wave of the first trips holds nothing else.  That those rays traverse at all is
    read off the oracle: the rays with d.y = -0 reach surfaces (a +0 component fails every box, FullKernel.cl:79-83), are shaded
    and scatter, and the waves behind them mix both kinds of ray.  (The branch itself leaves no mark in the results: the
    statistics build keeps the parent's step, and the production kernels count nothing per branch.)"""
    sc = flat_camera_scene()
    for v in (sc.cameraDirection, sc.cameraRight, sc.cameraUp):
        assert v[1] == 0.0
    want = flat_camera_oracle(True)
    assert want["counters"]["surface_hits"] > 0 and want["counters"]["shadow_rays"] > 0


def plain_deep_scene():
    """The deep tree (23 levels: workgroups of 64 lanes) with materials and lights a plain-shading launch admits - every
    material STANDART with a simple colour, one point light - so that the PLAIN instantiation of 64 lanes runs, which the
    textured stand-in never reaches."""
    if "plain_deep" not in _flat:
        sc = copy.copy(D.deep_scene())
        m = sc.materiaux.copy()
        m["type"] = S.MAT_STANDART
        m["isSimpleColor"] = 1
        sc.materiaux = m
        point = [i for i in range(len(sc.lights)) if sc.lights["type"][i] == S.LIGHT_POINT]
        sc.lights = sc.lights[point[:1]].copy()
        assert sc.lightsSize == 1
        _flat["plain_deep"] = sc
    return _flat["plain_deep"]


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_plain_deep_tree_in_workgroups_of_64_lanes_renders_the_oracle_at_every_level(da, monkeypatch):
    sc = plain_deep_scene()
    if ("plain_deep", da) not in _flat:
        color, count, hists, totals = O.oracle_render(sc, W, H, DEPTH, SPP, default_arithmetic=da)
        _flat["plain_deep", da] = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals)
    want = _flat["plain_deep", da]
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
        assert got["counters"] == want["counters"], (level, got["counters"], want["counters"])
