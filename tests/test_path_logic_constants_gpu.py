"""The launch constants a path-logic pass fetches with scalar loads - camera, sky rotation, the one light of the plain kernels
("The pass's memory chain") - against the CPU oracle, bit for bit: image, sample counts, depth histogram, totals.

A scalar load goes through the scalar cache, which vector stores and the host's copies do not update: a constant that outlived
the launch it was fetched in would show as an image of the scene as it WAS.  So the last test changes each of them between
launches of one context - ptmi_set_camera, then a second upload with the light moved and the sky recoloured - and every image
must be the oracle's for the scene as it then is.
"""
import copy

import numpy as np
import pytest

from opencl_pathtracer_amd import backend
import gpu_cases
import oracle_ffi as O
from gpu_cases import cached_scene

pytestmark = pytest.mark.gpu
W, H, DEPTH, ITERATIONS = 64, 64, 4, 3
DA = backend.FLAG_DEFAULT_ARITHMETIC
ARITHMETICS = pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])

_oracle = {}


def oracle_of(sc, key, flags):
    """The oracle's render of `sc`, computed once per (scene as it then is, arithmetic) and left unchanged."""
    k = (key, flags)
    if k not in _oracle:
        color, count, (depths, _, _), totals = O.oracle_render(sc, W, H, DEPTH, ITERATIONS, default_arithmetic=flags == DA)
        _oracle[k] = (color.view(np.uint32), count, depths, totals)
    return _oracle[k]


def assert_equals_oracle(be, sc, key, flags):
    color, count, depths, totals = oracle_of(sc, key, flags)
    got = gpu_cases.state(be)
    differ = int((got["color"] != color).any(axis=-1).sum())
    assert differ == 0, f"{key}: {differ} pixels differ from the oracle's"
    assert np.array_equal(got["count"], count), key
    assert np.array_equal(got["stats"][0], depths), key
    assert got["counters"] == totals, (key, got["counters"], totals)


def render_and_compare(sc, key, flags):
    be = gpu_cases.context(sc, W, H, depth=DEPTH, flags=flags)
    try:
        be.render(0, ITERATIONS)
        assert_equals_oracle(be, sc, key, flags)
    finally:
        be.release()


def random_triangles():
    """Small, but with leaves enough that the upload picks the CULLING instantiation (ptmi_scene_memory.cpp: 1024 cullable
    leaves), plain shading, one point light: the flagship's kernel.  Most of its paths miss: sky, light and camera."""
    sc = cached_scene("tris8k", W, H)
    assert int((sc.bvh["isLeaf"] != 0).sum()) >= 2048 and sc.lightsSize == 1
    return sc


@ARITHMETICS
def test_random_triangles_plain_culling_kernel(flags):
    render_and_compare(random_triangles(), "tris8k", flags)


@ARITHMETICS
@pytest.mark.parametrize("name", ["matmix", "mayalike_s"])
def test_general_shading_several_lights_and_cube_map_sky(name, flags):
    render_and_compare(cached_scene(name, W, H), name, flags)


def moved_camera(sc):
    out = copy.copy(sc)
    a = np.float32(0.09)
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    d, u = np.asarray(sc.cameraDirection, np.float32), np.asarray(sc.cameraUp, np.float32)
    out.cameraPosition = (np.asarray(sc.cameraPosition, np.float32) + np.float32([0.4, -0.7, 0.3, 0])).astype(np.float32)
    out.cameraDirection = (c * d + s * u).astype(np.float32)
    out.cameraUp = (c * u - s * d).astype(np.float32)
    return out


def moved_light_and_recoloured_sky(sc):
    out = copy.copy(sc)
    out.lights = sc.lights.copy()
    out.lights["position"][0] = np.float32([7.0, -4.0, 8.0, 1.0])
    out.lights["color"][0] = np.float32([1.0, 0.8, 0.6, 1.0])
    out.lights["power"][0] = np.float32(45.0)
    out.texturesData = sc.texturesData.copy()
    out.texturesData[0] = (40, 90, 220, 255)
    return out


@ARITHMETICS
def test_constants_of_an_earlier_launch_do_not_outlive_it(flags):
    first = random_triangles()
    second = moved_camera(first)
    third = moved_light_and_recoloured_sky(second)
    be = gpu_cases.context(first, W, H, depth=DEPTH, flags=flags)
    try:
        be.render(0, ITERATIONS)
        assert_equals_oracle(be, first, "tris8k", flags)
        be.set_camera(second.cameraPosition, second.cameraDirection, second.cameraRight, second.cameraUp)
        be.clear()
        be.render(0, ITERATIONS)
        assert_equals_oracle(be, second, "tris8k, camera moved", flags)
        be.initialize_memory(third)
        be.clear()
        be.render(0, ITERATIONS)
        assert_equals_oracle(be, third, "tris8k, camera and light moved, sky recoloured", flags)
    finally:
        be.release()
    # (each change shows: the three images differ)
    images = [oracle_of(sc, key, flags)[0] for sc, key in ((first, "tris8k"), (second, "tris8k, camera moved"),
                                                           (third, "tris8k, camera and light moved, sky recoloured"))]
    assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[1], images[2])
