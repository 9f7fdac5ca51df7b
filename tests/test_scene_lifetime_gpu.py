"""A second ptmi_initialize_memory on a context that has used everything a scene can own: nothing of the first scene survives.

Scene A is rendered, updated in place, snapshot and queried, its accumulators bound to a caller's buffers and unbound again -
which allocates every lazily made per-scene buffer (stage sets, the update's arrays, a snapshot buffer with its event, and on
two devices the landing buffer and the sum).  Then scene B, with another triangle count, goes to the same context.  A slot of
A's ring must read as empty, and every word read from then on - hits of a query, image, sample counts, histograms, counters -
must be what a fresh context that only ever saw B gives for the same calls.
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError
from gpu_cases import assert_same_state, cached_scene, state
import ray_query_cases as Q

pytestmark = pytest.mark.gpu
W, H, DEPTH = 16, 16, 3
STATE, UNSUPPORTED = -6, -7


def scene(name):
    sc = cached_scene(name, W, H)
    with np.errstate(all="ignore"):
        return sc, Q.mixed_rays(sc, 8, W, H)


def query(be, rays):
    return Q.words(be.query_rays(rays["origin"], rays["direction"], rays["max_squared_distance"])).copy()


def life_with(be, name):
    """Steps 5 and 6: what a context holding scene `name` renders, answers and counts."""
    sc, rays = scene(name)
    be.render(0, 2)
    be.update_triangles(sc.triangulation)
    hits = query(be, rays)
    return dict(state(be), hits=hits)


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_device", "two_devices"])
def test_a_second_upload_starts_from_nothing(devices):
    (a, rays_a), (b, _) = scene("cornell"), scene("tris500")
    assert a.triangulation.shape[0] != b.triangulation.shape[0] and a.lightsSize == b.lightsSize
    fresh = Backend().setup_context(W, H, DEPTH, b.lightsSize, devices=devices)
    try:
        fresh.initialize_memory(b)
        want = life_with(fresh, "tris500")
    finally:
        fresh.release()

    be = Backend().setup_context(W, H, DEPTH, a.lightsSize, devices=devices)
    try:
        be.initialize_memory(a)
        be.render(0, 2)
        be.update_triangles(a.triangulation)
        be.snapshot(1)
        be.read_snapshot(1)
        query(be, rays_a)
        if devices is None:
            import torch
            from opencl_pathtracer_amd.distributed import FusedAccumulators
            fb = FusedAccumulators(W, H, torch.device("cuda", 0))
            fb.bind(be)
            be.bind_accumulators(0, 0)
        else:  # (partial sums cannot be bound)
            with pytest.raises(PtmiError) as e:
                be.bind_accumulators(0, 0)
            assert e.value.code == UNSUPPORTED
        be.initialize_memory(b)
        with pytest.raises(PtmiError) as e:
            be.read_snapshot(1)
        assert e.value.code == STATE, str(e.value)
        got = life_with(be, "tris500")
    finally:
        be.release()
    assert np.array_equal(got["hits"], want["hits"])
    assert_same_state(got, want)
    assert got["count"].sum() > 0 and got["counters"]["paths"] > 0  # (the comparison is not of two empty images)
