"""Shared by the GPU tests that hold one context against another (test_ray_query_gpu.py, test_guide_buffers_gpu.py,
test_scene_update_gpu.py, test_scene_lifetime_gpu.py): the scenes they share, a context with a scene loaded, and everything a
render leaves behind, compared word for word."""
import numpy as np

from opencl_pathtracer_amd import Backend, bvh_create, scenes, structs as S
import scene_update_cases as U

_scenes = {}


def cached_scene(name, width, height):
    """`big_leaf`, `empty_leaves` (of cornell), or a name scenes.build knows, with its tree; built once per image size."""
    key = (name, width, height)
    if key not in _scenes:
        if name == "big_leaf":
            sc = bvh_create(U.big_leaf_scene(width, height))
            assert sc.bvh["nbTriangles"][sc.bvh["isLeaf"] != 0].max() >= 9
        elif name == "empty_leaves":
            sc = U.with_empty_leaves(cached_scene("cornell", width, height))
        else:
            sc = bvh_create(scenes.build(name, width, height))
        _scenes[key] = sc
    return _scenes[key]


def context(sc, width, height, depth=4, flags=0, sampler=S.JITTERED, super_sampling=False, devices=None):
    be = Backend().setup_context(width, height, depth, sc.lightsSize, sampler, super_sampling=super_sampling, flags=flags, devices=devices)
    be.initialize_memory(sc)
    return be


def require_probe_tools():
    """The two libraries the record checks read a context's scene with; a GPU test without them fails, it does not skip."""
    import pytest
    import scene_record_cases as R
    if R.model() is None:
        pytest.fail("oracle/build/libscene_refit_model.so not built (make -C oracle probe)", pytrace=False)
    if R.probe() is None:
        pytest.fail("oracle/build/libscene_record_probe.so not built (make -C oracle probe)", pytrace=False)


def tensor_on_device(array):
    """The array as a torch tensor on the device, copied before this returns (the context's stream is not torch's)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(array)).cuda()
    torch.cuda.synchronize()
    return t


def bytes_of(tensor):
    import torch
    torch.cuda.synchronize()
    return tensor.view(torch.int32).cpu().numpy().tobytes()


def state(be, variance=False):
    color, count = be.read_image()
    out = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[s.copy() for s in be.read_statistics()], counters=be.counters())
    if variance:
        out["variance"] = be.read_variance().view(np.uint32).copy()
    return out


def assert_same_state(a, b):
    assert a["counters"] == b["counters"], (a["counters"], b["counters"])
    for x, y in zip(a["stats"], b["stats"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["count"], b["count"])
    diff = int((a["color"] != b["color"]).any(axis=-1).sum())
    assert diff == 0, f"{diff} pixels differ"
    if "variance" in a or "variance" in b:
        assert np.array_equal(a["variance"], b["variance"])
