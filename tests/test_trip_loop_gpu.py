"""The trip loop of the wavefront kernel with the node step under the trip's mask (kernel_wavefront.hip: kMaskedStep; the
assembly side: tests/test_trip_loop_copies.py) renders what the CPU oracle renders: image, sample counts, the three histograms
and the totals of ptmi_counters, word for word, in both arithmetics.

Shapes: 40 x 24 pixels - 15 tiles of 8 x 8, the right-hand ones cut - and 2 iterations: 1920 paths for 1024 lanes of the first
workgroups, so waves run node trips and leaf passes side by side, change between them, and refill lanes from the job queues.
  tris20k    depth 4   the plain culling instantiation, a deep tree        (and once more with PTMI_LEAF_CULL=0, and with statistics)
  cornell    depth 4   the plain instantiation without culling code, leaves next to the root
  matmix     depth 6   general shading: the top of the stack in a register (kTos)
  mayalike_s depth 4   the instantiation tests/test_parity_gpu.py's mayalike_s case selects (textured: general shading)
One oracle render per scene and arithmetic, shared.
"""
import numpy as np
import pytest

import gpu_cases as C
import oracle_ffi as O
from opencl_pathtracer_amd import backend as backend_flags

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 24, 2
SCENES = [("tris20k", 4), ("cornell", 4), ("matmix", 6), ("mayalike_s", 4)]
DA = backend_flags.FLAG_DEFAULT_ARITHMETIC
_oracle = {}


def oracle(name, depth, da):
    key = (name, depth, da)
    if key not in _oracle:
        color, count, hists, totals = O.oracle_render(C.cached_scene(name, W, H), W, H, depth, SPP, default_arithmetic=da)
        _oracle[key] = dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals)
    return _oracle[key]


def rendered(name, depth, flags):
    be = C.context(C.cached_scene(name, W, H), W, H, depth, flags=flags)
    try:
        be.render(0, SPP)
        got = C.state(be)
        scheduler = be.scheduler_stats() if flags & backend_flags.FLAG_SCHEDULER_STATS else None
    finally:
        be.release()
    return got, scheduler


@pytest.fixture
def production_switches(monkeypatch):
    for switch in ("PTMI_LEAF_CULL", "PTMI_GENERIC_SHADING", "PTMI_GENERIC_TRIANGLES", "PTMI_GENERIC_BOXES"):
        monkeypatch.delenv(switch, raising=False)
    return monkeypatch


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
@pytest.mark.parametrize("name,depth", SCENES, ids=[name for name, _ in SCENES])
def test_renders_the_oracle(name, depth, da, production_switches):
    got, _ = rendered(name, depth, DA if da else 0)
    C.assert_same_state(got, oracle(name, depth, da))


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_renders_the_oracle_without_culling_code(da, production_switches):
    production_switches.setenv("PTMI_LEAF_CULL", "0")
    got, _ = rendered("tris20k", 4, DA if da else 0)
    C.assert_same_state(got, oracle("tris20k", 4, da))


@pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
def test_statistics_build_renders_the_oracle_and_reads_no_stale_item(da, production_switches):
    got, scheduler = rendered("tris20k", 4, (DA if da else 0) | backend_flags.FLAG_SCHEDULER_STATS)
    C.assert_same_state(got, oracle("tris20k", 4, da))
    assert scheduler["leaf_item_violations"] == 0
    assert scheduler["trips_node"] > 0 and scheduler["trips_triangle"] > 0 and scheduler["trips_path"] > 0
