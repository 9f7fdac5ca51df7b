"""The wavefront kernel's assembly for the tests that pin static figures: kernel_wavefront.hip is cross-compiled (hipcc needs
no GPU) once per arithmetic per process, and every test file reads its figures off that one assembly.  The parsing is the
resource tool's (tools/kernel_resources.py); this module only keeps what it returns, in one cache keyed by (what, arithmetic).
resources() lets the tool parse the assembly once more (under a second) instead of handing it blocks() and cfg().
A new static-figure test imports this module, marks its tests `needs_hipcc` and asks for blocks(), cfg(), trip_loops() or
resources(); it keeps its own pinned table and nothing else."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as R  # noqa: E402
from kernel_resources import node_step_waits, trip_loop_text  # noqa: E402,F401  (what the tests apply to a kernel's blocks)

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
_cache = {}


def _once(what, arithmetic, make):
    if (what, arithmetic) not in _cache:
        _cache[what, arithmetic] = make()
    return _cache[what, arithmetic]


def _compile(arithmetic):
    print(f"kernel_figures: compiling kernel_wavefront.hip, arithmetic {arithmetic}", file=sys.stderr)
    return R.compile_to_assembly(ROOT, arithmetic)


def assembly(arithmetic):
    """-> (path of the assembly, hipcc's resource remarks)"""
    return _once("assembly", arithmetic, lambda: _compile(arithmetic))


def blocks(arithmetic):
    """{instantiation key: [(loop depth, instructions)]}"""
    return _once("blocks", arithmetic, lambda: R.kernel_blocks(assembly(arithmetic)[0]))


def cfg(arithmetic):
    """{instantiation key: [block with its successors]}"""
    return _once("cfg", arithmetic, lambda: R.kernel_cfg(assembly(arithmetic)[0]))


def trip_loops(arithmetic):
    """{instantiation key: what a trip of the traversal loop costs beyond its work (the tool's trip_loop_copies)}"""
    return _once("trip loops", arithmetic, lambda: {key: R.trip_loop_copies(kernel) for key, kernel in cfg(arithmetic).items()})


def resources(arithmetic, region_forms=False):
    """{instantiation key: every figure the tool prints}; the forms that render a rectangle (key suffix r) only when asked"""
    found = _once("resources", arithmetic, lambda: R.figures_of(*assembly(arithmetic), region_forms=True))
    return {key: v for key, v in found.items() if region_forms or not key.endswith("r")}
