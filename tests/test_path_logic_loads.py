"""The memory chain of a path-logic pass, read from the assembly ("The pass's memory chain").

A pass of the wavefront kernel fetched its launch constants - the camera, the sky's rotation, the one light of the plain
instantiations - with vector loads: one address for the whole wave, fetched by every active lane, each a round trip of its own
through the L1 queue the traversal keeps full.  They are scalar loads now (ptmi_device.hpp: as_constant).  Counted per production
instantiation, in both arithmetics, by the resource tool's parsing (through tests/kernel_figures.py) over the body of the outer
loop (the depth-1 blocks of the assembly hipcc makes of kernel_wavefront.hip; it cross-compiles without a GPU): vector loads from
memory, scalar loads, and waits that let no vector memory operation stay outstanding.

PARENT holds the same tool's figures for the parent commit (recorded in profiles/path_logic_constants_ab.txt), PINNED the
figures of this tree, which are upper bounds from now on, as the spill budgets of tests/test_resources.py are.

How many vector loads must go: the flagship's instantiation held these loads of wave-uniform launch constants - the sky's
rotation (one dwordx2), the light for the lit term (a dword and two dwordx4), the light again for the shadow ray (one dwordx4),
the camera (four dwordx4): NINE.  (The two other loads of the sky branch - the header of the face a lane looks at and its texel -
have addresses of the lane's own: they stay vector loads.)  The general instantiations index their lights per lane and lose
five: the rotation and the camera.
"""
import pytest

import kernel_figures as K

# STATS PRE SS PLAIN NANSAFE [b64] [c] (tests/test_node_step_waits.py: PRODUCTION) ->
# (VGPRs, spilled VGPRs, static LDS bytes, vector loads, scalar loads, full vector-memory waits of the pass); key: arithmetic
PARENT = {
    0: {"00000": (96, 58, 192, 39, 0, 61), "00001": (96, 59, 192, 39, 0, 54), "01000": (96, 57, 192, 39, 0, 54), "01001": (96, 38, 192, 39, 0, 55),
        "01010": (96, 8, 192, 25, 0, 21), "01011": (96, 9, 192, 25, 0, 23), "01000b64": (96, 55, 192, 39, 0, 53), "01010b64": (96, 4, 192, 25, 0, 20),
        "01000c": (96, 57, 192, 39, 0, 55), "01010c": (96, 4, 192, 25, 0, 21), "01000b64c": (96, 55, 192, 39, 0, 53), "01010b64c": (96, 4, 192, 25, 0, 20)},
    1: {"00000": (96, 29, 192, 39, 0, 50), "00001": (96, 31, 192, 39, 0, 50), "01000": (96, 29, 192, 39, 0, 49), "01001": (96, 26, 192, 39, 0, 49),
        "01010": (96, 4, 192, 25, 0, 21), "01011": (96, 4, 192, 25, 0, 21), "01000b64": (96, 25, 192, 39, 0, 49), "01010b64": (96, 4, 192, 25, 0, 20),
        "01000c": (96, 28, 192, 39, 0, 49), "01010c": (96, 4, 192, 25, 0, 21), "01000b64c": (96, 27, 192, 39, 0, 49), "01010b64c": (96, 4, 192, 25, 0, 21)},
}
PINNED = {
    0: {"00000": (96, 58, 192, 34, 2, 62), "00001": (96, 59, 192, 34, 2, 55), "01000": (96, 57, 192, 34, 2, 56), "01001": (96, 38, 192, 34, 2, 56),
        "01010": (96, 8, 192, 16, 5, 17), "01011": (96, 9, 192, 16, 5, 19), "01000b64": (96, 55, 192, 34, 2, 57), "01010b64": (96, 4, 192, 16, 5, 16),
        "01000c": (96, 57, 192, 34, 2, 57), "01010c": (96, 4, 192, 16, 5, 17), "01000b64c": (96, 55, 192, 34, 2, 56), "01010b64c": (96, 4, 192, 16, 5, 16)},
    1: {"00000": (96, 26, 192, 34, 2, 49), "00001": (96, 30, 192, 34, 2, 50), "01000": (96, 26, 192, 34, 2, 48), "01001": (96, 25, 192, 34, 2, 47),
        "01010": (96, 4, 192, 16, 5, 17), "01011": (96, 4, 192, 16, 5, 17), "01000b64": (96, 24, 192, 34, 2, 46), "01010b64": (96, 4, 192, 16, 5, 16),
        "01000c": (96, 28, 192, 34, 2, 50), "01010c": (96, 4, 192, 16, 5, 17), "01000b64c": (96, 27, 192, 34, 2, 49), "01010b64c": (96, 4, 192, 16, 5, 17)},
}
FLAGSHIP = "01010c"  # bench.py's kernel: precomputed records, plain shading, culling, 256 lanes
UNIFORM_LOADS_PLAIN, UNIFORM_LOADS_GENERAL = 9, 5


def figures(arithmetic):
    return {k: (v["VGPRs"], v["VGPRs Spill"], v["LDS Size"], v["pass vector loads"], v["pass scalar loads"], v["pass full waits"])
            for k, v in K.resources(arithmetic).items()}


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_the_pass_keeps_its_memory_counts(arithmetic):
    got = figures(arithmetic)
    assert set(PINNED[arithmetic]) <= set(got), sorted(got)
    for key, pinned in sorted(PINNED[arithmetic].items()):
        print(key, "vector loads, scalar loads, full waits:", got[key][3:], "pinned", pinned[3:])
        for name, now, bound in zip(("vector loads", "scalar loads", "full vector-memory waits"), got[key][3:], pinned[3:]):
            assert now <= bound, (key, name, now, bound)


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_the_uniform_loads_left_the_vector_memory_queue(arithmetic):
    got, parent = figures(arithmetic), PARENT[arithmetic]
    print(FLAGSHIP, "vector loads", parent[FLAGSHIP][3], "->", got[FLAGSHIP][3], "scalar loads", got[FLAGSHIP][4])
    assert got[FLAGSHIP][3] <= parent[FLAGSHIP][3] - UNIFORM_LOADS_PLAIN
    for key, before in sorted(parent.items()):
        plain = key[3] == "1"
        assert got[key][3] <= before[3] - (UNIFORM_LOADS_PLAIN if plain else UNIFORM_LOADS_GENERAL), (key, got[key], before)
        assert got[key][4] >= 1, (key, got[key])  # (something IS fetched by scalar loads: the counts did not fall by dead code)


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_no_production_instantiation_pays_in_registers_spills_or_lds(arithmetic):
    got = figures(arithmetic)
    for key, before in sorted(PARENT[arithmetic].items()):
        print(key, "VGPRs, spilled, LDS bytes:", got[key][:3], "parent", before[:3])
        assert got[key][0] <= before[0], (key, "VGPRs", got[key], before)
        assert got[key][1] <= before[1], (key, "spilled VGPRs", got[key], before)
        assert got[key][2] <= before[2], (key, "LDS bytes", got[key], before)
