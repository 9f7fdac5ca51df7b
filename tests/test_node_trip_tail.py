"""The node trip's tail of the wavefront kernel, read off the assembly ("The node trip's tail").

hipcc cross-compiles kernel_wavefront.hip without a GPU; the resource tool's parsing (through tests/kernel_figures.py) reads the whole trip,
node_trip_tail the node-trip path from the step's push (the ds_write_b32 behind the record loads) to the back edge.

CHOICE: the instantiations whose trip's kind is the step's exec mask (plain shading, culling, or 64 lanes; the statistics builds
  apart) take the trip choice of csrc/trip_choice.h.  Their node trip's and leaf pass's scalar instructions are strictly below
  the parent's, pinned at what the change reached; vector instructions, v_mov, copies, registers, spills and scratch are not
  above the parent's; the stack's reads and waits behind the push are the parent's.
ALONE: the general instantiations of 256 lanes without culling and the statistics builds compile to the parent's registers,
  spills, scratch, trip-loop figures and tail, number for number.
(The other half of the issue - ONE read point for the stack behind the push, in the instantiations without a top-of-stack
register - reached reads 2, read points 1, waits with lgkmcnt(0) 1 on this measure, at 156 / 88, and measured slower on the
GPU: taken out, profiles/node_trip_tail_ab.txt.  So every tail below is the parent's: two reads at two points, two waits.)

PARENT: the parent commit's figures, [strict, default] = ((VGPRs, spilled, scratch bytes), (v_mov in the loop, node trip vector,
scalar, leaf pass vector, scalar, copies in, full waits in, copies out), (tail: LDS reads, read points, waits with lgkmcnt(0),
vector, scalar)).
"""
import pytest

import kernel_figures as K

PARENT = {
    "00000": [((96, 58, 108), (70, 141, 93, 221, 123, 6, 1, 8), (2, 1, 2, 29, 36)),
              ((96, 26, 92), (50, 141, 93, 179, 123, 6, 1, 8), (2, 1, 2, 29, 36))],
    "00001": [((96, 59, 124), (94, 141, 94, 261, 136, 6, 1, 8), (2, 1, 2, 29, 37)),
              ((96, 30, 100), (80, 141, 94, 221, 135, 6, 1, 8), (2, 1, 2, 29, 37))],
    "01000": [((96, 57, 104), (43, 141, 93, 165, 123, 6, 1, 8), (2, 1, 2, 29, 36)),
              ((96, 26, 92), (43, 141, 93, 160, 123, 6, 1, 8), (2, 1, 2, 29, 36))],
    "01000b64": [((96, 55, 96), (29, 125, 88, 153, 108, 0, 0, 2), (2, 1, 1, 19, 31)),
                 ((96, 24, 84), (29, 125, 88, 147, 108, 0, 0, 2), (2, 1, 1, 19, 31))],
    "01000b64c": [((96, 55, 96), (30, 162, 100, 152, 108, 0, 0, 2), (2, 1, 1, 25, 32)),
                  ((96, 27, 96), (30, 162, 100, 148, 108, 0, 0, 2), (2, 1, 1, 25, 32))],
    "01000c": [((96, 57, 104), (34, 180, 104, 152, 108, 0, 0, 3), (3, 3, 3, 42, 44)),
               ((96, 28, 100), (34, 180, 104, 147, 108, 0, 0, 3), (3, 3, 3, 42, 44))],
    "01001": [((96, 38, 108), (66, 141, 94, 204, 135, 6, 1, 8), (2, 1, 2, 29, 37)),
              ((96, 25, 96), (73, 141, 94, 202, 135, 6, 1, 8), (2, 1, 2, 29, 37))],
    "01010": [((96, 8, 20), (23, 119, 87, 150, 108, 0, 0, 0), (2, 2, 2, 18, 32)),
              ((96, 4, 12), (23, 119, 87, 146, 108, 0, 0, 0), (2, 2, 2, 18, 32))],
    "01010b64": [((96, 4, 12), (23, 119, 87, 151, 108, 0, 0, 0), (2, 2, 2, 18, 32)),
                 ((96, 4, 12), (23, 119, 87, 146, 108, 0, 0, 0), (2, 2, 2, 18, 32))],
    "01010b64c": [((96, 4, 12), (24, 156, 100, 151, 108, 0, 0, 0), (2, 2, 2, 24, 33)),
                  ((96, 4, 12), (24, 156, 100, 146, 108, 0, 0, 0), (2, 2, 2, 24, 33))],
    "01010c": [((96, 4, 20), (24, 157, 100, 151, 108, 0, 0, 0), (2, 2, 2, 24, 33)),
               ((96, 4, 12), (24, 156, 100, 145, 108, 0, 0, 0), (2, 2, 2, 24, 33))],   # <- the flagship's kernel
    "01011": [((96, 9, 32), (43, 119, 87, 187, 118, 0, 0, 0), (2, 2, 2, 18, 32)),
              ((96, 0, 0), (43, 119, 87, 181, 118, 0, 0, 0), (2, 2, 2, 18, 32))],
    "10001": [((96, 77, 164), (96, 143, 98, 268, 145, 6, 1, 9), (2, 1, 2, 31, 42)),
              ((96, 67, 148), (83, 143, 98, 230, 145, 6, 1, 9), (2, 1, 2, 31, 42))],
    "10101": [((96, 91, 172), (96, 143, 98, 270, 145, 6, 0, 9), (2, 1, 2, 31, 42)),
              ((96, 79, 156), (83, 143, 98, 231, 145, 6, 1, 9), (2, 1, 2, 31, 42))],
    "11001c": [((96, 84, 164), (60, 184, 110, 201, 131, 1, 0, 3), (3, 3, 3, 44, 44)),
               ((96, 70, 156), (60, 184, 110, 196, 131, 1, 0, 3), (3, 3, 3, 44, 44))],
    "11101c": [((96, 87, 176), (60, 184, 110, 202, 131, 1, 0, 3), (3, 3, 3, 44, 44)),
               ((96, 87, 168), (60, 184, 110, 197, 131, 1, 0, 3), (3, 3, 3, 44, 44))],
}
CHOICE = {"01010", "01010b64", "01010c", "01010b64c", "01011", "01000b64", "01000b64c", "01000c"}
ALONE = set(PARENT) - CHOICE
# scalar instructions of the node trip and of the leaf pass as the change left them (the parent's: 87 .. 104 and 108, 118): upper bounds
SCALAR = {"01010": (74, 95), "01010b64": (74, 95), "01011": (74, 105), "01010c": (87, 95), "01010b64c": (87, 95),
          "01000b64": (75, 95), "01000b64c": (87, 95), "01000c": (91, 95)}


def figures(arithmetic):
    return {key: ((v["VGPRs"], v["VGPRs Spill"], v["ScratchSize"]), tuple(map(int, K.trip_loop_text(v["trip loop"]).split())),
                  tuple(v["tail"].values())) for key, v in K.resources(arithmetic).items()}


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_the_trip_choice_takes_scalar_instructions_out_of_both_kinds_of_trip(arithmetic):
    found = figures(arithmetic)
    assert set(PARENT) == set(found), sorted(found)
    for key in sorted(CHOICE):
        regs, trip, tail = found[key]
        p_regs, p_trip, p_tail = PARENT[key][arithmetic]
        print(key, "node trip", trip[1:3], "parent", p_trip[1:3], "leaf pass", trip[3:5], "parent", p_trip[3:5], "tail", tail, "parent", p_tail)
        assert trip[2] < p_trip[2] and trip[2] <= SCALAR[key][0], (key, trip)   # node trip, scalar: strictly below, and where it was left
        assert trip[4] < p_trip[4] and trip[4] <= SCALAR[key][1], (key, trip)   # leaf pass, scalar
        assert trip[1] <= p_trip[1] and trip[3] <= p_trip[3], (key, trip)       # vector: not above the parent's
        assert trip[0] <= p_trip[0] and trip[5:] == p_trip[5:], (key, trip, p_trip)  # v_mov; copies and full waits on the way in and out
        assert regs[0] <= 96 and regs[1] <= p_regs[1] and regs[2] <= p_regs[2], (key, regs, p_regs)
        assert tail[:4] == p_tail[:4] and tail[4] < p_tail[4], (key, tail, p_tail)  # the stack's reads and waits behind the push: the parent's


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_every_instantiation_left_alone_is_the_parents(arithmetic):
    found = figures(arithmetic)
    for key in sorted(ALONE):
        assert found[key] == PARENT[key][arithmetic], (key, found[key], PARENT[key][arithmetic])
