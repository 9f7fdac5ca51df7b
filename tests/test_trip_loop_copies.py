"""A node trip of the wavefront kernel's traversal loop updates the lane's cursor in place ("The trip loop's copies").

While a trip's kind was a branch around the node step (`if (pass) { leaf_pass(); survey(); continue; } if (want_inner)
node_step(); survey();`), the leaf pass and the node step met in one flow block of the structurised loop, and the cursor the
step leaves - p_bbx, p_tri, tri_end, tri_i, cur, sp - reached that block as PHIs the register coalescer did not fold: every node
trip began with a full vmcnt(0) and five to seven v_mov into temporaries and ended with five to ten v_mov back, under the full
exec mask.  With the kind as the step's exec mask (kernel_wavefront.hip: kMaskedStep) the step works on the home registers.

Read from the assembly hipcc makes of kernel_wavefront.hip (it cross-compiles without a GPU) with the resource tool's
parsing (through tests/kernel_figures.py: trip_loops), for every production instantiation in both arithmetics:
  - the way IN - the node-trip path from the loop header to the step's first record load - holds no v_mov between two vector
    registers (and no full vector-memory wait: there is nothing the step's address waits for);
  - the way OUT - from the step's last LDS operation to the back edge - holds none either;
  - the loop's v_mov_b32 count (constants included) is at most what the change reached;
  - the loop holds no scratch access.

Two exceptions, named here:
  OLD_FORM: the general-shading instantiations of 256 lanes without culling keep the branch.  Under the mask the register
    allocator spills more of them than tests/test_path_logic_loads.py pins (default arithmetic <0,0,0,0,0> 30 registers for 29
    and <0,1,0,0,1> 44 for 26, strict <0,1,0,0,0> 58 for 57, each with one full wait more in the path-logic pass), and the strict
    build of <0,0,0,0,1> reloads a fourth spilled register inside the loop where tests/test_resources.py allows it three.  They
    must stay what they were: the parent's v_mov counts, the parent's three reloads in the strict <0,0,0,0,1>.
  TOS: the general-shading instantiations hold the top of the lane's stack in a register (kTos), so their pop IS a copy
    (cur <- tos) and the refill reaches tos through the register the LDS read returns in: two v_mov behind the last LDS
    operation, a third where a culled leaf pops twice.  Pinned at that; the way in holds none, as everywhere.
"""
import pytest

import kernel_figures as K

# STATS PRE SS PLAIN NANSAFE [b64: workgroups of 64 lanes] [c: culls leaves]: tests/test_node_step_waits.py's set
PRODUCTION = {"00000", "00001", "01000", "01001", "01010", "01011", "01000b64", "01010b64", "01000c", "01010c", "01000b64c", "01010b64c"}
OLD_FORM = {"00000", "00001", "01000", "01001"}
TOS = {k for k in PRODUCTION if k[3] == "0"} - OLD_FORM
TOS_COPIES_OUT = lambda key: 3 if key.endswith("c") else 2

# v_mov_b32 in the traversal loop, [strict, default]; the parent's figures behind
V_MOV = {
    "00000": [70, 50],      # parent 70, 50 (OLD_FORM)
    "00001": [94, 80],      # parent 94, 80 (OLD_FORM)
    "01000": [43, 43],      # parent 43, 43 (OLD_FORM)
    "01000b64": [29, 29],   # parent 43, 43
    "01000c": [34, 34],     # parent 52, 52
    "01000b64c": [34, 34],  # parent 52, 52
    "01001": [66, 73],      # parent 66, 73 (OLD_FORM)
    "01010": [23, 23],      # parent 35, 35
    "01010b64": [23, 23],   # parent 35, 35
    "01010c": [24, 24],     # parent 40, 40   <- the flagship's kernel
    "01010b64c": [24, 24],  # parent 40, 40
    "01011": [43, 43],      # parent 55, 55
}


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_node_trip_updates_the_cursor_in_place(arithmetic):
    found = K.trip_loops(arithmetic)
    assert PRODUCTION <= set(found), sorted(found)
    for key in sorted(PRODUCTION - OLD_FORM):
        t = found[key]
        assert t is not None, key
        print(key, t)
        assert t["copies in"] == [], (key, t["copies in"])
        assert t["full waits in"] == 0, key
        assert t["copies out"] is not None, key  # (every step ends in LDS operations: the push, the pops)
        if key in TOS:
            assert len(t["copies out"]) <= TOS_COPIES_OUT(key), (key, t["copies out"])
        else:
            assert t["copies out"] == [], (key, t["copies out"])


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_loop_v_mov_count_and_no_scratch(arithmetic):
    found = K.trip_loops(arithmetic)
    for key in sorted(PRODUCTION):
        t = found[key]
        print(key, t["loop v_mov"], t["loop scratch"], "node trip", t["node trip"], "leaf pass", t["leaf pass"])
        assert t["loop v_mov"] <= V_MOV[key][arithmetic], (key, t["loop v_mov"])
        # (<0,0,0,0,1>, strict, OLD_FORM: the three reloads it had, tests/test_resources.py's allowance)
        assert t["loop scratch"] <= (3 if key == "00001" and arithmetic == 0 else 0), (key, t["loop scratch"])


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_old_form_is_what_it_was(arithmetic):
    """The instantiations that keep the branch still show what the others lost: the measure sees the copies."""
    for key in sorted(OLD_FORM):
        t = K.trip_loops(arithmetic)[key]
        assert len(t["copies in"]) >= 5 and t["full waits in"] == 1 and len(t["copies out"]) >= 5, (key, t)
