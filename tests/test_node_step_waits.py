"""The node step of the wavefront kernel uses its record's four quads as they arrive ("The node step's waits").

A node step issues four global_load_dwordx4 from one address (offsets 0, 16, 32, 48) and needs them in that order: the first
box test reads quads a and b, the second b and c, and quad d (child references, axis, cull bits) only after both.  The waits
the compiler places must follow that: vmcnt(3), (2), (1), and vmcnt(0) only where quad d is read.  They did not while the
kernel held flat_ instructions in path logic (a generic pointer to the scene's rare fields): with a flat operation possibly
pending, the first wait behind the loads waited for all four.  Read from the assembly hipcc makes of kernel_wavefront.hip
(it cross-compiles without a GPU), with the parsing tests/kernel_figures.py shares, for every production instantiation in
both arithmetics.

"Before the block ends": the compiler ends the basic block of the loads at the branch between the ordered and the literal box
test, so the waits are followed in layout order through the blocks of the traversal loop that come next, up to the first that
carries vmcnt(0) - which must stand before the loop issues another vector memory load (the leaf pass's) or ends.
"""
import pytest

import kernel_figures as K

# STATS PRE SS PLAIN NANSAFE [b64: workgroups of 64 lanes] [c: culls leaves] - the instantiations instance_for() launches
# without scheduler statistics and without SUPER_SAMPLING (tests/test_resources.py names the same set, before culling)
PRODUCTION = {"00000", "00001", "01000", "01001", "01010", "01011", "01000b64", "01010b64", "01000c", "01010c", "01000b64c", "01010b64c"}
# every instantiation reads the rare scene fields through a global pointer: none got the fence instead
CAUSE_REMOVED = PRODUCTION


def waits_behind_the_loads(kernel):
    found = K.node_step_waits(kernel)
    assert found is not None, "no block of the traversal loop loads four quads from one address"
    return found


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_node_step_waits_for_its_quads_one_by_one(arithmetic):
    kernels = K.blocks(arithmetic)
    assert PRODUCTION <= set(kernels), sorted(kernels)
    for key in sorted(PRODUCTION):
        offsets, waits, found = waits_behind_the_loads(kernels[key])
        print(key, offsets, waits)
        assert offsets == [0, 16, 32, 48], (key, offsets)  # box 1 needs a and b, box 2 b and c, d last
        assert waits, key
        assert "vmcnt(0)" not in waits[0], (key, waits)
        assert found and "vmcnt(0)" in waits[-1], (key, waits)
        assert len(waits) >= 2, (key, waits)  # (the list ends at the first vmcnt(0): it is not the first wait)


@K.needs_hipcc
@pytest.mark.parametrize("arithmetic", [0, 1], ids=["strict", "default"])
def test_no_flat_instruction_in_or_before_the_traversal_loop(arithmetic):
    """Where the cause was removed: no flat_ instruction in the traversal loop (the depth-2 blocks), in the path-logic loop around
    it, or in front of the loops.  (As built, the kernels hold none at all; what follows the loops - the counter flush - is not
    a path into them and is left free.)"""
    kernels = K.blocks(arithmetic)
    for key in sorted(CAUSE_REMOVED):
        kernel = kernels[key]
        last_loop = max(i for i, (depth, _) in enumerate(kernel) if depth > 0)
        flat = [line for _, lines in kernel[:last_loop + 1] for line in lines if line.startswith("flat_")]
        assert not flat, (key, flat[:4])
