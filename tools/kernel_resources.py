#!/usr/bin/env python3
"""Register budget of every render_wavefront_kernel instantiation (hipcc cross-compiles without a GPU): VGPRs, spilled VGPRs,
scratch bytes, occupancy, and the number of scratch instructions INSIDE the traversal loop (depth-2 blocks), plus the static
instruction mix of that loop, what a trip of it costs beyond its work (v_mov, the two trip paths' instruction counts, the register
copies and full waits around the node step: trip_loop_copies), the kernel's flat instructions, the memory chain of a path-logic pass (the outer loop's body:
vector loads, scalar loads, full vector-memory waits), and the waits of the node step: the s_waitcnt sequence from the
step's four record loads to the first vmcnt(0) (the first wait must not be the one that waits for all four), and
the node trip's tail: the stack's LDS reads and the waits behind the step's push (node_trip_tail).
usage: tools/kernel_resources.py [source tree, default the repo] [arithmetic 0|1, default 1]"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the mangled template arguments: five bools, the workgroup's lanes, whether the instantiation culls leaves (leaf_cull.h), and
# whether it is the form that renders a rectangle (ptmi_render_region: key suffix r; the forms without it keep their keys)
NAME = r"\w+?23render_wavefront_kernelI((?:Lb[01]E){5})(?:Li(\d+)E)?(?:Lb([01])E)?(?:Lb([01])E)?E"


def key_of(m):
    return "".join(re.findall(r"Lb([01])E", m.group(1))) + ("b" + m.group(2) if m.group(2) not in (None, "256") else "") + ("c" if m.group(3) == "1" else "") + ("r" if m.group(4) == "1" else "")


def compile_to_assembly(tree=ROOT, arithmetic=1, extra=()):
    """kernel_wavefront.hip with the Makefile's flags -> (path of the assembly, hipcc's resource remarks)"""
    csrc = os.path.join(tree, "opencl_pathtracer_amd", "csrc")
    out = os.path.join(tempfile.mkdtemp(), "wf.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           f"-DPTMI_DEFAULT_ARITHMETIC={arithmetic}", "-I" + os.path.join(tree, "include"), "-I" + csrc, "--cuda-device-only", "-S",
           os.path.join(csrc, "kernel_wavefront.hip"), "-o", out, "-Rpass-analysis=kernel-resource-usage", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-3000:])
    return out, r.stderr


def kernel_blocks(asm_path):
    """{instantiation key: [(loop depth of the block, [its instructions, comments stripped])]} in the order of the assembly"""
    blocks, cur = {}, None
    for line in open(asm_path):
        m = re.match(NAME + r"\w*:", line)
        if m:
            cur = blocks.setdefault(key_of(m), [])
            cur.append((0, []))
        elif cur is None:
            continue
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"(\.LBB|; %bb\.)", line):
            d = re.search(r"Depth=(\d+)", line)
            cur.append((int(d.group(1)) if d else 0, []))
        elif re.match(r"\s+[a-z]", line) and not line.lstrip().startswith("."):
            cur[-1][1].append(line.split(";")[0].strip())
    return blocks


def node_step_waits(blocks):
    """The node step inside the traversal loop (the depth-2 blocks): the block that loads a record's four quads - four
    global_load_dwordx4 from ONE address at offsets 0, 16, 32, 48 - and the s_waitcnt instructions behind them, in layout
    order through the loop's following blocks (the compiler ends the loads' block at the branch between the two box tests),
    up to the first that carries vmcnt(0).  -> (offsets in issue order, [operands of each wait], whether that vmcnt(0) stands
    before the loop's next vector memory load and before its end), or None where the loop holds no such block."""
    loop = [lines for depth, lines in blocks if depth == 2]
    for b, lines in enumerate(loop):
        loads = [(i, re.match(r"global_load_dwordx4 v\[\d+:\d+\], (\S+), (\S+?)(?: offset:(\d+))?$", l)) for i, l in enumerate(lines)]
        loads = [(i, m.group(1) + " " + m.group(2), int(m.group(3) or 0)) for i, m in loads if m]
        for k in range(len(loads) - 3):
            group = loads[k:k + 4]
            if len({base for _, base, _ in group}) != 1 or sorted(off for _, _, off in group) != [0, 16, 32, 48]:
                continue
            waits = []
            for l in lines[group[-1][0] + 1:] + [l for later in loop[b + 1:] for l in later]:
                if l.startswith("s_waitcnt "):
                    waits.append(l.split(None, 1)[1])
                    if "vmcnt(0)" in l:
                        return [off for _, _, off in group], waits, True
                elif re.match(r"(global|buffer|flat|scratch)_(load|atomic)", l):
                    break
            return [off for _, _, off in group], waits, False
    return None


def kernel_cfg(asm_path):
    """{instantiation key: [block]} in the order of the assembly, block = dict(label, header: it heads the traversal loop,
    loop: it belongs to that loop (the depth-2 loop), lines: its instructions, succ: indices of the blocks it can go on to)."""
    kernels, cur = {}, None
    for line in open(asm_path):
        m = re.match(NAME + r"\w*:", line)
        if m:
            cur = kernels.setdefault(key_of(m), [])
            cur.append(dict(label=None, header=False, loop=False, lines=[]))
        elif cur is None:
            continue
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            label = line.split(":")[0]
            cur.append(dict(label=label[1:] if label.startswith(".") else None, header=False, loop="Depth=2" in line and "Parent Loop" not in line, lines=[]))
        elif "Inner Loop Header: Depth=2" in line:  # (the comment line behind the header's label)
            cur[-1]["header"] = cur[-1]["loop"] = True
        elif re.match(r"\s+[a-z]", line) and not line.lstrip().startswith("."):
            cur[-1]["lines"].append(line.split(";")[0].strip())
    for blocks in kernels.values():
        at = {b["label"]: i for i, b in enumerate(blocks) if b["label"]}
        for i, b in enumerate(blocks):
            succ, falls = [], True
            for l in b["lines"]:
                m = re.match(r"s_c?branch\w* \.(LBB\d+_\d+)$", l)
                if m:
                    succ.append(at[m.group(1)])
                falls = not re.match(r"(s_branch|s_endpgm|s_setpc)", l)
            if falls and i + 1 < len(blocks):
                succ.append(i + 1)
            b["succ"] = succ
    return kernels


def _reach(blocks, start, allowed, forward=True):
    """indices reachable from `start` through `allowed` blocks, never going on THROUGH the loop header (a trip ends there)"""
    if forward:
        nxt = lambda i: [] if blocks[i]["header"] and i != start else blocks[i]["succ"]
    else:
        pred = {}
        for i, b in enumerate(blocks):
            for s in b["succ"]:
                if not blocks[s]["header"]:
                    pred.setdefault(s, []).append(i)
        nxt = lambda i: pred.get(i, [])
    seen, todo = {start}, [start]
    while todo:
        for j in nxt(todo.pop()):
            if j in allowed and j not in seen:
                seen.add(j)
                todo.append(j)
    return seen


def _is_record_block(lines):
    loads = [re.match(r"global_load_dwordx4 v\[\d+:\d+\], (\S+), (\S+?)(?: offset:(\d+))?$", l) for l in lines]
    loads = [(m.group(1) + " " + m.group(2), int(m.group(3) or 0)) for m in loads if m]
    return any(len({b for b, _ in loads[k:k + 4]}) == 1 and sorted(o for _, o in loads[k:k + 4]) == [0, 16, 32, 48] for k in range(len(loads) - 3))


def trip_paths(blocks):
    """The two kinds of trip of the traversal loop as block sets of kernel_cfg's blocks: every block that lies on a way from the
    loop header through the node step's record loads back to the header WITHOUT a block of the leaf pass's ray fetch
    (ds_bpermute), and the other way round.  -> dict(header, loop, node: the record block, node_path, leaf_path) of indices;
    None where the loop has no record block."""
    loop = {i for i, b in enumerate(blocks) if b["loop"]}
    header = next((i for i in loop if blocks[i]["header"]), None)
    node = next((i for i in sorted(loop) if _is_record_block(blocks[i]["lines"])), None)
    leaf = {i for i in loop if any(l.startswith("ds_bpermute") for l in blocks[i]["lines"])}
    if header is None or node is None or not leaf:
        return None

    def through(marks, avoid):
        allowed = loop - avoid
        ends = {i for i in allowed if header in blocks[i]["succ"]}  # (the back edges)
        from_header = _reach(blocks, header, allowed)
        to_header = set().union(*[_reach(blocks, e, allowed, forward=False) for e in ends]) if ends else set()
        path = set()
        for m in marks:
            before = from_header & _reach(blocks, m, allowed, forward=False)
            after = _reach(blocks, m, allowed) & to_header
            if m in from_header and m in to_header:
                path |= before | after
        return path

    return dict(header=header, loop=loop, node=node, node_path=through({node}, leaf), leaf_path=through(leaf, {node}))


def _mix(lines):
    vector = sum(l.startswith("v_") for l in lines)
    scalar = sum(l.startswith("s_") and not re.match(r"s_(waitcnt|nop)\b", l) for l in lines)
    return vector, scalar


REG_COPY = re.compile(r"v_mov_b(32|64)_e32 v\[?\d+(:\d+\])?, v\[?\d+")  # a v_mov between two vector registers (not a constant)


def trip_loop_copies(blocks):
    """What a trip of the traversal loop costs beyond its work, read off the assembly ("The trip loop's copies"):
    the loop's v_mov_b32 count and scratch accesses, the vector / scalar instructions (without waits and nops) of the node-trip
    path and of the leaf-pass path from the loop header to the back edge, and the register-to-register v_mov on the node trip's
    way IN (header to the first record load) and OUT (behind the step's last LDS operation to the back edge)."""
    p = trip_paths(blocks)
    if p is None:
        return None
    loop_lines = [l for i in sorted(p["loop"]) for l in blocks[i]["lines"]]
    lines_of = lambda idx: [l for i in sorted(idx) for l in blocks[i]["lines"]]
    node, allowed = p["node"], p["node_path"]
    # in: the path's blocks in front of the record block, and that block up to its first record load
    before = (_reach(blocks, node, allowed, forward=False) - {node}) & allowed
    first_load = next(k for k, l in enumerate(blocks[node]["lines"]) if l.startswith("global_load_dwordx4"))
    way_in = lines_of(before) + blocks[node]["lines"][:first_load]
    # out: behind the last LDS operation of the step (in layout order among the path's blocks behind the record block)
    behind = _reach(blocks, node, allowed)
    last = max((i for i in behind if any(l.startswith("ds_") for l in blocks[i]["lines"])), default=None)
    way_out = None
    if last is not None:
        k = max(k for k, l in enumerate(blocks[last]["lines"]) if l.startswith("ds_"))
        way_out = blocks[last]["lines"][k + 1:] + lines_of((_reach(blocks, last, allowed) - {last}) & behind)
    return {"loop v_mov": sum(l.startswith("v_mov_b32") for l in loop_lines),
            "loop scratch": sum(l.startswith("scratch_") for l in loop_lines),
            "node trip": _mix(lines_of(p["node_path"])), "leaf pass": _mix(lines_of(p["leaf_path"])),
            "copies in": [l for l in way_in if REG_COPY.match(l)],
            "copies out": None if way_out is None else [l for l in way_out if REG_COPY.match(l)],
            "full waits in": sum(l.startswith("s_waitcnt") and "vmcnt(0)" in l for l in way_in)}


def node_trip_tail(blocks):
    """The node trip's tail ("The node trip's tail"): the node-trip path from the step's push - the ds_write_b32
    behind the record loads - to the back edge, in layout order.  -> dict(reads: the ds_read instructions there, read points:
    the runs of them that no s_waitcnt divides, full lgkm waits: the s_waitcnt that carry lgkmcnt(0), scalar / vector: the
    instructions of that stretch, without waits and nops); None where the loop has no node step."""
    p = trip_paths(blocks)
    if p is None:
        return None
    behind = sorted(_reach(blocks, p["node"], p["node_path"]))
    push = next(((i, k) for i in behind for k, l in enumerate(blocks[i]["lines"]) if l.startswith("ds_write_b32")), None)
    if push is None:
        return None
    lines = blocks[push[0]]["lines"][push[1] + 1:] + [l for i in behind if i > push[0] for l in blocks[i]["lines"]]
    points, open_run = 0, False
    for l in lines:
        if l.startswith("ds_read"):
            points += not open_run
            open_run = True
        elif l.startswith("s_waitcnt"):
            open_run = False
    vector, scalar = _mix(lines)
    return {"reads": sum(l.startswith("ds_read") for l in lines), "read points": points,
            "full lgkm waits": sum(l.startswith("s_waitcnt") and "lgkmcnt(0)" in l for l in lines), "vector": vector, "scalar": scalar}


def resources(tree=ROOT, arithmetic=1, extra=(), region_forms=False):
    """region_forms: also the forms that render a rectangle (key suffix r).  Without them the keys are those of before regions
    existed: every launch of ptmi_render runs one of these, and the tests that pin figures name them."""
    return figures_of(*compile_to_assembly(tree, arithmetic, extra), region_forms=region_forms)


def figures_of(out, remarks, region_forms=False):
    """resources() of an assembly that exists: compile_to_assembly's (path, remarks) -> the dictionary, without compiling"""
    res = {}
    wanted = lambda key: region_forms or not key.endswith("r")
    for block in re.split(r"Function Name: ", remarks)[1:]:
        m = re.match(NAME, block)
        if not m or not wanted(key_of(m)):
            continue
        key = key_of(m)  # STATS PRE SS PLAIN NANSAFE [bN: lanes per workgroup] [c: the culling instantiation] [r: renders a rectangle]
        res[key] = {k.strip(): int(v) for k, v in re.findall(r"remark: [^\n]*?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", block)}
    for name, blocks in kernel_blocks(out).items():
        if not wanted(name):
            continue
        v = res[name]
        c = Counter(l.split()[0] for depth, lines in blocks if depth == 2 for l in lines)
        tot = lambda p: sum(n for i, n in c.items() if i.startswith(p))
        v["loop scratch"] = tot("scratch_")
        v["loop VALU"], v["loop SALU"], v["loop LDS"], v["loop VMEM"] = tot("v_"), tot("s_"), tot("ds_"), tot("global_") + tot("buffer_")
        # flat instructions: inside the traversal loop / on the way into it (the path-logic loop around it and the prologue:
        # everything but the depth-0 blocks behind the last loop block)
        last_loop = max((i for i, (depth, _) in enumerate(blocks) if depth > 0), default=-1)
        v["loop flat"] = tot("flat_")
        v["flat before loop"] = sum(l.startswith("flat_") for depth, lines in blocks[:last_loop + 1] if depth != 2 for l in lines)
        v["flat"] = sum(l.startswith("flat_") for _, lines in blocks for l in lines)
        v["node step"] = node_step_waits(blocks)
        v.update(outer_loop_memory(blocks))
    for name, blocks in kernel_cfg(out).items():
        if not wanted(name):
            continue
        res[name]["trip loop"] = trip_loop_copies(blocks)
        res[name]["tail"] = node_trip_tail(blocks)
    return res


def outer_loop_memory(blocks):
    """The body of the OUTER loop - the path-logic pass, the depth-1 blocks - as its memory chain shows in the assembly
    ("The pass's memory chain"): vector loads from memory (global_ / buffer_; spill reloads are scratch_ and are
    not counted), scalar loads, and the waits that let no vector memory operation stay outstanding (vmcnt(0))."""
    pass_lines = [l for depth, lines in blocks if depth == 1 for l in lines]
    return {"pass vector loads": sum(bool(re.match(r"(global|buffer)_load_", l)) for l in pass_lines),
            "pass scalar loads": sum(bool(re.match(r"s_(buffer_)?load_", l)) for l in pass_lines),
            "pass full waits": sum(l.startswith("s_waitcnt ") and "vmcnt(0)" in l for l in pass_lines)}


def trip_loop_text(t):
    if t is None:
        return "(no node step in the loop)"
    out = "-" if t["copies out"] is None else len(t["copies out"])
    return f'{t["loop v_mov"]} {t["node trip"][0]} {t["node trip"][1]} {t["leaf pass"][0]} {t["leaf pass"][1]} {len(t["copies in"])} {t["full waits in"]} {out}'


if __name__ == "__main__":
    tree = sys.argv[1] if len(sys.argv) > 1 else ROOT
    arith = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    res = resources(tree, arith, region_forms=True)
    print("STATS PRE SS PLAIN NANSAFE [b64: narrow workgroups] [c: culls leaves] [r: renders a rectangle, ptmi_render_region] | VGPRs spilled scratch occupancy | traversal loop: scratch VALU SALU LDS VMEM | flat: in the loop, "
          "before it, kernel | path-logic pass (the outer loop's body): vector loads, scalar loads, full vector-memory waits | "
          "node step: load offsets, then its waits | trip loop: v_mov in the loop; node-trip path vector, scalar instructions; leaf-pass path "
          "vector, scalar; register copies on a node trip's way in (header to the first record load), full vector-memory waits there, "
          "copies on its way out (behind the step's last LDS operation to the back edge) | node trip's tail (the push to the back edge): "
          "LDS reads, read points (runs of reads no wait divides), waits with lgkmcnt(0), vector, scalar instructions")
    for k in sorted(res):
        v = res[k]
        offsets, waits, closed = v["node step"] or ([], [], False)
        print("   ".join(k[:5]) + ("  " + k[5:] if len(k) > 5 else ""), "|", v["VGPRs"], v["VGPRs Spill"], v["ScratchSize"], v["Occupancy"], "|", v["loop scratch"], v["loop VALU"], v["loop SALU"],
              v["loop LDS"], v["loop VMEM"], "|", v["loop flat"], v["flat before loop"], v["flat"], "|",
              v["pass vector loads"], v["pass scalar loads"], v["pass full waits"], "|", ",".join(map(str, offsets)), "|", " / ".join(waits) + ("" if closed else " / (no vmcnt(0) before the next load)"), "|", trip_loop_text(v["trip loop"]), "|",
              " ".join(str(x) for x in v["tail"].values()) if v.get("tail") else "-")
