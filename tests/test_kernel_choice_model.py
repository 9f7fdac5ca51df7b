"""Which kernel a ptmi_render launch gets (csrc/kernel_choice.h) and the reader of the developer switches (csrc/dev_switches.h),
checked without a GPU.

tests/kernel_choice_model.cpp plays the header over the full product of its inputs, once per environment: the PTMI_LEAF_CULL
setting {unset, 0, 1, 2} times every other choice-affecting switch switched on alone.  This file holds the rules as the commit
before the header had them, spread over scene_layout.cpp, ptmi_scene_memory.cpp, ptmi_api.cpp and kernel_wavefront.hip, written out
independently (parent_*, transcriptions), and checks:
- every field of the upload's choice, the kernel kind and the launch's choice equals the parent's rule;
- for every choice, with_instance() finds an instantiation, and the one its callback was instantiated with equals the choice
  field by field - CULL and BLOCK change no result bit, so no render can check them;
- the instantiations the header lists are exactly the ones the parent's instance_for names: none unreachable, none new;
- a choice outside the list is refused;
- getenv occurs under csrc/ only in the reader and in the shim, and every switch of the reader's table has a row in
  INTEGRATION.md 4 that names the same moment.
"""
import itertools
import os
import re
import subprocess

import pytest

import model_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
MODEL_SRC = os.path.join(ROOT, "tests", "kernel_choice_model.cpp")
MAX_DEPTH = 30  # PTMI_BVH_MAX_DEPTH
WIDE, NARROW = 256, 64  # kWfBlock, kWfBlockNarrow
JITTERED, UNIFORM, RANDOM = 0, 1, 2  # the model's sampler index
WALK = (11, 22, 33)  # the NaN walk's counts the model uploads
OTHER_SWITCHES = ["PTMI_GENERIC_SHADING", "PTMI_GENERIC_TRIANGLES", "PTMI_GENERIC_BOXES", "PTMI_WIDE_RECORDS", "PTMI_WIDE_WORKGROUPS",
                  "PTMI_LITERAL_KERNEL", "PTMI_WALK_NAN_RAYS"]
ENVIRONMENTS = [dict(([("PTMI_LEAF_CULL", lc)] if lc is not None else []) + ([(sw, "1")] if sw else []))
                for lc in (None, "0", "1", "2") for sw in [None] + OTHER_SWITCHES]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return model_build.program([MODEL_SRC], tmp_path_factory.mktemp("kernel_choice"), "kernel_choice_model", opt="-O1", werror=True,
                               includes=[CSRC, os.path.join(ROOT, "include")])


def run(model, mode, env=None):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PTMI_")}
    return subprocess.run([model, mode], check=True, capture_output=True, text=True, env={**clean, **(env or {})}).stdout.splitlines()


# ---------------------------------------------------------------------------------------------------------------------------
# the parent commit's rules

def parent_leaf_cull_setting(env):
    """ptmi_api.cpp:115 (ptmi_ctx::leaf_cull starts at -1)"""
    v = env.get("PTMI_LEAF_CULL")
    return -1 if v is None else 0 if v[:1] == "0" else 2 if v[:1] == "2" else 1


def parent_upload(env, leaf_cull, nan, pre, plain, boxes, n_records, leaves):
    """scene_layout.cpp:150,172 and ptmi_scene_memory.cpp:133,189-204: (tris_precomputed, plain_shading, wide_records,
    boxes_ordered, nan_safe, nan_walk_box_tests, nan_walk_tri_tests, nan_walk_last_tri, leaf_cull)"""
    pre = pre and "PTMI_GENERIC_TRIANGLES" not in env
    plain = plain and "PTMI_GENERIC_SHADING" not in env
    wide = n_records > (1 << 26) or "PTMI_WIDE_RECORDS" in env
    walk = (0xFFFFFFFF, 0xFFFFFFFF, WALK[2]) if "PTMI_WALK_NAN_RAYS" in env else WALK
    ordered = boxes and "PTMI_GENERIC_BOXES" not in env
    cull_bits = pre and not nan
    cull = leaves >= 1024 if leaf_cull < 0 else leaf_cull != 0
    mask = (1 | 2 | (0 if leaf_cull == 1 else 4)) if cull and cull_bits else 0
    return (int(pre), int(plain), int(wide), int(ordered), int(nan), *walk, mask)


def parent_one_path_per_lane(env, mega, nan, sampler):
    """ptmi_scene_memory.cpp:21-27"""
    if mega:
        return True
    if not nan:
        return False
    return sampler == RANDOM or env.get("PTMI_LITERAL_KERNEL", "")[:1] == "1"


def parent_instance_for(ss, pre, nan_safe, leaf_cull, scheduler_stats, plain, narrow):
    """kernel_wavefront.hip:1282-1303: (STATS, PRE, SS, PLAIN, NANSAFE, BLOCK, CULL)"""
    T, F = True, False
    cull = pre and leaf_cull != 0
    if ss:
        return (T, T, T, F, T, WIDE, T) if pre else (T, F, T, F, T, WIDE, F)
    if scheduler_stats:
        return (T, T, F, F, T, WIDE, T) if pre else (T, F, F, F, T, WIDE, F)
    if nan_safe:
        if plain:
            return (F, T, F, T, T, WIDE, F)
        return (F, T, F, F, T, WIDE, F) if pre else (F, F, F, F, T, WIDE, F)
    if plain:
        if cull:
            return (F, T, F, T, F, NARROW, T) if narrow else (F, T, F, T, F, WIDE, T)
        return (F, T, F, T, F, NARROW, F) if narrow else (F, T, F, T, F, WIDE, F)
    if pre:
        if cull:
            return (F, T, F, F, F, NARROW, T) if narrow else (F, T, F, F, F, WIDE, T)
        return (F, T, F, F, F, NARROW, F) if narrow else (F, T, F, F, F, WIDE, F)
    return (F, F, F, F, F, WIDE, F)


def parent_launch(env, up, ss, scheduler_stats, sampler, rr, lights, depth, fit):
    """kernel_wavefront.hip:1187-1199,1347-1362: the instantiation, then (stack levels, wait_debt, LDS bytes)"""
    pre, plain_shading, nan_safe, leaf_cull = up[0], up[1], up[4], up[8]
    lv = min(max(depth, 1), MAX_DEPTH)
    plain = bool(pre and plain_shading and sampler == JITTERED and not rr and lights == 1 and not ss and not scheduler_stats)
    wait_debt = 768 if lv >= 16 else (320 if plain else 512)
    narrow = not fit and "PTMI_WIDE_WORKGROUPS" not in env
    inst = parent_instance_for(ss, pre, nan_safe, leaf_cull, scheduler_stats, plain, narrow)
    return (*map(int, inst), lv, wait_debt, (lv + 1 + 4 + 4) * inst[5] * 4)


PARENT_INSTANCES = {parent_instance_for(*a) for a in itertools.product((0, 1), (0, 1), (0, 1), (0, 7), (False, True), (False, True), (False, True))
                    if not (a[5] and not a[1])}  # (`plain` implies precomputed records)


# ---------------------------------------------------------------------------------------------------------------------------

def ints(part):
    return tuple(map(int, part.split()))


def test_the_upload_fields(model):
    n = 0
    for env in ENVIRONMENTS:
        setting = parent_leaf_cull_setting(env)
        for line in run(model, "upload", env):
            key, got = map(ints, line.split(" | "))
            leaf_cull, nan, pre, plain, boxes, r, leaves = key
            assert leaf_cull == setting, (env, line)
            want = parent_upload(env, setting, nan, pre, plain, boxes, (1, 1 << 26, (1 << 26) + 1)[r], leaves)
            assert got == want, (env, line, want)
            n += 1
    assert n == len(ENVIRONMENTS) * 2 ** 4 * 3 * 3


def test_every_choice_is_the_parents_and_is_dispatched_as_chosen(model):
    """The full product; the line's last part is the tuple with_instance()'s callback was instantiated with."""
    keys, reached = set(), set()
    for env in ENVIRONMENTS:
        setting = parent_leaf_cull_setting(env)
        lines = run(model, "table", env)
        assert lines.pop() == "refused 1 1", env
        for line in lines:
            parts = line.split(" | ")
            assert parts[4] != "none", (env, line)  # an instantiation exists
            key, up, kind, choice, called = map(ints, parts)
            leaf_cull, ss, stats, nan, pre, plain, sampler, rr, lights, mega, leaves, depth, fit = key
            assert leaf_cull == setting, (env, line)
            assert up == parent_upload(env, setting, nan, pre, plain, 1, 1000, leaves), (env, line)
            assert kind == (int(parent_one_path_per_lane(env, mega, nan, sampler)),), (env, line)
            want = parent_launch(env, up, ss, stats, sampler, rr, lights, depth, fit)
            assert choice == want, (env, line, want)
            assert called == choice[:7], (env, line)
            keys.add((tuple(sorted(env.items())), key))
            reached.add(choice[:7])
    depths = (1, 15, 16, 22, 23, MAX_DEPTH, MAX_DEPTH + 1)
    assert len(keys) == len(ENVIRONMENTS) * 2 ** 7 * 3 * 2 * 3 * len(depths) * 2
    assert {k[1][11] for k in keys} == set(depths) and {k[1][10] for k in keys} == {0, 1023, 1024}
    # none of the listed instantiations is unreachable
    assert reached == {tuple(map(int, i)) for i in PARENT_INSTANCES}


def test_the_header_lists_the_parents_instantiations(model):
    listed = [ints(line) for line in run(model, "list")]
    assert len(listed) == len(set(listed)) == 16
    assert set(listed) == {tuple(map(int, i)) for i in PARENT_INSTANCES}


# ---------------------------------------------------------------------------------------------------------------------------
# the sources

PARSE = ["is set", "first character", "integer", "reduce mode"]
# dev_switches.h's Moment, in its order: what a row of INTEGRATION.md 4 must say
MOMENTS = ["once per process", "`ptmi_setup_context`", "`ptmi_initialize_memory`", "kernel kind", "`ptmi_render` call", "wavefront launch",
           "ray-query launch", "guide launch", "readback"]


def test_getenv_only_in_the_reader_and_the_shim():
    found = set()
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), errors="replace") as f:
            if "getenv" in f.read():
                found.add(name)
    assert found == {"dev_switches.h", "PathTracer_HIP.cpp"}
    with open(os.path.join(CSRC, "dev_switches.h")) as f:
        assert f.read().count("getenv(") == 1


def test_every_switch_has_its_row_in_the_integration_guide(model):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = text[text.index("## 4. Switches"):]
    section = section[:section.index("\n## ", 1)] if "\n## " in section[1:] else section
    rows = {}
    for line in section.splitlines():
        m = re.match(r"\| `(PTMI_[A-Z_]+)[^|]*\| ([^|]+) \|", line)
        if m:
            rows[m.group(1)] = m.group(2).strip()
    table = [line.split() for line in run(model, "switches")]
    assert len(table) == 16 and all(int(parse) < len(PARSE) for _, parse, _ in table)
    for name, _, moment in table:
        assert name in rows, name + " has no row in INTEGRATION.md 4"
        assert rows[name] == MOMENTS[int(moment)], (name, rows[name])
    # ... and the guide lists no switch of the library that the reader does not know (PTMI_LIBRARY is the Python binding's)
    assert set(rows) - {name for name, _, _ in table} == {"PTMI_LIBRARY"}
