"""The random scene call sequences of api_fuzz_cases.py, checked without a GPU: the conditions their inputs must meet for a stale
scene to be noticed - the states, the looks (materials, lights, sky) and the reprojection's two tolerance sets included - what
the shipped scripts cover, and that the executor catches a backend with a defect.  The backend here is
a fake made of the same oracle and yardstick data as the model, with one switch per defect; its filter is the yardstick of
denoise_cases.py on its own image and guide planes, so a defect in what the filter reads, guides itself by or leaves behind is
a switch like the others; so are its path sums, its reprojection (reproject_cases.py) and its display (display_cases.py).  The
states walked: every (camera, version) at the base look, and every look at (camera 0, version 0) and at one other (camera,
version), not the full product.  A failed condition is mended by choosing other seeds in api_fuzz_cases.py (VERSION_SEEDS, RAY_SEED,
GENERATOR_SEED, the looks), never by relaxing the condition."""
import itertools

import numpy as np
import pytest

from opencl_pathtracer_amd import PtmiError, backend, output
import api_fuzz_cases as F
import display_cases as DC
import guide_cases as G
import path_query_cases as P
import ray_query_cases as Q
import scene_update_cases as U

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (the hostile scenes divide 0 by 0 on purpose, as the importer would)
WORLD = F.WORLD
BASE = F.BASE_LOOK
# every (camera, version) at the base look, and every look at (camera 0, version 0) and at one other (camera, version)
STATES = {name: F.states_of(name) for name in F.SCENES}
ARITHMETICS = pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
GUIDE_ITERATIONS = range(max(F.GUIDE_FIRSTS) + 3)


def tree_bytes(bvh):
    return np.ascontiguousarray(bvh).tobytes()


# ---------------------------------------------------------------------------------------------- conditions on the chosen inputs

@pytest.mark.parametrize("name", F.SCENES)
def test_variants_are_accepted(name):
    anchor = WORLD.anchor(name)
    for t in F.VERSIONS:  # (the NANSAFE scenes are sent versions 1 and 2 as well, to be refused for another reason)
        rc, msg, _ = U.bvh_refit(WORLD.triangles(name, t), anchor.bvh)
        assert rc == 0, (t, msg)
    for state in STATES[name]:
        backend.validate_scene(WORLD.scene(state), F.W, F.H, F.D)  # raises with the library's message
    assert tree_bytes(WORLD.scene((name, 0, 0, BASE)).bvh) == tree_bytes(anchor.bvh)  # a refit to version 0 is the tree as built


@pytest.mark.parametrize("name", [n for n in F.SCENES if n not in F.NANSAFE])
def test_refit_order_does_not_matter(name):
    base = WORLD.anchor(name).bvh
    direct = {}
    for t in F.VERSIONS:
        rc, msg, direct[t] = U.bvh_refit(WORLD.triangles(name, t), base)
        assert rc == 0, msg
    for chain in ((0, 1, 2), (0, 2, 1), (1, 0), (2, 0), (1, 2, 0), (2, 1, 2)):
        tree = base
        for t in chain:
            rc, msg, tree = U.bvh_refit(WORLD.triangles(name, t), tree)
            assert rc == 0, msg
        assert tree_bytes(tree) == tree_bytes(direct[chain[-1]]), chain


@ARITHMETICS
@pytest.mark.parametrize("name", F.SCENES)
def test_states_are_distinguishable(name, da):
    """Iteration 0's image and the guide planes of iteration 0 differ between any two states of a scene, and so do the expected
    hits of both kinds wherever the two states differ in their triangles.  The camera is no input of a ray query (the rays are
    the caller's, the same in every state), so two states with the same triangles MUST expect the same hits: asserted too.
    Neither is a look: it changes the image (test_every_look_shows) and not one hit."""
    for a, b in itertools.combinations(STATES[name], 2):
        image_a, image_b = WORLD.per_iteration(a, da, 0)[0], WORLD.per_iteration(b, da, 0)[0]
        assert not np.array_equal(image_a.view(np.uint32), image_b.view(np.uint32)), (a, b)
        if a[:3] != b[:3]:  # (the lights are on no guide plane, and a sky only where the camera sees it)
            assert G.describe_difference(WORLD.planes(a, da, 0, 1)[0], WORLD.planes(b, da, 0, 1)[0]), (a, b)
        for any_hit in (False, True):
            same = np.array_equal(Q.words(WORLD.hits(a, da)[1][any_hit]), Q.words(WORLD.hits(b, da)[1][any_hit]))
            assert same == (a[2] == b[2]), (a, b, any_hit)
            if a[2] != b[2]:  # ... and already in the 257 rays of the middle batch
                assert not np.array_equal(Q.words(WORLD.hits(a, da)[1][any_hit][:257]), Q.words(WORLD.hits(b, da)[1][any_hit][:257])), (a, b)


@ARITHMETICS
@pytest.mark.parametrize("name", F.SCENES)
def test_every_look_shows(name, da):
    """The conditions on the looks (api_fuzz_cases.MATERIAL_LOOKS, LIGHT_LOOKS, SKY_LOOKS), met by the oracle alone: every scene
    is accepted; at every camera any two looks differ in iteration 0's image, so that no axis is a sky no path reaches or a
    light that lights nothing; material looks 1 and 2 each change the albedo plane of the guides; the path sums of the scene's
    rays differ between any two looks; and the plain / general verdict is what the look was made for."""
    looks = F.looks_of(name)
    for c in F.CAMERAS:
        images = {}
        for look in looks:
            backend.validate_scene(WORLD.scene((name, c, 0, look)), F.W, F.H, F.D)
            images[look] = WORLD.per_iteration((name, c, 0, look), da, 0)[0].view(np.uint32)
        for a, b in itertools.combinations(looks, 2):
            assert not np.array_equal(images[a], images[b]), (c, a, b)
    base = WORLD.planes((name, 0, 0, BASE), da, 0, 1)[0]["albedo"].view(np.uint32)
    for m in (1, 2):
        assert not np.array_equal(WORLD.planes((name, 0, 0, (m, 0, 0)), da, 0, 1)[0]["albedo"].view(np.uint32), base), m
    sums = {look: P.words(WORLD.path_sums((name, 0, 0, look), da, 257, 0, 1, 0)) for look in looks}
    for a, b in itertools.combinations(looks, 2):
        assert not np.array_equal(sums[a], sums[b]), (a, b)
    for look in looks:
        plain = F.plain_verdict(WORLD.scene((name, 0, 0, look)))
        assert plain == (name == "cornell" and look[:2] == (0, 0)), look
    scene, m = F.TEXTURE_FLIP  # the look that makes a plain colour textured, on a scene that has a texture; cornell has none
    before, after = WORLD.materials(scene, 0), WORLD.materials(scene, m)
    assert ((before["isSimpleColor"] != 0) & (after["isSimpleColor"] == 0)).any() and len(WORLD.anchor(scene).textures)
    assert len(WORLD.anchor("cornell").textures) == 0


@ARITHMETICS
@pytest.mark.parametrize("name", [n for n in F.SCENES if n not in F.NANSAFE])
def test_path_sums_follow_the_triangles(name, da):
    """... and differ between any two triangle versions: a path call that ignores an update is seen."""
    sums = {t: P.words(WORLD.path_sums((name, 0, t, BASE), da, 257, 0, 1, 0)) for t in F.VERSIONS}
    for a, b in itertools.combinations(F.VERSIONS, 2):
        assert not np.array_equal(sums[a], sums[b]), (a, b)


@ARITHMETICS
@pytest.mark.parametrize("name", F.SCENES)
def test_the_reprojection_has_something_to_do(name, da):
    """Between any two of the cameras, after three iterations: with the default tolerances some hit pixels keep their history
    and some lose it; the narrow set carries fewer pixels and caps the count at its max_history of 2.  A condition on the
    cameras and the two sets chosen, met by the yardsticks alone."""
    for a, b in itertools.permutations(F.CAMERAS, 2):
        kept = {}
        for tolerances in F.REPROJECT_SETS:
            m = F.Model(WORLD, da)
            m.upload((name, a, 0, BASE))
            m.render(0, 3)
            m.reprojected(b, tolerances, 0, 1)
            assert m.state == (name, b, 0, BASE)
            kept[tolerances] = m.count
        hit = WORLD.planes((name, b, 0, BASE), da, 0, 1)[0]["hit_count"] > 0
        default, narrow = kept["defaults"] > 0, kept["narrow"] > 0
        assert not (default & ~hit).any() and default.any() and (hit & ~default).any(), (a, b, int(default.sum()), int(hit.sum()))
        assert narrow.any() and narrow.sum() < default.sum() and kept["narrow"].max() == 2 and kept["defaults"].max() == 3, (a, b)


def filtered(state, da, sigmas, demodulate, passes):
    """the filter's yardstick on iteration 0's image, guided by iteration 0's planes"""
    color, count = WORLD.per_iteration(state, da, 0)[:2]
    params = dict(F.SIGMA_SETS[sigmas], passes=passes, demodulate=demodulate, guide_iterations=1)
    return F.denoise_yardstick((color, count), WORLD.planes(state, da, 0, 1)[0], params)


FILTERS = [(sigmas, demodulate) for sigmas in sorted(F.SIGMA_SETS) for demodulate in (False, True)]


@ARITHMETICS
@pytest.mark.parametrize("name", F.SCENES)
def test_the_filter_has_something_to_do(name, da):
    """Five passes change at least a quarter of the pixels against none, in every state, with either set of sigmas, demodulated
    or not: a filter that ran fewer passes, or none, is seen.  The quarter is a condition on the scenes and sigmas chosen (the
    yardstick alone gives at least 0.35 on every one of them), not a measurement of any filter."""
    for state in STATES[name]:
        for sigmas, demodulate in FILTERS:
            five, none = (filtered(state, da, sigmas, demodulate, passes).view(np.uint32)[..., :3] for passes in (5, 0))
            changed = (five != none).any(axis=2).mean()
            assert changed >= 0.25, (state, sigmas, demodulate, changed)


@ARITHMETICS
@pytest.mark.parametrize("name", F.SCENES)
def test_filtered_states_are_distinguishable(name, da):
    """The filtered iteration-0 images of any two states of a scene differ, whichever of the scripts' filters made them: a
    filter guided by, or fed from, a stale scene is seen."""
    for sigmas, demodulate in FILTERS:
        for passes in (0, 5):
            images = {state: filtered(state, da, sigmas, demodulate, passes).view(np.uint32) for state in STATES[name]}
            for a, b in itertools.combinations(STATES[name], 2):
                assert not np.array_equal(images[a], images[b]), (a, b, sigmas, demodulate, passes)


@ARITHMETICS
@pytest.mark.parametrize("name", F.SCENES)
def test_the_ray_set_is_mixed(name, da):
    for state in STATES[name]:
        rays, want, replaced = WORLD.hits(state, da)
        n = len(rays)
        assert n == F.N_RAYS == max(F.BATCHES) and len(replaced) < n // 20
        hit = want[False]["triangle_id"] != Q.MISS
        limited = np.isfinite(rays["max_squared_distance"])
        assert (~hit).sum() >= 0.10 * n and hit.sum() >= 0.30 * n, (state, int(hit.sum()), n)
        assert limited.sum() >= 0.10 * n and (hit & limited).any() and (~hit & limited).any(), state
        assert (want[True]["triangle_id"] != Q.MISS).sum() >= 0.30 * n


@ARITHMETICS
@pytest.mark.parametrize("name", F.SCENES)
def test_guide_exclusions_stay_under_the_cap(name, da):
    """... over every sample of every iteration a script can ask for (the yardstick checks each hit's primary ray on the way)."""
    for state in STATES[name]:
        census = WORLD.yardstick(state, da).census(GUIDE_ITERATIONS)
        assert census["hits"] > 0.1 * (census["hits"] + census["misses"]), (state, census)
        assert census["excluded"] < G.MAX_EXCLUDED * census["hits"], (state, census)


# ---------------------------------------------------------------------------------------------- what the shipped scripts cover

def shipped_scripts():
    return [((seed, cap, ids), F.script(seed, F.DEVICES[ids], cap)) for seed, cap, ids in F.shipped_cases()]


def test_scripts_are_deterministic_plain_tuples():
    for (seed, cap, ids), ops in shipped_scripts()[:6]:
        assert ops == F.script(seed, F.DEVICES[ids], cap) and ops[0][0] == "upload" and F.N_OPS <= len(ops) <= F.N_OPS + 3
        assert all(type(op) is tuple for op, _ in F.flat(ops))
    for seed in F.SUPER_SAMPLING_SEEDS:
        assert F.script(seed, None, None, super_sampling=True) == F.script(seed, None, None, super_sampling=True)


def test_script_coverage():
    total = dict.fromkeys(F.NEW_OPS, 0)
    positions = {p: set() for p in ("mid-walk", "after a burst", "between a snapshot and its read, several devices", "first after an upload", "cap 1")}
    nansafe_update = back_to_base = scratch_grows = device_route = 0
    for (seed, cap, ids), ops in shipped_scripts():
        for i, op in enumerate(ops):
            if op[0] in F.NEW_OPS and i:
                before = ops[i - 1]
                if before[0] == "burst":
                    positions["after a burst"].add(op[0])
                if before[0] == "upload":
                    positions["first after an upload"].add(op[0])
                if ids != "one" and before[0] == "snapshot" and i + 1 < len(ops) and ops[i + 1][:2] == ("read_slot", before[1]):
                    positions["between a snapshot and its read, several devices"].add(op[0])
        name, uploaded, updated, smaller, grown = None, 0, False, False, False
        for op, in_walk in F.flat(ops):
            kind = op[0]
            if kind in F.NEW_OPS:
                total[kind] += 1
                if in_walk:
                    positions["mid-walk"].add(kind)
                if cap == 1:
                    positions["cap 1"].add(kind)
                device_route += kind in ("query", "guides") and op[-1] == "device"
                # (device pointers: one device only; the display calls are sent to several all the same, to be refused)
                assert ids == "one" or op[-1] != "device" or kind in ("tonemap", "histogram")
            if kind == "upload":
                name, uploaded, updated = op[1], op[3], False
            elif kind == "update":
                nansafe_update += name in F.NANSAFE
                back_to_base += uploaded != 0 and not updated and op[1] == 0
                updated = True
            elif kind == "query" and op[3] == "host":  # (a device-pointer query does not go through the context's scratch)
                scratch_grows += op[2] > 1024 and smaller and not grown
                grown |= op[2] > 1024
                smaller |= op[2] <= 1024
    assert all(n >= 20 for n in total.values()), total
    for where, kinds in positions.items():
        assert kinds == set(F.NEW_OPS), (where, sorted(set(F.NEW_OPS) - kinds))
    assert nansafe_update and back_to_base and scratch_grows and device_route, (nansafe_update, back_to_base, scratch_grows, device_route)
    union = set()
    for seed in F.SUPER_SAMPLING_SEEDS:
        kinds = {op[0] for op in F.script(seed, None, None, super_sampling=True)}
        assert {"camera", "update", "query", "guides"} <= kinds, (seed, kinds)
        union |= kinds
    assert {"variance", "resume", "snapshot", "read_slot", "upload", "bad_update", "bad_camera"} <= union, union
    assert {"reprojected", "materials", "lights", "sky", "paths", "tonemap", "histogram", "update_device"} <= union, union
    denoise_coverage()
    new_operation_coverage()


def made_in_order(ops):
    """the calls in the order they are made: an operation inside a walk, and the one behind a walk, follow a call of the walk"""
    made, behind_a_walk_call = [], False
    for op, in_walk in F.flat(ops):
        made += [("walk call",), op] if in_walk or behind_a_walk_call else [op]
        behind_a_walk_call = in_walk or op[0] == "walk"
    return made


def not_waited_for(op, ids):
    """a call through device pointers that returns before its work is done"""
    if op[0] in ("query", "guides", "paths"):
        return op[-1] == "device"
    if op[0] == "denoise":
        return op[-1] in ("device", "planes")
    return op[0] in ("tonemap", "histogram") and (op[-1] in ("planes", "mean") or (op[-1] == "device" and ids == "one"))


def new_operation_coverage():
    """What the shipped scripts ask of the path, reprojection, display and scene-edit calls (the positions and the counts of
    every kind: test_script_coverage)."""
    routes = {kind: set() for kind in ("paths", "tonemap", "histogram")}
    behind_async, by_call, by_upload, plain_flips, behind, lazy_copy = set(), set(), set(), set(), set(), set()
    refusals, display_params, path_params, tolerances = set(), set(), set(), set()
    nansafe_lights = texture_flip = pipeline = refused_display = same_camera = 0
    for (seed, cap, ids), ops in shipped_scripts():
        made = made_in_order(ops)
        name, look, camera = None, None, None
        for i, op in enumerate(made):
            kind = op[0]
            before = made[i - 1] if i else ("start",)
            if kind in F.NEW_OPS and not_waited_for(before, ids):
                behind_async.add(kind)
            if kind in routes:
                routes[kind].add(op[-1])
            if kind == "upload":
                name, camera, look = op[1], op[2], list(op[4])
                by_upload |= {(axis, value) for axis, value in enumerate(op[4])}
            elif kind == "camera":
                camera = op[1]
            elif kind == "materials":
                by_call.add((0, op[1]))
                if name == "cornell" and look[1] == 0 and (look[0] == 0) != (op[1] == 0):
                    plain_flips.add(("materials", "out" if look[0] == 0 else "back"))
                before_table, after_table = WORLD.materials(name, look[0]), WORLD.materials(name, op[1])
                texture_flip += bool(((before_table["isSimpleColor"] != 0) & (after_table["isSimpleColor"] == 0)).any())
                look[0] = op[1]
            elif kind == "lights":
                nansafe_lights += name in F.NANSAFE
                if name not in F.NANSAFE:
                    by_call.add((1, op[1]))
                    if name == "cornell" and look[0] == 0 and look[1] != op[1]:
                        plain_flips.add(("lights", "out" if look[1] == 0 else "back"))
                    look[1] = op[1]
            elif kind == "sky":
                by_call.add((2, op[1]))
                look[2] = op[1]
            elif kind in ("bad_materials", "bad_lights", "bad_camera"):
                refusals.add((kind, op[1]))
            elif kind == "reprojected":
                behind.add("write of count 0" if before[0] == "write" and before[2] == 0 else before[0])
                tolerances.add(op[2])
                same_camera += op[1] == camera
                camera = op[1]
            elif kind == "tonemap":
                display_params |= {("tone", op[1]), ("transfer", op[2]), ("white", op[4]), ("rgba", op[5])}
                display_params.add(("exposure", op[3], "host" if op[-1] == "host" else "pointers"))
            elif kind == "paths":
                path_params |= {("batch", op[1]), ("iterations", op[3]), ("first_index", op[4])}
            if kind in ("tonemap", "histogram"):
                pipeline += op[-1] == "mean" and before[0] == "denoise" and before[-1] in ("device", "planes")
                refused_display += op[-1] == "device" and ids != "one"
        for i, op in enumerate(ops):  # (not inside a walk: a snapshot, the reprojected call, the read of that slot)
            if op[0] == "reprojected" and ops[i - 1][0] == "snapshot" and i + 1 < len(ops) and ops[i + 1][:2] == ("read_slot", ops[i - 1][1]):
                lazy_copy.add(ids)
    new = set(F.NEW_OPS[7:])
    assert new <= behind_async, sorted(new - behind_async)
    assert routes == {"paths": {"host", "device"}, "tonemap": set(F.DISPLAY_ROUTES), "histogram": set(F.DISPLAY_ROUTES)}, routes
    axes = {(0, m) for m in F.MATERIALS} | {(1, g) for g in F.LIGHTS} | {(2, k) for k in F.SKIES}
    assert by_call == axes and by_upload == axes, (sorted(axes - by_call), sorted(axes - by_upload))
    assert plain_flips == {(axis, way) for axis in ("materials", "lights") for way in ("out", "back")}, plain_flips
    assert {"render", "write of count 0", "clear"} <= behind, behind
    assert {"two", "three"} <= lazy_copy, lazy_copy
    assert refusals >= {("bad_materials", "beyond"), ("bad_materials", "texture"), ("bad_lights", "size"), ("bad_lights", "position")} | \
        {("bad_camera", which) for which in range(4)}, refusals
    assert tolerances == set(F.REPROJECT_SETS) and same_camera, (tolerances, same_camera)
    want = {("tone", v) for v in DC.TONES} | {("transfer", v) for v in DC.TRANSFERS} | {("white", v) for v in F.WHITES} | \
        {("rgba", v) for v in (False, True)} | {("exposure", v, how) for v in F.EXPOSURES for how in ("host", "pointers")}
    assert display_params == want, sorted(want - display_params, key=str)
    assert path_params == {("batch", v) for v in F.PATH_BATCHES} | {("iterations", v) for v in (1, 2, 3)} | \
        {("first_index", v) for v in F.PATH_FIRST_INDICES}, path_params
    assert nansafe_lights and texture_flip and pipeline and refused_display, (nansafe_lights, texture_flip, pipeline, refused_display)
    tried = set()
    for seed in F.SUPER_SAMPLING_SEEDS:  # (refused there, camera and all)
        tried |= {op[0] for op, _ in F.flat(F.script(seed, None, None, super_sampling=True))}
    assert "reprojected" in tried


def denoise_coverage():
    """What the shipped scripts ask of the filter: every pass count, both sigma sets with and without demodulation, both kernels
    of steps 1 and 2, all three routes, and a call directly behind each operation that changes what the filter reads."""
    passes, sigma_flags, untiled, routes, behind, lazy_copy = set(), set(), set(), set(), set(), set()
    nansafe = next_to_display = 0
    for (seed, cap, ids), ops in shipped_scripts():
        made = made_in_order(ops)
        name = None
        for i, op in enumerate(made):
            if op[0] == "upload":
                name = op[1]
            if op[0] != "denoise":
                continue
            _, first, n, p, sigmas, demodulate, tiles_off, route = op
            assert first in F.GUIDE_FIRSTS and 1 <= n <= 3 and sigmas in F.SIGMA_SETS and route in F.DENOISE_ROUTES
            passes.add(p)
            sigma_flags.add((sigmas, demodulate))
            if p >= 1:
                untiled.add(tiles_off)
            routes.add(route)
            nansafe += name in F.NANSAFE
            before, after = made[i - 1], made[i + 1] if i + 1 < len(made) else ("end",)
            next_to_display += "display" in (before[0], after[0])
            behind.add("write of count 0" if before[0] == "write" and before[2] == 0 else before[0])
        for i, op in enumerate(ops):  # (not inside a walk: a snapshot, the denoise, the read of that slot)
            if op[0] == "denoise" and op[7] == "host" and ops[i - 1][0] == "snapshot" and i + 1 < len(ops) and ops[i + 1][:2] == ("read_slot", ops[i - 1][1]):
                lazy_copy.add(ids)
    assert passes == set(F.DENOISE_PASSES), passes
    assert sigma_flags == {(s, d) for s in F.SIGMA_SETS for d in (False, True)}, sigma_flags
    assert untiled == {False, True} and routes == set(F.DENOISE_ROUTES), (untiled, routes)
    assert {"two", "three"} <= lazy_copy, lazy_copy
    assert {"update", "camera", "bad_update", "clear", "write of count 0"} <= behind, behind
    assert nansafe and next_to_display, (nansafe, next_to_display)
    for seed in F.SUPER_SAMPLING_SEEDS:
        assert any(op[0] == "denoise" for op, _ in F.flat(F.script(seed, None, None, super_sampling=True))), seed


# ---------------------------------------------------------------------------------------------- a backend with defects

DEFECTS = ("guides ignore the last camera", "queries ignore the last update", "the next two renders keep the old camera",
           "a refused update rewrites the triangles", "a query adds to the counters", "a guides call clears the accumulators",
           "the filter's guides ignore the last camera", "the filter's guides ignore the last update",
           "the filter reads the accumulators as they were before the last render", "a denoise call leaves its result in the accumulators",
           "several devices: a denoise overwrites the slot of the last snapshot", "the filter ignores the demodulation flag",
           "paths ignore the last triangle update", "paths ignore the last material edit", "a paths call adds to the counters",
           "the reprojected call keeps the image as it was", "the reprojection reads the accumulators as they were before the last render",
           "after a reprojected call the next two renders keep the old camera", "a refused reprojected call (super-sampling) moves the camera",
           "a reprojected call resets the counters", "the tone-mapped display ignores the exposure",
           "the display reads the accumulators as they were before the last render", "the histogram is taken after exposure",
           "a device triangle update does not reach the queries", "the guides' albedo ignores the last material edit",
           "after a lights edit the next two renders keep the old lights", "a sky edit restores the uploaded materials",
           "a refused lights edit on a NANSAFE scene changes the lights", "several devices: a material edit reaches devices[0] only")
READS = {"read_image", "read_slot", "statistics", "counters", "display", "walk", "walk call", "final image"}
# (the host routes of these three read the image behind their own call, and hold it against the model)
IMAGES = READS | {"denoise", "tonemap", "histogram"}
RENDERS = {"render", "walk", "walk call", "burst"}
ANYWHERE = IMAGES | {"guides", "paths", "materials", "reprojected"}  # (wherever the look shows)
# defect: (the operations at which it may come to light, the operations of which one must be among the calls reported with it)
# (a host-route denoise reads the image behind its own call, so what a denoise leaves in the accumulators may show there first)
# (the executor and HostIO ask render_guides for the planes every denoise is held against: a defect of the guides call may come to
# light at a denoise, or be set off by one)
SURFACES = {DEFECTS[0]: ({"guides", "denoise"}, {"camera"}), DEFECTS[1]: ({"query"}, {"update"}), DEFECTS[2]: (READS, {"camera"}),
            DEFECTS[3]: (READS | {"query", "guides", "denoise"}, {"bad_update"}), DEFECTS[4]: ({"counters", "walk"}, {"query"}),
            DEFECTS[5]: (IMAGES, {"guides", "denoise"}),
            DEFECTS[6]: ({"denoise"}, {"camera"}), DEFECTS[7]: ({"denoise"}, {"update"}),
            DEFECTS[8]: ({"denoise"}, {"render", "walk", "walk call", "burst"}), DEFECTS[9]: (READS | {"denoise"}, {"denoise"}),
            DEFECTS[10]: ({"read_slot"}, {"denoise"}), DEFECTS[11]: ({"denoise"}, {"denoise"}),
            DEFECTS[12]: ({"paths"}, {"update", "update_device"}), DEFECTS[13]: ({"paths"}, {"materials"}),
            DEFECTS[14]: ({"counters", "walk"}, {"paths"}), DEFECTS[15]: (IMAGES, {"reprojected"}), DEFECTS[16]: (IMAGES, {"reprojected"}),
            DEFECTS[17]: (IMAGES, {"reprojected"}), DEFECTS[18]: (ANYWHERE, {"reprojected"}), DEFECTS[19]: ({"counters", "walk"}, {"reprojected"}),
            DEFECTS[20]: ({"tonemap"}, {"tonemap"}), DEFECTS[21]: ({"tonemap"}, RENDERS), DEFECTS[22]: ({"tonemap", "histogram"}, {"tonemap"}),
            DEFECTS[23]: ({"query"}, {"update_device"}), DEFECTS[24]: ({"guides", "denoise"}, {"materials"}), DEFECTS[25]: (IMAGES, {"lights"}),
            DEFECTS[26]: (ANYWHERE, {"sky"}), DEFECTS[27]: (ANYWHERE, {"lights"}), DEFECTS[28]: (IMAGES, {"materials"})}
SUPER_SAMPLING_DEFECTS = (DEFECTS[18],)  # (what only a super-sampling context can get wrong: looked for in those scripts)


class FakeBackend:
    """The Backend methods the executor uses, answered from a model of its own."""

    def __init__(self, default_arithmetic, megakernel=False, super_sampling=False, defect=None, n_devices=1):
        assert defect is None or defect in DEFECTS
        self.m = F.Model(WORLD, default_arithmetic, super_sampling)
        self.megakernel, self.defect, self.n_devices = megakernel, defect, n_devices
        self.guide_camera = self.query_version = self.stale = None
        self.filter_camera = self.filter_version = self.before_render = self.last_slot = None
        self.path_version = self.path_materials = self.guide_materials = self.uploaded_materials = self.old_materials = None
        self.table, self.exposure = None, 1.0

    def initialize_memory(self, scene):
        self.m.upload(scene.fuzz_state)
        name, self.guide_camera, self.query_version, (m, _, _) = scene.fuzz_state
        _, self.filter_camera, self.filter_version, _ = scene.fuzz_state
        self.path_version, self.path_materials, self.guide_materials, self.uploaded_materials = self.query_version, m, m, m
        self.table = U.raw_copy(WORLD.materials(name, m))
        self.stale = self.before_render = self.last_slot = self.old_materials = None

    def literal_kernel_reason(self):
        return "records that can yield NaN distances" if self.m.state[0] in F.NANSAFE else None

    def _camera_id(self, vectors, who):
        if not all(np.isfinite(np.asarray(v, np.float32)).all() for v in vectors):
            raise PtmiError(F.UNSUPPORTED, f"{who}: a camera vector is not finite")
        for c in F.CAMERAS:
            sc = WORLD.camera(self.m.state[0], c)
            if all(np.array_equal(np.asarray(v, np.float32), np.asarray(w, np.float32)) for v, w in
                   zip(vectors, (sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp))):
                return c
        raise AssertionError("a camera the scripts do not have")

    def set_camera(self, *vectors):
        c = self._camera_id(vectors, "ptmi_set_camera")
        name, old, version, look = self.m.state
        if self.defect == DEFECTS[2] and c != old:
            self.stale = [dict(camera=old), 2]
        self.m.state = (name, c, version, look)
        if self.defect != DEFECTS[0]:
            self.guide_camera = c
        if self.defect != DEFECTS[6]:
            self.filter_camera = c

    def set_camera_reprojected(self, position, direction, right, up, guide_first_iteration=0, guide_iterations=1, **tolerances):
        c = self._camera_id((position, direction, right, up), "ptmi_set_camera_reprojected")
        name, old, version, look = self.m.state
        if self.m.ss:
            if self.defect == DEFECTS[18]:
                self.m.state, self.guide_camera, self.filter_camera = (name, c, version, look), c, c
            raise PtmiError(F.UNSUPPORTED, "ptmi_set_camera_reprojected: a super_sampling context's variance accumulator cannot be carried over")
        chosen = [key for key, values in F.REPROJECT_SETS.items() if values == tolerances]
        assert len(chosen) == 1, tolerances
        if self.defect == DEFECTS[15]:
            self.m.state = (name, c, version, look)
        else:
            image = self.before_render if self.defect == DEFECTS[16] and self.before_render else None
            self.m.reprojected(c, chosen[0], guide_first_iteration, guide_iterations, image=image)
        if self.defect == DEFECTS[17] and c != old:
            self.stale = [dict(camera=old), 2]
        if self.defect == DEFECTS[19]:
            self.m.totals = None
        self.guide_camera = self.filter_camera = c
        self.before_render = None

    def _triangles(self, tris, device=False):
        name, camera, version, look = self.m.state
        if len(tris) != len(WORLD.triangles(name, 0)):
            raise PtmiError(F.INVALID_ARGUMENT, "ptmi_update_triangles: the topology cannot change")
        if name in F.NANSAFE:
            raise PtmiError(F.UNSUPPORTED, "ptmi_update_triangles: the uploaded scene has records that can yield NaN distances")
        found = [t for t in F.VERSIONS if tris is WORLD.triangles(name, t)]
        if not found:
            if self.defect == DEFECTS[3]:  # (what bad triangles render has no yardstick: another version stands for them)
                self.query_version = self.filter_version = self.path_version = (version + 1) % 3
                self.m.state = (name, camera, self.query_version, look)
            raise PtmiError(F.UNSUPPORTED, "ptmi_update_triangles: a triangle is refused")
        self.m.state = (name, camera, found[0], look)
        if self.defect != (DEFECTS[23] if device else DEFECTS[1]):
            self.query_version = found[0]
        if self.defect != DEFECTS[7]:
            self.filter_version = found[0]
        if self.defect != DEFECTS[12]:
            self.path_version = found[0]
        return {}

    def update_triangles(self, tris):
        return self._triangles(tris)

    def device_update(self, tris):
        """what HostIO makes of ptmi_update_triangles_device"""
        return self._triangles(tris, device=True)

    def update_materials(self, first, materiaux):
        name, camera, version, (m, g, k) = self.m.state
        sc = WORLD.scene(self.m.state)
        if first + len(materiaux) > len(self.table):
            raise PtmiError(F.INVALID_ARGUMENT, "ptmi_update_materials: first + n beyond the uploaded materials")
        if ((materiaux["isSimpleColor"] == 0) & (materiaux["textureId"] >= len(sc.textures))).any():
            raise PtmiError(F.BAD_SCENE, "ptmi_update_materials: a texture that was not uploaded")
        flips = bool(((materiaux["isSimpleColor"] == 0) & (self.table["isSimpleColor"][first:first + len(materiaux)] != 0)).any())
        self.table[first:first + len(materiaux)] = materiaux
        found = [new for new in F.MATERIALS if WORLD.materials(name, new).tobytes() == self.table.tobytes()]
        assert found, "a material table the scripts do not have"
        new = (name, camera, version, (found[0], g, k))
        info = dict(plain_before=int(F.plain_verdict(sc)), plain_after=int(F.plain_verdict(WORLD.scene(new))),
                    screened_triangles=len(sc.triangulation) if flips else 0)
        if self.defect == DEFECTS[28] and self.n_devices > 1 and found[0] != m:
            self.old_materials = m
        self.m.state = new
        if self.defect != DEFECTS[13]:
            self.path_materials = found[0]
        if self.defect != DEFECTS[24]:
            self.guide_materials = found[0]
        return info

    def update_lights(self, lights):
        name, camera, version, (m, g, k) = self.m.state
        if len(lights) != len(WORLD.anchor(name).lights):
            raise PtmiError(F.INVALID_ARGUMENT, "ptmi_update_lights: lights_size is baked at setup")
        if name in F.NANSAFE:
            if self.defect == DEFECTS[27]:  # (these scenes have one set of lights: the other sky stands for other lights)
                self.m.state = (name, camera, version, (m, g, 1 - k))
            raise PtmiError(F.UNSUPPORTED, "ptmi_update_lights: the uploaded scene has records that can yield NaN distances")
        if not np.isfinite(lights["position"]).all():
            raise PtmiError(F.UNSUPPORTED, "ptmi_update_lights: a light's position is not finite")
        found = [new for new in F.LIGHTS if WORLD.lights(name, new).tobytes() == lights.tobytes()]
        assert found, "lights the scripts do not have"
        if self.defect == DEFECTS[25] and found[0] != g:
            self.stale = [dict(lights=g), 2]
        self.m.state = (name, camera, version, (m, found[0], k))

    def set_sky(self, sky):
        name, camera, version, (m, g, k) = self.m.state
        found = [new for new in F.SKIES if WORLD.sky(name, new).tobytes() == sky.tobytes()]
        assert found, "a sky the scripts do not have"
        if self.defect == DEFECTS[26]:
            m = self.path_materials = self.guide_materials = self.uploaded_materials
            self.table = U.raw_copy(WORLD.materials(name, m))
        self.m.state = (name, camera, version, (m, g, found[0]))

    def trace_paths(self, origins, directions, first_iteration=0, n_iterations=1, first_index=0, index_stride=None, out=None):
        name, camera, _, (_, g, k) = self.m.state
        assert index_stride == P.STRIDE and np.array_equal(origins, WORLD.path_rays(name)["origin"][:len(origins)])
        if self.defect == DEFECTS[14]:
            self.m.totals = {key: value + (len(origins) if key == "box_tests" else 0) for key, value in self.m.counters().items()}
        state = (name, camera, self.path_version, (self.path_materials, g, k))
        return WORLD.path_sums(state, self.m.da, len(origins), first_iteration, n_iterations, first_index).copy()

    def display(self, tone=None, transfer=None, exposure=None, white=None, rgba=False, out=None):
        image = self.before_render if self.defect == DEFECTS[21] and self.before_render else (self.m.color, self.m.count)
        self.exposure = exposure
        params = dict(tone=tone, transfer=transfer, exposure=1.0 if self.defect == DEFECTS[20] else exposure, white=white, rgba=rgba)
        pixels = F.display_yardstick(image, params)
        if out is None:
            return pixels
        out[...] = pixels
        return out

    def luminance_histogram(self):
        if self.defect == DEFECTS[22]:
            return DC.histogram(self.m.color * np.float32(self.exposure), self.m.count)
        return DC.histogram(self.m.color, self.m.count)

    def query_rays(self, origins, directions, max_squared_distance=None, any_hit=False, out=None):
        name, camera, _, look = self.m.state
        _, want, _ = WORLD.hits((name, camera, self.query_version, look), self.m.da, len(origins))
        if self.defect == DEFECTS[4]:
            self.m.totals = {key: value + (len(origins) if key == "box_tests" else 0) for key, value in self.m.counters().items()}
        return want[any_hit][:len(origins)].copy()

    def render_guides(self, first, n, planes=G.PLANES, out=None):
        name, _, version, (_, g, k) = self.m.state
        want, _ = WORLD.planes((name, self.guide_camera, version, (self.guide_materials, g, k)), self.m.da, first, n)
        if self.defect == DEFECTS[5]:
            self.m.reset()
        return {p: want[p].copy() for p in planes}

    def denoise(self, out=None, **params):
        """denoise_cases.denoise of the model's own image and the planes render_guides would return"""
        name, look = self.m.state[0], self.m.state[3]
        want, _ = WORLD.planes((name, self.filter_camera, self.filter_version, look), self.m.da, params["guide_first_iteration"], params["guide_iterations"])
        image = self.before_render if self.defect == DEFECTS[8] and self.before_render else (self.m.color, self.m.count)
        result = F.denoise_yardstick(image, want, dict(params, demodulate=params["demodulate"] or self.defect == DEFECTS[11]))
        if self.defect == DEFECTS[9]:
            self.m.write(result, result[..., 3])
        if self.defect == DEFECTS[10] and self.n_devices > 1 and self.last_slot in self.m.slots:
            self.m.slots[self.last_slot] = (result.copy(), result[..., 3].copy())
        if out is None:
            return result
        out[...] = result
        return out

    def _render_state(self):
        self.before_render = (self.m.color.copy(), self.m.count.copy()) if self.defect in (DEFECTS[8], DEFECTS[16], DEFECTS[21]) else None
        if not self.stale:
            return None
        name, camera, version, (m, g, k) = self.m.state
        state = (name, self.stale[0].get("camera", camera), version, (m, self.stale[0].get("lights", g), k))
        self.stale[1] -= 1
        if not self.stale[1]:
            self.stale = None
        return state

    def _render(self, first, n, state):
        if self.old_materials is None:
            return self.m.render(first, n, state)
        name, camera, version, (m, g, k) = state or self.m.state
        for it in range(first, first + n):  # (the devices take the iterations in turn: every second one on a device that was not told)
            self.m.render(it, 1, (name, camera, version, (self.old_materials if it % 2 else m, g, k)))

    def render(self, first, n):
        self._render(first, n, self._render_state())

    def render_snapshots(self, first, n, slot):
        if self.megakernel:
            raise PtmiError(F.UNSUPPORTED, "ptmi_render_snapshots wants the wavefront kernel")
        state = self._render_state()
        for k in range(n):
            self._render(first + k, 1, state)
            self.m.snapshot((slot + k) % F.RING)
        self.last_slot = (slot + n - 1) % F.RING

    def snapshot(self, slot):
        self.m.snapshot(slot)
        self.last_slot = slot

    @staticmethod
    def _out(arrays, out):
        if out is None:
            return tuple(a.copy() for a in arrays)
        for o, a in zip(out, arrays):
            o[...] = a
        return out

    def read_snapshot(self, slot, out=None):
        if slot not in self.m.slots:
            raise PtmiError(F.STATE, "no snapshot in this slot")
        return self._out(self.m.slots[slot], out)

    def read_image(self, out=None):
        return self._out((self.m.color, self.m.count), out)

    def read_variance(self):
        return self.m.variance.copy()

    def write_image(self, color, count):
        self.m.write(color, count)
        self.before_render = None

    def write_variance(self, variance):
        self.m.variance = variance.copy()

    def read_statistics(self):
        return tuple(a.astype(np.uint32) for a in self.m.stats)

    def counters(self):
        return self.m.counters()

    def clear(self):
        self.m.reset()
        self.before_render = None

    def read_display(self):
        rgb = output.to_display_rgb(self.m.color, self.m.count)
        out = np.zeros((F.H, (3 * F.W + 3) & ~3), np.uint8)
        out[:, :3 * F.W] = rgb[..., ::-1].reshape(F.H, 3 * F.W)
        return out

    def kernel_time(self):
        return 0.0, 0

    def synchronize(self):
        pass

    def pin_host_buffer(self, array):
        pass

    unpin_host_buffer = pin_host_buffer


def play(seed, cap, ids, defect=None, super_sampling=False):
    da, megakernel = F.flags_of(seed, super_sampling)
    ops = F.script(seed, F.DEVICES[ids], cap, super_sampling)
    fake = FakeBackend(da, megakernel, super_sampling, defect, n_devices=len(F.DEVICES[ids] or [0]))
    return F.run(ops, fake, F.Model(WORLD, da, super_sampling), exact=ids == "one")


def test_every_shipped_script_passes_on_a_backend_without_defects():
    made = {}
    for seed, cap, ids in F.shipped_cases():
        for kind, n in play(seed, cap, ids).items():
            made[kind] = made.get(kind, 0) + n
    for seed in F.SUPER_SAMPLING_SEEDS:
        play(seed, None, "one", super_sampling=True)
    assert all(made.get(kind, 0) >= 20 for kind in F.NEW_OPS), made


@pytest.mark.parametrize("defect", DEFECTS)
def test_a_defect_is_caught(defect):
    where, culprits = SURFACES[defect]
    cases = [(seed, None, "one", True) for seed in F.SUPER_SAMPLING_SEEDS] if defect in SUPER_SAMPLING_DEFECTS else \
        [case + (False,) for case in F.shipped_cases()]
    for seed, cap, ids, super_sampling in cases:
        try:
            play(seed, cap, ids, defect, super_sampling)
        except F.Mismatch as e:
            assert e.op[0] in where, str(e)
            # an upload undoes every one of these defects: the culprit must lie between the last upload and the mismatch
            kinds = [op[0] for op in e.history]
            since_upload = kinds[len(kinds) - kinds[::-1].index("upload"):] if "upload" in kinds else kinds
            assert culprits & set(since_upload), str(e)
            assert " ".join(str(op) for op in e.history[-3:]) in str(e)  # (the calls are in the message)
            return
    pytest.fail(f"no shipped script notices that {defect}")


def test_a_defect_is_caught_under_super_sampling():
    """... where every iteration depends on what the last one left: a render for the old camera."""
    for seed in F.SUPER_SAMPLING_SEEDS:
        try:
            play(seed, None, "one", DEFECTS[2], super_sampling=True)
        except F.Mismatch as e:
            assert "camera" in [op[0] for op in e.history], str(e)
            return
    pytest.fail("no super-sampling script notices a render for the old camera")
