"""The random scene call sequences of api_fuzz_cases.py, checked without a GPU: the conditions their inputs must meet for a stale
scene to be noticed, what the shipped scripts cover, and that the executor catches a backend with a defect.  The backend here is
a fake made of the same oracle and yardstick data as the model, with one switch per defect; its filter is the yardstick of
denoise_cases.py on its own image and guide planes, so a defect in what the filter reads, guides itself by or leaves behind is
a switch like the others.  A failed condition is mended by choosing other seeds in api_fuzz_cases.py (VERSION_SEEDS, RAY_SEED,
GENERATOR_SEED), never by relaxing the condition."""
import itertools

import numpy as np
import pytest

from opencl_pathtracer_amd import PtmiError, backend, output
import api_fuzz_cases as F
import guide_cases as G
import ray_query_cases as Q
import scene_update_cases as U

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (the hostile scenes divide 0 by 0 on purpose, as the importer would)
WORLD = F.WORLD
STATES = {name: [(name, c, t) for c in F.CAMERAS for t in F.versions_of(name)] for name in F.SCENES}
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
    assert tree_bytes(WORLD.scene((name, 0, 0)).bvh) == tree_bytes(anchor.bvh)  # a refit to version 0 is the tree as built


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
    the caller's, the same in every state), so two states with the same triangles MUST expect the same hits: asserted too."""
    for a, b in itertools.combinations(STATES[name], 2):
        image_a, image_b = WORLD.per_iteration(a, da, 0)[0], WORLD.per_iteration(b, da, 0)[0]
        assert not np.array_equal(image_a.view(np.uint32), image_b.view(np.uint32)), (a, b)
        assert G.describe_difference(WORLD.planes(a, da, 0, 1)[0], WORLD.planes(b, da, 0, 1)[0]), (a, b)
        for any_hit in (False, True):
            same = np.array_equal(Q.words(WORLD.hits(a, da)[1][any_hit]), Q.words(WORLD.hits(b, da)[1][any_hit]))
            assert same == (a[2] == b[2]), (a, b, any_hit)
            if a[2] != b[2]:  # ... and already in the 257 rays of the middle batch
                assert not np.array_equal(Q.words(WORLD.hits(a, da)[1][any_hit][:257]), Q.words(WORLD.hits(b, da)[1][any_hit][:257])), (a, b)


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
                assert ids == "one" or op[-1] != "device"  # (device pointers: one device only)
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
    denoise_coverage()


def denoise_coverage():
    """What the shipped scripts ask of the filter: every pass count, both sigma sets with and without demodulation, both kernels
    of steps 1 and 2, all three routes, and a call directly behind each operation that changes what the filter reads."""
    passes, sigma_flags, untiled, routes, behind, lazy_copy = set(), set(), set(), set(), set(), set()
    nansafe = next_to_display = 0
    for (seed, cap, ids), ops in shipped_scripts():
        # the calls in the order they are made: an operation inside a walk, and the one behind a walk, follow a call of the walk
        made, behind_a_walk_call = [], False
        for op, in_walk in F.flat(ops):
            made += [("walk call",), op] if in_walk or behind_a_walk_call else [op]
            behind_a_walk_call = in_walk or op[0] == "walk"
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
           "several devices: a denoise overwrites the slot of the last snapshot", "the filter ignores the demodulation flag")
READS = {"read_image", "read_slot", "statistics", "counters", "display", "walk", "walk call", "final image"}
# defect: (the operations at which it may come to light, the operations of which one must be among the calls reported with it)
# (a host-route denoise reads the image behind its own call, so what a denoise leaves in the accumulators may show there first)
SURFACES = {DEFECTS[0]: ({"guides"}, {"camera"}), DEFECTS[1]: ({"query"}, {"update"}), DEFECTS[2]: (READS, {"camera"}),
            DEFECTS[3]: (READS | {"query", "guides", "denoise"}, {"bad_update"}), DEFECTS[4]: ({"counters", "walk"}, {"query"}),
            DEFECTS[5]: (READS | {"denoise"}, {"guides"}),
            DEFECTS[6]: ({"denoise"}, {"camera"}), DEFECTS[7]: ({"denoise"}, {"update"}),
            DEFECTS[8]: ({"denoise"}, {"render", "walk", "walk call", "burst"}), DEFECTS[9]: (READS | {"denoise"}, {"denoise"}),
            DEFECTS[10]: ({"read_slot"}, {"denoise"}), DEFECTS[11]: ({"denoise"}, {"denoise"})}


class FakeBackend:
    """The Backend methods the executor uses, answered from a model of its own."""

    def __init__(self, default_arithmetic, megakernel=False, super_sampling=False, defect=None, n_devices=1):
        assert defect is None or defect in DEFECTS
        self.m = F.Model(WORLD, default_arithmetic, super_sampling)
        self.megakernel, self.defect, self.n_devices = megakernel, defect, n_devices
        self.guide_camera = self.query_version = self.stale = None
        self.filter_camera = self.filter_version = self.before_render = self.last_slot = None

    def initialize_memory(self, scene):
        self.m.upload(scene.fuzz_state)
        _, self.guide_camera, self.query_version = scene.fuzz_state
        _, self.filter_camera, self.filter_version = scene.fuzz_state
        self.stale = self.before_render = self.last_slot = None

    def literal_kernel_reason(self):
        return "records that can yield NaN distances" if self.m.state[0] in F.NANSAFE else None

    def set_camera(self, *vectors):
        if not all(np.isfinite(np.asarray(v, np.float32)).all() for v in vectors):
            raise PtmiError(F.UNSUPPORTED, "ptmi_set_camera: a camera vector is not finite")
        name, old, version = self.m.state
        for c in F.CAMERAS:
            sc = WORLD.camera(name, c)
            if all(np.array_equal(np.asarray(v, np.float32), np.asarray(w, np.float32)) for v, w in
                   zip(vectors, (sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp))):
                break
        else:
            raise AssertionError("a camera the scripts do not have")
        if self.defect == DEFECTS[2] and c != old:
            self.stale = [old, 2]
        self.m.state = (name, c, version)
        if self.defect != DEFECTS[0]:
            self.guide_camera = c
        if self.defect != DEFECTS[6]:
            self.filter_camera = c

    def update_triangles(self, tris):
        name, camera, version = self.m.state
        if len(tris) != len(WORLD.triangles(name, 0)):
            raise PtmiError(F.INVALID_ARGUMENT, "ptmi_update_triangles: the topology cannot change")
        if name in F.NANSAFE:
            raise PtmiError(F.UNSUPPORTED, "ptmi_update_triangles: the uploaded scene has records that can yield NaN distances")
        found = [t for t in F.VERSIONS if tris is WORLD.triangles(name, t)]
        if not found:
            if self.defect == DEFECTS[3]:  # (what bad triangles render has no yardstick: another version stands for them)
                self.query_version = self.filter_version = (version + 1) % 3
                self.m.state = (name, camera, self.query_version)
            raise PtmiError(F.UNSUPPORTED, "ptmi_update_triangles: a triangle is refused")
        self.m.state = (name, camera, found[0])
        if self.defect != DEFECTS[1]:
            self.query_version = found[0]
        if self.defect != DEFECTS[7]:
            self.filter_version = found[0]
        return {}

    def query_rays(self, origins, directions, max_squared_distance=None, any_hit=False, out=None):
        name, camera, _ = self.m.state
        _, want, _ = WORLD.hits((name, camera, self.query_version), self.m.da, len(origins))
        if self.defect == DEFECTS[4]:
            self.m.totals = {key: value + (len(origins) if key == "box_tests" else 0) for key, value in self.m.counters().items()}
        return want[any_hit][:len(origins)].copy()

    def render_guides(self, first, n, planes=G.PLANES, out=None):
        name, _, version = self.m.state
        want, _ = WORLD.planes((name, self.guide_camera, version), self.m.da, first, n)
        if self.defect == DEFECTS[5]:
            self.m.reset()
        return {p: want[p].copy() for p in planes}

    def denoise(self, out=None, **params):
        """denoise_cases.denoise of the model's own image and the planes render_guides would return"""
        name = self.m.state[0]
        want, _ = WORLD.planes((name, self.filter_camera, self.filter_version), self.m.da, params["guide_first_iteration"], params["guide_iterations"])
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
        self.before_render = (self.m.color.copy(), self.m.count.copy()) if self.defect == DEFECTS[8] else None
        if not self.stale:
            return None
        name, _, version = self.m.state
        state = (name, self.stale[0], version)
        self.stale[1] -= 1
        if not self.stale[1]:
            self.stale = None
        return state

    def render(self, first, n):
        self.m.render(first, n, self._render_state())

    def render_snapshots(self, first, n, slot):
        if self.megakernel:
            raise PtmiError(F.UNSUPPORTED, "ptmi_render_snapshots wants the wavefront kernel")
        state = self._render_state()
        for k in range(n):
            self.m.render(first + k, 1, state)
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
    for seed, cap, ids in F.shipped_cases():
        try:
            play(seed, cap, ids, defect)
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
