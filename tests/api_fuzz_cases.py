"""Random C-ABI call sequences that also move the scene, trace rays, render guides and denoise (test_api_fuzz_model.py on the CPU,
test_api_fuzz_scene_gpu.py on the GPU): a generator of scripts, the model of what a script means, and the executor that plays
a script against a backend and compares everything it reads with the model.  Pure Python and numpy; the product is imported
only to build scenes (and for its error class and ring size), as the other case modules do.

The script.  `script(seed, devices, cap)` is a list of plain tuples and depends on nothing but its arguments.  Next to the
operations of test_api_fuzz_gpu.py (render, walk, snapshot, burst, read_slot, read_image, statistics, counters, clear, upload,
write, sync, kernel_time, display, pin) it holds
    ("camera", c)                          ptmi_set_camera to camera c of the scene's three
    ("update", t)                          ptmi_update_triangles to triangle version t of the scene's three
    ("bad_update", kind)                   a triangulation that is refused (scene_update_cases.bad_triangles)
    ("bad_camera", which)                  an infinite position (0) or a NaN up vector (1): refused
    ("query", any_hit, batch, route)       the first `batch` of the scene's rays, through host arrays or device pointers
    ("guides", first, n, planes, route)    ptmi_render_guides for n iterations from `first`, a subset of the planes
    ("denoise", first, n, passes, sigmas, demodulate, untiled, route)
                                           the filter, guided by n iterations from `first`: 0 to 5 passes, one of SIGMA_SETS
and any of these also BETWEEN two calls of a walk (the last field of a walk: ((call index, operation), ...)), which is when
launches for calls that have not been made yet are in flight, directly behind a burst, behind an upload, and between a snapshot
and the read of its slot; a denoise also directly behind a write, a clear or a display.  A call through device pointers is not
waited for: what it wrote is collected and compared after the NEXT operation, so that the next operation - an update, a camera,
an upload - runs while it may still be in flight.

The filter.  Its expected value is denoise_cases.denoise, the NumPy float32 restatement, of arrays that are themselves held
against the model: one arithmetic, every word equal, a NaN where the yardstick has one, and no tolerance on any device count.
    * route "host": ptmi_denoise first, on whatever the operations before it left in flight (every other time into a third
      array that is pinned and unpinned with the other two); then ptmi_read_image and ptmi_render_guides.  The image must be the
      model's (same_image), the four planes the guide yardstick's, and the filtered image the yardstick of exactly those arrays.
      That holds bit for bit on several devices, where the model's colour sums do not, and does not rest on the few pixels
      whose albedo the guide yardstick leaves out.
    * route "device" (one device): ptmi_render_guides_device into four tensors, then ptmi_denoise_device on the context's own
      accumulators, neither waited for.  Collected: the planes against the guide yardstick, the result against the yardstick
      of those planes and a copy of the model's accumulators taken at the call.
    * route "planes" (any device count): the same with sum and count planes of the caller's (seeded_image: some counts are 0).
A denoise changes nothing in the model.

The states.  A state is (scene name, camera id, triangle version).  Camera c is scene_update_cases.moved_camera(anchor, step=c),
version 0 the triangles as built, versions 1 and 2 scene_update_cases.displaced of them (seeds VERSION_SEEDS, amplitude 0.02).
The yardstick scene of a state is the anchor with that camera and scene_update_cases.moved_scene(anchor, triangles[t]): one
ptmi_bvh_refit of the uploaded tree (for version 0 that is the built tree byte for byte, test_api_fuzz_model.py).  ("upload",
name, c, t) uploads exactly that scene, so a script reaches a state by upload as well as by camera / update.
    * The anchor is the scene as built, but for the camera of two scenes.  As built, the cameras of fuzz3_l1 and fuzz5h_l1
      look away from all geometry: every primary ray ends in the sky, and no image, guide plane or counter could tell one
      triangle version from another.  fuzz5h_l1 is seen the other way (cameraDirection and cameraRight negated).  Seen the other
      way, 13 % to 18 % of fuzz3_l1's first hits land on textured glass, water or varnish, for which the guide yardstick has no
      bit-exact albedo (guide_cases.MAX_EXCLUDED allows 10 %); its camera is the built one with the axes cycled (x, y, z ->
      y, z, x) and the position mirrored through the origin, which looks at the scene from a side where under 1 % do.
      (test_api_fuzz_gpu.py uploads these two scenes as built, so there they render sky alone; it could take these anchors too.)
    * The two NANSAFE scenes have triangle version 0 only: ptmi_update_triangles refuses them (UNSUPPORTED, nothing changes),
      which the scripts do try, and a displaced upload would recompute the normals that make them NANSAFE.
    * Rays.  The scene's rays are ray_query_cases.mixed_rays of the anchor with camera 0.  Where the walk refuses a ray in a state
      (ValueError: it does not decide a sign), that state sends the set's first ray, the centre pinhole ray, in its place.
      The guide yardstick refused no sample of any state (test_api_fuzz_model.py walks them all), so nothing is left out.

The model.  Accumulators, counts, histograms and totals are the sums of the oracle's per-iteration results, on the yardstick
scene of the state each iteration was rendered in, since the last clear / upload / write; a slot holds the accumulators as they
were when its snapshot was queued.  A refused call, a query, a guides call and a denoise change nothing; a camera or an update
keeps what was rendered.  A super-sampling model runs the oracle statefully on its own arrays instead.
"""
import copy
import warnings

import numpy as np

from opencl_pathtracer_amd import PtmiError, backend, bvh_create, scenes, structs as S
import denoise_cases as DN
import guide_cases as G
import oracle_ffi as O
import ray_query_cases as Q
import scene_update_cases as U

W, H, D, N_IDS = 40, 30, 3, 48
SCENES = ["cornell", "fuzz3_l1", "fuzz5h_l1", "fuzz41hr_l1"]  # (the last two: the NANSAFE instantiation)
NANSAFE = ("fuzz5h_l1", "fuzz41hr_l1")
TURNED, CYCLED = ("fuzz5h_l1",), ("fuzz3_l1",)  # as built they look at the sky alone (the module's docstring)
CAMERAS, VERSIONS = (0, 1, 2), (0, 1, 2)
VERSION_SEEDS = {1: 1, 2: 2}
AMPLITUDE = 0.02
N_RAYS, RAY_SEED = 1100, 0
BATCHES = (1, 257, 1100)  # (one ray, below the 1024-ray floor of the context's scratch, above it)
GUIDE_FIRSTS = (0, 1)
RING = backend.USER_SNAPSHOT_SLOTS
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
NEW_OPS = ("camera", "update", "bad_update", "bad_camera", "query", "guides", "denoise")
NEW_OP_WEIGHTS = (0.17, 0.19, 0.08, 0.07, 0.17, 0.16, 0.16)
DENOISE_PLANES = ("albedo", "normal", "position", "hit_count")  # (the planes the filter reads)
DENOISE_PASSES = (0, 1, 2, 3, 4, 5)
# the sigmas of test_denoise_gpu.py (its SIGMAS) and the shipped defaults
SIGMA_SETS = {"narrow": dict(sigma_color=0.6, sigma_normal=0.5, sigma_position=1.5),
              "defaults": {key: backend.DENOISE_DEFAULTS[key] for key in ("sigma_color", "sigma_normal", "sigma_position")}}
DENOISE_ROUTES = ("host", "device", "planes")
N_OPS, N_OPS_SUPER_SAMPLING = 120, 70
GENERATOR_SEED = 2  # (of every script's draws: chosen so that test_api_fuzz_model.py's coverage conditions and defect tests hold)
HIT_FIELDS = ("point", "squared_distance", "s", "t", "triangle_id", "front", "box_tests", "triangle_tests")
TOTALS = tuple(name for name, _ in O.PtoTotals._fields_)


DEVICES = {"one": None, "two": [0, 0], "three": [0, 0, 0]}
DEFAULT_SEEDS = 5  # (the fewest with which test_api_fuzz_model.py's coverage conditions and defect tests hold)
LOW_CAP_SEEDS = [(seed, cap) for cap, seeds in ((1, (1000, 1001)), (2, (1002, 1003)), (3, (1005, 1006))) for seed in seeds]
SUPER_SAMPLING_SEEDS = range(4)


def shipped_cases(n_seeds=DEFAULT_SEEDS):
    """[(seed, cap or None, devices id)] of test_random_scene_call_sequences"""
    return [(seed, cap, ids) for seed, cap in [(s, None) for s in range(n_seeds)] + LOW_CAP_SEEDS for ids in DEVICES]


def versions_of(name):
    return (0,) if name in NANSAFE else VERSIONS


def flags_of(seed, super_sampling=False):
    """(default arithmetic?, megakernel?) of a seed, as in test_api_fuzz_gpu.py"""
    if super_sampling:
        return seed % 2 == 0, False
    return seed % 3 != 0, seed % 5 == 4


# ---------------------------------------------------------------------------------------------- scenes and yardstick data

class World:
    """The scenes, their variants and every yardstick result, each computed when first asked for and kept."""

    def __init__(self):
        self._anchor, self._tris, self._scene, self._per_it, self._rays, self._hits, self._yard = {}, {}, {}, {}, {}, {}, {}

    def anchor(self, name):
        if name not in self._anchor:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (the hostile scenes divide 0 by 0 on purpose, as the importer would)
                sc = bvh_create(scenes.build(name, W, H))
            if name in TURNED:
                sc.cameraDirection = (-np.asarray(sc.cameraDirection, np.float32)).astype(np.float32)
                sc.cameraRight = (-np.asarray(sc.cameraRight, np.float32)).astype(np.float32)
            if name in CYCLED:
                cycle = lambda v: np.asarray(v, np.float32)[[1, 2, 0, 3]]
                sc.cameraPosition = (cycle(sc.cameraPosition) * np.float32([-1, -1, -1, 1])).astype(np.float32)
                sc.cameraDirection, sc.cameraRight, sc.cameraUp = cycle(sc.cameraDirection), cycle(sc.cameraRight), cycle(sc.cameraUp)
            self._anchor[name] = sc
        return self._anchor[name]

    def triangles(self, name, t):
        if (name, t) not in self._tris:
            base = self.anchor(name).triangulation
            with np.errstate(all="ignore"):
                self._tris[name, t] = base if t == 0 else U.displaced(base, VERSION_SEEDS[t], AMPLITUDE)
        return self._tris[name, t]

    def camera(self, name, c):
        return U.moved_camera(self.anchor(name), step=c)

    def scene(self, state):
        if state not in self._scene:
            name, c, t = state
            sc = U.moved_scene(self.camera(name, c), self.triangles(name, t))
            sc.fuzz_state = state
            self._scene[state] = sc
        return self._scene[state]

    def per_iteration(self, state, da, k):
        """(color, count, statistics, totals) of iteration k alone"""
        key = (state, da, k)
        if key not in self._per_it:
            self._per_it[key] = O.oracle_render(self.scene(state), W, H, D, 1, first_iteration=k, default_arithmetic=da)
        return self._per_it[key]

    def rays(self, name):
        if name not in self._rays:
            with np.errstate(all="ignore"):
                self._rays[name] = Q.mixed_rays(self.scene((name, 0, 0)), N_RAYS, W, H, seed=RAY_SEED)
        return self._rays[name]

    def hits(self, state, da, n=N_RAYS):
        """(the rays this state is sent, {any_hit: the hits ptmi_query_rays must return}, the indices of replaced rays), each
        valid for the first n rays: the walk goes as far into the set as a batch has asked so far"""
        key = (state, da)
        if key not in self._hits:
            rays = self.rays(state[0]).copy()
            self._hits[key] = [rays, {False: np.zeros(len(rays), S.RAY_HIT), True: np.zeros(len(rays), S.RAY_HIT)}, [], 0,
                               Q.Walker(self.scene(state), da)]
        entry = self._hits[key]
        rays, want, replaced, done, w = entry

        def both(r):
            return [w.walk(r["origin"], r["direction"], r["max_squared_distance"], any_hit) for any_hit in (False, True)]

        with np.errstate(all="ignore"):
            for k in range(done, n):
                try:
                    hs = both(rays[k])
                except ValueError:
                    rays[k] = rays[0]
                    replaced.append(k)
                    hs = both(rays[0])  # (the centre pinhole ray: a refusal of this one is an error of the ray set)
                for any_hit, h in zip((False, True), hs):
                    for name in HIT_FIELDS:
                        want[any_hit][name][k] = h[name]
        entry[3] = max(done, n)
        return rays, want, replaced

    def yardstick(self, state, da):
        key = (state, da)
        if key not in self._yard:
            self._yard[key] = G.Yardstick(self.scene(state), W, H, S.JITTERED, da)
        return self._yard[key]

    def planes(self, state, da, first, n):
        return self.yardstick(state, da).planes(first, n)


WORLD = World()


# ---------------------------------------------------------------------------------------------- the model

class Model:
    def __init__(self, world, default_arithmetic, super_sampling=False):
        self.world, self.da, self.ss = world, default_arithmetic, super_sampling
        self.state, self.slots = None, {}
        self.reset()

    def reset(self):
        self.color = np.zeros((H, W, 4), np.float32)
        self.count = np.zeros((H, W), np.float32)
        self.variance = np.zeros((H, W, 4), np.float32)
        kind = np.uint32 if self.ss else np.int64
        self.stats = [np.zeros(D + 1, kind), np.zeros(S.MAX_INTERSETCION_NUMBER, kind), np.zeros(S.MAX_INTERSETCION_NUMBER, kind)]
        self.totals = None

    def upload(self, state):
        self.state, self.slots = state, {}
        self.reset()

    def _add_totals(self, tot):
        self.totals = dict(tot) if self.totals is None else {key: self.totals[key] + tot[key] for key in tot}

    def render(self, first, n, state=None):
        """Iterations first .. first + n - 1 of `state` (default: the current one) on top of what is there."""
        state = state or self.state
        if self.ss:  # every iteration depends on the accumulators and the variance image it finds
            _, _, _, tot = O.oracle_render(self.world.scene(state), W, H, D, n, first_iteration=first, super_sampling=True,
                                           default_arithmetic=self.da, first_sample_guard=True,
                                           into=(self.color, self.count, tuple(self.stats), None), image_v=self.variance)
            self._add_totals(tot)
            return
        for k in range(first, first + n):
            c, cnt, st, tot = self.world.per_iteration(state, self.da, k)
            self.color = self.color + c  # float32 adds, in call order: what a single device does
            self.count = self.count + cnt
            for a, b in zip(self.stats, st):
                a += b
            self._add_totals(tot)

    def snapshot(self, slot):
        self.slots[slot] = (self.color.copy(), self.count.copy())

    def write(self, color, count, variance=None):
        self.color, self.count = color.copy(), count.copy()
        if variance is not None:
            self.variance = variance.copy()

    def counters(self):
        return dict(self.totals) if self.totals is not None else {key: 0 for key in TOTALS}


# ---------------------------------------------------------------------------------------------- the generator

class _Generator:
    def __init__(self, seed, devices, cap, super_sampling):
        self.rs = np.random.RandomState([int(seed), 2 if super_sampling else 1, GENERATOR_SEED])
        self.multi, self.ss = bool(devices), super_sampling
        self.bursts = not flags_of(seed, super_sampling)[1]  # (ptmi_render_snapshots wants the wavefront kernel)
        self.few = RING if seed % 2 else 6  # (even seeds: six slots, so that snapshots overwrite each other all the time)
        self.names = [["cornell", "fuzz3_l1"][seed % 4 == 3]] if super_sampling else SCENES
        self.name, self.uploaded_version, self.updated = self.names[0], 0, False
        self.slots, self.queried = set(), False

    def choice(self, items):
        return items[int(self.rs.randint(0, len(items)))]

    def denoise(self):
        rs = self.rs
        first = GUIDE_FIRSTS[int(rs.rand() < 0.15)]  # (as for guides: the yardstick's iterations are traced once and kept)
        n = int(rs.choice([1, 1, 1, 2, 3]))
        passes, sigmas = self.choice(DENOISE_PASSES), self.choice(sorted(SIGMA_SETS))
        demodulate, untiled = bool(rs.rand() < 0.5), bool(rs.rand() < 0.5)
        # the context's own accumulators through device pointers: one device only (several: refused, test_denoise_gpu.py)
        route = str(rs.choice(DENOISE_ROUTES, p=[0.6, 0.0, 0.4] if self.multi else [0.4, 0.3, 0.3]))
        return ("denoise", first, n, passes, sigmas, demodulate, untiled, route)

    def new_op(self):
        rs = self.rs
        kind = str(rs.choice(NEW_OPS, p=NEW_OP_WEIGHTS))
        if kind == "denoise":
            return self.denoise()
        if kind == "camera":
            return ("camera", self.choice(CAMERAS))
        if kind == "update":
            back = self.uploaded_version != 0 and not self.updated and rs.rand() < 0.5  # back to version 0 from a variant uploaded as one
            t = 0 if back else self.choice(VERSIONS)
            self.updated = True
            return ("update", t)
        if kind == "bad_update":
            return ("bad_update", self.choice(U.BAD_TRIANGLES))
        if kind == "bad_camera":
            return ("bad_camera", int(rs.randint(0, 2)))
        route = "device" if not self.multi and rs.rand() < 0.4 else "host"
        if kind == "query":
            # the first one small, so that the scratch grows later; the large batch one time in five (its walk is the dearest)
            batch = BATCHES[2] if self.queried and rs.rand() < 0.2 else self.choice(BATCHES[:2])
            self.queried = True
            return ("query", bool(rs.rand() < 0.4), batch, route)
        planes = tuple(p for p in G.PLANES if rs.rand() < 0.5) or (self.choice(G.PLANES),)
        # mostly one iteration, mostly from iteration 0: an iteration of a state is traced once and kept, and it is the dearest yardstick
        first = GUIDE_FIRSTS[int(rs.rand() < 0.15)]
        return ("guides", first, int(rs.choice([1, 1, 1, 2, 3])), planes, route)

    def upload(self):
        name = self.choice(self.names)
        variant = self.rs.rand() < 0.5
        c = self.choice(CAMERAS) if variant else 0
        t = self.choice(versions_of(name)) if variant else 0
        self.name, self.uploaded_version, self.updated = name, t, False
        self.slots = set()
        return ("upload", name, c, t)

    def read_slot(self, slot=None):
        if not self.slots:
            return ("read_empty_slot", int(self.rs.randint(0, RING)))
        slot = self.choice(sorted(self.slots)) if slot is None else slot
        return ("read_slot", slot, bool(self.rs.rand() < 0.5))

    def plain_op(self):
        """One operation, and the operations that must follow it directly."""
        rs = self.rs
        if self.ss:
            op = str(rs.choice(["render", "render", "render", "read_image", "variance", "statistics", "counters", "clear", "save", "resume",
                                "snapshot", "read_slot", "upload", "new", "new", "new", "new"]))
        else:
            op = str(rs.choice(["render", "render", "render", "snapshot", "burst", "read_slot", "read_slot", "read_image", "statistics",
                                "counters", "clear", "upload", "write", "sync", "kernel_time", "display", "pin", "walk",
                                "new", "new", "new", "new", "new", "new", "new"]))
        if op == "new":
            return [self.new_op()]
        if op == "render" and self.ss:
            return [("render", int(rs.randint(0, 40)), int(rs.choice([1, 2, 4, 9])))]
        if op == "render":
            return [("render", int(rs.randint(0, N_IDS - 6)), int(rs.choice([1, 1, 2, 3, 5])))]
        if op == "walk":
            # the reference's loop for a while: one short call after the other, waiting for each - what the library renders AHEAD of
            n = int(rs.choice([1, 1, 1, 2, 3]))
            calls = int(rs.randint(2, 14))
            first = int(rs.randint(0, N_IDS - calls * n + 1))
            look, look_at = int(rs.randint(0, calls)), ("counters" if rs.rand() < 0.5 else "image")
            inserts = []
            if rs.rand() < 0.75:
                for c in sorted(set(int(v) for v in rs.randint(0, calls - 1, int(rs.randint(1, 3))))):
                    inserts.append((c, self.new_op()))
            return [("walk", first, n, calls, look, look_at, tuple(inserts))]
        if op == "snapshot":
            slot = int(rs.randint(0, 5 if self.ss else self.few))
            self.slots.add(slot)
            if rs.rand() < 0.5:  # something new between the snapshot and the read of its slot (several devices: a lazy copy)
                return [("snapshot", slot), self.new_op(), self.read_slot(slot)]
            return [("snapshot", slot)]
        if op == "burst":
            if not self.bursts:
                return [("refused_burst",)]
            first, n, slot = int(rs.randint(0, N_IDS - 8)), int(rs.randint(1, 8)), int(rs.randint(0, self.few))
            self.slots |= {(slot + k) % RING for k in range(n)}
            return [("burst", first, n, slot)] + ([self.new_op()] if rs.rand() < 0.6 else [])
        if op == "read_slot":
            return [self.read_slot()]
        if op == "read_image":
            return [("read_image", bool(rs.rand() < 0.5))]
        if op == "upload":
            return [self.upload()] + ([self.new_op()] if rs.rand() < 0.6 else [])
        # the filter on accumulators that were just written, emptied or shown (the display shares the host form's internal slot)
        behind = [self.denoise()] if op in ("write", "clear", "display") and rs.rand() < 0.35 else []
        if op == "write":
            return [("write", int(rs.randint(0, 1 << 30)), int(rs.randint(0, 9)))] + behind
        return [(op,)] + behind  # statistics, counters, clear, sync, kernel_time, display, pin, variance, save, resume


def script(seed, devices, cap, super_sampling=False):
    """The operations of one case: [("upload", first scene, 0, 0), ...].  `cap` (PTMI_ITERATIONS_PER_LAUNCH of the case) does
    not change the script: it is an argument so that every case has one signature."""
    g = _Generator(seed, devices, cap, super_sampling)
    ops = [("upload", g.name, 0, 0)]
    n_ops = N_OPS_SUPER_SAMPLING if super_sampling else N_OPS
    while len(ops) < n_ops:
        ops += g.plain_op()
    return ops


def flat(ops):
    """The operations of a script with those inside walks, in the order they are made: (operation, inside a walk?)"""
    for op in ops:
        yield op, False
        if op[0] == "walk":
            for _, inner in op[6]:
                yield inner, True


# ---------------------------------------------------------------------------------------------- the executor

class Mismatch(AssertionError):
    def __init__(self, what, op, history):
        super().__init__(f"{what} at {op}; calls so far: ... " + " ".join(str(c) for c in history[-40:]))
        self.what, self.op, self.history = what, op, list(history[-40:])


class HostIO:
    """The 'device pointer' route of a backend that has no device: the host calls, answered at once."""

    def query(self, be, rays, any_hit):
        got = be.query_rays(rays["origin"], rays["direction"], rays["max_squared_distance"], any_hit=any_hit)
        return lambda: got

    def guides(self, be, first, n, planes):
        got = be.render_guides(first, n, planes=planes)
        return lambda: got

    def denoise(self, be, first, n, image, params):
        """-> a function that returns (the filtered image, the four guide planes it was guided by).  image None: the backend's
        accumulators, through be.denoise.  The host calls have no way to pass image planes: (colour sums, counts) are filtered
        here, by the yardstick on the backend's guide planes, so that route checks nothing of a backend without a device."""
        guides = be.render_guides(first, n, planes=DENOISE_PLANES)
        if image is None:
            got = be.denoise(**params)
        else:
            got = denoise_yardstick(image, guides, params)
        return lambda: (got, guides)


def denoise_parameters(op):
    """The keywords of Backend.denoise / denoise_device for a ("denoise", ...) operation."""
    _, first, n, passes, sigmas, demodulate, untiled, _ = op
    return dict(passes=passes, demodulate=demodulate, untiled=untiled, guide_first_iteration=first, guide_iterations=n, **SIGMA_SETS[sigmas])


def denoise_yardstick(image, guides, params):
    """denoise_cases.denoise of (colour sums, counts) and the four guide planes under the keywords of denoise_parameters
    (`untiled` chooses a kernel, not an arithmetic)"""
    return DN.denoise(image[0], image[1], **{name: guides[name] for name in DENOISE_PLANES}, passes=params["passes"],
                      flags=DN.DEMODULATE if params["demodulate"] else 0, guide_iterations=params["guide_iterations"],
                      sigma_color=params["sigma_color"], sigma_normal=params["sigma_normal"], sigma_position=params["sigma_position"])


def seeded_image(seed):
    """Colour sums uniform in [0, 4) with per-pixel sample counts from 0 to 8, some of them 0: the planes a caller hands the filter"""
    rs = np.random.RandomState(seed)
    color = rs.uniform(0, 4, (H, W, 4)).astype(np.float32)
    return color, rs.randint(0, 9, (H, W)).astype(np.float32)


def bad_camera(sc, which):
    bad = copy.copy(sc)
    if which == 0:
        bad.cameraPosition = np.float32([np.inf, 0, 0, 1])
    else:
        bad.cameraUp = np.float32([0, np.nan, 0, 0])
    return bad


def run(script_ops, be, model, io=None, exact=True):
    """Plays `script_ops` against `be` (a Backend with its context set up, or something that looks like one) and holds everything
    it reads against `model`.  `io`: how calls through device pointers are made, an object with query(), guides() and denoise()
    that return a function to collect the result with (HostIO: through the host calls).  `exact`: colour sums bit for bit (one
    device); else within the association error of several devices' partial sums.  Raises Mismatch with the last 40 calls.
    Returns the number of operations made, per kind."""
    from opencl_pathtracer_amd import output
    io = io or HostIO()
    world, m = model.world, model
    history, made, pending = [], {}, []
    pinned = [np.empty((H, W, 4), np.float32), np.empty((H, W), np.float32)]
    pinned_result = np.empty((H, W, 4), np.float32)  # (where every other host-route denoise lands; pinned and unpinned with the two)
    host_denoises = [0]
    is_pinned = [False]
    saved = [None]

    def check(ok, what, op):
        if not ok:
            raise Mismatch(what, op, history)

    def same_image(got, want_color, want_count, what, op):
        color, count = got
        check(np.array_equal(count, want_count), f"{what}: sample counts {np.unique(count).tolist()[:8]} instead of {np.unique(want_count).tolist()[:8]}", op)
        if exact:
            check(np.array_equal(color.view(np.uint32), want_color.view(np.uint32)), f"{what}: image bits differ", op)
        else:
            check(np.allclose(color, want_color, rtol=3e-6, atol=1e-6), f"{what}: image differs (max {float(np.abs(color - want_color).max())})", op)

    def same_counters(op):
        got = be.counters()
        check(got == m.counters(), f"counters {got} instead of {m.counters()}", op)

    def refused(call, code, op):
        try:
            call()
        except PtmiError as e:
            check(code is None or e.code == code, f"refused with {e.code} instead of {code}: {e}", op)
        else:
            check(False, f"accepted, where {code} was expected", op)

    def step(op, body):
        """One call sequence with what the PREVIOUS one left in flight collected behind it."""
        due, pending[:] = list(pending), []
        history.append(op)
        made[op[0]] = made.get(op[0], 0) + 1
        body()
        for collect in due:
            collect()

    def do(op):
        kind = op[0]
        name, cam, version = m.state if m.state else (None, None, None)
        if kind == "upload":
            state = tuple(op[1:])
            be.initialize_memory(world.scene(state))
            check((be.literal_kernel_reason() is not None) == (state[0] in NANSAFE), f"literal_kernel_reason() is {be.literal_kernel_reason()!r}", op)
            m.upload(state)
            saved[0] = None
        elif kind == "camera":
            sc = world.camera(name, op[1])
            be.set_camera(sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp)
            m.state = (name, op[1], version)
        elif kind == "update":
            tris = world.triangles(name, op[1])
            if name in NANSAFE:  # the kernel instantiation was chosen at upload: refused, and the scene stays
                refused(lambda: be.update_triangles(tris), UNSUPPORTED, op)
            else:
                be.update_triangles(tris)
                m.state = (name, cam, op[1])
        elif kind == "bad_update":
            tris = U.bad_triangles(world.scene(m.state), op[1])
            refused(lambda: be.update_triangles(tris), INVALID_ARGUMENT if op[1] == "wrong_count" else UNSUPPORTED, op)
        elif kind == "bad_camera":
            sc = bad_camera(world.camera(name, cam), op[1])
            refused(lambda: be.set_camera(sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp), UNSUPPORTED, op)
        elif kind == "query":
            _, any_hit, batch, route = op
            rays, want, _ = world.hits(m.state, m.da, batch)
            rays, want = rays[:batch].copy(), want[any_hit][:batch].copy()

            def compare(got):
                msg = Q.describe_difference(got, want)
                check(not msg, "query: " + msg, op)

            if route == "device":
                collect = io.query(be, rays, any_hit)
                pending.append(lambda: compare(collect()))
            else:
                compare(be.query_rays(rays["origin"], rays["direction"], rays["max_squared_distance"], any_hit=any_hit))
        elif kind == "guides":
            _, first, n, planes, route = op
            want, excluded = world.planes(m.state, m.da, first, n)

            def compare(got):
                check(set(got) == set(planes), f"guides: planes {sorted(got)} instead of {sorted(planes)}", op)
                msg = G.describe_difference(got, want, excluded)
                check(not msg, "guides: " + msg, op)

            if route == "device":
                collect = io.guides(be, first, n, planes)
                pending.append(lambda: compare(collect()))
            else:
                compare(be.render_guides(first, n, planes=planes))
        elif kind == "denoise":
            route, params = op[7], denoise_parameters(op)
            first, n = op[1], op[2]
            want_planes, excluded = world.planes(m.state, m.da, first, n)

            def compare(got, image, guides):
                check(set(guides) == set(DENOISE_PLANES), f"denoise: planes {sorted(guides)}", op)
                msg = G.describe_difference(guides, want_planes, excluded)
                check(not msg, "denoise: the guide planes: " + msg, op)
                msg = DN.describe_difference(got, denoise_yardstick(image, guides, params))
                check(not msg, f"denoise ({route}): " + msg, op)

            if route == "host":
                # first the call, on whatever the operations before it left in flight; then what it had to filter
                host_denoises[0] += 1
                out = pinned_result if host_denoises[0] % 2 else None
                if out is not None:
                    out.fill(-1.0)
                got = be.denoise(out=out, **params)
                image = be.read_image()
                guides = be.render_guides(first, n, planes=DENOISE_PLANES)
                same_image(image, m.color, m.count, "image behind a denoise", op)
                compare(got, image, guides)
            else:
                # through device pointers, not waited for: the context's accumulators as the model has them now (one device:
                # exact), or planes of the caller's
                image = (m.color.copy(), m.count.copy()) if route == "device" else seeded_image([len(history), first, n, op[3]])
                collect = io.denoise(be, first, n, None if route == "device" else image, params)

                def collected():
                    got, guides = collect()
                    compare(got, image, guides)

                pending.append(collected)
        elif kind == "render":
            be.render(op[1], op[2])
            m.render(op[1], op[2])
        elif kind == "snapshot":
            be.snapshot(op[1])
            m.snapshot(op[1])
        elif kind == "burst":
            _, first, n, slot = op
            be.render_snapshots(first, n, slot)
            for k in range(n):
                m.render(first + k, 1)
                m.snapshot((slot + k) % RING)
        elif kind == "refused_burst":
            refused(lambda: be.render_snapshots(0, 2, 0), None, op)
        elif kind == "read_slot":
            same_image(be.read_snapshot(op[1], out=pinned if op[2] else None), *m.slots[op[1]], f"slot {op[1]}", op)
        elif kind == "read_empty_slot":
            try:
                be.read_snapshot(op[1])
            except PtmiError:
                pass
            else:
                check(False, "a slot without a snapshot was read", op)
        elif kind == "read_image":
            same_image(be.read_image(out=pinned if op[1] else None), m.color, m.count, "image", op)
        elif kind == "variance":
            check(np.array_equal(be.read_variance().view(np.uint32), m.variance.view(np.uint32)), "variance image bits differ", op)
        elif kind == "statistics":
            got = be.read_statistics()
            check(all(np.array_equal(np.asarray(a).astype(np.int64), b.astype(np.int64)) for a, b in zip(got, m.stats)), "histograms differ", op)
        elif kind == "counters":
            same_counters(op)
        elif kind == "clear":
            be.clear()
            m.reset()
        elif kind == "write":
            rs = np.random.RandomState(op[1])
            color = rs.uniform(0, 4, (H, W, 4)).astype(np.float32)
            count = np.full((H, W), float(op[2]), np.float32)
            be.write_image(color, count)
            m.write(color, count)
        elif kind == "save":
            saved[0] = (m.color.copy(), m.count.copy(), m.variance.copy())
        elif kind == "resume":
            if saved[0] is not None:
                be.write_image(saved[0][0], saved[0][1])
                be.write_variance(saved[0][2])
                m.write(*saved[0])
        elif kind == "pin":
            for a in pinned + [pinned_result]:
                (be.unpin_host_buffer if is_pinned[0] else be.pin_host_buffer)(a)
            is_pinned[0] = not is_pinned[0]
        elif kind == "sync":
            be.synchronize()
        elif kind == "kernel_time":
            ms, launches = be.kernel_time()
            check(ms >= 0 and launches >= 0, f"kernel_time() is {(ms, launches)}", op)
        elif kind == "display":
            got = be.read_display()
            if exact:
                want = output.to_display_rgb(m.color, m.count)
                check(np.array_equal(got[:, :3 * W].reshape(H, W, 3)[..., ::-1], want), "display bytes differ", op)
        else:
            raise ValueError(f"unknown operation {op!r}")

    def walk(op):
        _, first, n, calls, look, look_at, inserts = op
        for c in range(calls):
            def call(c=c):
                be.render(first + c * n, n)
                be.synchronize()
                m.render(first + c * n, n)
                if c == look and look_at == "counters":
                    same_counters(op)
                elif c == look:
                    same_image(be.read_image(), m.color, m.count, f"image at call {c} of a walk", op)
            step(op if c == 0 else ("walk call", c), call)
            for at, inner in inserts:
                if at == c:
                    step(inner, lambda inner=inner: do(inner))

    for op in script_ops:
        if op[0] == "walk":
            walk(op)
        else:
            step(op, lambda op=op: do(op))
    step(("final image",), lambda: same_image(be.read_image(), m.color, m.count, "final image", ("final image",)))
    for collect in pending:
        collect()
    if is_pinned[0]:
        for a in pinned + [pinned_result]:
            be.unpin_host_buffer(a)
    made.pop("walk call", None)
    made.pop("final image", None)
    return made
