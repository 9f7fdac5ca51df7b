"""Random C-ABI call sequences that also move and edit the scene, trace rays and paths, render guides, denoise, reproject and
display (test_api_fuzz_model.py on the CPU, test_api_fuzz_scene_gpu.py on the GPU): a generator of scripts, the model of what a
script means, and the executor that plays a script against a backend and compares everything it reads with the model.  Pure Python and numpy; the product is imported
only to build scenes (and for its error class and ring size), as the other case modules do.

The script.  `script(seed, devices, cap)` is a list of plain tuples and depends on nothing but its arguments.  Next to the
operations of test_api_fuzz_gpu.py (render, walk, snapshot, burst, read_slot, read_image, statistics, counters, clear, upload,
write, sync, kernel_time, display, pin) it holds
    ("camera", c)                          ptmi_set_camera to camera c of the scene's three
    ("update", t)                          ptmi_update_triangles to triangle version t of the scene's three
    ("bad_update", kind)                   a triangulation that is refused (scene_update_cases.bad_triangles)
    ("bad_camera", which)                  an infinite position (0, 2) or a NaN up vector (1, 3): refused, by ptmi_set_camera
                                           (0, 1) or by ptmi_set_camera_reprojected (2, 3)
    ("query", any_hit, batch, route)       the first `batch` of the scene's rays, through host arrays or device pointers
    ("guides", first, n, planes, route)    ptmi_render_guides for n iterations from `first`, a subset of the planes
    ("denoise", first, n, passes, sigmas, demodulate, untiled, route)
                                           the filter, guided by n iterations from `first`: 0 to 5 passes, one of SIGMA_SETS
    ("materials", m) ("lights", g) ("sky", k)
                                           ptmi_update_materials / ptmi_update_lights / ptmi_set_sky to that look of the scene
    ("bad_materials", kind)                a range beyond the table (INVALID_ARGUMENT) or a texture never uploaded (BAD_SCENE)
    ("bad_lights", kind)                   a wrong lights_size (INVALID_ARGUMENT) or a position that is not finite (UNSUPPORTED)
    ("update_device", t)                   ("update", t) through ptmi_update_triangles_device, the records in a device tensor
    ("paths", batch, first_iteration, n_iterations, first_index, route)
                                           ptmi_trace_paths(_device) for the first `batch` of the scene's path rays
    ("reprojected", c, tolerances, first, n)
                                           ptmi_set_camera_reprojected to camera c (it may be the current one) with one of
                                           REPROJECT_SETS, guided by n iterations from `first`
    ("tonemap", tone, transfer, exposure, white, rgba, route) ("histogram", route)
                                           ptmi_read_display_tonemapped / ptmi_display_device, ptmi_luminance_histogram(_device)
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

Paths.  Expected: path_query_cases.Yardstick(scene of the state, depth D).sums, every word, a NaN where it has one; index_stride
is path_query_cases.STRIDE.  Route "device" (one device) is not waited for.  Nothing in the model changes, the counters included.

The reprojection.  The model's new accumulators are reproject_cases.reproject of (the old camera; normal, position and hit_count
of the guide yardstick under the old state with the model's colour sums and counts; the yardstick's planes under the new state);
then the state moves to camera c; histograms, totals and slots stay.  A super-sampling context refuses the call (UNSUPPORTED,
camera and all), which its scripts try.  One device: the next read is bit for bit.  Several devices: counts exactly, colours
within the executor's rtol = 3e-6, atol = 1e-6 (same_image), which stays what it was.  Why: every test of the reprojection (the
frame, position, normal, the finiteness of a tap, min(sn / sw, max_history)) reads guide planes and COUNTS, which are exact on
any device count, so both sides take the same taps with the same weights w_k and the same n.  A colour is
(sum_k w_k * (c_k / n_k) / sw) * n with c_k >= 0: a convex combination of means times an exact integer.  Where every c_k carries a
relative error of at most e (what summing the devices' shares in another order leaves), so does the result, plus the roundings
of one division, four multiply-adds, one division and one product - eleven, each 2^-24 relative, on either side, none
cancelling since nothing is negative: at most e + 22 * 2^-24 = e + 1.3e-6 in the worst case, and about sqrt(22) * 2^-25 = 1.4e-7
where the roundings are independent.  That is the error eleven more accumulated iterations would add, of which a script renders
dozens between two clears under the same bound; the bound is therefore kept, and not tuned on a device.

The display.  Expected: display_cases.tonemap + pack_bgr24 / pack_rgba32 and display_cases.histogram: every byte, every word.
    * route "host": the call first, on whatever is in flight (one in three into a page-locked array; the exposure "histogram"
      is backend.exposure_from_histogram of ptmi_luminance_histogram called just before); then ptmi_read_image, held against
      the model (same_image); then the bytes and the words against the yardstick of exactly that image: any device count.
    * route "device": the context's own accumulators through device pointers, not waited for, against a copy of the model's
      accumulators taken at the call (one device); several devices refuse it (UNSUPPORTED), which is tried.
    * route "planes": sums and counts of the caller's (seeded_image: some counts are 0); "mean": a mean plane alone - the tensor
      the ptmi_denoise_device call made just before on the same stream has written, where the script has one (the viewer's
      pipeline), else a seeded one.  Any device count, not waited for.
A display call changes nothing in the model.  (The old "display" operation, ptmi_read_display, stays.)

The states.  A state is (scene name, camera id, triangle version, look), look = (m, g, k): materials, lights, sky (MATERIAL_LOOKS,
LIGHT_LOOKS, SKY_LOOKS below; (0, 0, 0) is the scene as built).  The yardstick scene of a state is scene_edit_cases.edited of the
scene described next with that look's arrays, so the oracle and the guide and path yardsticks see the edits with no further
work.  Materials look 1 is an edit of a sub-range (first > 0), which on cornell leaves the plain kernel instantiation (ptmi.h: all
materials plain-colour MAT_STANDART, all lights point lights); look 2 rewrites the table, and on fuzz3_l1 makes a plain colour
textured, so that the device screen of the texture coordinates runs.  Lights look 1 moves the light, and on cornell makes it a
spot.  Sky look 1 turns the sky and rescales the ground.  test_api_fuzz_model.py holds the looks to their conditions.
Camera c is scene_update_cases.moved_camera(anchor, step=c), version 0 the triangles as built, versions 1 and 2
scene_update_cases.displaced of them (seeds VERSION_SEEDS, amplitude 0.02).  The scene of (camera, version) is the anchor with
that camera and scene_update_cases.moved_scene(anchor, triangles[t]): one ptmi_bvh_refit of the uploaded tree (for version 0
that is the built tree byte for byte, test_api_fuzz_model.py).  ("upload", name, c, t, look) uploads exactly that scene, so a script reaches a state by upload as well as by camera / update / edit.
    * The anchor is the scene as built, but for the camera of two scenes (and eight texels behind cornell's one, for its sky
      look to point at: as built, the six sky faces of cornell and fuzz3_l1 are one texel, which no rotation changes).
      As built, the cameras of fuzz3_l1 and fuzz5h_l1 look away from all geometry: every primary ray ends in the sky, and no
      image, guide plane or counter could tell one triangle version from another.  fuzz5h_l1 is seen the other way (cameraDirection and cameraRight negated).  Seen the other
      way, 13 % to 18 % of fuzz3_l1's first hits land on textured glass, water or varnish, for which the guide yardstick has no
      bit-exact albedo (guide_cases.MAX_EXCLUDED allows 10 %); its camera is the built one with the axes cycled (x, y, z ->
      y, z, x) and the position mirrored through the origin, which looks at the scene from a side where under 1 % do.
      (test_api_fuzz_gpu.py uploads these two scenes as built, so there they render sky alone; it could take these anchors too.)
    * The two NANSAFE scenes have triangle version 0 only: ptmi_update_triangles refuses them (UNSUPPORTED, nothing changes),
      which the scripts do try, and a displaced upload would recompute the normals that make them NANSAFE.  They have lights
      look 0 only: ptmi_update_lights refuses them likewise, which the scripts try too.
    * Caches.  Hits depend on (scene, triangle version, arithmetic) alone; path sums on (scene, version, look, arithmetic); guide
      planes and per-iteration renders on the whole state.
    * Rays.  The scene's rays are ray_query_cases.mixed_rays of the anchor with camera 0.  Where the walk refuses a ray in a state
      (ValueError: it does not decide a sign), that state sends the set's first ray, the centre pinhole ray, in its place.
      The guide yardstick refused no sample of any state test_api_fuzz_model.py walks (states_of: every (camera, version) at
      the base look, every look at two of them).  The path calls send path_query_cases.mixed_rays of the same scene, of
      which no direction component is an exact zero (the yardstick asserts it).

The model.  Accumulators, counts, histograms and totals are the sums of the oracle's per-iteration results, on the yardstick
scene of the state each iteration was rendered in, since the last clear / upload / write; a slot holds the accumulators as they
were when its snapshot was queued.  A refused call, a query, a guides call, a denoise, a paths call and a display call change
nothing; a camera, an update or an edit keeps what was rendered; a reprojected camera resamples it.  A super-sampling model runs
the oracle statefully on its own arrays instead.
"""
import copy
import warnings

import numpy as np

from opencl_pathtracer_amd import PtmiError, backend, bvh_create, scenes, structs as S
import denoise_cases as DN
import display_cases as DC
import guide_cases as G
import oracle_ffi as O
import path_query_cases as P
import ray_query_cases as Q
import reproject_cases as R
import scene_edit_cases as E
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
INVALID_ARGUMENT, BAD_SCENE, STATE, UNSUPPORTED = -1, -5, -6, -7
NEW_OPS = ("camera", "update", "bad_update", "bad_camera", "query", "guides", "denoise",
           "materials", "lights", "sky", "bad_materials", "bad_lights", "update_device", "paths", "reprojected", "tonemap", "histogram")
# (the weights: the seven old kinds keep about their proportions in 0.42 of the draws, the ten new ones share the rest, the
# refusals lighter, the reprojection, the materials and the tone-mapped display heavier: they have the most values to reach.
# Behind a burst, an upload and a call that is not waited for, and between a snapshot and the read of its slot, the kinds are
# not drawn but taken in turn - _Generator.turn_op - so that few scripts put every kind into every such place.)
NEW_OP_WEIGHTS = (0.06, 0.07, 0.04, 0.04, 0.07, 0.07, 0.07,
                  0.07, 0.06, 0.06, 0.04, 0.04, 0.05, 0.06, 0.08, 0.07, 0.05)

# The looks.  A look is (m, g, k): which materials, lights and sky a state has; (0, 0, 0) is the scene as built.  Plain data: a
# material look is (first, one dict of Material fields per record from `first` on), laid over the records as built; a lights look
# the fields laid over light 0; a sky look (rotation angle, ground scale, the six faces (width, height, offset) or None: as built).
BASE_LOOK = (0, 0, 0)
MATERIALS, LIGHTS, SKIES = (0, 1, 2), (0, 1), (0, 1)
_STD, _WATER, _GLASS, _VARNISH, _METAL = S.MAT_STANDART, S.MAT_WATER, S.MAT_GLASS, S.MAT_VARNHISHED, S.MAT_METAL
MATERIAL_LOOKS = {
    # all three plain MAT_STANDART as built: look 1 makes material 1 (the red wall) a metal - first = 1, one record - and leaves
    # the plain instantiation; look 2 repaints the whole table and varnishes the green wall
    "cornell": {1: (1, (dict(type=_METAL, simpleColor=(0.8, 0.6, 0.2, 0)),)),
                2: (0, (dict(simpleColor=(0.25, 0.35, 0.8, 0)), dict(simpleColor=(0.9, 0.8, 0.1, 0)), dict(type=_VARNISH)))},
    # as built: textured glass, two plain varnishes.  Look 1: material 1 a plain red MAT_STANDART; look 2: material 0 a plain
    # colour, material 1 TEXTURED MAT_STANDART - plain colour to textured: the device screen of the texture coordinates runs
    "fuzz3_l1": {1: (1, (dict(type=_STD, simpleColor=(0.9, 0.2, 0.1, 0)),)),
                 2: (0, (dict(isSimpleColor=1), dict(type=_STD, isSimpleColor=0, textureId=0), dict(simpleColor=(0.1, 0.6, 0.3, 0))))},
    # as built: plain metal, plain water, textured metal
    "fuzz5h_l1": {1: (2, (dict(isSimpleColor=1, type=_STD),)),
                  2: (0, (dict(type=_VARNISH), dict(simpleColor=(0.2, 0.9, 0.4, 0)), dict(type=_GLASS, isSimpleColor=1)))},
    # as built: a plain colour of type 255, textured MAT_STANDART, a plain colour of type 5
    "fuzz41hr_l1": {1: (2, (dict(type=_STD, simpleColor=(0.3, 0.8, 0.5, 0)),)),
                    2: (0, (dict(simpleColor=(0.1, 0.3, 0.9, 0)), dict(isSimpleColor=1), dict(type=_GLASS)))},
}
TEXTURE_FLIP = ("fuzz3_l1", 2)  # (scene, materials look) that makes a plain-colour material textured
LIGHT_LOOKS = {  # (the two NANSAFE scenes: ptmi_update_lights is refused, so they have look 0 only)
    "cornell": {1: dict(type=S.LIGHT_SPOT, position=(200.0, 300.0, 400.0, 1.0), direction=(0.2, -0.1, -1.0, 0.0),
                        cosOfInnerFallOffAngle=0.9, cosOfOuterFallOffAngle=0.4)},
    "fuzz3_l1": {1: dict(position=(-1.5, 1.0, -2.0, 1.0))},
    # (no looks of these two, lights_of(): what the call that is refused sends)
    "fuzz5h_l1": {1: dict(direction=(0.3, 0.8, -0.5, 0.0))},
    "fuzz41hr_l1": {1: dict(direction=(0.3, 0.8, -0.5, 0.0))},
}
SKY_LOOKS = {
    # cornell and fuzz3_l1 are built with a sky of six faces of the one texel 0, which no rotation changes: their look 1 also
    # points the faces at other texels (cornell's anchor carries CORNELL_SKY_TEXELS behind its one texel for this, and no texture)
    "cornell": {1: (0.7, 2.5, ((2, 2, 1), (2, 2, 5), (3, 1, 2), (1, 3, 4), (2, 2, 3), (1, 1, 8)))},
    "fuzz3_l1": {1: (0.7, 2.5, ((3, 3, 1), (2, 2, 10), (4, 4, 20), (1, 1, 40), (5, 2, 45), (2, 1, 57)))},
    "fuzz5h_l1": {1: (0.7, 2.5, None)},
    "fuzz41hr_l1": {1: (-1.1, 0.5, None)},
}
CORNELL_SKY_TEXELS = [[250, 40, 40, 0], [40, 250, 40, 0], [40, 40, 250, 0], [250, 250, 40, 0], [40, 250, 250, 0], [250, 40, 250, 0],
                      [250, 250, 250, 0], [20, 20, 20, 0]]

PATH_BATCHES, PATH_FIRST_INDICES = (1, 257), (0, 1000, P.STRIDE - 257)  # (the last: the batch's last index is STRIDE - 1)
PATH_RAY_SEED = 0
REPROJECT_SETS = {"defaults": dict(backend.REPROJECT_DEFAULTS),
                  "narrow": dict(position_tolerance=0.02, normal_tolerance=0.25, max_history=2.0)}
EXPOSURES = (0.5, 1.0, 2.7, "histogram")  # (the last: backend.exposure_from_histogram of the image's own histogram)
WHITES = (float("inf"), 2.0)
DISPLAY_ROUTES = ("host", "device", "planes", "mean")
ASYNC = ("query", "guides", "denoise", "paths", "tonemap", "histogram")  # (kinds with a route through device pointers that is not waited for)
DENOISE_PLANES = ("albedo", "normal", "position", "hit_count")  # (the planes the filter reads)
DENOISE_PASSES = (0, 1, 2, 3, 4, 5)
# the sigmas of test_denoise_gpu.py (its SIGMAS) and the shipped defaults
SIGMA_SETS = {"narrow": dict(sigma_color=0.6, sigma_normal=0.5, sigma_position=1.5),
              "defaults": {key: backend.DENOISE_DEFAULTS[key] for key in ("sigma_color", "sigma_normal", "sigma_position")}}
DENOISE_ROUTES = ("host", "device", "planes")
N_OPS, N_OPS_SUPER_SAMPLING = 120, 90
# GENERATOR_SEED, DEFAULT_SEEDS and N_OPS were picked together, the weights above fixed first: N_OPS stayed 120, and of the
# generator seeds 0 to 39 none meets test_api_fuzz_model.py's coverage conditions with 5, 6 or 7 default seeds; with 8, seed 11
# is the first that does, and every defect test holds with it.  (Super-sampling scripts grew from 70 to 90 operations: they take
# the seventeen kinds in turn, about a quarter of their operations.)
GENERATOR_SEED = 11  # (of every script's draws)
HIT_FIELDS = ("point", "squared_distance", "s", "t", "triangle_id", "front", "box_tests", "triangle_tests")
TOTALS = tuple(name for name, _ in O.PtoTotals._fields_)


DEVICES = {"one": None, "two": [0, 0], "three": [0, 0, 0]}
DEFAULT_SEEDS = 8  # (the fewest with which test_api_fuzz_model.py's coverage conditions and defect tests hold: GENERATOR_SEED)
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

def plain_verdict(scene):
    """ptmi.h's rule for the kernel instantiation: plain where every material is a plain-colour MAT_STANDART and every light a
    point light"""
    m, l = scene.materiaux, scene.lights
    return bool((m["type"] == S.MAT_STANDART).all() and (m["isSimpleColor"] != 0).all() and (l["type"] == S.LIGHT_POINT).all())


def states_of(name, cameras=CAMERAS):
    """The states of a scene that the CPU tests walk: every (camera, version) at the base look, and every look at (camera 0,
    version 0) and at one other (camera, version)."""
    out = [(name, c, t, BASE_LOOK) for c in cameras for t in versions_of(name)]
    for c, t in ((0, 0), (2, versions_of(name)[-1])):
        out += [(name, c, t, look) for look in looks_of(name) if look != BASE_LOOK and c in cameras]
    return out


def looks_of(name):
    return [(m, g, k) for m in MATERIALS for g in lights_of(name) for k in SKIES]


def lights_of(name):
    return (0,) if name in NANSAFE else LIGHTS


class World:
    """The scenes, their variants and every yardstick result, each computed when first asked for and kept."""

    def __init__(self):
        self._anchor, self._tris, self._scene, self._per_it, self._rays, self._hits, self._yard = {}, {}, {}, {}, {}, {}, {}
        self._materials, self._lights, self._sky, self._path_rays, self._path_yard, self._sums = {}, {}, {}, {}, {}, {}

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
            if name == "cornell":  # texels for the sky of look 1 to point at (no texture: a textured material stays a refusal)
                sc.texturesData = np.concatenate([np.ascontiguousarray(sc.texturesData).reshape(-1, 4), np.array(CORNELL_SKY_TEXELS, np.uint8)])
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

    def materials(self, name, m):
        """the whole material table of materials look m"""
        if (name, m) not in self._materials:
            mats = U.raw_copy(self.anchor(name).materiaux)
            if m:
                first, records = MATERIAL_LOOKS[name][m]
                for k, fields in enumerate(records):
                    for field, value in fields.items():
                        mats[field][first + k] = value
            self._materials[name, m] = mats
        return self._materials[name, m]

    def lights(self, name, g):
        if (name, g) not in self._lights:
            lights = U.raw_copy(self.anchor(name).lights)
            if g:
                for field, value in LIGHT_LOOKS[name][g].items():
                    lights[field][0] = value
            self._lights[name, g] = lights
        return self._lights[name, g]

    def sky(self, name, k):
        if (name, k) not in self._sky:
            sky = self.anchor(name).sky.copy()
            if k:
                angle, ground, faces = SKY_LOOKS[name][k]
                sky["groundScale"] = ground
                sky["cosRotationAngle"], sky["sinRotationAngle"] = np.float32(np.cos(angle)), np.float32(np.sin(angle))
                for f, face in enumerate(faces or ()):
                    sky["skyTextures"][..., f] = face
            self._sky[name, k] = sky
        return self._sky[name, k]

    def scene(self, state):
        if state not in self._scene:
            name, c, t, (m, g, k) = state
            sc = U.moved_scene(self.camera(name, c), self.triangles(name, t))
            sc = E.edited(sc, materiaux=self.materials(name, m), lights=self.lights(name, g), sky=self.sky(name, k))
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
                self._rays[name] = Q.mixed_rays(self.scene((name, 0, 0, BASE_LOOK)), N_RAYS, W, H, seed=RAY_SEED)
        return self._rays[name]

    def hits(self, state, da, n=N_RAYS):
        """(the rays this state is sent, {any_hit: the hits ptmi_query_rays must return}, the indices of replaced rays), each
        valid for the first n rays: the walk goes as far into the set as a batch has asked so far.  Hits depend on the scene,
        its triangle version and the arithmetic alone - the rays are the caller's, and no look moves a triangle."""
        key = (state[0], state[2], da)
        if key not in self._hits:
            rays = self.rays(state[0]).copy()
            self._hits[key] = [rays, {False: np.zeros(len(rays), S.RAY_HIT), True: np.zeros(len(rays), S.RAY_HIT)}, [], 0,
                               Q.Walker(self.scene((state[0], 0, state[2], BASE_LOOK)), da)]
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

    def path_rays(self, name):
        """The rays the path calls send to a scene: path_query_cases.mixed_rays of the anchor (no direction component is an exact
        zero: the generators assert it)"""
        if name not in self._path_rays:
            with np.errstate(all="ignore"):
                self._path_rays[name] = P.mixed_rays(self.scene((name, 0, 0, BASE_LOOK)), max(PATH_BATCHES), W, H, seed=PATH_RAY_SEED)
        return self._path_rays[name]

    def path_sums(self, state, da, batch, first_iteration, n_iterations, first_index):
        """What ptmi_trace_paths must return: path sums depend on the scene, its triangle version, the look and the arithmetic,
        not on the camera (the rays are the caller's)."""
        name, _, t, look = state
        key = (name, t, look, da)
        if key not in self._path_yard:
            self._path_yard[key] = P.Yardstick(self.scene((name, 0, t, look)), depth=D, sampler=S.JITTERED, default_arithmetic=da)
        full = key + (batch, first_iteration, n_iterations, first_index)
        if full not in self._sums:
            self._sums[full] = self._path_yard[key].sums(self.path_rays(name)[:batch], first_iteration, n_iterations, first_index, P.STRIDE)
        return self._sums[full]


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

    def reprojected(self, c, tolerances, first, n, image=None):
        """ptmi_set_camera_reprojected to camera c: the accumulators (`image`: other planes in their place) resampled by
        reproject_cases.reproject between the guide yardstick's planes of the old and of the new state; then the state moves.
        Histograms, totals and slots stay."""
        name, _, t, look = self.state
        new = (name, c, t, look)
        sc = self.world.scene(self.state)
        previous, _ = self.world.planes(self.state, self.da, first, n)
        current, _ = self.world.planes(new, self.da, first, n)
        color, count = image if image is not None else (self.color, self.count)
        previous = dict(normal=previous["normal"], position=previous["position"], hit_count=previous["hit_count"], color=color, ray_nb=count)
        self.color, self.count = R.reproject((sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp), previous, current,
                                             **REPROJECT_SETS[tolerances])
        self.state = new


# ---------------------------------------------------------------------------------------------- the generator

class _Generator:
    def __init__(self, seed, devices, cap, super_sampling):
        self.rs = np.random.RandomState([int(seed), 2 if super_sampling else 1, GENERATOR_SEED])
        self.multi, self.ss, self.seed = bool(devices), super_sampling, int(seed)
        self.bursts = not flags_of(seed, super_sampling)[1]  # (ptmi_render_snapshots wants the wavefront kernel)
        self.few = RING if seed % 2 else 6  # (even seeds: six slots, so that snapshots overwrite each other all the time)
        self.names = [["cornell", "fuzz3_l1"][seed % 4 == 3]] if super_sampling else SCENES
        self.name, self.uploaded_version, self.updated = self.names[0], 0, False
        self.slots, self.queried, self.look = set(), False, [0, 0, 0]
        self.turns = {}

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

    def other(self, values, now):
        """mostly a value other than the one the scene has, so that the call changes something"""
        others = [v for v in values if v != now]
        return self.choice(others) if others and self.rs.rand() < 0.85 else now

    def display_route(self):
        # the context's own accumulators through device pointers: several devices refuse them (UNSUPPORTED), which is tried
        return str(self.rs.choice(DISPLAY_ROUTES, p=[0.4, 0.1, 0.25, 0.25] if self.multi else [0.3, 0.3, 0.2, 0.2]))

    def reprojected(self):
        rs = self.rs
        first = GUIDE_FIRSTS[int(rs.rand() < 0.15)]  # (as for guides)
        return ("reprojected", self.choice(CAMERAS), self.choice(sorted(REPROJECT_SETS)), first, int(rs.choice([1, 1, 1, 2, 3])))

    def turn_op(self, place):
        """The next kind of NEW_OPS in turn - every place has its own turn, from a start that depends on the seed - for the
        places every kind has to reach with few scripts: behind a burst, an upload and a call that is not waited for, and
        between a snapshot and its read."""
        self.turns[place] = self.turns.get(place, 7 * self.seed + 4 * len(self.turns)) + 1
        return self.new_op(NEW_OPS[self.turns[place] % len(NEW_OPS)])

    def new_op(self, kind=None):
        rs = self.rs
        kind = str(rs.choice(NEW_OPS, p=NEW_OP_WEIGHTS)) if kind is None else kind
        if kind == "denoise":
            return self.denoise()
        if kind == "camera":
            return ("camera", self.choice(CAMERAS))
        if kind in ("update", "update_device"):
            back = self.uploaded_version != 0 and not self.updated and rs.rand() < 0.5  # back to version 0 from a variant uploaded as one
            t = 0 if back else self.choice(VERSIONS)
            self.updated = True
            return (kind, t)
        if kind == "bad_update":
            return ("bad_update", self.choice(U.BAD_TRIANGLES))
        if kind == "bad_camera":
            return ("bad_camera", int(rs.randint(0, 4)))
        if kind == "materials":
            self.look[0] = self.other(MATERIALS, self.look[0])
            return ("materials", self.look[0])
        if kind == "lights":  # (a NANSAFE scene refuses it, which is tried: its lights stay)
            g = self.other(LIGHTS, self.look[1])
            self.look[1] = self.look[1] if self.name in NANSAFE else g
            return ("lights", g)
        if kind == "sky":
            self.look[2] = self.other(SKIES, self.look[2])
            return ("sky", self.look[2])
        if kind == "bad_materials":
            return ("bad_materials", self.choice(("beyond", "texture")))
        if kind == "bad_lights":
            return ("bad_lights", self.choice(("size", "position")))
        if kind == "reprojected":
            return self.reprojected()
        if kind == "tonemap":
            return ("tonemap", self.choice(DC.TONES), self.choice(DC.TRANSFERS), self.choice(EXPOSURES), self.choice(WHITES),
                    bool(rs.rand() < 0.4), self.display_route())
        if kind == "histogram":
            return ("histogram", self.display_route())
        route = "device" if not self.multi and rs.rand() < 0.4 else "host"
        if kind == "paths":
            # mostly one iteration from iteration 0 of the smaller indices: a path of an (index, iteration) is traced once and kept
            batch = PATH_BATCHES[int(rs.rand() < 0.5)]
            return ("paths", batch, int(rs.choice([0, 0, 1, 5])), int(rs.choice([1, 1, 2, 3])), self.choice(PATH_FIRST_INDICES), route)
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
        look = tuple(self.choice(values) if variant and self.rs.rand() < 0.4 else 0 for values in (MATERIALS, lights_of(name), SKIES))
        self.name, self.uploaded_version, self.updated, self.look = name, t, False, list(look)
        self.slots = set()
        return ("upload", name, c, t, look)

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
            new = self.turn_op("new") if self.ss else self.new_op()  # (the few super-sampling scripts: every kind in turn)
            # behind a call through device pointers, which is not waited for: the call that has to wait for the stream
            waits = new[0] in ASYNC and new[-1] in ("device", "planes", "mean") and rs.rand() < 0.7
            return [new] + ([self.turn_op("waits")] if waits else [])
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
                    inserts.append((c, self.turn_op("walk") if rs.rand() < 0.5 else self.new_op()))
            return [("walk", first, n, calls, look, look_at, tuple(inserts))]
        if op == "snapshot":
            slot = int(rs.randint(0, 5 if self.ss else self.few))
            self.slots.add(slot)
            if rs.rand() < 0.75:  # something new between the snapshot and the read of its slot (several devices: a lazy copy)
                return [("snapshot", slot), self.turn_op("snapshot"), self.read_slot(slot)]
            return [("snapshot", slot)]
        if op == "burst":
            if not self.bursts:
                return [("refused_burst",)]
            first, n, slot = int(rs.randint(0, N_IDS - 8)), int(rs.randint(1, 8)), int(rs.randint(0, self.few))
            self.slots |= {(slot + k) % RING for k in range(n)}
            return [("burst", first, n, slot)] + ([self.turn_op("burst")] if rs.rand() < 0.8 else [])
        if op == "read_slot":
            return [self.read_slot()]
        if op == "read_image":
            return [("read_image", bool(rs.rand() < 0.5))]
        if op == "upload":
            return [self.upload()] + ([self.turn_op("upload")] if rs.rand() < 0.8 else [])
        # the filter on accumulators that were just written, emptied or shown (the display shares the host form's internal slot);
        # a reprojection of them
        behind = []
        if op in ("write", "clear", "display") and not self.ss:
            draw = rs.rand()
            behind = [self.denoise()] if draw < 0.3 else [self.reprojected()] if draw < 0.55 and op != "display" else []
        elif op in ("write", "clear", "display") and rs.rand() < 0.35:
            behind = [self.denoise()]
        if op == "write":
            return [("write", int(rs.randint(0, 1 << 30)), int(rs.choice([0, 0, 1, 2, 3, 4, 5, 6, 7, 8])))] + behind
        return [(op,)] + behind  # statistics, counters, clear, sync, kernel_time, display, pin, variance, save, resume


def script(seed, devices, cap, super_sampling=False):
    """The operations of one case: [("upload", first scene, 0, 0, BASE_LOOK), ...].  `cap` (PTMI_ITERATIONS_PER_LAUNCH of the case) does
    not change the script: it is an argument so that every case has one signature."""
    g = _Generator(seed, devices, cap, super_sampling)
    ops = [("upload", g.name, 0, 0, BASE_LOOK)]
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
        self.denoised = got
        return lambda: (got, guides)

    def update(self, be, tris):
        return getattr(be, "device_update", be.update_triangles)(tris)

    def paths(self, be, rays, first_iteration, n_iterations, first_index):
        got = be.trace_paths(rays["origin"], rays["direction"], first_iteration, n_iterations, first_index, P.STRIDE)
        return lambda: got

    def _planes(self, be, image):
        """(colour, count or None) of an image given as None (the backend's accumulators: not here), (sums, counts), ("mean",
        plane) or ("denoised",): the result of the denoise call made just before"""
        if not isinstance(image[0], str):
            return image
        return (self.denoised if image[0] == "denoised" else image[1]), None

    def display(self, be, image, params):
        """-> a function that returns (the pixels, the mean plane they were made of or None).  As for denoise: planes of the
        caller's are displayed here by the yardstick, so those routes check nothing of a backend without a device."""
        if image is None:
            if getattr(be, "n_devices", 1) > 1:
                raise PtmiError(UNSUPPORTED, "ptmi_display_device: a multi-device context has partial sums per device")
            got = be.display(**params)
            return lambda: (got, None)
        color, count = self._planes(be, image)
        got = display_yardstick((color, count), params)
        return lambda: (got, color if count is None else None)

    def histogram(self, be, image):
        if image is None:
            if getattr(be, "n_devices", 1) > 1:
                raise PtmiError(UNSUPPORTED, "ptmi_luminance_histogram_device: a multi-device context has partial sums per device")
            got = be.luminance_histogram()
            return lambda: (got, None)
        color, count = self._planes(be, image)
        got = DC.histogram(color, count)
        return lambda: (got, color if count is None else None)


def display_yardstick(image, params):
    """display_cases.tonemap of (colour sums, counts) - counts None: a mean plane - packed as the call's format asks"""
    rgb = DC.tonemap(image[0], image[1], params)
    return DC.pack_rgba32(rgb) if params["rgba"] else DC.pack_bgr24(rgb, (3 * W + 3) & ~3)


def seeded_mean(seed):
    """A mean plane of the caller's: seeded_image's colours, the fourth word (which nothing may read) a NaN in every other pixel"""
    plane = seeded_image(seed)[0].copy()
    plane[..., 3].reshape(-1)[::2] = np.nan
    return plane


def material_range(name, m, current, target):
    """(first, n) of the ptmi_update_materials call that turns the table `current` into `target`, look m's table: the look's own
    range (look 0: none), widened by whatever else differs; nothing at all: the whole table"""
    differ = [i for i in range(len(target)) if current[i].tobytes() != target[i].tobytes()]
    lo, hi = (MATERIAL_LOOKS[name][m][0], MATERIAL_LOOKS[name][m][0] + len(MATERIAL_LOOKS[name][m][1])) if m else (len(target), 0)
    if differ:
        lo, hi = min(lo, differ[0]), max(hi, differ[-1] + 1)
    return (lo, hi - lo) if hi > lo else (0, len(target))


def bad_materials(sc, kind):
    """(first, records) of a refused ptmi_update_materials: one record beyond the table, or a texture that was not uploaded"""
    mats = U.raw_copy(sc.materiaux)
    if kind == "beyond":
        return len(mats) - 1, mats[:2]
    bad = mats[:1]
    bad["isSimpleColor"], bad["textureId"] = 0, len(sc.textures)
    return 1, bad


def bad_lights(sc, kind):
    lights = U.raw_copy(sc.lights)
    if kind == "size":
        return np.concatenate([lights, lights])
    lights["position"][0] = (np.inf, 0, 0, 1)
    return lights


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
    it reads against `model`.  `io`: how calls through device pointers are made, an object with query(), guides(), denoise(),
    update(), paths(), display() and histogram(), which (but for the synchronous update) return a function to collect the result
    with (HostIO: through the host calls).  `exact`: one device - colour sums bit for bit, and the context's own accumulators
    served through device pointers; else colours within the association error of several devices' partial sums, and those
    calls refused.  Raises Mismatch with the last 40 calls.  Returns the number of operations made, per kind."""
    from opencl_pathtracer_amd import output
    io = io or HostIO()
    world, m = model.world, model
    history, made, pending = [], {}, []
    pinned = [np.empty((H, W, 4), np.float32), np.empty((H, W), np.float32)]
    pinned_result = np.empty((H, W, 4), np.float32)  # (where every other host-route denoise lands; pinned and unpinned with the two)
    host_denoises, host_displays = [0], [0]
    pinned_pixels = {False: np.empty((H, (3 * W + 3) & ~3), np.uint8), True: np.empty((H, W, 4), np.uint8)}  # (a host tonemap in three)
    io.denoised = None
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
        name, cam, version, look = m.state if m.state else (None, None, None, None)
        if kind == "upload":
            state = tuple(op[1:])
            be.initialize_memory(world.scene(state))
            check((be.literal_kernel_reason() is not None) == (state[0] in NANSAFE), f"literal_kernel_reason() is {be.literal_kernel_reason()!r}", op)
            m.upload(state)
            saved[0] = None
        elif kind == "camera":
            sc = world.camera(name, op[1])
            be.set_camera(sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp)
            m.state = (name, op[1], version, look)
        elif kind in ("update", "update_device"):
            tris = world.triangles(name, op[1])
            update = be.update_triangles if kind == "update" else (lambda t: io.update(be, t))
            if name in NANSAFE:  # the kernel instantiation was chosen at upload: refused, and the scene stays
                refused(lambda: update(tris), UNSUPPORTED, op)
            else:
                update(tris)
                m.state = (name, cam, op[1], look)
        elif kind == "bad_update":
            tris = U.bad_triangles(world.scene(m.state), op[1])
            refused(lambda: be.update_triangles(tris), INVALID_ARGUMENT if op[1] == "wrong_count" else UNSUPPORTED, op)
        elif kind == "bad_camera":
            sc = bad_camera(world.camera(name, cam), op[1] & 1)
            vectors = (sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp)
            if op[1] >= 2:  # the same through the entry point that takes the image along
                refused(lambda: be.set_camera_reprojected(*vectors, **REPROJECT_SETS["defaults"]), UNSUPPORTED, op)
            else:
                refused(lambda: be.set_camera(*vectors), UNSUPPORTED, op)
        elif kind == "materials":
            current, target = world.materials(name, look[0]), world.materials(name, op[1])
            first, n = material_range(name, op[1], current, target)
            new = (name, cam, version, (op[1], look[1], look[2]))
            info = be.update_materials(first, target[first:first + n])
            want = (plain_verdict(world.scene(m.state)), plain_verdict(world.scene(new)))
            got = (bool(info["plain_before"]), bool(info["plain_after"]))
            check(got == want, f"materials: (plain_before, plain_after) is {got} instead of {want}", op)
            flips = bool(((target["isSimpleColor"][first:first + n] == 0) & (current["isSimpleColor"][first:first + n] != 0)).any())
            check((info["screened_triangles"] > 0) == flips, f"materials: screened_triangles is {info['screened_triangles']}, a plain colour "
                  f"turns textured: {flips}", op)
            m.state = new
        elif kind == "lights":
            lights = world.lights(name, op[1])
            if name in NANSAFE:  # refused, and the lights stay
                refused(lambda: be.update_lights(lights), UNSUPPORTED, op)
            else:
                be.update_lights(lights)
                m.state = (name, cam, version, (look[0], op[1], look[2]))
        elif kind == "sky":
            be.set_sky(world.sky(name, op[1]))
            m.state = (name, cam, version, (look[0], look[1], op[1]))
        elif kind == "bad_materials":
            first, records = bad_materials(world.scene(m.state), op[1])
            refused(lambda: be.update_materials(first, records), INVALID_ARGUMENT if op[1] == "beyond" else BAD_SCENE, op)
        elif kind == "bad_lights":
            lights = bad_lights(world.scene(m.state), op[1])
            refused(lambda: be.update_lights(lights), INVALID_ARGUMENT if op[1] == "size" else UNSUPPORTED, op)
        elif kind == "reprojected":
            _, c, tolerances, first, n = op
            sc = world.camera(name, c)
            vectors = (sc.cameraPosition, sc.cameraDirection, sc.cameraRight, sc.cameraUp)
            params = dict(REPROJECT_SETS[tolerances], guide_first_iteration=first, guide_iterations=n)
            if m.ss:  # refused: nothing changes, the camera included
                refused(lambda: be.set_camera_reprojected(*vectors, **params), UNSUPPORTED, op)
            else:
                be.set_camera_reprojected(*vectors, **params)
                m.reprojected(c, tolerances, first, n)
        elif kind == "paths":
            _, batch, first_iteration, n_iterations, first_index, route = op
            rays = world.path_rays(name)[:batch].copy()
            want = world.path_sums(m.state, m.da, batch, first_iteration, n_iterations, first_index)

            def compare(got):
                msg = P.describe_difference(got, want)
                check(not msg, "paths: " + msg, op)

            if route == "device":
                collect = io.paths(be, rays, first_iteration, n_iterations, first_index)
                pending.append(lambda: compare(collect()))
            else:
                compare(be.trace_paths(rays["origin"], rays["direction"], first_iteration, n_iterations, first_index, P.STRIDE))
        elif kind in ("tonemap", "histogram"):
            route = op[-1]
            params = dict(tone=op[1], transfer=op[2], exposure=op[3], white=op[4], rgba=op[5]) if kind == "tonemap" else None
            if route == "host":
                # first the call, on whatever is in flight; then the image it had to show
                host_displays[0] += 1
                histogram = be.luminance_histogram() if kind == "histogram" or params["exposure"] == "histogram" else None
                if kind == "tonemap":
                    if params["exposure"] == "histogram":
                        params["exposure"] = backend.exposure_from_histogram(histogram)
                    out = None if host_displays[0] % 3 else pinned_pixels[params["rgba"]]
                    if out is not None:
                        out.fill(7)
                    got = be.display(out=out, **params)
                image = be.read_image()
                same_image(image, m.color, m.count, f"image behind a {kind}", op)
                if histogram is not None:
                    check(np.array_equal(histogram, DC.histogram(*image)), f"{kind}: the luminance histogram differs", op)
                if kind == "tonemap":
                    check(np.array_equal(got, display_yardstick(image, params)), f"tonemap (host, {params}): bytes differ", op)
            else:
                before = history[-2] if len(history) > 1 else ("none",)
                if route == "device":
                    image, planes = None, (m.color.copy(), m.count.copy())
                elif route == "planes":
                    image = planes = seeded_image([len(history), 7])
                elif before[0] == "denoise" and before[7] != "host" and io.denoised is not None:
                    image, planes = ("denoised",), None  # the viewer's pipeline: the tensor ptmi_denoise_device has just written
                else:
                    image = ("mean", seeded_mean([len(history), 11]))
                    planes = (image[1], None)
                if kind == "tonemap" and params["exposure"] == "histogram":
                    params["exposure"] = backend.exposure_from_histogram(DC.histogram(*planes)) if planes else 1.3
                call = (lambda: io.display(be, image, params)) if kind == "tonemap" else (lambda: io.histogram(be, image))
                if route == "device" and not exact:  # several devices: each holds partial sums
                    refused(call, UNSUPPORTED, op)
                    return
                collect = call()

                def collected():
                    got, mean = collect()
                    source = planes if planes else (mean, None)
                    want = display_yardstick(source, params) if kind == "tonemap" else DC.histogram(*source)
                    check(np.array_equal(got, want), f"{kind} ({route}, {params}): {'bytes' if kind == 'tonemap' else 'words'} differ", op)

                pending.append(collected)
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
            for a in pinned + [pinned_result] + list(pinned_pixels.values()):
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
        for a in pinned + [pinned_result] + list(pinned_pixels.values()):
            be.unpin_host_buffer(a)
    made.pop("walk call", None)
    made.pop("final image", None)
    return made
