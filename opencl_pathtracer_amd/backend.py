"""Host-side mirror of the reference's device backend, on top of the C ABI of ``libptmi.so``.

The reference's orchestration drives its backend with three calls
(``Controleur/PathTracer_OpenCL.h:17-19``, called from ``PathTracer.cpp:74,76,82``)::

    OpenCL_SetupContext(globalVars, sampler)
    OpenCL_InitializeMemory(globalVars)
    OpenCL_RunKernel(globalVars, UpdateWindowFunc, numImagesToRender, &t1, &t2, &t3)

``Backend`` exposes the same three steps with the same meaning and order
(`setup_context`, `initialize_memory`, `run_kernel`) plus the range form the
MI355X build adds (`render(first_iteration, n)`).  Python here is plumbing: every
pixel is computed by the HIP kernels behind ``include/ptmi.h``; if the library or a
GPU is missing the calls raise -- there is no CPU path in the product.

Errors: the reference throws ``std::runtime_error`` for any backend failure
(PathTracer_OpenCL.cpp:350-387,485); here every non-zero status raises ``PtmiError``
(a RuntimeError) carrying ``ptmi_last_error``.
"""
import ctypes as C
import os
import time

import numpy as np

from . import structs as S

# PTMI_LIBRARY lets a developer A/B another in-tree build of the same ABI (tools/build_variants.sh, tools/run_variants.sh)
_LIB_PATH = os.environ.get("PTMI_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libptmi.so")
_lib = None


class PtmiError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"ptmi error {code}: {message}")
        self.code = code


class Float4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("image_width", C.c_uint32),
                ("image_height", C.c_uint32), ("ray_max_depth", C.c_uint32), ("lights_size", C.c_uint32),
                ("sampler", C.c_uint32), ("super_sampling", C.c_uint32), ("flags", C.c_uint32),
                ("n_devices", C.c_uint32), ("devices", C.c_int32 * 16)]


class SceneDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32),
                ("bvh", C.c_void_p), ("bvh_size", C.c_uint32),
                ("triangulation", C.c_void_p), ("triangulation_size", C.c_uint32),
                ("lights", C.c_void_p), ("lights_size", C.c_uint32),
                ("materiaux", C.c_void_p), ("materiaux_size", C.c_uint32),
                ("textures", C.c_void_p), ("textures_size", C.c_uint32),
                ("textures_data", C.c_void_p), ("textures_data_size", C.c_uint32),
                ("sky", C.c_void_p),
                ("camera_position", Float4), ("camera_direction", Float4), ("camera_right", Float4),
                ("camera_up", Float4)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("paths", "segments", "surface_hits", "shadow_rays", "box_tests",
                                         "triangle_tests")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BvhBuildInfo(C.Structure):
    """ptmi_bvh_build_info: what ptmi_bvh_create_device did (fallback: 0 none, 1 stale axis, 2 host error, 3 records)."""
    _fields_ = [("struct_size", C.c_uint32), ("built_on_device", C.c_uint32), ("fallback", C.c_uint32), ("levels", C.c_uint32),
                ("device_ms", C.c_double), ("total_ms", C.c_double), ("upload_ms", C.c_double), ("download_ms", C.c_double),
                ("permute_ms", C.c_double), ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class UpdateInfo(C.Structure):
    """ptmi_update_info: what ptmi_update_triangles did (level passes of the refit, and where the time went)."""
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_uint32), ("upload_ms", C.c_double), ("device_ms", C.c_double),
                ("total_ms", C.c_double), ("validate_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MeshTopology(C.Structure):
    """ptmi_mesh_topology: host arrays ptmi_bind_mesh copies (None = the default ptmi.h names)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_triangles", C.c_uint32), ("n_vertices", C.c_uint32), ("reserved", C.c_uint32),
                ("indices", C.c_void_p), ("uvp", C.c_void_p), ("uvn", C.c_void_p), ("mat_pos", C.c_void_p), ("mat_neg", C.c_void_p),
                ("ids", C.c_void_p)]


class VertexBuffers(C.Structure):
    """ptmi_vertex_buffers: host or device addresses of the positions and (None: a flat mesh) the normals, strides in bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("n_vertices", C.c_uint32), ("position_stride", C.c_uint32), ("normal_stride", C.c_uint32),
                ("positions", C.c_void_p), ("normals", C.c_void_p)]


class MaterialUpdateInfo(C.Structure):
    """ptmi_material_update_info: what ptmi_update_materials did (whether its device screen ran, and the plain-shading flip)."""
    _fields_ = [("struct_size", C.c_uint32), ("screened_triangles", C.c_uint32), ("plain_before", C.c_uint32),
                ("plain_after", C.c_uint32), ("validate_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Guides(C.Structure):
    """ptmi_guides: the planes ptmi_render_guides fills (host or device addresses; None = not written)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("albedo", C.c_void_p), ("normal", C.c_void_p),
                ("position", C.c_void_p), ("hit_count", C.c_void_p), ("ids", C.c_void_p)]


GUIDE_PLANES = ("albedo", "normal", "position", "hit_count", "ids")  # ptmi_guides, in the struct's order


class DenoiseParams(C.Structure):
    """ptmi_denoise_params: the filter of ptmi_denoise / ptmi_denoise_device (ptmi.h states its arithmetic)."""
    _fields_ = [("struct_size", C.c_uint32), ("passes", C.c_uint32), ("flags", C.c_uint32), ("guide_first_iteration", C.c_uint32),
                ("guide_iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float), ("reserved", C.c_uint32 * 2)]


class ReprojectParams(C.Structure):
    """ptmi_reproject_params: the tests of ptmi_reproject_device / ptmi_set_camera_reprojected (ptmi.h states its arithmetic)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("guide_first_iteration", C.c_uint32),
                ("guide_iterations", C.c_uint32), ("position_tolerance", C.c_float), ("normal_tolerance", C.c_float),
                ("max_history", C.c_float), ("reserved", C.c_uint32)]


class DisplayParams(C.Structure):
    """ptmi_display_params: exposure, tone operator, transfer function and pixel format of ptmi_read_display_tonemapped /
    ptmi_display_device (ptmi.h states its arithmetic)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("tone", C.c_uint32), ("transfer", C.c_uint32),
                ("format", C.c_uint32), ("row_stride", C.c_uint32), ("exposure", C.c_float), ("white", C.c_float),
                ("reserved", C.c_uint32 * 4)]


class PathParams(C.Structure):
    """ptmi_path_params: which iterations ptmi_trace_paths traces for every ray, and the index its seeds come from."""
    _fields_ = [("struct_size", C.c_uint32), ("first_iteration", C.c_uint32), ("n_iterations", C.c_uint32),
                ("first_index", C.c_uint32), ("index_stride", C.c_uint32), ("reserved", C.c_uint32 * 3)]


MAX_PATH_ITERATIONS = 4096  # ptmi.h: PTMI_MAX_PATH_ITERATIONS

DENOISE_DEMODULATE_ALBEDO, DENOISE_UNTILED = 1, 2  # ptmi.h: PTMI_DENOISE_*
# The shipped defaults: the RMSE minimum against a 1024-spp render of the Cornell box at 4 spp, over the grid of
# profiles/denoise_quality_cornell.json (tests/test_denoise_gpu.py holds them to it).  sigma_position is in scene units.
# That box is 555 units wide: scale sigma_position with the scene (about 3 % of its extent).
DENOISE_DEFAULTS = dict(passes=5, sigma_color=8.0, sigma_normal=1.0, sigma_position=16.0)

# The shipped defaults of the reprojection: the RMSE minimum against 1024 further iterations after a small orbit of the Cornell
# camera, 16 iterations before the move and 4 after it, over the grid of profiles/reproject_quality_cornell.json
# (tests/test_reproject_gpu.py holds them to it).  position_tolerance is relative to the distance from the previous camera.
# From 0.64 on the position test rejects nothing in that box (RMSE is flat from 0.08 on), so THIS DEFAULT IN EFFECT SWITCHES THE
# POSITION TEST OFF and the normal test and the image's frame do the work: tighten it to a few pixel spacings
# (a pixel is 1 / W of the distance wide) where parallel surfaces lie at different depths.
REPROJECT_DEFAULTS = dict(position_tolerance=0.64, normal_tolerance=1.0, max_history=16.0)

TONE_CLAMP, TONE_REINHARD, TONE_FILMIC = 0, 1, 2  # ptmi.h: PTMI_TONE_*
TRANSFER_LINEAR, TRANSFER_SRGB, TRANSFER_GAMMA22 = 0, 1, 2  # ptmi.h: PTMI_TRANSFER_*
PIXELS_BGR24, PIXELS_RGBA32 = 0, 1  # ptmi.h: PTMI_PIXELS_*
LUMINANCE_WORDS = 260  # ptmi.h: PTMI_LUMINANCE_WORDS
# What a viewer wants by default, and not what read_display gives (the reference viewer's linear clamp, kept for parity): a
# filmic curve that rolls the highlights off instead of clipping them, and the sRGB encoding displays expect.
DISPLAY_DEFAULTS = dict(tone=TONE_FILMIC, transfer=TRANSFER_SRGB, exposure=1.0, white=float("inf"))


BVH_FALLBACK_NONE, BVH_FALLBACK_STALE_AXIS, BVH_FALLBACK_HOST_ERROR, BVH_FALLBACK_RECORDS = 0, 1, 2, 3


class SchedulerStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("trips_node", "lanes_node", "trips_triangle", "lanes_triangle", "trips_path",
                                         "lanes_path", "cycles_path", "cycles_loop", "leaf_item_violations", "paths_retraced", "textured_hits", "workgroup_lanes",
                                         "resident_workgroups")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


USER_SNAPSHOT_SLOTS = 64  # ptmi.h: PTMI_MAX_SNAPSHOT_SLOTS - 1 (the last slot is the library's own)
class InvariantChecks(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("sample_out_of_range", "normal_not_facing_ray", "negative_direct_radiance",
                                         "scattered_below_surface", "statistics_out_of_range", "refraction_undefined_in_reference")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


FLAG_NO_HISTOGRAMS = 1
FLAG_SCHEDULER_STATS = 4  # collect scheduler_stats() (off by default)
FLAG_MEGAKERNEL = 2  # one path per lane instead of the persistent wavefront kernel (same results)
FLAG_RUSSIAN_ROULETTE = 8  # non-parity mode: the reference's commented-out termination block (FullKernel.cl:1306-1314)
# the arithmetic of the build the reference's own build line gives (OpenCL default: fused a*b+c, v_rcp_f32 division, v_sqrt_f32);
# without it the strict arithmetic (-ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt).  Both bit for bit.
FLAG_DEFAULT_ARITHMETIC = 16
FLAG_SOURCE_SEED = 32  # non-parity mode: seed 1 (as the source text reads) where the compiled reference keeps seed 0 (1 path in 65536)

# every symbol include/ptmi.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = ["ptmi_setup_context", "ptmi_initialize_memory", "ptmi_render", "ptmi_synchronize", "ptmi_read_image",
               "ptmi_write_image", "ptmi_pin_host_buffer", "ptmi_unpin_host_buffer", "ptmi_snapshot", "ptmi_render_snapshots", "ptmi_read_snapshot", "ptmi_write_variance", "ptmi_read_display", "ptmi_read_statistics", "ptmi_clear", "ptmi_release", "ptmi_get_counters", "ptmi_get_scheduler_stats", "ptmi_get_invariant_checks", "ptmi_literal_kernel_reason", "ptmi_validate_scene",
               "ptmi_kernel_time", "ptmi_reduce_path",
               "ptmi_set_stream", "ptmi_device_accumulators", "ptmi_bind_accumulators", "ptmi_read_variance",
               "ptmi_device_variance", "ptmi_last_error",
               "ptmi_abi_version", "ptmi_device_count", "ptmi_device_share", "ptmi_bvh_create",
               "ptmi_bvh_create_device", "ptmi_set_camera", "ptmi_update_triangles", "ptmi_update_triangles_device", "ptmi_bvh_refit",
               "ptmi_bind_mesh", "ptmi_update_vertices", "ptmi_update_vertices_device", "ptmi_assemble_triangles",
               "ptmi_update_materials", "ptmi_update_lights", "ptmi_set_sky",
               "ptmi_query_rays", "ptmi_query_rays_device", "ptmi_render_guides", "ptmi_render_guides_device",
               "ptmi_denoise", "ptmi_denoise_device", "ptmi_trace_paths", "ptmi_trace_paths_device",
               "ptmi_reproject_device", "ptmi_set_camera_reprojected",
               "ptmi_display_table", "ptmi_read_display_tonemapped", "ptmi_display_device", "ptmi_luminance_histogram",
               "ptmi_luminance_histogram_device", "ptmi_render_region", "ptmi_read_region"]

QUERY_CLOSEST, QUERY_ANY = 0, 1  # ptmi.h: PTMI_QUERY_*


def display_table(transfer):
    """float32[256]: the thresholds of a ``TRANSFER_*`` function - byte k is shown from T[k] on (ptmi_display_table; no device)."""
    lib = load_library()
    out = np.empty(256, np.float32)
    rc = lib.ptmi_display_table(transfer, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise PtmiError(rc, lib.ptmi_last_error(None).decode())
    return out


def exposure_from_histogram(hist, key=0.18):
    """The exposure that brings the image's log-average luminance to ``key`` (middle grey), from ``luminance_histogram``'s words:
    bin b stands for log2 luminance L_b = (b >> 2) - 32 + log2(1 + ((b & 3) + 0.5) / 4), the middle of its quarter octave;
    exposure = key / 2 ** (sum(hist[b] * L_b) / sum(hist[b])) over words 0..255.  1.0 where no pixel is positive.  Host only, in
    Python double."""
    import math
    counts = [int(x) for x in hist[:256]]
    total = sum(counts)
    if total == 0:
        return 1.0
    mean = sum(n * ((b >> 2) - 32 + math.log2(1 + ((b & 3) + 0.5) / 4)) for b, n in enumerate(counts) if n) / total
    return key / 2.0 ** mean


def library_path():
    return _LIB_PATH


def load_library():
    """Load libptmi.so (built in-tree by ``__graft_entry__.build()`` / ``make lib``).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise PtmiError(-7, f"{_LIB_PATH} is missing: build it with `make lib` (there is no fallback path)")
    lib = C.CDLL(_LIB_PATH)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.ptmi_setup_context.argtypes = [C.POINTER(vp), C.POINTER(Config)]
    lib.ptmi_initialize_memory.argtypes = [vp, C.POINTER(SceneDesc)]
    lib.ptmi_render.argtypes = [vp, u32, u32]
    lib.ptmi_synchronize.argtypes = [vp]
    lib.ptmi_read_image.argtypes = [vp, vp, vp]
    lib.ptmi_read_display.argtypes = [vp, vp, u32]
    lib.ptmi_snapshot.argtypes = [vp, u32]
    lib.ptmi_render_snapshots.argtypes = [vp, u32, u32, u32]
    lib.ptmi_pin_host_buffer.argtypes = [vp, vp, C.c_size_t]
    lib.ptmi_unpin_host_buffer.argtypes = [vp, vp]
    lib.ptmi_read_snapshot.argtypes = [vp, u32, vp, vp]
    lib.ptmi_write_variance.argtypes = [vp, vp]
    lib.ptmi_write_image.argtypes = [vp, vp, vp]
    lib.ptmi_read_statistics.argtypes = [vp, vp, vp, vp]
    lib.ptmi_clear.argtypes = [vp]
    lib.ptmi_release.argtypes = [vp]
    lib.ptmi_release.restype = None
    lib.ptmi_get_counters.argtypes = [vp, C.POINTER(Counters)]
    lib.ptmi_get_scheduler_stats.argtypes = [vp, C.POINTER(SchedulerStats)]
    lib.ptmi_get_invariant_checks.argtypes = [vp, C.POINTER(InvariantChecks)]
    lib.ptmi_validate_scene.argtypes = [C.POINTER(Config), C.POINTER(SceneDesc)]
    lib.ptmi_literal_kernel_reason.argtypes = [vp]
    lib.ptmi_literal_kernel_reason.restype = C.c_char_p
    lib.ptmi_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    lib.ptmi_reduce_path.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ptmi_set_stream.argtypes = [vp, vp]
    lib.ptmi_device_accumulators.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.ptmi_bind_accumulators.argtypes = [vp, vp, vp]
    lib.ptmi_read_variance.argtypes = [vp, vp]
    lib.ptmi_device_variance.argtypes = [vp, C.POINTER(vp)]
    lib.ptmi_last_error.argtypes = [vp]
    lib.ptmi_last_error.restype = C.c_char_p
    lib.ptmi_bvh_create.argtypes = [vp, u32, vp, C.POINTER(u32), C.POINTER(u32)]
    lib.ptmi_bvh_create_device.argtypes = [C.c_int32, vp, u32, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(BvhBuildInfo)]
    lib.ptmi_set_camera.argtypes = [vp, C.POINTER(Float4), C.POINTER(Float4), C.POINTER(Float4), C.POINTER(Float4)]
    lib.ptmi_update_triangles.argtypes = [vp, vp, u32, C.POINTER(UpdateInfo)]
    lib.ptmi_update_triangles_device.argtypes = [vp, vp, u32, C.POINTER(UpdateInfo)]
    lib.ptmi_bind_mesh.argtypes = [vp, C.POINTER(MeshTopology)]
    lib.ptmi_update_vertices.argtypes = [vp, C.POINTER(VertexBuffers), C.POINTER(UpdateInfo)]
    lib.ptmi_update_vertices_device.argtypes = [vp, C.POINTER(VertexBuffers), C.POINTER(UpdateInfo)]
    lib.ptmi_assemble_triangles.argtypes = [C.POINTER(MeshTopology), C.POINTER(VertexBuffers), vp]
    lib.ptmi_update_materials.argtypes = [vp, u32, vp, u32, C.POINTER(MaterialUpdateInfo)]
    lib.ptmi_update_lights.argtypes = [vp, vp, u32]
    lib.ptmi_set_sky.argtypes = [vp, vp]
    lib.ptmi_bvh_refit.argtypes = [vp, u32, vp, u32]
    lib.ptmi_query_rays.argtypes = [vp, u32, vp, u32, vp]
    lib.ptmi_query_rays_device.argtypes = [vp, u32, vp, u32, vp]
    lib.ptmi_trace_paths.argtypes = [vp, C.POINTER(PathParams), vp, u32, vp]
    lib.ptmi_trace_paths_device.argtypes = [vp, C.POINTER(PathParams), vp, u32, vp]
    lib.ptmi_render_guides.argtypes = [vp, u32, u32, C.POINTER(Guides)]
    lib.ptmi_render_guides_device.argtypes = [vp, u32, u32, C.POINTER(Guides)]
    lib.ptmi_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp]
    lib.ptmi_denoise_device.argtypes = [vp, C.POINTER(DenoiseParams), C.POINTER(Guides), vp, vp, vp]
    lib.ptmi_reproject_device.argtypes = [vp, C.POINTER(ReprojectParams), C.POINTER(Float4 * 4), C.POINTER(Guides), vp, vp, C.POINTER(Guides), vp, vp]
    lib.ptmi_set_camera_reprojected.argtypes = [vp, C.POINTER(Float4), C.POINTER(Float4), C.POINTER(Float4), C.POINTER(Float4),
                                                C.POINTER(ReprojectParams)]
    lib.ptmi_display_table.argtypes = [u32, vp]
    lib.ptmi_read_display_tonemapped.argtypes = [vp, C.POINTER(DisplayParams), vp]
    lib.ptmi_display_device.argtypes = [vp, C.POINTER(DisplayParams), vp, vp, vp]
    lib.ptmi_luminance_histogram.argtypes = [vp, vp]
    lib.ptmi_luminance_histogram_device.argtypes = [vp, vp, vp, vp]
    lib.ptmi_render_region.argtypes = [vp, vp, u32, u32]
    lib.ptmi_read_region.argtypes = [vp, vp, vp, vp]
    lib.ptmi_device_share.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    lib.ptmi_device_share.restype = None
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _f4(v):
    v = np.asarray(v, np.float32)
    return Float4(float(v[0]), float(v[1]), float(v[2]), float(v[3]))


def make_rays(origins, directions, max_squared_distance=None):
    """A ``structs.RAY`` array from float32 (n,3) / (n,4) origins and directions (w = 0 for (n,3)) and a scalar or n distance
    limits (None: INFINITY)."""
    o, d = np.asarray(origins, np.float32), np.asarray(directions, np.float32)
    if o.ndim != 2 or d.ndim != 2 or o.shape[0] != d.shape[0] or o.shape[1] not in (3, 4) or d.shape[1] not in (3, 4):
        raise PtmiError(-1, "origins and directions must be (n,3) or (n,4) arrays of the same length")
    rays = np.zeros(len(o), S.RAY)
    rays["origin"][:, :o.shape[1]] = o
    rays["direction"][:, :d.shape[1]] = d
    rays["max_squared_distance"] = np.inf if max_squared_distance is None else np.asarray(max_squared_distance, np.float32)
    return rays


def device_share(first_iteration, n_iterations, k, n_devices):
    """(first_k, n_k): the iteration ids device ``k`` of ``n_devices`` takes from a render call (ids = k mod n_devices)."""
    lib = load_library()
    f, n = C.c_uint32(0), C.c_uint32(0)
    lib.ptmi_device_share(first_iteration, n_iterations, k, n_devices, C.byref(f), C.byref(n))
    return f.value, n.value


def bvh_create(scene, device=None):
    """``BVH_Create(globalVars)`` (PathTracer_BVH.cpp:12-37): builds ``scene.bvh`` and reorders
    ``scene.triangulation`` in place, exactly like the reference.  ``device=None``: on the host (no GPU needed);
    an ordinal: ``ptmi_bvh_create_device`` on that HIP device - the same bytes - with its ``BvhBuildInfo`` in
    ``scene.bvh_build_info`` (whether the device built the tree or handed the scene to the host builder, and timings)."""
    lib = load_library()
    tris = np.ascontiguousarray(scene.triangulation)
    if tris.dtype != S.Triangle:
        raise PtmiError(-1, "triangulation must have the 336-byte structs.Triangle dtype")
    n = len(tris)
    nodes = np.zeros(max(2 * n - 1, 1), dtype=S.Node)
    size, depth = C.c_uint32(0), C.c_uint32(0)
    if device is None:
        rc = lib.ptmi_bvh_create(_ptr(tris), n, _ptr(nodes), C.byref(size), C.byref(depth))
    else:
        info = BvhBuildInfo()
        rc = lib.ptmi_bvh_create_device(int(device), _ptr(tris), n, _ptr(nodes), C.byref(size), C.byref(depth), C.byref(info))
        scene.bvh_build_info = info
    if rc:
        raise PtmiError(rc, lib.ptmi_last_error(None).decode())
    scene.triangulation = tris
    # byte-level copy (numpy's .copy() of a padded struct dtype leaves the padding bytes undefined)
    scene.bvh = np.frombuffer(bytearray(nodes[:size.value].tobytes()), dtype=S.Node)
    scene.bvhMaxDepth = depth.value
    return scene


def bvh_refit(scene):
    """``ptmi_bvh_refit``: the boxes of ``scene.bvh`` recomputed in place from ``scene.triangulation`` (moved vertices, same
    topology), on the host; what ``Backend.update_triangles`` does to the tree a context holds."""
    lib = load_library()
    tris = np.ascontiguousarray(scene.triangulation)
    bvh = np.ascontiguousarray(scene.bvh)
    if tris.dtype != S.Triangle or bvh.dtype != S.Node:
        raise PtmiError(-1, "triangulation / bvh must have the structs.Triangle / structs.Node dtype")
    if not bvh.flags.writeable:
        bvh = np.frombuffer(bytearray(bvh.tobytes()), dtype=S.Node)
    rc = lib.ptmi_bvh_refit(_ptr(tris), len(tris), _ptr(bvh), len(bvh))
    if rc:
        raise PtmiError(rc, lib.ptmi_last_error(None).decode())
    scene.triangulation, scene.bvh = tris, bvh
    return scene


def mesh_topology(mesh):
    """(ptmi_mesh_topology pointing into contiguous copies of ``mesh``'s arrays, those arrays - keep them alive while it is
    used).  ``mesh``: a ``scenes.Mesh``, or anything with its fields; uvp, uvn, mat_neg and ids may be None (ptmi.h's defaults)."""
    def arr(x, dtype, shape):
        return None if x is None else np.ascontiguousarray(x, dtype).reshape(shape)
    n = len(mesh.indices)
    keep = dict(indices=arr(mesh.indices, np.uint32, (n, 3)), uvp=arr(getattr(mesh, "uvp", None), np.float32, (n, 3, 2)),
                uvn=arr(getattr(mesh, "uvn", None), np.float32, (n, 3, 2)), mat_pos=arr(mesh.mat_pos, np.uint32, (n,)),
                mat_neg=arr(getattr(mesh, "mat_neg", None), np.uint32, (n,)), ids=arr(getattr(mesh, "ids", None), np.uint32, (n,)))
    t = MeshTopology(C.sizeof(MeshTopology), n, len(mesh.positions), 0)
    for name, a in keep.items():
        setattr(t, name, None if a is None else a.ctypes.data)
    return t, keep


def _host_vertex_buffers(positions, normals):
    """(ptmi_vertex_buffers over float32 (V, 3+) arrays whose rows are ``strides[0]`` bytes apart, the arrays to keep alive)"""
    def rows(a):
        a = np.asarray(a)
        if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] < 3 or (len(a) and a.strides[1] != 4) or (len(a) > 1 and a.strides[0] <= 0):
            a = np.ascontiguousarray(a, np.float32).reshape(len(a), -1)
        return a, (a.strides[0] if len(a) > 1 else 4 * a.shape[1])
    p, ps = rows(positions)
    b = VertexBuffers(C.sizeof(VertexBuffers), len(p), ps, 0, p.ctypes.data, None)
    keep = [p]
    if normals is not None:
        m, ms = rows(normals)
        if len(m) != len(p):
            raise PtmiError(-1, "positions and normals differ in length")
        b.normal_stride, b.normals = ms, m.ctypes.data
        keep.append(m)
    return b, keep


MESH_NORMALS = object()  # assemble_triangles(normals=...): the mesh's own normal buffer (None there means a flat mesh)


def assemble_triangles(mesh, positions=None, normals=MESH_NORMALS):
    """``ptmi_assemble_triangles``: the 336-byte records ``update_vertices`` would give the context, on the host (no GPU needed).
    ``positions`` / ``normals``: (V, 3) float32 arrays (rows may be strided views), default ``mesh``'s own; normals None: flat."""
    lib = load_library()
    t, keep = mesh_topology(mesh)
    b, keep2 = _host_vertex_buffers(mesh.positions if positions is None else positions,
                                    getattr(mesh, "normals", None) if normals is MESH_NORMALS else normals)
    out = np.frombuffer(bytearray(max(t.n_triangles, 1) * S.Triangle.itemsize), dtype=S.Triangle)[:t.n_triangles]
    rc = lib.ptmi_assemble_triangles(C.byref(t), C.byref(b), out.ctypes.data_as(C.c_void_p))
    del keep, keep2
    if rc:
        raise PtmiError(rc, lib.ptmi_last_error(None).decode())
    return out


def scene_desc(scene):
    """(ptmi_scene struct pointing into contiguous copies of the scene's arrays, those arrays - keep them alive while it is used)"""
    arrays = dict(bvh=np.ascontiguousarray(scene.bvh), tri=np.ascontiguousarray(scene.triangulation),
                  lights=np.ascontiguousarray(scene.lights), mats=np.ascontiguousarray(scene.materiaux),
                  tex=np.ascontiguousarray(scene.textures), texels=np.ascontiguousarray(scene.texturesData),
                  sky=np.ascontiguousarray(scene.sky))
    assert arrays["bvh"].dtype == S.Node and arrays["tri"].dtype == S.Triangle
    d = SceneDesc()
    d.struct_size = C.sizeof(SceneDesc)
    d.bvh, d.bvh_size = _ptr(arrays["bvh"]), len(arrays["bvh"])
    d.triangulation, d.triangulation_size = _ptr(arrays["tri"]), len(arrays["tri"])
    d.lights, d.lights_size = _ptr(arrays["lights"]), len(arrays["lights"])
    d.materiaux, d.materiaux_size = _ptr(arrays["mats"]), len(arrays["mats"])
    d.textures, d.textures_size = _ptr(arrays["tex"]), len(arrays["tex"])
    d.textures_data, d.textures_data_size = _ptr(arrays["texels"]), len(arrays["texels"])
    d.sky = arrays["sky"].ctypes.data_as(C.c_void_p)
    d.camera_position, d.camera_direction = _f4(scene.cameraPosition), _f4(scene.cameraDirection)
    d.camera_right, d.camera_up = _f4(scene.cameraRight), _f4(scene.cameraUp)
    return d, arrays


def validate_scene(scene, image_width, image_height, ray_max_depth, sampler=S.JITTERED, super_sampling=False, flags=0):
    """ptmi_validate_scene: would initialize_memory accept this scene on such a context?  Host-only (no GPU needed).  Raises
    PtmiError with the library's message if not."""
    lib = load_library()
    cfg = Config(C.sizeof(Config), 0, image_width, image_height, ray_max_depth, scene.lightsSize, sampler, 1 if super_sampling else 0, flags)
    d, keep = scene_desc(scene)
    rc = lib.ptmi_validate_scene(C.byref(cfg), C.byref(d))
    del keep
    if rc:
        raise PtmiError(rc, lib.ptmi_last_error(None).decode())


class Backend:
    """One render context = the file-scope OpenCL objects of PathTracer_OpenCL.cpp:19-47."""

    def __init__(self):
        self._lib = load_library()
        self._ctx = C.c_void_p(None)
        self.cfg = None
        self._scene_keepalive = None

    # -- error convention ---------------------------------------------------------------
    def _check(self, rc):
        if rc:
            raise PtmiError(rc, self._lib.ptmi_last_error(self._ctx).decode())

    # -- OpenCL_SetupContext(globalVars, sampler), OpenCL.cpp:316-402 ---------------------
    def setup_context(self, image_width, image_height, ray_max_depth, lights_size, sampler=S.JITTERED,
                      super_sampling=False, device=0, flags=0, devices=None):
        """``devices``: list of HIP ordinals that share every render (spp shards inside the library, summed on the
        first one); None = the single ``device``, like the reference's devices[0] (OpenCL.cpp:363-366)."""
        if self._ctx:
            self.release()
        cfg = Config(C.sizeof(Config), device, image_width, image_height, ray_max_depth, lights_size, sampler,
                     1 if super_sampling else 0, flags)
        if devices:
            cfg.device = devices[0]
            cfg.n_devices = len(devices)
            for i, o in enumerate(devices):
                cfg.devices[i] = o
        ctx = C.c_void_p(None)
        rc = self._lib.ptmi_setup_context(C.byref(ctx), C.byref(cfg))
        if rc:
            raise PtmiError(rc, self._lib.ptmi_last_error(None).decode())
        self._ctx, self.cfg = ctx, cfg
        return self

    # -- OpenCL_InitializeMemory(globalVars), OpenCL.cpp:149-198 --------------------------
    def initialize_memory(self, scene):
        d, keep = scene_desc(scene)
        self._check(self._lib.ptmi_initialize_memory(self._ctx, C.byref(d)))
        del keep
        return self

    # -- the loaded scene, updated in place (no counterpart in the reference) --------------
    def set_camera(self, position, direction, right, up):
        """A new camera for the scene the context holds.  What has been rendered stays: call clear() for a fresh image."""
        v = [_f4(x) for x in (position, direction, right, up)]
        self._check(self._lib.ptmi_set_camera(self._ctx, *[C.byref(x) for x in v]))

    def update_triangles(self, triangulation):
        """New records for the triangles the context holds (same count, same order); the tree is refit on the device.  Returns
        the UpdateInfo as a dict.  What has been rendered stays: call clear() for a fresh image."""
        tris = np.ascontiguousarray(triangulation)
        if tris.dtype != S.Triangle:
            raise PtmiError(-1, "triangulation must have the 336-byte structs.Triangle dtype")
        info = UpdateInfo()
        self._check(self._lib.ptmi_update_triangles(self._ctx, tris.ctypes.data_as(C.c_void_p), len(tris), C.byref(info)))
        return info.as_dict()

    def update_triangles_device(self, d_triangulation, n_triangles):
        """The same from ``n_triangles`` 336-byte ``structs.Triangle`` records at device address ``d_triangulation`` on the
        context's first device (e.g. ``tensor.data_ptr()`` of a float32 (n, 84) tensor, 16-byte aligned): the records are checked
        and read where they are, none crosses the bus.  Synchronous; the buffer is not written.  Returns the UpdateInfo as a dict."""
        info = UpdateInfo()
        self._check(self._lib.ptmi_update_triangles_device(self._ctx, C.c_void_p(d_triangulation), n_triangles, C.byref(info)))
        return info.as_dict()

    def bind_mesh(self, mesh):
        """``ptmi_bind_mesh``: the topology of ``mesh`` (a ``scenes.Mesh``: face i is triangle i of the uploaded array) copied to
        the context's first device, for ``update_vertices``.  None unbinds.  Touches nothing of the scene."""
        if mesh is None:
            self._check(self._lib.ptmi_bind_mesh(self._ctx, None))
            return
        t, keep = mesh_topology(mesh)
        self._check(self._lib.ptmi_bind_mesh(self._ctx, C.byref(t)))
        del keep

    def update_vertices(self, positions, normals=None):
        """New positions (and vertex normals; None: a flat mesh) for the bound mesh, from host arrays of shape (V, 3) float32
        (rows may be strided views): the records are derived and checked on the device, the tree is refit.  Returns the
        UpdateInfo as a dict.  What has been rendered stays: call clear() for a fresh image."""
        b, keep = _host_vertex_buffers(positions, normals)
        info = UpdateInfo()
        self._check(self._lib.ptmi_update_vertices(self._ctx, C.byref(b), C.byref(info)))
        del keep
        return info.as_dict()

    def update_vertices_device(self, n_vertices, d_positions, d_normals=None, position_stride=12, normal_stride=12):
        """The same from device addresses on the context's first device, 16-byte aligned (``tensor.data_ptr()`` of a contiguous
        float32 (V, 3) tensor: stride 12): nothing crosses the bus.  Synchronous; the buffers are not written."""
        b = VertexBuffers(C.sizeof(VertexBuffers), n_vertices, position_stride, normal_stride, d_positions, d_normals)
        info = UpdateInfo()
        self._check(self._lib.ptmi_update_vertices_device(self._ctx, C.byref(b), C.byref(info)))
        return info.as_dict()

    def update_materials(self, first, materiaux):
        """``materiaux`` (a ``structs.Material`` array) replace the materials from index ``first`` on; their number stays.  The
        checks are initialize_memory's; a material that turns textured has its triangles' texture coordinates checked on the
        device.  Returns the MaterialUpdateInfo as a dict.  What has been rendered stays: call clear() for a fresh image."""
        mats = np.ascontiguousarray(materiaux).reshape(-1)
        if mats.dtype != S.Material:
            raise PtmiError(-1, "materiaux must have the 48-byte structs.Material dtype")
        info = MaterialUpdateInfo()
        self._check(self._lib.ptmi_update_materials(self._ctx, first, mats.ctypes.data_as(C.c_void_p), len(mats), C.byref(info)))
        return info.as_dict()

    def update_lights(self, lights):
        """The whole light array anew (a ``structs.Light`` array of the ``lights_size`` the context was set up with).  What has
        been rendered stays: call clear() for a fresh image."""
        lights = np.ascontiguousarray(lights).reshape(-1)
        if lights.dtype != S.Light:
            raise PtmiError(-1, "lights must have the 64-byte structs.Light dtype")
        self._check(self._lib.ptmi_update_lights(self._ctx, lights.ctypes.data_as(C.c_void_p), len(lights)))

    def set_sky(self, sky):
        """A new sky record (``structs.Sky``): rotation, scales and the six faces, which must lie inside the uploaded texels.
        What has been rendered stays: call clear() for a fresh image."""
        sky = np.ascontiguousarray(sky).reshape(-1)
        if sky.dtype != S.Sky or len(sky) != 1:
            raise PtmiError(-1, "sky must be one record of the 92-byte structs.Sky dtype")
        self._check(self._lib.ptmi_set_sky(self._ctx, sky.ctypes.data_as(C.c_void_p)))

    # -- rays of the caller's own against the loaded scene (no counterpart in the reference) --
    def query_rays(self, origins, directions, max_squared_distance=None, any_hit=False, out=None):
        """``BVH_IntersectRay`` (or, ``any_hit``, ``BVH_IntersectShadowRay``) for n rays of the caller's: ``origins`` and
        ``directions`` are float32 (n,3) or (n,4) arrays (w = 0 for (n,3)), ``max_squared_distance`` a scalar or n values
        (None: unlimited).  Returns a ``structs.RAY_HIT`` array (``out``: fill this one, e.g. a page-locked array);
        ``triangle_id`` indexes the triangulation the context was given, ``structs.RAY_MISS`` = no hit.  Touches nothing that
        has been rendered."""
        rays = make_rays(origins, directions, max_squared_distance)
        hits = np.zeros(len(rays), S.RAY_HIT) if out is None else out
        if hits.dtype != S.RAY_HIT or len(hits) != len(rays) or not hits.flags.c_contiguous:
            raise PtmiError(-1, "out must be a contiguous structs.RAY_HIT array with one record per ray")
        self._check(self._lib.ptmi_query_rays(self._ctx, QUERY_ANY if any_hit else QUERY_CLOSEST, rays.ctypes.data_as(C.c_void_p),
                                              len(rays), hits.ctypes.data_as(C.c_void_p)))
        return hits

    def query_rays_device(self, d_rays, n, d_hits, any_hit=False):
        """The same for ``n`` 48-byte ``structs.RAY`` records at device address ``d_rays`` (e.g. ``tensor.data_ptr()``), hits to
        ``d_hits``: asynchronous on the context's stream."""
        self._check(self._lib.ptmi_query_rays_device(self._ctx, QUERY_ANY if any_hit else QUERY_CLOSEST, C.c_void_p(d_rays), n,
                                                     C.c_void_p(d_hits)))

    # -- full paths along rays of the caller's own (no counterpart in the reference) ----------
    def path_params(self, n_rays, first_iteration=0, n_iterations=1, first_index=0, index_stride=None):
        """A ``PathParams``; ``index_stride`` None = ``n_rays``: consecutive iterations then draw from consecutive blocks of indices."""
        return PathParams(C.sizeof(PathParams), first_iteration, n_iterations, first_index, n_rays if index_stride is None else index_stride)

    def trace_paths(self, origins, directions, first_iteration=0, n_iterations=1, first_index=0, index_stride=None, out=None):
        """The radiance that arrives along n rays of the caller's: each is traced as a full path of the integrator (every light,
        every bounce up to ``ray_max_depth``) for iterations [first_iteration, first_iteration + n_iterations), the random
        numbers of ray i in iteration it being those of index ``first_index + i + it * index_stride`` (None: n).  ``origins`` and
        ``directions`` as for ``query_rays``.  Returns a ``structs.PATH_SUM`` array (``out``: fill this one, e.g. a page-locked
        array): ``radiance`` is the SUM over the iterations - divide by ``n_iterations`` for the mean - next to the counts of
        those paths.  One lane traces one ray for all its iterations: with few rays, repeat them with different ``first_index``
        instead of raising ``n_iterations`` (at most ``MAX_PATH_ITERATIONS`` per call).  Touches nothing that has been rendered."""
        rays = make_rays(origins, directions)
        sums = np.zeros(len(rays), S.PATH_SUM) if out is None else out
        if sums.dtype != S.PATH_SUM or len(sums) != len(rays) or not sums.flags.c_contiguous:
            raise PtmiError(-1, "out must be a contiguous structs.PATH_SUM array with one record per ray")
        p = self.path_params(len(rays), first_iteration, n_iterations, first_index, index_stride)
        self._check(self._lib.ptmi_trace_paths(self._ctx, C.byref(p), rays.ctypes.data_as(C.c_void_p), len(rays),
                                               sums.ctypes.data_as(C.c_void_p)))
        return sums

    def trace_paths_device(self, d_rays, n, d_sums, first_iteration=0, n_iterations=1, first_index=0, index_stride=None):
        """The same for ``n`` 48-byte ``structs.RAY`` records at device address ``d_rays`` (e.g. ``tensor.data_ptr()``), 48-byte
        ``structs.PATH_SUM`` records to ``d_sums``: asynchronous on the context's stream."""
        p = self.path_params(n, first_iteration, n_iterations, first_index, index_stride)
        self._check(self._lib.ptmi_trace_paths_device(self._ctx, C.byref(p), C.c_void_p(d_rays), n, C.c_void_p(d_sums)))

    # -- what the camera sees, per pixel (no counterpart in the reference) ------------------
    def guide_plane(self, name):
        """An empty array of the shape and type ``render_guides`` fills for plane ``name``."""
        h, w = self.cfg.image_height, self.cfg.image_width
        if name not in GUIDE_PLANES:
            raise PtmiError(-1, f"unknown guide plane {name!r}: one of {GUIDE_PLANES}")
        return np.empty((h, w) if name == "hit_count" else (h, w, 4), np.uint32 if name == "ids" else np.float32)

    def render_guides(self, first_iteration, n_iterations, planes=GUIDE_PLANES, out=None):
        """The first hit of the primary rays ``render`` traces for iterations [first_iteration, first_iteration + n_iterations),
        summed per pixel: ``albedo``, ``normal``, ``position`` float32[H,W,4], ``hit_count`` float32[H,W] (a miss adds the sky's
        colour to ``albedo`` and nothing else), and ``ids`` uint32[H,W,4] = (triangle, material, front, 0) of iteration
        ``first_iteration`` (triangle ``structs.RAY_MISS`` = no hit).  Returns a dict of the ``planes`` asked for; ``out`` = a dict
        of arrays to fill instead (e.g. page-locked ones).  Touches nothing that has been rendered."""
        arrays = {}
        for name in planes:
            a = self.guide_plane(name) if out is None or name not in out else out[name]
            want = self.guide_plane(name)
            if a.dtype != want.dtype or a.shape != want.shape or not a.flags.c_contiguous:
                raise PtmiError(-1, f"out[{name!r}] must be a contiguous {want.dtype} array of shape {want.shape}")
            arrays[name] = a
        g = Guides(C.sizeof(Guides), 0)
        for name, a in arrays.items():
            setattr(g, name, a.ctypes.data)
        self._check(self._lib.ptmi_render_guides(self._ctx, first_iteration, n_iterations, C.byref(g)))
        return arrays

    def render_guides_device(self, first_iteration, n_iterations, **device_planes):
        """The same to device addresses (e.g. ``albedo=tensor.data_ptr()``), 16-byte aligned, one keyword per plane wanted:
        asynchronous on the context's stream."""
        g = Guides(C.sizeof(Guides), 0)
        for name, address in device_planes.items():
            if name not in GUIDE_PLANES:
                raise PtmiError(-1, f"unknown guide plane {name!r}: one of {GUIDE_PLANES}")
            setattr(g, name, address)
        self._check(self._lib.ptmi_render_guides_device(self._ctx, first_iteration, n_iterations, C.byref(g)))

    # -- the filter between the accumulators and the display (no counterpart in the reference) --
    @staticmethod
    def denoise_params(passes=None, sigma_color=None, sigma_normal=None, sigma_position=None, demodulate=True, guide_first_iteration=0,
                       guide_iterations=1, untiled=False):
        """A ``DenoiseParams``; what is None takes its value from ``DENOISE_DEFAULTS``."""
        given = dict(passes=passes, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_position=sigma_position)
        v = {k: DENOISE_DEFAULTS[k] if x is None else x for k, x in given.items()}
        flags = (DENOISE_DEMODULATE_ALBEDO if demodulate else 0) | (DENOISE_UNTILED if untiled else 0)
        return DenoiseParams(C.sizeof(DenoiseParams), v["passes"], flags, guide_first_iteration, guide_iterations, v["sigma_color"],
                             v["sigma_normal"], v["sigma_position"])

    def denoise(self, out=None, **params):
        """The mean image, filtered on the device by ``passes`` a-trous passes guided by the first-hit planes of iterations
        [guide_first_iteration, guide_first_iteration + guide_iterations): float32[H,W,4] = (r, g, b, sample count).  Keywords as
        for ``denoise_params`` (``sigma_position`` is in scene units); ``out`` = an array to fill (e.g. a page-locked one).  Touches
        nothing that has been rendered."""
        h, w = self.cfg.image_height, self.cfg.image_width
        image = np.empty((h, w, 4), np.float32) if out is None else out
        if image.dtype != np.float32 or image.shape != (h, w, 4) or not image.flags.c_contiguous:
            raise PtmiError(-1, f"out must be a contiguous float32 array of shape {(h, w, 4)}")
        p = self.denoise_params(**params)
        self._check(self._lib.ptmi_denoise(self._ctx, C.byref(p), image.ctypes.data_as(C.c_void_p)))
        return image

    def denoise_device(self, out, guides, image_color=None, image_ray_nb=None, **params):
        """The same between device addresses (e.g. ``tensor.data_ptr()``), 16-byte aligned: ``out`` float4[W*H], ``guides`` a dict
        with the ``albedo``, ``normal``, ``position`` and ``hit_count`` planes ``render_guides_device`` filled over
        ``guide_iterations`` iterations, and the image's sum and count planes (both None: the context's own accumulators).
        Asynchronous on the context's stream; ``out`` must not alias an input."""
        g = Guides(C.sizeof(Guides), 0)
        for name, address in guides.items():
            if name not in GUIDE_PLANES:
                raise PtmiError(-1, f"unknown guide plane {name!r}: one of {GUIDE_PLANES}")
            setattr(g, name, address)
        p = self.denoise_params(**params)
        self._check(self._lib.ptmi_denoise_device(self._ctx, C.byref(p), C.byref(g), C.c_void_p(image_color), C.c_void_p(image_ray_nb),
                                                  C.c_void_p(out)))

    # -- the image carried across a camera move (no counterpart in the reference) ---------------
    @staticmethod
    def reproject_params(position_tolerance=None, normal_tolerance=None, max_history=None, guide_first_iteration=0, guide_iterations=1):
        """A ``ReprojectParams``; what is None takes its value from ``REPROJECT_DEFAULTS``."""
        given = dict(position_tolerance=position_tolerance, normal_tolerance=normal_tolerance, max_history=max_history)
        v = {k: REPROJECT_DEFAULTS[k] if x is None else x for k, x in given.items()}
        return ReprojectParams(C.sizeof(ReprojectParams), 0, guide_first_iteration, guide_iterations, v["position_tolerance"],
                               v["normal_tolerance"], v["max_history"], 0)

    def set_camera_reprojected(self, position, direction, right, up, **params):
        """``set_camera`` that takes the image along: every pixel whose surface the previous camera saw too keeps its mean and
        (up to ``max_history``) its sample count, every other pixel restarts as after ``clear()``.  Keywords as for
        ``reproject_params``: the guides of both cameras are rendered for [guide_first_iteration, + guide_iterations)."""
        v = [_f4(x) for x in (position, direction, right, up)]
        p = self.reproject_params(**params)
        self._check(self._lib.ptmi_set_camera_reprojected(self._ctx, *[C.byref(x) for x in v], C.byref(p)))

    def reproject_device(self, out_color, out_ray_nb, previous_camera, previous_guides, previous_color, previous_ray_nb, current_guides,
                         **params):
        """The reprojection alone, between device addresses (e.g. ``tensor.data_ptr()``), 16-byte aligned: ``previous_camera`` =
        (position, direction, right, up) the previous planes were made with; both guides are dicts with the ``normal``,
        ``position`` and ``hit_count`` planes of ``render_guides_device``; the previous image's sums float4[W*H] and counts
        float[W*H]; the result's likewise.  Asynchronous on the context's stream; the result must not alias an input."""
        cam = (Float4 * 4)(*[_f4(x) for x in previous_camera])
        structs = []
        for guides in (previous_guides, current_guides):
            g = Guides(C.sizeof(Guides), 0)
            for name, address in guides.items():
                if name not in GUIDE_PLANES:
                    raise PtmiError(-1, f"unknown guide plane {name!r}: one of {GUIDE_PLANES}")
                setattr(g, name, address)
            structs.append(g)
        p = self.reproject_params(**params)
        self._check(self._lib.ptmi_reproject_device(self._ctx, C.byref(p), C.byref(cam), C.byref(structs[0]), C.c_void_p(previous_color),
                                                    C.c_void_p(previous_ray_nb), C.byref(structs[1]), C.c_void_p(out_color),
                                                    C.c_void_p(out_ray_nb)))

    # -- one launch of the loop body of OpenCL_RunKernel, generalised to a range ----------
    def render(self, first_iteration, n_iterations):
        self._check(self._lib.ptmi_render(self._ctx, first_iteration, n_iterations))

    @staticmethod
    def region(x, y, width, height):
        """ptmi_region as a one-element ``structs.REGION`` array: pixels [x, x + width) x [y, y + height), row 0 first."""
        r = np.zeros(1, S.REGION)
        r["x"], r["y"], r["width"], r["height"] = x, y, width, height
        return r

    def render_region(self, x, y, width, height, first_iteration, n_iterations):
        """render() for the work-items of one rectangle (ptmi_render_region): the very paths render() traces there, nothing
        outside read or written with the JITTERED / UNIFORM samplers."""
        r = self.region(x, y, width, height)
        self._check(self._lib.ptmi_render_region(self._ctx, _ptr(r), first_iteration, n_iterations))

    def read_region(self, x, y, width, height, out=None):
        """(color float32[height,width,4], count float32[height,width]): the rectangle of what read_image() would return now
        (ptmi_read_region); ``out`` = (color, count) arrays to fill, DMA'd into directly if page-locked with pin_host_buffer."""
        r = self.region(x, y, width, height)
        color, count = out if out is not None else (np.empty((height, width, 4), np.float32), np.empty((height, width), np.float32))
        self._check(self._lib.ptmi_read_region(self._ctx, _ptr(r), None if color is None else _ptr(color), None if count is None else _ptr(count)))
        return color, count

    def synchronize(self):
        self._check(self._lib.ptmi_synchronize(self._ctx))

    def clear(self):
        self._check(self._lib.ptmi_clear(self._ctx))

    def read_image(self, out=None):
        """(imageColor float32[H,W,4], imageRayNb float32[H,W]) -- the per-image readback, OpenCL.cpp:97-98."""
        h, w = self.cfg.image_height, self.cfg.image_width
        color, count = out if out is not None else (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32))
        self._check(self._lib.ptmi_read_image(self._ctx, _ptr(color), _ptr(count)))
        return color, count

    def pin_host_buffer(self, array):
        """Page-lock a numpy array that read_image / read_snapshot will fill repeatedly (keep it alive until unpin / release)."""
        self._check(self._lib.ptmi_pin_host_buffer(self._ctx, _ptr(array), array.nbytes))

    def unpin_host_buffer(self, array):
        self._check(self._lib.ptmi_unpin_host_buffer(self._ctx, _ptr(array)))

    def snapshot(self, slot=0):
        """Queue a device-side copy of the accumulators behind the launches issued so far (ptmi_snapshot)."""
        self._check(self._lib.ptmi_snapshot(self._ctx, slot))

    def render_snapshots(self, first_iteration, n_iterations, first_slot=0):
        """render() that also leaves a snapshot after each of its iterations (slots first_slot, first_slot + 1, ...)."""
        self._check(self._lib.ptmi_render_snapshots(self._ctx, first_iteration, n_iterations, first_slot))

    def read_snapshot(self, slot=0, out=None):
        """Wait for snapshot ``slot`` only and return it; ``out`` = (color, count) arrays to fill (DMA'd into directly
        if they were page-locked with pin_host_buffer)."""
        h, w = self.cfg.image_height, self.cfg.image_width
        color, count = out if out is not None else (np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32))
        self._check(self._lib.ptmi_read_snapshot(self._ctx, slot, _ptr(color), _ptr(count)))
        return color, count

    def write_image(self, image_color=None, image_ray_nb=None):
        """Load the accumulators (resume a saved render); the inverse of read_image."""
        c = None if image_color is None else np.ascontiguousarray(image_color, np.float32)
        n = None if image_ray_nb is None else np.ascontiguousarray(image_ray_nb, np.float32)
        self._check(self._lib.ptmi_write_image(self._ctx, None if c is None else _ptr(c), None if n is None else _ptr(n)))

    def read_display(self):
        """Padded B,G,R scanlines uint8[H, (3W+3)&~3] quantised on the device as the reference's viewer does on the
        host (ConvertRGBAToBMPBuffer, Alone/PathTracer_bitmap.cpp:237-286)."""
        h, w = self.cfg.image_height, self.cfg.image_width
        stride = (3 * w + 3) & ~3
        out = np.empty((h, stride), np.uint8)
        self._check(self._lib.ptmi_read_display(self._ctx, _ptr(out), stride))
        return out

    # -- the display stage: any image plane -> 8-bit pixels on the device (no counterpart in the reference) --
    def display_params(self, tone=None, transfer=None, exposure=None, white=None, rgba=False, row_stride=None):
        """A ``DisplayParams`` for this context's image; what is None takes its value from ``DISPLAY_DEFAULTS``, ``row_stride``
        the BMP stride (3W rounded up to 4) or, with ``rgba``, 4W."""
        given = dict(tone=tone, transfer=transfer, exposure=exposure, white=white)
        v = {k: DISPLAY_DEFAULTS[k] if x is None else x for k, x in given.items()}
        w = self.cfg.image_width
        stride = (4 * w if rgba else (3 * w + 3) & ~3) if row_stride is None else row_stride
        return DisplayParams(C.sizeof(DisplayParams), 0, v["tone"], v["transfer"], PIXELS_RGBA32 if rgba else PIXELS_BGR24, stride,
                             v["exposure"], v["white"])

    def display(self, tone=None, transfer=None, exposure=None, white=None, rgba=False, out=None):
        """The image ``read_image`` would return, exposed, tone-mapped, encoded and quantised on the device: padded B,G,R
        scanlines uint8[H, (3W+3)&~3] (``save_bmp_rows`` writes them as they are) or, with ``rgba``, uint8[H, W, 4] = R, G, B, 255.
        ``out`` = an array to fill (e.g. a page-locked one).  Touches nothing that has been rendered."""
        h, w = self.cfg.image_height, self.cfg.image_width
        p = self.display_params(tone, transfer, exposure, white, rgba)
        shape = (h, w, 4) if rgba else (h, p.row_stride)
        pixels = np.empty(shape, np.uint8) if out is None else out
        if pixels.dtype != np.uint8 or pixels.shape != shape or not pixels.flags.c_contiguous:
            raise PtmiError(-1, f"out must be a contiguous uint8 array of shape {shape}")
        self._check(self._lib.ptmi_read_display_tonemapped(self._ctx, C.byref(p), _ptr(pixels)))
        return pixels

    def display_device(self, out, image_color=None, image_ray_nb=None, **params):
        """The same between device addresses (e.g. ``tensor.data_ptr()``), 16-byte aligned: ``out`` holds H * row_stride bytes;
        both planes = float4 sums and float counts, ``image_color`` alone = a mean plane (what ``denoise_device`` writes), neither =
        the context's own accumulators.  Keywords as for ``display_params``.  Asynchronous on the context's stream."""
        p = self.display_params(**params)
        self._check(self._lib.ptmi_display_device(self._ctx, C.byref(p), C.c_void_p(image_color), C.c_void_p(image_ray_nb), C.c_void_p(out)))

    def luminance_histogram(self):
        """uint32[260] of the image ``read_image`` would return: words 0..255 count the pixels of positive finite mean luminance in
        quarter-octave bins (bin 128 starts at 1.0), word 256 the pixels that are not positive, word 257 the infinite ones
        (ptmi.h).  ``exposure_from_histogram`` turns it into an exposure."""
        out = np.empty(LUMINANCE_WORDS, np.uint32)
        self._check(self._lib.ptmi_luminance_histogram(self._ctx, _ptr(out)))
        return out

    def luminance_histogram_device(self, out, image_color=None, image_ray_nb=None):
        """The same between device addresses, the planes as for ``display_device``; ``out`` holds 260 words, which the call zeroes
        on the stream before it counts.  Asynchronous on the context's stream."""
        self._check(self._lib.ptmi_luminance_histogram_device(self._ctx, C.c_void_p(image_color), C.c_void_p(image_ray_nb), C.c_void_p(out)))

    def read_statistics(self):
        """(rayDepths[D+1], rayIntersectedBBx[5000], rayIntersectedTri[5000]), OpenCL.cpp:110-112."""
        d = np.zeros(self.cfg.ray_max_depth + 1, np.uint32)
        b = np.zeros(S.MAX_INTERSETCION_NUMBER, np.uint32)
        t = np.zeros(S.MAX_INTERSETCION_NUMBER, np.uint32)
        self._check(self._lib.ptmi_read_statistics(self._ctx, _ptr(d), _ptr(b), _ptr(t)))
        return d, b, t

    def counters(self):
        c = Counters()
        self._check(self._lib.ptmi_get_counters(self._ctx, C.byref(c)))
        return c.as_dict()

    def scheduler_stats(self):
        s = SchedulerStats()
        self._check(self._lib.ptmi_get_scheduler_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    def invariant_checks(self):
        """Failures of the reference's -D LOG_INFO device-side checks, counted by FLAG_SCHEDULER_STATS builds (ptmi.h)."""
        s = InvariantChecks()
        self._check(self._lib.ptmi_get_invariant_checks(self._ctx, C.byref(s)))
        return s.as_dict()

    def literal_kernel_reason(self):
        """None, or why the uploaded scene is rendered by the one-path-per-lane kernel (records on which the reference's
        triangle test yields NaN distances: ptmi.h)."""
        r = self._lib.ptmi_literal_kernel_reason(self._ctx)
        return r.decode() if r else None

    def reduce_path(self):
        """How a multi-device context sums its partial images: dict(rccl_state, communicators, nccl_version) (ptmi_reduce_path)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.ptmi_reduce_path(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return {"rccl_state": a.value, "communicators": b.value, "nccl_version": c.value}

    def kernel_time(self):
        """(total_ms, launches) of the integrator kernel since the last call (HIP events on its stream)."""
        ms, n = C.c_double(0), C.c_uint32(0)
        self._check(self._lib.ptmi_kernel_time(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_stream(self, hip_stream):
        self._check(self._lib.ptmi_set_stream(self._ctx, C.c_void_p(hip_stream)))

    def device_accumulators(self):
        a, b = C.c_void_p(None), C.c_void_p(None)
        self._check(self._lib.ptmi_device_accumulators(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def read_variance(self):
        """imageV float32[H,W,4] (SUPER_SAMPLING only): per-channel sum of squared deviations, FullKernel.cl:1346-1349."""
        h, w = self.cfg.image_height, self.cfg.image_width
        v = np.empty((h, w, 4), np.float32)
        self._check(self._lib.ptmi_read_variance(self._ctx, _ptr(v)))
        return v

    def write_variance(self, image_v):
        v = np.ascontiguousarray(image_v, np.float32)
        self._check(self._lib.ptmi_write_variance(self._ctx, _ptr(v)))

    def device_variance(self):
        a = C.c_void_p(None)
        self._check(self._lib.ptmi_device_variance(self._ctx, C.byref(a)))
        return a.value

    def bind_accumulators(self, d_color, d_count):
        self._check(self._lib.ptmi_bind_accumulators(self._ctx, C.c_void_p(d_color), C.c_void_p(d_count)))

    # -- OpenCL_RunKernel(globalVars, UpdateWindowFunc, numImagesToRender, t1, t2, t3), OpenCL.cpp:56-140
    def run_kernel(self, update_window_func=None, num_images_to_render=1, images_per_launch=1):
        """The reference's render loop: launch, read the accumulators back, call the display callback,
        once per image; statistics after the loop; then release.  Returns
        (imageColor, imageRayNb, (rayDepths, bbx, tri), (pathTracingTime, memoryTime, displayTime)) with the
        times in seconds.  ``images_per_launch`` > 1 batches iterations per launch (callback every batch)."""
        t_path = t_mem = t_disp = 0.0
        color = count = None
        image_id = 0
        while image_id < num_images_to_render:
            n = min(images_per_launch, num_images_to_render - image_id)
            t0 = time.perf_counter()
            self.render(image_id, n)
            self.synchronize()
            t1 = time.perf_counter()
            color, count = self.read_image()
            t2 = time.perf_counter()
            if update_window_func is not None:
                update_window_func()  # return value ignored, as in OpenCL.cpp:103
            t3 = time.perf_counter()
            t_path += t1 - t0
            t_mem += t2 - t1
            t_disp += t3 - t2
            image_id += n
        stats = self.read_statistics()
        self.release()
        return color, count, stats, (t_path, t_mem, t_disp)

    def release(self):
        if self._ctx:
            self._lib.ptmi_release(self._ctx)
            self._ctx = C.c_void_p(None)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def render_scene(scene, width, height, ray_max_depth, n_iterations, first_iteration=0, sampler=S.JITTERED, device=0,
                 flags=0, super_sampling=False, devices=None):
    """Convenience used by tests/bench: full life cycle for one iteration range."""
    be = Backend().setup_context(width, height, ray_max_depth, scene.lightsSize, sampler, super_sampling=super_sampling,
                                 device=device, flags=flags, devices=devices)
    try:
        be.initialize_memory(scene)
        be.render(first_iteration, n_iterations)
        color, count = be.read_image()
        stats = be.read_statistics()
        counters = be.counters()
    finally:
        be.release()
    return color, count, stats, counters
