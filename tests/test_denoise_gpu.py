"""ptmi_denoise / ptmi_denoise_device against the yardstick of denoise_cases.py, every word of the result equal (compared as
uint32; where the yardstick's word is a NaN the kernel's must be a NaN): synthetic planes on the image sizes that take each edge
of the kernels, rendered scenes in both arithmetics, and what the feature promises around the kernels - a denoise call changes
nothing that was rendered, it is ordered on the context's stream, errors leave the context rendering as before - and that the
filter, with the shipped defaults, brings a 4-spp image closer to the converged one."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, structs as S
from gpu_cases import assert_same_state, state
import denoise_cases as D
import gpu_cases
import guide_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = G.W, G.H
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
GUIDE_NAMES = ("albedo", "normal", "position", "hit_count")
SIGMAS = dict(sigma_color=0.6, sigma_normal=0.5, sigma_position=1.5)


def assert_equal(got, want):
    msg = D.describe_difference(got, want)
    assert not msg, msg


to_device = gpu_cases.tensor_on_device


def empty_image(w, h):
    import torch
    t = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return t


def device_guides(be, first, n, w=W, h=H):
    """the four planes the filter reads, rendered into tensors by ptmi_render_guides_device (not waited for)"""
    import torch
    t = {name: torch.empty((h, w) if name == "hit_count" else (h, w, 4), dtype=torch.float32, device="cuda") for name in GUIDE_NAMES}
    torch.cuda.synchronize()
    be.render_guides_device(first, n, **{name: x.data_ptr() for name, x in t.items()})
    return t


def pointers(tensors):
    return {name: t.data_ptr() for name, t in tensors.items()}


def yardstick_of(be, first, n, **params):
    """the yardstick on the image and the guide planes the context itself returns"""
    color, count = be.read_image()
    guides = be.render_guides(first, n, planes=GUIDE_NAMES)
    flags = D.DEMODULATE if params.pop("demodulate", True) else 0
    return D.denoise(color, count, **guides, flags=flags, guide_iterations=n, **params)


# ---------------------------------------------------------------------------------------------- the kernels against the yardstick

SIZES = [(1, 1), (5, 3), (33, 9), (64, 16), (70, 37), (130, 66)]


@pytest.mark.parametrize("passes", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_planes(size, passes):
    """One pixel; less than one footprint; a ragged row of tiles; two tiles by two of the tiled form's 32 x 8 (one by four
    workgroups of the direct form's 64 x 4) with nothing ragged; more than one tile each way with ragged edges; and an image in
    which step 16 reaches across several tiles and out of the image.  With and without demodulation, steps 1 and 2 from the LDS
    tile and from memory; every pass count, so that each step's kernel is also the last one, which stores the re-modulated
    image."""
    w, h = size
    planes, g = D.synthetic(w, h, seed=w * 1000 + h)
    tensors = {name: to_device(a) for name, a in planes.items()}
    be = gpu_cases.context(G.scene("one_triangle"), w, h)
    try:
        for demodulate in (True, False):
            want = D.denoise(**planes, passes=passes, flags=D.DEMODULATE if demodulate else 0, guide_iterations=g, **D.SYNTHETIC_SIGMAS)
            for untiled in (False, True):
                out = empty_image(w, h)
                be.denoise_device(out.data_ptr(), pointers({k: tensors[k] for k in GUIDE_NAMES}), tensors["color"].data_ptr(),
                                  tensors["ray_nb"].data_ptr(), passes=passes, demodulate=demodulate, guide_iterations=g, untiled=untiled,
                                  **D.SYNTHETIC_SIGMAS)
                be.synchronize()
                assert_equal(out.cpu().numpy(), want)
    finally:
        be.release()


@pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])
@pytest.mark.parametrize("name", ["cornell", "matmix", "feat_textured"])
def test_rendered_scenes(name, flags):
    """The filter's arithmetic is the same in both modes; its inputs are not."""
    be = gpu_cases.context(G.scene(name), W, H, flags=flags)
    try:
        be.render(0, 3)
        for params in (dict(passes=5, **SIGMAS), dict(passes=2, demodulate=False, **SIGMAS)):
            want = yardstick_of(be, 1, 2, **dict(params))
            assert not np.array_equal(want, yardstick_of(be, 1, 2, **dict(params, passes=0)))  # (the filter has something to do)
            assert_equal(be.denoise(guide_first_iteration=1, guide_iterations=2, **params), want)
        assert_equal(be.denoise(), yardstick_of(be, 0, 1, **backend.DENOISE_DEFAULTS))  # every default
    finally:
        be.release()


def test_device_form_on_the_contexts_own_accumulators_equals_the_host_form():
    import torch
    be = gpu_cases.context(G.scene("cornell"), W, H)
    try:
        be.render(0, 3)
        host = be.denoise(guide_first_iteration=0, guide_iterations=3, **SIGMAS)
        assert_equal(host, yardstick_of(be, 0, 3, passes=5, **SIGMAS))
        guides, out = device_guides(be, 0, 3), empty_image(W, H)
        be.denoise_device(out.data_ptr(), pointers(guides), guide_iterations=3, **SIGMAS)
        be.synchronize()
        assert_equal(out.cpu().numpy(), host)
        # ... on a stream of the caller's, read by torch behind the call, and into a page-locked result
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        be.set_stream(stream.cuda_stream)
        again = empty_image(W, H)
        be.denoise_device(again.data_ptr(), pointers(guides), guide_iterations=3, **SIGMAS)
        with torch.cuda.stream(stream):
            copy = again.clone()
        stream.synchronize()
        assert_equal(copy.cpu().numpy(), host)
        pinned = np.full((H, W, 4), -1.0, np.float32)
        be.pin_host_buffer(pinned)
        assert be.denoise(out=pinned, guide_first_iteration=0, guide_iterations=3, **SIGMAS) is pinned
        assert_equal(pinned, host)
        be.unpin_host_buffer(pinned)
        be.set_stream(None)
    finally:
        be.release()


def test_two_listed_devices():
    """The host form filters the summed image; the device form has no accumulators to default to, and takes planes as ever."""
    be = gpu_cases.context(G.scene("cornell"), W, H, devices=[0, 0])
    try:
        be.render(0, 4)
        baseline = state(be)
        want = yardstick_of(be, 0, 2, passes=5, **SIGMAS)
        assert_equal(be.denoise(guide_first_iteration=0, guide_iterations=2, **SIGMAS), want)
        guides, out = device_guides(be, 0, 2), empty_image(W, H)
        with pytest.raises(PtmiError) as e:
            be.denoise_device(out.data_ptr(), pointers(guides), guide_iterations=2, **SIGMAS)
        assert e.value.code == UNSUPPORTED
        be.synchronize()
        assert bool((out == -1).all())
        color, count = (to_device(a) for a in be.read_image())  # (kept alive until the call has run)
        be.denoise_device(out.data_ptr(), pointers(guides), color.data_ptr(), count.data_ptr(), guide_iterations=2, **SIGMAS)
        be.synchronize()
        assert_equal(out.cpu().numpy(), want)
        assert_equal(be.denoise(guide_first_iteration=0, guide_iterations=2, **SIGMAS), want)  # (the host form behind a device-form call)
        assert_same_state(state(be), baseline)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- denoising and renders

def test_denoising_is_invisible_to_renders():
    sc = G.scene("cornell")

    def play(with_denoise):
        be = gpu_cases.context(sc, W, H)
        try:
            be.render(0, 2)
            be.snapshot(5)
            guides, out = device_guides(be, 0, 2), empty_image(W, H)
            if with_denoise:
                be.denoise(guide_iterations=2, **SIGMAS)
            be.render(2, 2)
            for k in range(4, 12):  # one-iteration calls of a caller that waits: rendered ahead of
                be.render(k, 1)
                be.synchronize()
                if with_denoise:
                    be.denoise_device(out.data_ptr(), pointers(guides), guide_iterations=2, **SIGMAS)
                    if k % 3 == 0:
                        be.denoise(passes=1, demodulate=False)
            kept = be.read_snapshot(5)
            return state(be), [a.view(np.uint32).copy() for a in kept]
        finally:
            be.release()

    (a, kept_a), (b, kept_b) = play(True), play(False)
    assert_same_state(a, b)
    assert all(np.array_equal(x, y) for x, y in zip(kept_a, kept_b)) and kept_a[1].view(np.float32).max() == 2


def test_denoising_leaves_the_scheduler_statistics():
    be = gpu_cases.context(G.scene("cornell"), W, H, flags=backend.FLAG_SCHEDULER_STATS)
    try:
        be.render(0, 2)
        before, checks, counters = be.scheduler_stats(), be.invariant_checks(), be.counters()
        assert before["trips_node"] > 0
        be.denoise(guide_iterations=2)
        guides, out = device_guides(be, 0, 2), empty_image(W, H)
        be.denoise_device(out.data_ptr(), pointers(guides), guide_iterations=2)
        be.synchronize()
        assert be.scheduler_stats() == before and be.invariant_checks() == checks and be.counters() == counters
    finally:
        be.release()


def test_a_call_in_flight_is_ordered_before_set_camera():
    """Guides and filter of the old camera, not waited for; ptmi_set_camera; guides and filter of the new one."""
    moved = G.scene("feat_two_sided_from_behind")
    be = gpu_cases.context(G.scene("feat_two_sided"), W, H)
    try:
        be.render(0, 3)
        want_old = yardstick_of(be, 5, 2, passes=5, **SIGMAS)
        out_old, out_new = empty_image(W, H), empty_image(W, H)
        guides_old = device_guides(be, 5, 2)
        be.denoise_device(out_old.data_ptr(), pointers(guides_old), guide_iterations=2, **SIGMAS)  # not waited for: set_camera must
        be.set_camera(moved.cameraPosition, moved.cameraDirection, moved.cameraRight, moved.cameraUp)
        guides_new = device_guides(be, 5, 2)
        be.denoise_device(out_new.data_ptr(), pointers(guides_new), guide_iterations=2, **SIGMAS)
        be.synchronize()
        want_new = yardstick_of(be, 5, 2, passes=5, **SIGMAS)
        assert not np.array_equal(want_old, want_new)
        assert_equal(out_old.cpu().numpy(), want_old)
        assert_equal(out_new.cpu().numpy(), want_new)
        assert_equal(be.denoise(guide_first_iteration=5, guide_iterations=2, **SIGMAS), want_new)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- errors

def test_refusals_leave_the_context_rendering():
    sc = G.scene("cornell")
    lib = backend.load_library()
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        with pytest.raises(PtmiError) as e:
            be.denoise()
        assert e.value.code == STATE and "before ptmi_initialize_memory" in str(e.value)
        with pytest.raises(PtmiError) as e:
            be.denoise_device(256, dict(albedo=256, normal=256, position=256, hit_count=256))
        assert e.value.code == STATE
        be.initialize_memory(sc)
        be.render(0, 3)
        baseline = state(be)
        guides, out = device_guides(be, 0, 1), empty_image(W, H)
        be.synchronize()
        host_out = np.full((H, W, 4), -1.0, np.float32)
        color, count = (to_device(a) for a in be.read_image())

        def params(**changes):
            p = backend.Backend.denoise_params()
            for k, v in changes.items():
                setattr(p, k, v)
            return p

        def reserved(i):
            p = params()
            p.reserved[i] = 1
            return p

        bad_params = [None, params(struct_size=36), params(struct_size=44), params(passes=6), params(flags=4), params(flags=0x80000001),
                      reserved(0), reserved(1), params(guide_iterations=0), params(guide_iterations=1 << 24)]
        for name in ("sigma_color", "sigma_normal", "sigma_position"):
            bad_params += [params(**{name: v}) for v in (0.0, -1.0, float("inf"), float("nan"))]
        good_guides = backend.Guides(C.sizeof(backend.Guides), 0, **pointers(guides))
        vp = C.c_void_p
        attempts = []
        for p in bad_params:
            ref = None if p is None else C.byref(p)
            attempts.append(lambda ref=ref: lib.ptmi_denoise(be._ctx, ref, host_out.ctypes.data_as(vp)))
            attempts.append(lambda ref=ref: lib.ptmi_denoise_device(be._ctx, ref, C.byref(good_guides), None, None, vp(out.data_ptr())))
        good = params()
        device_call = lambda g, c, n, o: lib.ptmi_denoise_device(be._ctx, C.byref(good), None if g is None else C.byref(g), vp(c), vp(n), vp(o))  # noqa: E731
        attempts.append(lambda: lib.ptmi_denoise(be._ctx, C.byref(good), None))
        attempts.append(lambda: device_call(None, None, None, out.data_ptr()))
        attempts.append(lambda: device_call(backend.Guides(C.sizeof(backend.Guides) + 8, 0, **pointers(guides)), None, None, out.data_ptr()))
        for name in GUIDE_NAMES:  # a missing plane, a misaligned one
            attempts.append(lambda name=name: device_call(backend.Guides(C.sizeof(backend.Guides), 0, **dict(pointers(guides), **{name: None})),
                                                          None, None, out.data_ptr()))
            attempts.append(lambda name=name: device_call(backend.Guides(C.sizeof(backend.Guides), 0, **dict(pointers(guides), **{name: guides[name].data_ptr() + 4})),
                                                          None, None, out.data_ptr()))
        attempts.append(lambda: device_call(good_guides, None, None, None))
        attempts.append(lambda: device_call(good_guides, None, None, out.data_ptr() + 8))
        attempts.append(lambda: device_call(good_guides, color.data_ptr(), None, out.data_ptr()))  # one image plane without the other
        attempts.append(lambda: device_call(good_guides, None, count.data_ptr(), out.data_ptr()))
        attempts.append(lambda: device_call(good_guides, color.data_ptr() + 4, count.data_ptr(), out.data_ptr()))
        attempts.append(lambda: device_call(good_guides, color.data_ptr(), count.data_ptr() + 4, out.data_ptr()))
        for attempt in attempts:
            assert attempt() == INVALID_ARGUMENT and len(lib.ptmi_last_error(be._ctx)) > 0
        be.synchronize()
        assert bool((out == -1).all()) and (host_out == -1).all()  # nothing was launched
        be.clear()
        be.render(0, 3)
        assert_same_state(state(be), baseline)
        # ids is ignored, and a good call still works
        with_ids = backend.Guides(C.sizeof(backend.Guides), 0, **dict(pointers(guides), ids=12))
        assert lib.ptmi_denoise_device(be._ctx, C.byref(params(sigma_color=0.6, sigma_normal=0.5, sigma_position=1.5)), C.byref(with_ids), None,
                                       None, vp(out.data_ptr())) == 0
        be.synchronize()
        assert_equal(out.cpu().numpy(), yardstick_of(be, 0, 1, passes=5, **SIGMAS))
        assert_same_state(state(be), baseline)
    finally:
        be.release()


def test_the_random_sampler_has_no_guides_for_the_host_form():
    be = gpu_cases.context(G.scene("cornell"), W, H, sampler=S.RANDOM)
    try:
        be.render(0, 2)
        baseline = state(be)
        with pytest.raises(PtmiError) as e:
            be.denoise()
        assert e.value.code == UNSUPPORTED and "RANDOM" in str(e.value)
        assert_same_state(state(be), baseline)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- it helps

SPP, TRUTH_SPP = 4, 1024
_quality = {}


def quality():
    """Cornell at 64 x 48: the raw 4-spp mean, the truth (1024 further iterations of the integrator), and the filtered image at
    every point of the committed grid of sigmas, passes = 5 and demodulation on.  Computed once, printed, and written to
    profiles/denoise_quality_cornell.json."""
    if _quality:
        return _quality
    be = gpu_cases.context(G.scene("cornell"), W, H)
    try:
        be.render(SPP, TRUTH_SPP)
        color, count = be.read_image()
        truth = color[..., :3] / count[..., None]
        be.clear()
        be.render(0, SPP)
        color, count = be.read_image()
        raw = color[..., :3] / count[..., None]
        grid = []
        for sc in D.GRID_SIGMA_COLOR:
            for sn in D.GRID_SIGMA_NORMAL:
                for sp in D.GRID_SIGMA_POSITION:
                    image = be.denoise(passes=5, sigma_color=sc, sigma_normal=sn, sigma_position=sp, guide_iterations=SPP)
                    grid.append(dict(sigma_color=sc, sigma_normal=sn, sigma_position=sp, rmse=D.rmse(image, truth)))
        shipped = D.rmse(be.denoise(guide_iterations=SPP), truth)
    finally:
        be.release()
    _quality.update(scene="cornell", width=W, height=H, spp=SPP, truth_spp=TRUTH_SPP, rmse_raw=D.rmse(raw, truth), rmse_denoised=shipped,
                    ratio=shipped / D.rmse(raw, truth), defaults=backend.DENOISE_DEFAULTS, grid=grid)
    print(json.dumps({k: v for k, v in _quality.items() if k != "grid"}))
    print("grid minimum:", min(grid, key=lambda r: r["rmse"]))
    with open(os.path.join(ROOT, "profiles", "denoise_quality_cornell.json"), "w") as f:
        json.dump(_quality, f, indent=1)
        f.write("\n")
    return _quality


def test_it_helps():
    """The denoised image is closer to the truth than the raw one.  Measured on the MI355X
    (profiles/denoise_quality_cornell.json): RMSE 0.0852 raw, 0.0326 denoised, ratio 0.383."""
    q = quality()
    assert q["rmse_denoised"] < q["rmse_raw"], q


def test_defaults_are_the_grids_minimum():
    q = quality()
    best = min(q["grid"], key=lambda r: r["rmse"])
    assert best["rmse"] < q["rmse_raw"], (best, q["rmse_raw"])
    assert q["rmse_denoised"] == best["rmse"], (backend.DENOISE_DEFAULTS, best)
