"""ptmi_read_display_tonemapped / ptmi_display_device and ptmi_luminance_histogram / ptmi_luminance_histogram_device against the
yardstick of display_cases.py, every byte and every count equal: synthetic planes that hit every threshold of every transfer
table from both sides on the image sizes that take each edge of the kernels, rendered scenes in both arithmetics, a multi-device
context, and what the feature promises around the kernels - a display call changes nothing that was rendered, it is ordered on
the context's stream, errors leave the context rendering as before."""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend
from gpu_cases import assert_same_state, state
import display_cases as D
import gpu_cases
import guide_cases as G

pytestmark = pytest.mark.gpu
W, H = G.W, G.H
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
GUIDE_NAMES = ("albedo", "normal", "position", "hit_count")
EXPOSURES = (1.0, 0.25, 3.5)
PARAMS = [dict(tone=tone, transfer=transfer, exposure=exposure, white=white) for tone in D.TONES for transfer in D.TRANSFERS
          for exposure in EXPOSURES for white in ((2.0, np.inf) if tone == D.REINHARD else (np.inf,))]
A_FEW = [PARAMS[0], dict(backend.DISPLAY_DEFAULTS), dict(tone=D.REINHARD, transfer=D.GAMMA22, exposure=3.5, white=2.0),
         dict(tone=D.FILMIC, transfer=D.LINEAR, exposure=0.25, white=np.inf)]


def stride_of(w):
    return (3 * w + 3) & ~3


to_device = gpu_cases.tensor_on_device


def filled(n_bytes):
    """0xAA everywhere: a byte the call leaves unwritten shows"""
    import torch
    t = torch.full((n_bytes,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def garbage_words():
    import torch
    t = torch.full((D.WORDS,), -559038737, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def pointer(tensor):
    return None if tensor is None else tensor.data_ptr()


def device_bgr(be, color, count, w, h, stride=None, **params):
    stride = stride_of(w) if stride is None else stride
    out = filled(h * stride)
    be.display_device(out.data_ptr(), pointer(color), pointer(count), row_stride=stride, **params)
    be.synchronize()
    return out.cpu().numpy().reshape(h, stride)


def device_rgba(be, color, count, w, h, **params):
    out = filled(h * w * 4)
    be.display_device(out.data_ptr(), pointer(color), pointer(count), rgba=True, **params)
    be.synchronize()
    return out.cpu().numpy().reshape(h, w, 4)


def device_histogram(be, color, count):
    out = garbage_words()
    be.luminance_histogram_device(out.data_ptr(), pointer(color), pointer(count))
    be.synchronize()
    return out.cpu().numpy().view(np.uint32)


def assert_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, f"{what}: {len(wrong)} bytes differ, the first at {tuple(wrong[0])}: {got[tuple(wrong[0])]} for {want[tuple(wrong[0])]}"


# ---------------------------------------------------------------------------------------------- the kernels against the yardstick

SIZES = [(1, 1), (2, 3), (3, 3), (4, 3), (5, 3), (70, 37), (130, 66), (259, 2)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_planes(size):
    """W mod 4 takes every value, so the BMP stride pads a row by 1, 2, 3 and 0 bytes; a ragged last group of four pixels; more
    than one workgroup each way; a row longer than a workgroup.  Both formats, every tone with every transfer at three exposures
    (REINHARD with a white of 2 and of infinity), the planes read as sums with counts and as means; then every stride from 3W
    to 3W + 3, of which three take the kernel's byte stores.  The planes hold every threshold of every table with its two
    neighbours (as many as the image has room for), infinities, NaNs, negatives, denormals and counts that are no counts."""
    w, h = size
    color, count = D.synthetic(w, h, seed=w * 1000 + h)
    d_color, d_count = to_device(color), to_device(count)
    be = gpu_cases.context(G.scene("one_triangle"), w, h)
    try:
        for n, d_n in ((count, d_count), (None, None)):
            form = "sums" if n is not None else "means"
            assert np.array_equal(device_histogram(be, d_color, d_n), D.histogram(color, n)), form
            for params in PARAMS:
                rgb = D.tonemap(color, n, params)
                assert_bytes(device_bgr(be, d_color, d_n, w, h, **params), D.pack_bgr24(rgb, stride_of(w)), (form, "BGR24", params))
                assert_bytes(device_rgba(be, d_color, d_n, w, h, **params), D.pack_rgba32(rgb), (form, "RGBA32", params))
            rgb = D.tonemap(color, n, A_FEW[1])
            for stride in range(3 * w, 3 * w + 4):
                assert_bytes(device_bgr(be, d_color, d_n, w, h, stride=stride, **A_FEW[1]), D.pack_bgr24(rgb, stride), (form, stride))
    finally:
        be.release()


def test_synthetic_planes_hit_every_threshold_from_both_sides():
    """... in the two largest sizes above: with CLAMP and exposure 1 the three values around T[k] show k - 1, k, k."""
    for w, h in SIZES[5:7]:
        color, count = D.synthetic(w, h, seed=w * 1000 + h)
        triples = {tuple(v) for v in color[count == 1][:, :3].view(np.uint32).tolist()}
        values = D.threshold_values().view(np.uint32).reshape(-1, 3)
        assert all(tuple(v) in triples for v in values.tolist())
    for transfer in D.TRANSFERS:
        three = D.threshold_values().reshape(3, 256, 3)[transfer]
        image = np.concatenate([three, np.zeros((256, 1), np.float32)], -1)[None]
        byte = D.tonemap(image, None, dict(tone=D.CLAMP, transfer=transfer, exposure=1.0))[0].astype(int)
        k = np.arange(256)
        assert (byte[:, 0] == np.maximum(k - 1, 0)).all() and (byte[:, 1] == k).all() and (byte[:, 2] == k).all()


def device_guides(be, first, n):
    import torch
    t = {name: torch.empty((H, W) if name == "hit_count" else (H, W, 4), dtype=torch.float32, device="cuda") for name in GUIDE_NAMES}
    torch.cuda.synchronize()
    be.render_guides_device(first, n, **{name: x.data_ptr() for name, x in t.items()})
    return t


@pytest.mark.parametrize("flags", [0, DA], ids=["strict", "default"])
@pytest.mark.parametrize("name", ["cornell", "matmix"])
def test_rendered_scenes(name, flags):
    """The display's arithmetic is the same in both modes; its inputs are not."""
    import torch
    be = gpu_cases.context(G.scene(name), W, H, flags=flags)
    try:
        be.render(0, 3)
        color, count = be.read_image()
        assert np.array_equal(be.luminance_histogram(), D.histogram(color, count))
        assert np.array_equal(device_histogram(be, None, None), D.histogram(color, count))
        for params in A_FEW:
            rgb = D.tonemap(color, count, params)
            assert rgb.max() > rgb.min()  # (the scene shows something)
            host = be.display(**params)
            assert_bytes(host, D.pack_bgr24(rgb, stride_of(W)), params)
            assert_bytes(be.display(rgba=True, **params), D.pack_rgba32(rgb), params)
            # the device form on the context's own accumulators equals the host form
            assert_bytes(device_bgr(be, None, None, W, H, **params), host, params)
        assert_bytes(be.display(), D.pack_bgr24(D.tonemap(color, count, backend.DISPLAY_DEFAULTS), stride_of(W)), "every default")
        # the device form on denoise_device's output, a mean plane, equals the yardstick on the host form's
        guides = device_guides(be, 0, 3)
        mean = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        be.denoise_device(mean.data_ptr(), {k: t.data_ptr() for k, t in guides.items()}, guide_iterations=3)
        denoised = be.denoise(guide_first_iteration=0, guide_iterations=3)
        for params in A_FEW:
            rgb = D.tonemap(denoised, None, params)
            assert_bytes(device_bgr(be, mean, None, W, H, **params), D.pack_bgr24(rgb, stride_of(W)), ("denoised", params))
            assert_bytes(device_rgba(be, mean, None, W, H, **params), D.pack_rgba32(rgb), ("denoised", params))
        assert np.array_equal(device_histogram(be, mean, None), D.histogram(denoised, None))
    finally:
        be.release()


def test_three_listed_devices():
    """The host forms show the summed image; the device forms have no accumulators to default to, and take planes as ever."""
    be = gpu_cases.context(G.scene("cornell"), W, H, devices=[0, 0, 0])
    try:
        be.render(0, 6)
        baseline = state(be)
        color, count = be.read_image()
        assert count.max() == 6
        for params in A_FEW:
            rgb = D.tonemap(color, count, params)
            assert_bytes(be.display(**params), D.pack_bgr24(rgb, stride_of(W)), params)
            assert_bytes(be.display(rgba=True, **params), D.pack_rgba32(rgb), params)
        assert np.array_equal(be.luminance_histogram(), D.histogram(color, count))
        out, words = filled(H * stride_of(W)), garbage_words()
        with pytest.raises(PtmiError) as e:
            be.display_device(out.data_ptr())
        assert e.value.code == UNSUPPORTED
        with pytest.raises(PtmiError) as e:
            be.luminance_histogram_device(words.data_ptr())
        assert e.value.code == UNSUPPORTED
        be.synchronize()
        assert bool((out == 0xAA).all()) and bool((words == -559038737).all())
        d_color, d_count = to_device(color), to_device(count)
        assert_bytes(device_bgr(be, d_color, d_count, W, H), be.display(), "planes of the caller's")
        assert np.array_equal(device_histogram(be, d_color, d_count), D.histogram(color, count))
        assert_same_state(state(be), baseline)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- display calls and renders

def test_display_calls_are_invisible_to_renders():
    sc = G.scene("cornell")

    def play(with_display):
        be = gpu_cases.context(sc, W, H, flags=backend.FLAG_SCHEDULER_STATS)
        try:
            be.render(0, 2)
            be.snapshot(5)
            out, words = filled(H * stride_of(W)), garbage_words()
            if with_display:
                be.display()
                be.luminance_histogram()
            be.render(2, 2)
            for k in range(4, 10):  # one-iteration calls of a caller that waits: rendered ahead of
                be.render(k, 1)
                be.synchronize()
                if with_display:
                    before = state(be), be.scheduler_stats()
                    be.display_device(out.data_ptr())
                    be.luminance_histogram_device(words.data_ptr())
                    if k % 3 == 0:
                        be.display(rgba=True, tone=D.REINHARD, white=2.0)
                        be.luminance_histogram()
                    assert_same_state(state(be), before[0])
                    assert be.scheduler_stats() == before[1]
            kept = be.read_snapshot(5)
            return state(be), [a.view(np.uint32).copy() for a in kept]
        finally:
            be.release()

    (a, kept_a), (b, kept_b) = play(True), play(False)
    assert_same_state(a, b)
    assert all(np.array_equal(x, y) for x, y in zip(kept_a, kept_b)) and kept_a[1].view(np.float32).max() == 2


def test_device_forms_are_ordered_on_the_contexts_stream():
    import torch
    be = gpu_cases.context(G.scene("cornell"), W, H)
    try:
        out, words = filled(H * stride_of(W)), garbage_words()
        be.render(0, 4)  # not waited for: the calls behind it must see all four iterations
        be.display_device(out.data_ptr())
        be.luminance_histogram_device(words.data_ptr())
        be.synchronize()
        color, count = be.read_image()
        assert count.max() == 4
        want = D.pack_bgr24(D.tonemap(color, count, backend.DISPLAY_DEFAULTS), stride_of(W))
        assert_bytes(out.cpu().numpy().reshape(H, -1), want, "behind a render in flight")
        assert np.array_equal(words.cpu().numpy().view(np.uint32), D.histogram(color, count))
        # ... on a stream of the caller's, read by torch behind the call
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        be.set_stream(stream.cuda_stream)
        again, words_again = filled(H * stride_of(W)), garbage_words()
        be.display_device(again.data_ptr())
        be.luminance_histogram_device(words_again.data_ptr())
        with torch.cuda.stream(stream):
            copy, words_copy = again.clone(), words_again.clone()
        stream.synchronize()
        assert_bytes(copy.cpu().numpy().reshape(H, -1), want, "on the caller's stream")
        assert np.array_equal(words_copy.cpu().numpy().view(np.uint32), D.histogram(color, count))
        assert_bytes(be.display(), want, "the host form on the caller's stream")
        be.set_stream(None)
        # a page-locked result is landed in directly, and equals the unpinned one
        pinned = np.full((H, stride_of(W)), 0xAA, np.uint8)
        be.pin_host_buffer(pinned)
        assert be.display(out=pinned) is pinned
        assert_bytes(pinned, want, "page-locked")
        be.unpin_host_buffer(pinned)
        pinned_rgba = np.full((H, W, 4), 0xAA, np.uint8)
        be.pin_host_buffer(pinned_rgba)
        assert_bytes(be.display(rgba=True, out=pinned_rgba), be.display(rgba=True), "page-locked RGBA32")
        be.unpin_host_buffer(pinned_rgba)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- errors

def test_refusals_leave_the_context_rendering():
    sc = G.scene("cornell")
    lib = backend.load_library()
    vp = C.c_void_p
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    fresh = gpu_cases.context(sc, W, H)
    try:
        for call in (be.display, be.luminance_histogram, lambda: be.display_device(256), lambda: be.luminance_histogram_device(256)):
            with pytest.raises(PtmiError) as e:
                call()
            assert e.value.code == STATE and "before ptmi_initialize_memory" in str(e.value)
        be.initialize_memory(sc)
        be.render(0, 3)
        baseline = state(be)
        out, words = filled(H * stride_of(W)), garbage_words()
        host_out = np.full((H, stride_of(W)), 0xAA, np.uint8)
        host_words = np.full(D.WORDS, 0xAAAAAAAA, np.uint32)
        color, count = (to_device(a) for a in be.read_image())

        def params(**changes):
            p = be.display_params(tone=D.REINHARD, white=2.0)
            for k, v in changes.items():
                setattr(p, k, v)
            return p

        def reserved(i):
            p = params()
            p.reserved[i] = 1
            return p

        inf, nan = float("inf"), float("nan")
        bad_params = [None, params(struct_size=44), params(struct_size=52), params(flags=1), params(flags=0x80000000)]
        bad_params += [reserved(i) for i in range(4)]
        bad_params += [params(tone=3), params(transfer=3), params(format=2), params(tone=0xFFFFFFFF)]
        bad_params += [params(row_stride=3 * W - 1), params(row_stride=3 * W + 4), params(row_stride=4 * W), params(row_stride=0)]
        bad_params += [params(format=backend.PIXELS_RGBA32, row_stride=s) for s in (3 * W, 4 * W - 1, 4 * W + 1, 4 * W + 4)]
        bad_params += [params(exposure=v) for v in (0.0, -1.0, inf, -inf, nan)]
        bad_params += [params(white=v) for v in (0.0, -0.0, -2.0, -inf, nan)]
        attempts = []
        for p in bad_params:
            ref = None if p is None else C.byref(p)
            attempts.append(lambda ref=ref: lib.ptmi_read_display_tonemapped(be._ctx, ref, host_out.ctypes.data_as(vp)))
            attempts.append(lambda ref=ref: lib.ptmi_display_device(be._ctx, ref, None, None, vp(out.data_ptr())))
        good = params()
        display = lambda c, n, o: lib.ptmi_display_device(be._ctx, C.byref(good), vp(c), vp(n), vp(o))  # noqa: E731
        histogram = lambda c, n, o: lib.ptmi_luminance_histogram_device(be._ctx, vp(c), vp(n), vp(o))  # noqa: E731
        attempts.append(lambda: lib.ptmi_read_display_tonemapped(be._ctx, C.byref(good), None))
        attempts.append(lambda: lib.ptmi_luminance_histogram(be._ctx, None))
        for call, result in ((display, out), (histogram, words)):
            attempts.append(lambda call=call: call(None, None, None))                                          # no result
            attempts.append(lambda call=call, r=result: call(None, None, r.data_ptr() + 8))                    # a misaligned one
            attempts.append(lambda call=call, r=result: call(None, count.data_ptr(), r.data_ptr()))            # counts without sums
            attempts.append(lambda call=call, r=result: call(color.data_ptr() + 4, count.data_ptr(), r.data_ptr()))
            attempts.append(lambda call=call, r=result: call(color.data_ptr(), count.data_ptr() + 4, r.data_ptr()))
            attempts.append(lambda call=call, r=result: call(color.data_ptr() + 8, None, r.data_ptr()))
        for attempt in attempts:
            assert attempt() == INVALID_ARGUMENT and len(lib.ptmi_last_error(be._ctx)) > 0
            assert_same_state(state(be), baseline)
        be.synchronize()
        assert bool((out == 0xAA).all()) and bool((words == -559038737).all())  # nothing was launched
        assert (host_out == 0xAA).all() and (host_words == 0xAAAAAAAA).all()
        # what the struct allows: a white that nobody reads, an infinite one, every stride
        for p in (params(tone=D.CLAMP, white=nan), params(tone=D.FILMIC, white=-1.0), params(white=inf), params(row_stride=3 * W),
                  params(row_stride=3 * W + 3)):
            assert lib.ptmi_display_device(be._ctx, C.byref(p), None, None, vp(out.data_ptr())) == 0
        assert_bytes(be.display(tone=D.REINHARD, white=2.0), D.pack_bgr24(D.tonemap(*be.read_image(), dict(tone=D.REINHARD, transfer=D.SRGB, white=2.0)),
                                                                       stride_of(W)), "a good call after the refusals")
        assert_same_state(state(be), baseline)
        # a following render gives the image of a context that never saw a refusal
        be.render(3, 2)
        fresh.render(0, 3)
        fresh.render(3, 2)
        assert_same_state(state(be), state(fresh))
    finally:
        be.release()
        fresh.release()
