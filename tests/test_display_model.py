"""The display stage without a GPU: the new ABI is held against the header, ptmi_display_table and the generated file against the
double formulae, and the yardstick of the GPU tests (display_cases.py) against the properties that make the contract a display:
monotone, round-to-nearest beside the reference viewer's truncation, black for what is not a colour, white for infinity."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from opencl_pathtracer_amd import backend, output
from abi_cases import declared_symbols, exported_symbols, header_values
import display_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"ptmi_display_table", "ptmi_read_display_tonemapped", "ptmi_display_device", "ptmi_luminance_histogram",
               "ptmi_luminance_histogram_device"}
f32 = np.float32


# ---------------------------------------------------------------------------------------------- ABI

def test_header_binding_list_and_library_agree(built):
    declared = set(declared_symbols())
    assert NEW_SYMBOLS <= declared and declared == set(backend.ABI_SYMBOLS)
    assert NEW_SYMBOLS <= exported_symbols()
    assert backend.load_library().ptmi_abi_version() == 4


FIELDS = "struct_size flags tone transfer format row_stride exposure white reserved".split()
CONSTANTS = dict(PTMI_TONE_CLAMP=backend.TONE_CLAMP, PTMI_TONE_REINHARD=backend.TONE_REINHARD, PTMI_TONE_FILMIC=backend.TONE_FILMIC,
                 PTMI_TRANSFER_LINEAR=backend.TRANSFER_LINEAR, PTMI_TRANSFER_SRGB=backend.TRANSFER_SRGB,
                 PTMI_TRANSFER_GAMMA22=backend.TRANSFER_GAMMA22, PTMI_PIXELS_BGR24=backend.PIXELS_BGR24,
                 PTMI_PIXELS_RGBA32=backend.PIXELS_RGBA32, PTMI_LUMINANCE_WORDS=backend.LUMINANCE_WORDS, PTMI_ABI_VERSION=4)


def test_ctypes_struct_and_constants_match_the_header():
    out = header_values(["SIZE(ptmi_display_params);"] + [f"OFFSET(ptmi_display_params, {f});" for f in FIELDS] +
                        [f'VALUE("{name}", {name});' for name in CONSTANTS])
    want = {"ptmi_display_params": C.sizeof(backend.DisplayParams), **CONSTANTS}
    want.update({f"ptmi_display_params.{name}": getattr(backend.DisplayParams, name).offset for name, _ in backend.DisplayParams._fields_})
    assert [name for name, _ in backend.DisplayParams._fields_] == FIELDS
    assert out == want
    assert C.sizeof(backend.DisplayParams) == 48
    assert (D.CLAMP, D.REINHARD, D.FILMIC, D.LINEAR, D.SRGB, D.GAMMA22, D.WORDS) == (0, 1, 2, 0, 1, 2, backend.LUMINANCE_WORDS)


def test_default_parameters():
    assert backend.DISPLAY_DEFAULTS == dict(tone=backend.TONE_FILMIC, transfer=backend.TRANSFER_SRGB, exposure=1.0, white=float("inf"))
    be = backend.Backend.__new__(backend.Backend)
    be.cfg = backend.Config(image_width=5, image_height=3)
    p = be.display_params()
    assert (p.struct_size, p.flags, p.tone, p.transfer, p.format, p.row_stride, p.exposure, p.white) == (48, 0, 2, 1, 0, 16, 1.0, float("inf"))
    assert list(p.reserved) == [0, 0, 0, 0]
    assert be.display_params(rgba=True).row_stride == 20 and be.display_params(rgba=True).format == backend.PIXELS_RGBA32


def test_argument_validation_needs_no_gpu(built):
    lib = backend.load_library()
    good = backend.DisplayParams(48, 0, 0, 0, 0, 12, 1.0, 1.0)
    pixels = np.zeros(64, np.uint8)
    words = np.zeros(260, np.uint32)
    for p in (C.byref(good), None):  # a NULL context: refused whatever else is given
        assert lib.ptmi_read_display_tonemapped(None, p, pixels.ctypes.data_as(C.c_void_p)) == -1
        assert lib.ptmi_display_device(None, p, 256, 256, 256) == -1
    assert lib.ptmi_luminance_histogram(None, words.ctypes.data_as(C.c_void_p)) == -1
    assert lib.ptmi_luminance_histogram_device(None, None, None, 256) == -1


# ---------------------------------------------------------------------------------------------- the tables

@pytest.mark.parametrize("transfer", D.TRANSFERS)
def test_display_table_equals_the_double_formulae_bit_for_bit(built, transfer):
    got, want = backend.display_table(transfer), D.tables()[transfer]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == 0 and got[255] < 1 and (np.diff(got) > 0).all()
    # the thresholds are where the encoded value rounds: k / 255 decodes into [T[k], T[k + 1])
    centres = np.array([D.eotf(transfer, k / 255.0) for k in range(256)])
    assert (got.astype(np.float64) <= centres).all() and (centres[:-1] < got[1:].astype(np.float64)).all()


def test_display_table_refuses_an_unknown_transfer_and_a_null_table(built):
    lib = backend.load_library()
    table = np.full(256, -1, f32)
    assert lib.ptmi_display_table(3, table.ctypes.data_as(C.c_void_p)) == -1
    assert b"transfer" in lib.ptmi_last_error(None) and (table == -1).all()
    assert lib.ptmi_display_table(0xFFFFFFFF, table.ctypes.data_as(C.c_void_p)) == -1
    assert lib.ptmi_display_table(backend.TRANSFER_SRGB, None) == -1
    assert b"NULL" in lib.ptmi_last_error(None)
    with pytest.raises(backend.PtmiError) as e:
        backend.display_table(7)
    assert e.value.code == -1


def generator():
    spec = importlib.util.spec_from_file_location("make_display_tables", os.path.join(ROOT, "tools", "make_display_tables.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_generator_reproduces_the_committed_file():
    g = generator()
    with open(os.path.join(ROOT, "opencl_pathtracer_amd", "csrc", "display_tables.inc")) as f:
        assert f.read() == g.text()
    for transfer in D.TRANSFERS:
        assert np.array_equal(g.table(transfer).view(np.uint32), D.tables()[transfer].view(np.uint32))
    # the literals of the file, read back: the same floats
    literals = [float.fromhex(x[:-1]) for x in g.text().replace(",", " ").split() if x.startswith("0x")]
    assert np.array_equal(np.array(literals, np.float64), np.concatenate([D.tables()[t] for t in D.TRANSFERS]).astype(np.float64))
    assert g.margin() >= 0.0019  # no libm that is right to a thousandth of a float32 ulp rounds a threshold the other way


# ---------------------------------------------------------------------------------------------- what makes the contract a display

ALL = [dict(tone=tone, transfer=transfer, white=white) for tone in D.TONES for transfer in D.TRANSFERS
       for white in ((2.0, np.inf) if tone == D.REINHARD else (np.inf,))]


def ramp():
    """every float32 between neighbours of the thresholds, a dense ramp over 0 .. 4, and octaves up to the largest float"""
    x = np.concatenate([D.threshold_values(), np.linspace(0, 4, 20001).astype(f32), np.ldexp(f32(1), np.arange(-149, 128)).astype(f32)])
    x = np.sort(x[x >= 0])
    return np.repeat(x[None, :, None], 4, -1)  # an image of one row; r = g = b


@pytest.mark.parametrize("params", ALL, ids=lambda p: f"tone{p['tone']}-transfer{p['transfer']}-white{p['white']}")
def test_the_byte_is_monotone_in_the_value(params):
    image = ramp()
    for exposure in (1.0, 0.25, 3.5):
        byte = D.tonemap(image, None, dict(params, exposure=exposure))[0, :, 0].astype(int)
        assert (np.diff(byte) >= 0).all() and byte[0] == 0
        assert byte[-1] == 255  # (also where 3.4e38 * 3.5 is infinite and the curve's inf / inf a NaN)


def test_linear_clamp_is_the_reference_viewers_byte_or_one_more():
    """Round to nearest against truncation: with CLAMP, LINEAR and exposure 1, on pixels with finite non-negative sums and
    n > 0, the byte is that of output.to_display_rgb or the next."""
    color, count = D.synthetic(130, 66, seed=3)
    fine = (count > 0) & np.isfinite(count) & (np.isfinite(color[..., :3]) & (color[..., :3] >= 0)).all(-1)
    assert fine.sum() > 4000
    new = D.tonemap(color, count, dict(tone=D.CLAMP, transfer=D.LINEAR, exposure=1.0)).astype(int)[fine]
    with np.errstate(all="ignore"):  # (the pixels that are not `fine` overflow there)
        old = output.to_display_rgb(color, count).astype(int)[fine]
    assert ((new == old) | (new == old + 1)).all()
    assert (new == old).any() and (new == old + 1).any()


@pytest.mark.parametrize("params", ALL, ids=lambda p: f"tone{p['tone']}-transfer{p['transfer']}-white{p['white']}")
def test_what_is_no_colour_is_black_and_infinity_is_white(params):
    black = np.array([np.nan, -1.0, -0.0, 0.0, -np.inf, -1e-40], f32)
    image = np.repeat(black[None, :, None], 4, -1)
    assert (D.tonemap(image, None, dict(params, exposure=2.0)) == 0).all()
    assert (D.tonemap(image, np.ones((1, 6), f32), dict(params, exposure=2.0)) == 0).all()
    # never sampled, whatever the sums hold: a count that is zero, negative or NaN
    sums = np.full((1, 4, 4), 5.0, f32)
    unsampled = np.array([[0.0, -0.0, -3.0, np.nan]], f32)
    assert (D.tonemap(sums, unsampled, dict(params, exposure=1.0)) == 0).all()
    assert D.histogram(sums, unsampled)[256] == 4
    white = np.full((1, 1, 4), np.inf, f32)
    for exposure in (1.0, 1e-30):
        assert (D.tonemap(white, None, dict(params, exposure=exposure)) == 255).all()
        assert (D.tonemap(white, np.ones((1, 1), f32), dict(params, exposure=exposure)) == 255).all()


def test_the_histograms_words_sum_to_the_pixel_count():
    for w, h, seed in ((1, 1, 0), (5, 3, 1), (70, 37, 2), (130, 66, 3)):
        color, count = D.synthetic(w, h, seed)
        for n in (count, None):
            hist = D.histogram(color, n)
            assert hist.dtype == np.uint32 and hist.shape == (260,) and int(hist.sum()) == w * h and hist[258] == hist[259] == 0
    assert hist[:256].sum() > 0 and hist[256] > 0 and hist[257] > 0
    # bin 128 starts at 1.0, a bin ends where the next starts, and a value lands in the bin that starts at or below it
    assert D.bin_start(128) == 1.0 and D.bin_start(129) == 1.25 and D.bin_start(132) == 2.0
    for b in (0, 1, 77, 128, 131, 254):
        for value in (D.bin_start(b), np.nextafter(f32(D.bin_start(b)), f32(0)), D.bin_start(b) * 1.1):
            grey = np.full((1, 1, 4), value, f32)
            Y = float(D.luminance(grey, None)[0, 0])  # (the three weights sum to 1 only nearly: it is Y that is binned)
            hist = D.histogram(grey, None)
            found = int(np.flatnonzero(hist)[0])
            assert hist.sum() == 1 and abs(found - b) <= 1 and (D.bin_start(found) <= Y or found == 0) and Y < D.bin_start(found + 1)
    huge = np.full((1, 1, 4), 3e38, f32)
    assert D.histogram(huge, None)[255] == 1 and D.histogram(np.full((1, 1, 4), 1e-45, f32), None)[[0, 256]].sum() == 1


# ---------------------------------------------------------------------------------------------- the exposure

def test_exposure_from_histogram_brings_a_constant_image_to_the_key():
    """A constant image of luminance Y lands in one bin; the bin's representative 1 + (i + 0.5) / 4 lies within
    (1 + (i + 0.5) / 4) / (1 + i / 4) <= 1.125 above the bin's start and (1 + (i + 1) / 4) / (1 + (i + 0.5) / 4) <= 1.112 below its
    end, so exposure * Y / key lies in [0.88, 1.12]."""
    rng = np.random.default_rng(4)
    for Y in np.concatenate([np.ldexp(rng.uniform(1, 2, 200), rng.integers(-12, 13, 200)), [1.0, 0.18, 2.0 ** -12, 4096.0]]):
        grey = np.full((4, 6, 4), Y, f32)
        hist = D.histogram(grey, None)
        assert hist[:256].sum() == 24
        luminance = float(D.luminance(grey, None)[0, 0])
        for key in (0.18, 0.5):
            exposure = backend.exposure_from_histogram(hist, key=key)
            assert isinstance(exposure, float) and 0.88 <= exposure * luminance / key <= 1.12, (Y, exposure)
    assert backend.exposure_from_histogram(hist) == backend.exposure_from_histogram(hist, key=0.18)


def test_exposure_of_an_all_black_histogram_is_one():
    hist = np.zeros(260, np.uint32)
    hist[256], hist[257] = 1000, 3
    assert backend.exposure_from_histogram(hist) == 1.0
    # the log-average: a quarter of the pixels four octaves up moves the mean one octave
    hist[:] = 0
    hist[128], hist[144] = 3, 1
    assert backend.exposure_from_histogram(hist, key=1.0) == pytest.approx(0.5 / 1.125, rel=1e-12)
