"""The function-level differential on the GPU: each device function of ptmi_device.hpp on the boundary inputs of
unit_probe_cases.py, held word for word (uint32) to the CPU oracle's export of the same reference function and to the
reference's OWN function compiled for this GPU (oracle/ref_unit_probe.cl), in both arithmetics:

    strict : ptmi_dev    == libpt_oracle.so    == ref_unit_probe.strict.hsaco
    default: ptmi_dev_da == libpt_oracle_da.so == ref_unit_probe.hsaco

The fast forms (box_hit_ordered; tri_hit_pre, tri_test<false>, tri_test<true>) are held to the literal ones inside the domain
their comments claim (unit_probe_cases.box_in_ordered_domain / triangle_domains) and not outside it, where only box_hit and
tri_hit answer to the reference.  NaN words: a word must be a NaN where the oracle's is.  NaN BITS are compared where no input is a NaN (then no NaN sits on the
right of a subtraction and no two meet; the rule test_ray_query_gpu.py states) - against the oracle where the NaN is an input's
copy, between product and reference where an instruction produced it (produced_nan_rule)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_ffi as O
import unit_probe_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "oracle", "build", "libunit_probe.so")
f32, u32 = np.float32, np.uint32
ARITHMETICS = [pytest.param(False, id="strict"), pytest.param(True, id="default")]


def ref_path(da):
    return os.path.join(O.REF_DIR, "ref_unit_probe.hsaco" if da else "ref_unit_probe.strict.hsaco")


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("oracle/build/libunit_probe.so not built (make -C oracle probe)", pytrace=False)
    for da in (False, True):
        if not os.path.exists(ref_path(da)):
            pytest.fail(os.path.relpath(ref_path(da), ROOT) + " not built (make -C oracle ref, where the reference tree exists)", pytrace=False)
    return C.CDLL(PROBE)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def product(probe, group, da, cases, out_words, *aux):
    fn = getattr(probe, f"unit_probe_{group}" + ("_da" if da else ""))
    fn.restype = C.c_int
    cases = np.ascontiguousarray(cases)
    out = np.zeros((len(cases), out_words), u32)
    args = [_vp(cases), C.c_uint32(len(cases))] + [(_vp(a) if isinstance(a, np.ndarray) else C.c_uint32(a)) for a in aux] + [_vp(out)]
    rc = fn(*args)
    assert rc == 0, f"unit_probe_{group}: {rc}"
    return out


def reference(probe, group, da, cases, out_words, aux0=None, aux1=None, image_8x8=False):
    probe.unit_probe_reference.restype = C.c_int
    cases = np.ascontiguousarray(cases)
    out = np.zeros((len(cases), out_words), u32)
    a0 = np.ascontiguousarray(aux0) if aux0 is not None else None
    a1 = np.ascontiguousarray(aux1) if aux1 is not None else None
    rc = probe.unit_probe_reference(ref_path(da).encode(), f"unit_{group}".encode(), _vp(cases), C.c_uint32(cases.shape[1]), C.c_uint32(len(cases)),
                                    _vp(out), C.c_uint32(out_words), _vp(a0) if a0 is not None else None, C.c_uint32(a0.nbytes if a0 is not None else 0),
                                    _vp(a1) if a1 is not None else None, C.c_uint32(a1.nbytes if a1 is not None else 0),
                                    C.c_uint32(1 if image_8x8 else 0))
    assert rc == 0, f"unit_probe_reference({group}): {rc}"
    return out


def has_nan_input(cases, columns):
    with np.errstate(invalid="ignore"):
        return np.isnan(cases.view(f32)[:, columns]).any(axis=1)


def check(group, names, outputs, cases, rows=None, nan_free=None):
    """all outputs equal on `rows`; NaN bits count on the rows of `nan_free` only"""
    rows = np.ones(len(cases), bool) if rows is None else rows
    nan_free = np.ones(len(cases), bool) if nan_free is None else nan_free
    for sel, bits in ((rows & nan_free, True), (rows & ~nan_free, False)):
        if sel.any():
            msg = K.describe_difference(group, names, [o[sel] for o in outputs], cases[sel], nan_bits=bits)
            assert msg == "", msg + f"\n  (case numbers count the {'NaN-free' if bits else 'NaN-carrying'} rows of this comparison)"


@pytest.mark.parametrize("da", ARITHMETICS)
def test_box(probe, da):
    lib = O.oracle(da)
    cases = K.box_cases()
    got = product(probe, "box", da, cases, 3)
    want = K.oracle_box(lib, cases)
    ref = reference(probe, "box", da, cases, 1)
    check("box: box_hit / oracle / reference", ["product", "oracle", "reference"], [got[:, 0:1], want, ref], cases)
    inside = K.box_in_ordered_domain(lib, cases)
    # the product's own predicate admits no ray the stated domain excludes
    _, inv = K.oracle_ray(lib, cases[:, 8:12], cases[:, 12:16])
    ordered = got[:, 2] == 1
    assert not (ordered & ~np.isfinite(inv).all(axis=1)).any()
    assert np.array_equal(ordered, np.isfinite(inv).all(axis=1) & np.isfinite(cases.view(f32)[:, 8:11]).all(axis=1)), \
        "ray_slabs_are_ordered differs from its stated condition"
    check("box: box_hit_ordered / reference inside the ordered domain", ["ordered", "oracle", "reference"], [got[:, 1:2], want, ref], cases, rows=inside)


@pytest.mark.parametrize("da", ARITHMETICS)
def test_triangle(probe, da):
    lib = O.oracle(da)
    cases, n_inside = K.triangle_cases(O.oracle(False))
    safe, equal_w = K.triangle_domains(cases)
    got = product(probe, "triangle", da, cases, 40)
    want = K.oracle_triangle(lib, cases)
    mats = np.zeros(2, O.S.Material)
    mats["isSimpleColor"] = 1
    ref = reference(probe, "triangle", da, cases, 10, aux0=mats)
    nan_free = ~has_nan_input(cases, slice(0, 25)) & safe
    names = ["tri_hit", "oracle", "reference"]
    check("triangle: tri_hit / oracle / reference", names, [got[:, 0:10], want, ref], cases, nan_free=nan_free)
    check("triangle: tri_test<false> inside the safe domain", ["tri_test"] + names, [got[:, 20:30], got[:, 0:10], want, ref], cases, rows=safe)
    check("triangle: tri_hit_pre inside the safe domain, equal w", ["tri_hit_pre"] + names, [got[:, 10:20], got[:, 0:10], want, ref], cases,
          rows=safe & equal_w)
    check("triangle: tri_test<true> inside the safe domain, equal w", ["tri_test_pre"] + names, [got[:, 30:40], got[:, 0:10], want, ref], cases,
          rows=safe & equal_w)


@pytest.mark.parametrize("da", ARITHMETICS)
def test_texture_and_sky(probe, da):
    lib = O.oracle(da)
    tex, texels = K.texture_data()
    cases = K.texture_cases()
    want, index = K.oracle_texture(lib, cases)
    assert ((index >= cases[:, 2]) & (index < cases[:, 2] + cases[:, 0] * cases[:, 1])).all()   # nothing is read outside the data
    got = product(probe, "texture", da, cases, 4, texels, len(texels))
    ref = reference(probe, "texture", da, cases, 4, aux0=texels, aux1=np.zeros(len(cases), O.S.Texture))
    check("texture", ["product", "oracle", "reference"], [got, want, ref], cases)
    sky = K.sky_cases()
    want, face, index = K.oracle_sky(lib, sky)
    assert (index < len(texels)).all()
    got = product(probe, "sky", da, sky, 4, np.ascontiguousarray(tex[len(K.TEXTURE_SIZES):]), texels, len(texels))
    ref = reference(probe, "sky", da, sky, 4, aux0=texels, aux1=K.skies_of(sky))
    check("sky", ["product", "oracle", "reference"], [got, want, ref], sky)


@pytest.mark.parametrize("da", ARITHMETICS)
def test_light(probe, da):
    cases = K.light_cases()
    got = product(probe, "light", da, cases, 1)
    want = K.oracle_light(O.oracle(da), cases)
    ref = reference(probe, "light", da, cases, 1)
    produced_nan_rule("light", cases, got, want, ref)


def produced_nan_rule(group, cases, got, want, ref):
    """No input of these groups is a NaN: every NaN word is PRODUCED (0 / 0, inf * 0, the square root of a negative number) and
    no two NaNs meet, so its bits are the producing instruction's - compared between the product and the reference, which run on
    the same hardware.  The CPU oracle's host produces the default NaN with the other sign: against it such a word must be a NaN,
    and every other word equal."""
    check(group + ": product / reference", ["product", "reference"], [got, ref], cases)
    check(group + ": product / oracle / reference", ["product", "oracle", "reference"], [got, want, ref], cases, nan_free=np.zeros(len(cases), bool))


@pytest.mark.parametrize("da", ARITHMETICS)
def test_material(probe, da):
    cases = K.material_cases()
    got = product(probe, "material", da, cases, K.MATERIAL_OUT)
    want = K.oracle_material(O.oracle(da), cases)
    ref = reference(probe, "material", da, cases, K.MATERIAL_OUT)
    produced_nan_rule("material", cases, got, want, ref)


@pytest.mark.parametrize("da", ARITHMETICS)
def test_sampling(probe, da):
    cases = K.sampling_cases()
    got = product(probe, "sampling", da, cases, K.SAMPLING_OUT)
    want = K.oracle_sampling(O.oracle(da), cases)
    ref = reference(probe, "sampling", da, cases, K.SAMPLING_OUT)
    check("sampling: product / oracle", ["product", "oracle"], [got, want], cases)
    w = K.SAMPLING_REFERENCE_WORDS
    check("sampling: product / oracle / reference", ["product", "oracle", "reference"], [got[:, w], want[:, w], ref[:, w]], cases)


@pytest.mark.parametrize("da", ARITHMETICS)
def test_pixel(probe, da):
    lib = O.oracle(da)
    cases = K.pixel_cases()
    got = product(probe, "pixel", da, cases, K.PIXEL_OUT)
    want = K.oracle_pixel(lib, cases)
    check("pixel: draw_sample, sample_pixel / oracle", ["product", "oracle"], [got, want], cases)
    # the reference's sampler(): its image size is a -D and its pixel the work-item's id, so the leg is the 8 x 8 JITTERED block
    block = K.pixel_reference_cases()
    w = K.PIXEL_REFERENCE_WORDS
    ref = reference(probe, "pixel", da, block, K.PIXEL_OUT, image_8x8=True)
    got8, want8 = product(probe, "pixel", da, block, K.PIXEL_OUT), K.oracle_pixel(lib, block)
    check("pixel: draw_sample / oracle / reference at 8 x 8", ["product", "oracle", "reference"], [got8[:, w], want8[:, w], ref[:, w]], block)
