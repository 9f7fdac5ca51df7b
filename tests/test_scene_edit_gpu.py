"""Editing a loaded scene in place: ptmi_update_materials, ptmi_update_lights and ptmi_set_sky against a fresh upload.

The yardstick is always a SECOND context that was given the edited scene through ptmi_initialize_memory - code that existed
before the edit calls did.  What the two contexts render after ptmi_clear must be bit-equal: image, sample counts, the three
histograms and ptmi_counters (gpu_cases.assert_same_state).  Every test also checks that the edit did change the image.  A
refused edit returns ptmi_validate_scene's status and words for the edited scene and leaves the old scene rendering as before.
Image 64 x 48, depth 4, 4 iterations: the sizes of test_scene_update_gpu.py.
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, bvh_create, scenes, structs as S
from gpu_cases import assert_same_state as assert_same, cached_scene, state
import gpu_cases
import scene_edit_cases as E
import scene_update_cases as U

pytestmark = pytest.mark.gpu
W, H = 64, 48
DA = backend.FLAG_DEFAULT_ARITHMETIC
ARITHMETICS = [pytest.param(0, id="strict"), pytest.param(DA, id="default")]
BALL = 2  # scenes.feature_scene: the sphere's material
PREFIXES = ("ptmi_update_materials: ", "ptmi_update_lights: ", "ptmi_set_sky: ", "ptmi_update_triangles: ", "ptmi_update_triangles_device: ")


def scene(name):
    return cached_scene(name, W, H)


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, **kw)


_rendered = {}


def rendered(key, sc, n=4, **kw):
    """What a fresh context of `sc` renders in n iterations; computed once per `key` (a name for `sc`) and settings, read-only."""
    k = (key, n, tuple(sorted(kw.items(), key=lambda x: x[0]))) if "devices" not in kw else None
    if k is not None and k in _rendered:
        return _rendered[k]
    be = context(sc, **kw)
    try:
        be.render(0, n)
        out = state(be, variance=kw.get("super_sampling", False))
    finally:
        be.release()
    if k is not None:
        _rendered[k] = out
    return out


def after(be, n=4, variance=False):
    be.clear()
    be.render(0, n)
    return state(be, variance=variance)


def differs(a, b):
    return not np.array_equal(a["color"], b["color"])


def outcome(call):
    """(status, message after the entry point's name) of a call that may refuse"""
    try:
        call()
        return 0, ""
    except PtmiError as e:
        text = str(e).split(": ", 1)[1]
        for prefix in PREFIXES:
            if text.startswith(prefix):
                return e.code, text[len(prefix):]
        return e.code, text


def validated(sc, **kw):
    """(status, message) ptmi_validate_scene gives for `sc`"""
    return outcome(lambda: backend.validate_scene(sc, W, H, 4, **kw))


def plain_now(be):
    """DScene::plain_shading as the context holds it (an empty material update reports it and does nothing)"""
    info = be.update_materials(0, np.zeros(0, S.Material))
    assert info["plain_before"] == info["plain_after"] and info["screened_triangles"] == 0
    return info["plain_after"]


def on_device(tris):
    t = gpu_cases.tensor_on_device(np.frombuffer(bytearray(np.ascontiguousarray(tris).tobytes()), np.float32).reshape(len(tris), 84))
    assert t.data_ptr() % 16 == 0
    return t


def update_device(be, tris):
    t = on_device(tris)
    return be.update_triangles_device(t.data_ptr(), len(tris))


# ---------------------------------------------------------------------------------------------- materials

def forth_and_back(feature, **kw):
    """feat_plain -> feat_<feature> by the one material that differs, and back: each against a fresh upload."""
    plain, other = scene("feat_plain"), scene("feat_" + feature)
    assert np.array_equal(plain.triangulation.tobytes(), other.triangulation.tobytes())  # one stage
    changed = [i for i in range(len(plain.materiaux)) if plain.materiaux[i:i + 1].tobytes() != other.materiaux[i:i + 1].tobytes()]
    assert changed == [BALL]
    variance = kw.get("super_sampling", False)
    want_plain = rendered("feat_plain", plain, **kw)
    want_other = rendered("feat_plain+" + feature, E.edited(plain, materiaux=other.materiaux), **kw)
    assert differs(want_plain, want_other)
    be = context(plain, **kw)
    try:
        be.render(0, 2)
        forth = be.update_materials(BALL, other.materiaux[BALL:BALL + 1])
        assert_same(after(be, variance=variance), want_other)
        back = be.update_materials(BALL, plain.materiaux[BALL:BALL + 1])
        assert_same(after(be, variance=variance), want_plain)
    finally:
        be.release()
    for info, (a, b) in ((forth, (1, 0)), (back, (0, 1))):
        assert info["struct_size"] == 32 and (info["plain_before"], info["plain_after"]) == (a, b), info
        assert info["screened_triangles"] == 0 and info["total_ms"] >= info["validate_ms"] >= 0


@pytest.mark.parametrize("flags", ARITHMETICS)
@pytest.mark.parametrize("feature", ["glass", "water", "varnish", "metal"])
def test_a_material_update_equals_a_fresh_upload(feature, flags):
    forth_and_back(feature, flags=flags)


@pytest.mark.parametrize("kw", [dict(flags=backend.FLAG_MEGAKERNEL), dict(super_sampling=True), dict(sampler=S.UNIFORM)],
                         ids=["megakernel", "super_sampling", "uniform"])
def test_a_material_update_with_the_other_kernel_adaptive_sampling_and_the_uniform_sampler(kw):
    forth_and_back("glass", **kw)


def textured_scenes():
    """feat_textured, the same with all four materials plain (its textures kept), and with the two texture ids exchanged"""
    tex = scene("feat_textured")
    flat = E.edited(tex, materiaux=E.all_plain(tex.materiaux))
    swapped = U.raw_copy(tex.materiaux)
    textured = np.flatnonzero(tex.materiaux["isSimpleColor"] == 0)
    assert len(textured) == 2 and len(tex.textures) == 2
    swapped["textureId"][textured] = tex.materiaux["textureId"][textured][::-1]
    return tex, flat, E.edited(tex, materiaux=swapped)


@pytest.mark.parametrize("flags", ARITHMETICS)
def test_plain_materials_turn_textured_and_change_their_texture(flags):
    tex, flat, swapped = textured_scenes()
    want_flat, want_tex = rendered("textured_flat", flat, flags=flags), rendered("feat_textured", tex, flags=flags)
    want_swapped = rendered("textured_swapped", swapped, flags=flags)
    assert differs(want_flat, want_tex) and differs(want_tex, want_swapped)
    be = context(flat, flags=flags)
    try:
        be.render(0, 2)
        first = be.update_materials(0, tex.materiaux)
        assert_same(after(be), want_tex)
        second = be.update_materials(0, swapped.materiaux)
        assert_same(after(be), want_swapped)
    finally:
        be.release()
    assert first["screened_triangles"] == len(tex.triangulation) and (first["plain_before"], first["plain_after"]) == (1, 0)
    assert second["screened_triangles"] == 0 and (second["plain_before"], second["plain_after"]) == (0, 0)


def test_the_guides_follow_a_material_update():
    tex, flat, _ = textured_scenes()
    yard = context(tex)
    try:
        want = yard.render_guides(0, 2)
    finally:
        yard.release()
    be = context(flat)
    try:
        before = be.render_guides(0, 2)
        be.update_materials(0, tex.materiaux)
        got = be.render_guides(0, 2)
    finally:
        be.release()
    assert np.array_equal(got["albedo"].view(np.uint32), want["albedo"].view(np.uint32))
    assert not np.array_equal(got["albedo"].view(np.uint32), before["albedo"].view(np.uint32))
    assert np.array_equal(got["ids"], before["ids"]) and np.array_equal(got["ids"], want["ids"])


# ---------------------------------------------------------------------------------------------- lights

@pytest.mark.parametrize("flags", ARITHMETICS)
@pytest.mark.parametrize("feature", ["spot", "directional"])
def test_a_light_of_another_type_and_back(feature, flags):
    plain, other = scene("feat_plain"), scene("feat_" + feature)
    assert plain.materiaux.tobytes() == other.materiaux.tobytes() and plain.triangulation.tobytes() == other.triangulation.tobytes()
    want_plain = rendered("feat_plain", plain, flags=flags)
    want_other = rendered("feat_plain+" + feature, E.edited(plain, lights=other.lights), flags=flags)
    assert differs(want_plain, want_other)
    be = context(plain, flags=flags)
    try:
        be.render(0, 2)
        assert plain_now(be) == 1
        be.update_lights(other.lights)
        assert plain_now(be) == 0
        assert_same(after(be), want_other)
        be.update_lights(plain.lights)
        assert plain_now(be) == 1
        assert_same(after(be), want_plain)
    finally:
        be.release()


def test_a_moved_point_light_stays_plain():
    plain = scene("feat_plain")
    lights = U.raw_copy(plain.lights)
    lights["position"][0] = np.float32([-2.5, -3.0, 4.0, 1.0])
    lights["power"][0] = 35.0
    moved = E.edited(plain, lights=lights)
    want = rendered("feat_plain+moved_light", moved)
    assert differs(want, rendered("feat_plain", plain))
    be = context(plain)
    try:
        be.update_lights(lights)
        assert plain_now(be) == 1
        assert_same(after(be), want)
    finally:
        be.release()


def test_both_lights_of_a_two_light_scene():
    sc = scene("fuzz3_l2")
    assert sc.lightsSize == 2
    lights = np.frombuffer(bytearray(2 * S.Light.itemsize), dtype=S.Light)
    lights[0] = scenes.light_spot((1.0, -2.0, 3.0), (-0.2, 0.5, -1.0), cone_angle=0.9, penumbra_angle=0.2, color=(1, 0.8, 0.7, 1), intensity=9.0)
    lights[1] = scenes.light_point((-2.0, 1.5, 2.5), color=(0.6, 0.8, 1, 1), power=25.0)
    want = rendered("fuzz3_l2+lights", E.edited(sc, lights=lights))
    assert differs(want, rendered("fuzz3_l2", sc))
    be = context(sc)
    try:
        assert be.literal_kernel_reason() is None
        be.render(0, 2)
        be.update_lights(lights)
        assert_same(after(be), want)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- sky

def test_a_new_sky_and_a_new_rotation():
    cube = scene("feat_cubemap")
    flat_sky = cube.sky.copy()
    for f in range(6):
        flat_sky["skyTextures"][f] = (1, 1, 5)  # all six faces one texel of the cube map's
    turned = cube.sky.copy()
    turned["cosRotationAngle"], turned["sinRotationAngle"] = np.float32(np.cos(1.9)), np.float32(np.sin(1.9))
    want_flat = rendered("cubemap_flat", E.edited(cube, sky=flat_sky))
    want_cube, want_turned = rendered("feat_cubemap", cube), rendered("cubemap_turned", E.edited(cube, sky=turned))
    assert differs(want_flat, want_cube) and differs(want_cube, want_turned)
    be = context(E.edited(cube, sky=flat_sky))
    try:
        be.render(0, 2)
        be.set_sky(cube.sky)
        assert_same(after(be), want_cube)
        be.set_sky(turned)
        assert_same(after(be), want_turned)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- the screen kernel

def screen_base():
    """tris20k with one 2x2 texture among its texels, its one material still plain; and that material textured"""
    base, textured = E.with_one_texture(scene("tris20k"))
    n = len(base.triangulation)
    assert n == 20000 and n % 64 == 32 and n % 256 == 32 and len(base.materiaux) == 1  # a ragged last wave and workgroup
    return base, textured


@pytest.mark.parametrize("k", [0, 63, 64, 255, 256, 19999])
def test_the_screen_refuses_what_validate_scene_refuses(k):
    base, textured = screen_base()
    for value in (np.nan, np.inf, E.up(2.0 ** 30)):
        held = E.edited(base, triangulation=E.with_bad_coordinate(base.triangulation, k, value))
        assert validated(held) == (0, "")  # under the plain material the upload accepts it
        want = validated(E.edited(held, materiaux=textured))
        assert want == (E.BAD_SCENE, E.message((k << 4) | E.TEXCOORD))
        be = context(held)
        try:
            before = after(be)
            assert outcome(lambda: be.update_materials(0, textured)) == want, (k, value)
            assert_same(after(be), before)
            # the old table is in force: the same records are still accepted, from the host and from the device
            be.update_triangles(held.triangulation)
            update_device(be, held.triangulation)
            assert outcome(lambda: be.update_materials(0, textured)) == want, (k, value)
            assert_same(after(be), before)
        finally:
            be.release()


def test_of_two_bad_triangles_the_lower_index_is_named():
    base, textured = screen_base()
    held = E.edited(base, triangulation=E.with_bad_coordinate(base.triangulation, [19000, 300], np.nan, slot=("UVP1", 0)))
    want = validated(E.edited(held, materiaux=textured))
    assert want == (E.BAD_SCENE, E.message((300 << 4) | E.TEXCOORD))
    be = context(held)
    try:
        assert outcome(lambda: be.update_materials(0, textured)) == want
    finally:
        be.release()


def test_the_accepted_update_on_20000_triangles_equals_a_fresh_upload():
    base, textured = screen_base()
    want = rendered("tris20k_textured", E.edited(base, materiaux=textured), depth=5)
    assert differs(want, rendered("tris20k_with_texture", base, depth=5))
    be = context(base, depth=5)
    try:
        be.render(0, 2)
        info = be.update_materials(0, textured)
        assert_same(after(be), want)
    finally:
        be.release()
    assert info["screened_triangles"] == 20000 and (info["plain_before"], info["plain_after"]) == (1, 0)


def test_the_table_of_the_triangle_updates_follows():
    base, textured = screen_base()
    bad = E.with_bad_coordinate(base.triangulation, 5, np.nan)
    refusal = (E.BAD_SCENE, E.message((5 << 4) | E.TEXCOORD))
    be = context(base)
    try:
        assert outcome(lambda: update_device(be, bad)) == (0, "")  # the material is a plain colour: accepted
        update_device(be, base.triangulation)
        be.update_materials(0, textured)
        assert outcome(lambda: update_device(be, bad)) == refusal
        assert outcome(lambda: be.update_triangles(bad)) == refusal
        update_device(be, base.triangulation)
        # ... and back: plain again, the records are accepted again
        be.update_materials(0, base.materiaux)
        assert outcome(lambda: update_device(be, bad)) == (0, "")
        assert outcome(lambda: be.update_triangles(bad)) == (0, "")
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_scene_alone():
    tex = scene("feat_textured")
    n_mats = len(tex.materiaux)
    bad_id = U.raw_copy(tex.materiaux[BALL:BALL + 1])
    bad_id["textureId"] = len(tex.textures)
    whole = U.raw_copy(tex.materiaux)
    whole["textureId"][BALL] = -1
    nan_light = U.raw_copy(tex.lights)
    nan_light["position"][0] = np.float32([np.nan, 0, 0, 1])
    far_light = U.raw_copy(tex.lights)
    far_light["direction"][0] = np.float32([0, E.up(2.0 ** 21), 0, 0])
    two_lights = np.frombuffer(tex.lights.tobytes() * 2, dtype=S.Light)
    bad_sky = tex.sky.copy()
    bad_sky["skyTextures"][4] = (2, 2, len(tex.texturesData) - 3)
    baseline = rendered("feat_textured", tex)
    be = context(tex)
    try:
        def refused(call, want):
            got = outcome(call)
            assert got[0] == want[0] and (want[1] is None or got[1] == want[1]), (got, want)
            assert len(got[1]) > 0
            assert_same(after(be), baseline)

        with_bad_id = U.raw_copy(tex.materiaux)
        with_bad_id["textureId"][BALL] = len(tex.textures)
        refused(lambda: be.update_materials(BALL, bad_id), validated(E.edited(tex, materiaux=with_bad_id)))
        assert outcome(lambda: be.update_materials(BALL, bad_id)) == (E.BAD_SCENE, f"material {BALL} has an invalid textureId")
        refused(lambda: be.update_materials(0, whole), validated(E.edited(tex, materiaux=whole)))
        refused(lambda: be.update_materials(n_mats - 1, tex.materiaux[:2]), (E.INVALID_ARGUMENT, None))
        refused(lambda: be.update_materials(n_mats + 1, tex.materiaux[:0]), (E.INVALID_ARGUMENT, None))
        refused(lambda: be.update_lights(two_lights), (E.INVALID_ARGUMENT, None))
        refused(lambda: be.update_lights(tex.lights[:0]), (E.INVALID_ARGUMENT, None))
        refused(lambda: be.update_lights(nan_light), (E.UNSUPPORTED, None))
        assert "light 0 is not finite (or beyond 2^21)" in outcome(lambda: be.update_lights(nan_light))[1]
        refused(lambda: be.update_lights(far_light), (E.UNSUPPORTED, None))
        refused(lambda: be.set_sky(bad_sky), validated(E.edited(tex, sky=bad_sky)))
        assert outcome(lambda: be.set_sky(bad_sky)) == (E.BAD_SCENE, "sky texture 4 outside textures_data")
        # ... and good edits still work after the refused ones
        other = scene("feat_spot")
        be.update_lights(other.lights)
        assert_same(after(be), rendered("feat_textured+spot", E.edited(tex, lights=other.lights)))
    finally:
        be.release()


def test_a_scene_with_a_literal_kernel_reason():
    """Zero-area triangles: a lights update is refused as a triangle update is (the reason may be a light's); materials cannot
    make a distance a NaN, nor can the sky, so those two are served."""
    base = scene("cornell")
    sc = bvh_create(scenes.add_zero_area_triangles(base, 3))
    mats = U.raw_copy(sc.materiaux)
    mats["type"][0] = S.MAT_METAL
    mats["simpleColor"][1] = np.float32([0.2, 0.9, 0.9, 0])
    sky = sc.sky.copy()
    sky["groundScale"] = 2.5
    sky["cosRotationAngle"], sky["sinRotationAngle"] = np.float32(np.cos(0.4)), np.float32(np.sin(0.4))
    baseline = rendered("cornell+3za", sc)
    want = rendered("cornell+3za+edits", E.edited(sc, materiaux=mats, sky=sky))
    assert differs(baseline, want)
    be = context(sc)
    try:
        assert be.literal_kernel_reason()
        got = outcome(lambda: be.update_lights(sc.lights))
        assert got[0] == E.UNSUPPORTED and "NaN distances" in got[1]
        assert_same(after(be), baseline)
        be.update_materials(0, mats)
        be.set_sky(sky)
        assert_same(after(be), want)
    finally:
        be.release()


def test_the_edits_before_initialize_memory_are_state_errors():
    sc = scene("feat_plain")
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        for call, name in ((lambda: be.update_materials(0, sc.materiaux), "ptmi_update_materials"), (lambda: be.update_lights(sc.lights), "ptmi_update_lights"),
                           (lambda: be.set_sky(sc.sky), "ptmi_set_sky")):
            with pytest.raises(PtmiError) as e:
                call()
            assert e.value.code == E.STATE and name + " before ptmi_initialize_memory" in str(e.value)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- what has been rendered, devices, render-ahead

def three_edits():
    """feat_textured's stage with all materials plain -> textured materials, a spot light, another sky rotation"""
    tex, flat, _ = textured_scenes()
    sky = tex.sky.copy()
    sky["groundScale"] = 2.0
    new = dict(materiaux=tex.materiaux, lights=scene("feat_spot").lights, sky=sky)

    def apply(be):
        be.update_materials(0, new["materiaux"])
        be.update_lights(new["lights"])
        be.set_sky(new["sky"])
    return flat, E.edited(flat, **new), apply


def test_the_edits_touch_nothing_that_has_been_rendered():
    flat, edited, apply = three_edits()
    be = context(flat)
    try:
        be.render(0, 2)
        before = state(be)
        apply(be)
        assert_same(state(be), before)
        be.render(2, 2)
        got = state(be)
    finally:
        be.release()
    yard = context(edited)
    try:
        yard.write_image(before["color"].view(np.float32), before["count"])
        yard.render(2, 2)
        want = state(yard)
    finally:
        yard.release()
    assert np.array_equal(got["color"], want["color"]) and np.array_equal(got["count"], want["count"])
    assert got["counters"] == {k: before["counters"][k] + want["counters"][k] for k in want["counters"]}


def test_two_listed_devices():
    flat, edited, apply = three_edits()
    want = rendered("three_edits", edited, n=5, devices=[0, 0])
    assert differs(want, rendered("textured_flat", flat, n=5, devices=[0, 0]))
    be = context(flat, devices=[0, 0])
    try:
        be.render(0, 3)
        apply(be)
        assert_same(after(be, n=5), want)
    finally:
        be.release()


def test_the_edits_under_render_ahead(monkeypatch):
    """The blocking one-iteration-per-call caller that is rendered ahead of: what ran ahead for the old scene is dropped."""
    monkeypatch.setenv("PTMI_RENDER_AHEAD", "2")
    flat, edited, apply = three_edits()

    def walk(be, first, n):
        for k in range(first, first + n):
            be.render(k, 1)
            be.synchronize()

    be = context(flat)
    try:
        walk(be, 0, 6)
        before = state(be)
        apply(be)
        walk(be, 6, 6)
        got = state(be)
    finally:
        be.release()
    yard = context(edited)
    try:
        yard.write_image(before["color"].view(np.float32), before["count"])
        walk(yard, 6, 6)
        want = state(yard)
    finally:
        yard.release()
    assert np.array_equal(got["color"], want["color"]) and np.array_equal(got["count"], want["count"])
    assert got["counters"] == {k: before["counters"][k] + want["counters"][k] for k in want["counters"]}
    assert differs(got, before)
