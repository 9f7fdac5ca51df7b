"""ptmi_update_triangles_device: a loaded scene's triangles updated from records that are on the device already.

Two yardsticks, both code that existed before the call did.  After an update the context holds, word for word, build_layout's
arrays for (new triangles, ptmi_bvh_refit's tree), read back with the probe of test_scene_records_gpu.py.  And on every record
the screen kernel gives the verdict of the host loop: the device form returns the status and the message ptmi_update_triangles
returns for the same records on a second context (after the entry point's name), the refused triangle's index included, and
leaves the bytes it leaves.  Every comparison is byte for byte or string for string.
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend
from gpu_cases import assert_same_state, bytes_of, state
import gpu_cases
import scene_record_cases as R
import scene_update_cases as U
import update_screen_cases as X

pytestmark = pytest.mark.gpu
W, H = R.W, R.H
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
ARITHMETICS = [pytest.param(0, id="strict"), pytest.param(DA, id="default")]
RECORD_FORMS = [pytest.param(False, id="precomputed"), pytest.param(True, id="generic")]
HOST, DEVICE = "ptmi_update_triangles: ", "ptmi_update_triangles_device: "


@pytest.fixture(scope="module", autouse=True)
def tools():
    gpu_cases.require_probe_tools()


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, **kw)


def on_device(tris):
    """The records as a float32 (n, 84) torch tensor on the device (a byte copy: the payload of a NaN travels as it is)"""
    t = gpu_cases.tensor_on_device(np.frombuffer(bytearray(np.ascontiguousarray(tris).tobytes()), np.float32).reshape(len(tris), 84))
    assert t.data_ptr() % 16 == 0
    return t


def update_device(be, tris):
    """update_triangles_device of `tris` from a torch tensor, which must come back unchanged.  Returns the info dict."""
    t = on_device(tris)
    try:
        return be.update_triangles_device(t.data_ptr(), len(tris))
    finally:
        assert bytes_of(t) == np.ascontiguousarray(tris).tobytes(), "the caller's buffer was written"


def outcome(call):
    """(status, message after the entry point's name) of a call that may refuse"""
    try:
        call()
        return 0, ""
    except PtmiError as e:
        text = str(e).split(": ", 1)[1]
        for prefix in (HOST, DEVICE):
            if text.startswith(prefix):
                return e.code, text[len(prefix):]
        return e.code, text


def assert_holds(be, want, what, device_index=0):
    got = R.read_records(be, want, device_index)
    msg = R.describe_difference(got, want, what)
    assert msg == "", msg
    return got


def expected(lay, tris, flags):
    return R.with_default_arithmetic_denominators(lay, tris) if flags & DA else lay


# ---------------------------------------------------------------------------------------------- records after an update

@pytest.mark.parametrize("generic", RECORD_FORMS)
@pytest.mark.parametrize("flags", ARITHMETICS)
@pytest.mark.parametrize("name", ["cornell", "big_leaf", "empty_leaves", "feat_textured", "signed_zero-s0", "tris20k"])
def test_a_device_update_holds_the_layout_of_a_fresh_upload(name, flags, generic, monkeypatch):
    if generic:
        monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    else:
        monkeypatch.delenv("PTMI_GENERIC_TRIANGLES", raising=False)
    sc = R.scene(name)
    tris = U.moved_triangles(sc, name)
    host_new = R.layout_in_mode(U.moved_scene(sc, tris), generic)
    old = expected(R.cached_layout(name, generic), sc.triangulation, flags)
    new = expected(host_new, tris, flags)
    if name == "tris20k":
        assert len(tris) % 64 == 32 and len(tris) % 256 == 32  # a ragged last wave and workgroup
    be = context(sc, flags=flags)
    try:
        before = assert_holds(be, old, f"{name} before the update")
        assert not np.array_equal(before["recs"], new["recs"])
        info = update_device(be, tris)
        after = assert_holds(be, new, f"{name} after ptmi_update_triangles_device")
    finally:
        be.release()
    assert np.array_equal(after["tri_ids"], before["tri_ids"]) and np.array_equal(after["big_leaves"], before["big_leaves"])
    assert info["struct_size"] == 40 and info["levels"] == int(host_new["info"][5])
    assert info["upload_ms"] == 0 and info["validate_ms"] > 0 and info["device_ms"] > 0 and info["total_ms"] >= info["validate_ms"]


# ---------------------------------------------------------------------------------------------- verdict parity

PLACES = {"feat_textured": lambda n: [0, n // 2, n - 1], "tris20k": lambda n: [0, 63, 64, 255, 256, n - 1]}


@pytest.fixture(scope="module")
def pairs():
    """Per base scene two contexts - the device form's and the host form's - and the records both hold, kept for the module."""
    made = {}

    def get(name):
        if name not in made:
            sc = R.scene(name)
            made[name] = dict(dev=context(sc), host=context(sc), held=R.cached_layout(name, False))
        return made[name]
    yield get
    for p in made.values():
        p["dev"].release()
        p["host"].release()


def targets_of(case, places):
    return [[i] for i in places] if case.targets == 1 else [list(places[k:k + 2]) for k in range(0, len(places) - 1, 2)]


@pytest.mark.parametrize("case", [c.name for c in X.CASES])
@pytest.mark.parametrize("name", ["feat_textured", "tris20k"])
def test_the_device_verdict_is_the_host_verdict(pairs, name, case):
    case = X.BY_NAME[case]
    sc = R.scene(name)
    facts = X.Facts.of(sc, precomputed=bool(R.cached_layout(name, False)["info"][4]))
    assert facts.precomputed
    if name == "feat_textured":
        assert facts.material(True) is not None
    pair = pairs(name)
    for at in targets_of(case, PLACES[name](len(sc.triangulation))):
        tris = case.apply(sc.triangulation, at, facts)
        want_word = case.word(at, facts)
        got_dev = outcome(lambda: update_device(pair["dev"], tris))
        got_host = outcome(lambda: pair["host"].update_triangles(tris))
        assert got_dev == got_host, (case.name, at, got_dev, got_host)
        if want_word == X.ACCEPTED:
            assert got_dev == (0, ""), (case.name, at, got_dev)
            a = R.read_records(pair["dev"], pair["held"])
            b = R.read_records(pair["host"], pair["held"])
            msg = R.describe_difference(a, b, f"{case.name} at {at}: device form against host form")
            assert msg == "", msg
            pair["held"] = dict(a, info=pair["held"]["info"])
        else:
            assert got_dev == (X.STATUS[want_word & 15], X.message(want_word)), (case.name, at, got_dev)
            for be, who in ((pair["dev"], "device"), (pair["host"], "host")):
                assert_holds(be, pair["held"], f"{case.name} at {at}: the {who} form's context after the refusal")


def test_of_two_defective_triangles_the_first_is_named(pairs):
    sc = R.scene("tris20k")
    facts = X.Facts.of(sc)
    pair = pairs("tris20k")
    case = X.BY_NAME["later_triangle_earlier_check"]
    tris = case.apply(sc.triangulation, [300, 19000], facts)
    assert X.codes(tris, facts)[19000] == X.VERTEX  # (an earlier check than triangle 300's)
    got = outcome(lambda: update_device(pair["dev"], tris))
    assert got == (UNSUPPORTED, X.message((300 << 4) | X.EMPTY_BOX)) and got == outcome(lambda: pair["host"].update_triangles(tris))
    both = X.BY_NAME["nan_vertex_and_empty_box"].apply(sc.triangulation, [19000], facts)
    got = outcome(lambda: update_device(pair["dev"], both))
    assert got == (UNSUPPORTED, X.message((19000 << 4) | X.VERTEX)) and got == outcome(lambda: pair["host"].update_triangles(both))
    assert_holds(pair["dev"], pair["held"], "after the two refusals")


# ---------------------------------------------------------------------------------------------- arguments

def test_argument_refusals_leave_every_byte():
    sc = R.scene("cornell")
    tris = U.moved_triangles(sc, "cornell")
    old = R.cached_layout("cornell", False)
    n = len(tris)
    spare = np.frombuffer(tris.tobytes() + tris[:1].tobytes(), dtype=tris.dtype)  # (one record more than the context holds)
    t = on_device(spare)
    be = context(sc)
    try:
        for call, words in ((lambda: be.update_triangles_device(0, n), "d_triangulation is NULL"),
                            (lambda: be.update_triangles_device(t.data_ptr() + 8, n), "d_triangulation is not 16-byte aligned"),
                            (lambda: be.update_triangles_device(t.data_ptr(), n + 1), f"{n + 1} triangles, the context holds {n} (the topology cannot change)"),
                            (lambda: be.update_triangles_device(t.data_ptr(), n - 1), f"{n - 1} triangles, the context holds {n} (the topology cannot change)")):
            assert outcome(call) == (INVALID_ARGUMENT, words)
            assert_holds(be, old, "after a refused argument")
        assert outcome(lambda: be.update_triangles(spare)) == (INVALID_ARGUMENT, f"{n + 1} triangles, the context holds {n} (the topology cannot change)")
    finally:
        be.release()
    assert bytes_of(t) == spare.tobytes()


def test_a_call_before_initialize_memory_is_a_state_error():
    sc = R.scene("cornell")
    t = on_device(sc.triangulation)
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        with pytest.raises(PtmiError) as e:
            be.update_triangles_device(t.data_ptr(), len(sc.triangulation))
        assert e.value.code == STATE and "ptmi_update_triangles_device before ptmi_initialize_memory" in str(e.value)
    finally:
        be.release()


def test_deep_chain_27_is_refused_as_a_whole():
    sc = R.scene("deep_chain_27")
    want = R.cached_layout("deep_chain_27", False)
    be = context(sc)
    try:
        for tris in (sc.triangulation, U.displaced(sc.triangulation, 7)):
            got_dev = outcome(lambda: update_device(be, tris))
            assert got_dev[0] == UNSUPPORTED and "NaN distances" in got_dev[1]
            assert got_dev == outcome(lambda: be.update_triangles(tris))
            assert_holds(be, want, "deep_chain_27 after the refused update")
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- context variants

def test_both_listed_devices_hold_the_same_records():
    sc = R.scene("cornell")
    tris = U.moved_triangles(sc, "cornell")
    new = R.layout_in_mode(U.moved_scene(sc, tris), False)
    be = context(sc, devices=[0, 0])
    try:
        info = update_device(be, tris)
        got = [assert_holds(be, new, f"listed device {i} after the update", device_index=i) for i in (0, 1)]
        assert got[0]["n_devices"] == 2 and R.same_arrays(got[0], got[1])
        assert info["upload_ms"] > 0  # (the copy to the second listed device)
    finally:
        be.release()


def test_a_device_update_under_render_ahead(monkeypatch):
    monkeypatch.setenv("PTMI_RENDER_AHEAD", "2")
    sc = R.scene("cornell")
    tris = U.moved_triangles(sc, "cornell")
    new = R.layout_in_mode(U.moved_scene(sc, tris), False)
    be = context(sc)
    try:
        for k in range(4):
            be.render(k, 1)
            be.synchronize()
        update_device(be, tris)
        assert_holds(be, new, "after a device update under PTMI_RENDER_AHEAD=2")
        be.render(4, 1)
        assert_holds(be, new, "after one more iteration")
    finally:
        be.release()


def test_host_form_device_form_host_form_on_one_context():
    sc = R.scene("tris20k")
    tris1 = U.displaced(sc.triangulation, seed=1, amplitude=0.01)
    tris2 = U.displaced(tris1, seed=2, amplitude=0.01)
    tris3 = U.displaced(tris2, seed=3, amplitude=0.01)
    once = U.moved_scene(sc, tris1)
    twice = U.moved_scene(once, tris2)
    wants = [R.layout_in_mode(s, False) for s in (once, twice, U.moved_scene(twice, tris3))]
    be = context(sc)
    try:
        be.update_triangles(tris1)
        assert_holds(be, wants[0], "after the host form")
        update_device(be, tris2)
        assert_holds(be, wants[1], "after the device form")
        be.update_triangles(tris3)
        assert_holds(be, wants[2], "after the host form again")
    finally:
        be.release()


def test_a_context_that_only_ever_uses_the_device_form():
    """Two device updates and a refused one between them on a single-device context: no host form ever allocates its scratch."""
    sc = R.scene("tris20k")
    tris1 = U.displaced(sc.triangulation, seed=1, amplitude=0.01)
    tris2 = U.displaced(tris1, seed=2, amplitude=0.01)
    once = U.moved_scene(sc, tris1)
    want1, want2 = R.layout_in_mode(once, False), R.layout_in_mode(U.moved_scene(once, tris2), False)
    be = context(sc)
    try:
        first = update_device(be, tris1)
        assert_holds(be, want1, "after the first device update")
        assert outcome(lambda: update_device(be, U.bad_triangles(once, "empty_aabb")))[0] == UNSUPPORTED
        second = update_device(be, tris2)
        assert_holds(be, want2, "after the second device update")
    finally:
        be.release()
    assert first["levels"] == second["levels"] > 0 and first["upload_ms"] == second["upload_ms"] == 0


# ---------------------------------------------------------------------------------------------- invisible to renders

@pytest.mark.parametrize("flags", ARITHMETICS)
def test_render_device_update_render_on_equals_the_host_form(flags):
    sc = R.scene("cornell")
    tris = U.moved_triangles(sc, "cornell")

    def play(update):
        be = context(sc, flags=flags)
        try:
            be.render(0, 3)
            before = state(be)
            update(be)
            assert_same_state(state(be), before)  # the update itself touched nothing that was rendered
            be.render(3, 3)
            return state(be)
        finally:
            be.release()

    assert_same_state(play(lambda be: update_device(be, tris)), play(lambda be: be.update_triangles(tris)))
