"""ptmi_bind_mesh / ptmi_update_vertices(_device): a loaded scene's triangles updated from vertex buffers and a bound topology.

The yardstick is code that existed before the calls did, applied to the NumPy restatement of the record (vertex_update_cases.py):
after an update the context holds, word for word, build_layout's arrays for (the restated records, ptmi_bvh_refit's tree), read
back with the probe of test_scene_records_gpu.py; and every refusal is the one ptmi_update_triangles gives for the restated
records on a second context, message and triangle index included.  Nothing is compared against a scene's uploaded records: a
round trip through an indexed mesh does not reproduce N's last bit.
"""
import ctypes as C
import types

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend
from gpu_cases import assert_same_state, bytes_of, state
import gpu_cases
import scene_record_cases as R
import scene_update_cases as U
import update_screen_cases as X
import vertex_update_cases as V

pytestmark = pytest.mark.gpu
W, H = R.W, R.H
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
ARITHMETICS = [pytest.param(0, id="strict"), pytest.param(DA, id="default")]
RECORD_FORMS = [pytest.param(False, id="precomputed"), pytest.param(True, id="generic")]
PREFIXES = ("ptmi_update_triangles: ", "ptmi_update_vertices_device: ", "ptmi_update_vertices: ", "ptmi_bind_mesh: ")
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def tools():
    gpu_cases.require_probe_tools()


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, **kw)


def on_device(a, stride=12):
    """The (V, 3) array as a float32 (V, stride / 4) torch tensor on the device, NaN in every word of padding"""
    t = gpu_cases.tensor_on_device(V.padded(a, stride).base)
    assert t.data_ptr() % 16 == 0
    return t


def update_device(be, m, stride=12):
    """update_vertices_device of mesh `m`'s buffers from torch tensors, which must come back unchanged.  Returns the info dict."""
    p = on_device(m.positions, stride)
    n = None if m.normals is None else on_device(m.normals, stride)
    kept = [bytes_of(p), None if n is None else bytes_of(n)]
    try:
        return be.update_vertices_device(len(m.positions), p.data_ptr(), None if n is None else n.data_ptr(), stride, stride)
    finally:
        assert bytes_of(p) == kept[0] and (n is None or bytes_of(n) == kept[1]), "the caller's buffer was written"


def update_host(be, m, stride=12):
    return be.update_vertices(V.padded(m.positions, stride), None if m.normals is None else V.padded(m.normals, stride))


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


def assert_holds(be, want, what, device_index=0):
    got = R.read_records(be, want, device_index)
    msg = R.describe_difference(got, want, what)
    assert msg == "", msg
    return got


def expected(lay, tris, flags):
    return R.with_default_arithmetic_denominators(lay, tris) if flags & DA else lay


def the_motion(name):
    return V.moved(name, perturb_normals=name == "feat_textured")


_wanted = {}


def wanted(name, generic=False):
    """(the restated records of the moved mesh of scene `name`, build_layout's arrays for them and ptmi_bvh_refit's tree), once"""
    if (name, generic) not in _wanted:
        tris = V.restate(the_motion(name))[0]
        _wanted[name, generic] = tris, R.layout_in_mode(U.moved_scene(R.scene(name), tris), generic)
    return _wanted[name, generic]


# ---------------------------------------------------------------------------------------------- records after an update

@pytest.mark.parametrize("generic", RECORD_FORMS)
@pytest.mark.parametrize("flags", ARITHMETICS)
@pytest.mark.parametrize("name", ["cornell", "big_leaf", "empty_leaves", "feat_textured", "signed_zero-s0", "tris20k"])
def test_a_vertex_update_holds_the_layout_of_a_fresh_upload(name, flags, generic, monkeypatch):
    if generic:
        monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    else:
        monkeypatch.delenv("PTMI_GENERIC_TRIANGLES", raising=False)
    sc = R.scene(name)
    tris, host_new = wanted(name, generic)
    old = expected(R.cached_layout(name, generic), sc.triangulation, flags)
    new = expected(host_new, tris, flags)
    if name == "tris20k":
        assert len(tris) % 64 == 32 and len(tris) % 256 == 32  # a ragged last wave and workgroup
    be = context(sc, flags=flags)
    try:
        before = assert_holds(be, old, f"{name} before the update")
        be.bind_mesh(V.derived(name))
        assert_holds(be, old, f"{name} after ptmi_bind_mesh")
        info = update_device(be, the_motion(name))
        after = assert_holds(be, new, f"{name} after ptmi_update_vertices_device")
    finally:
        be.release()
    assert not np.array_equal(before["recs"], after["recs"])
    assert np.array_equal(after["tri_ids"], before["tri_ids"]) and np.array_equal(after["big_leaves"], before["big_leaves"])
    assert info["struct_size"] == 40 and info["levels"] == int(host_new["info"][5])
    assert info["upload_ms"] == 0 and info["validate_ms"] > 0 and info["device_ms"] > 0 and info["total_ms"] >= info["validate_ms"]


def test_a_flat_update_takes_its_normals_from_the_plane():
    sc = R.scene("cornell")
    flat = V.with_buffers(the_motion("cornell"), normals=None)
    tris = V.restate(flat)[0]
    new = R.layout_in_mode(U.moved_scene(sc, tris), False)
    be = context(sc)
    try:
        be.bind_mesh(V.derived("cornell"))
        update_device(be, flat)
        assert_holds(be, new, "after a device update without a normal buffer")
        update_host(be, flat)
        assert_holds(be, new, "after a host update without a normal buffer")
    finally:
        be.release()


# what ptmi.h lets a topology leave out, each on its own and all at once: the 24-byte layout without texture-coordinate planes
# (and its tail plane at another offset), uvp NULL = zeros beside a given uvn, uvn NULL = uvp, mat_neg NULL = mat_pos, ids NULL = i
LEFT_OUT = [("uvp", "uvn"), ("uvp",), ("uvn",), ("mat_neg",), ("ids",), ("uvp", "uvn", "mat_neg", "ids")]


@pytest.mark.parametrize("left_out", LEFT_OUT, ids=["-".join(x) for x in LEFT_OUT])
@pytest.mark.parametrize("name", ["feat_textured", "tris20k"])
def test_a_bind_with_defaults_holds_the_layout_of_the_restatement(name, left_out):
    sc = R.scene(name)
    m = edited(the_motion(name), **{field: None for field in left_out})
    if "mat_neg" in left_out:  # (so that the default shows: the back of every triangle gets another material than its front)
        m.mat_pos = ((m.mat_pos + 1) % len(sc.materiaux)).astype(np.uint32)
    tris = V.restate(m)[0]
    if "uvp" in left_out:
        assert not tris["UVP1"].any() and ("uvn" in left_out or name != "feat_textured" or tris["UVN1"].any())
    new = R.layout_in_mode(U.moved_scene(sc, tris), False)
    be = context(sc)
    try:
        be.bind_mesh(m)
        update_device(be, m)
        assert_holds(be, new, f"{name} bound without {left_out}, device form")
        be.update_triangles(sc.triangulation)
        update_host(be, m)
        assert_holds(be, new, f"{name} bound without {left_out}, host form")
    finally:
        be.release()


def test_interleaved_host_buffers_that_end_with_the_last_normal():
    """positions and normals as two views of one (V, 6) array, stride 24: the normals' last row ends the allocation"""
    sc = R.scene("feat_textured")
    m = the_motion("feat_textured")
    _, new = wanted("feat_textured")
    both = np.ascontiguousarray(np.concatenate([m.positions, m.normals], axis=1), f32)
    be = context(sc)
    try:
        be.bind_mesh(m)
        be.update_vertices(both[:, :3], both[:, 3:])
        assert_holds(be, new, "after a host update from interleaved buffers")
    finally:
        be.release()


@pytest.mark.parametrize("name", ["feat_textured", "tris20k"])
def test_host_form_and_device_form_leave_the_same_bytes(name):
    sc = R.scene(name)
    _, new = wanted(name)
    a, b = context(sc), context(sc)
    try:
        for be in (a, b):
            be.bind_mesh(V.derived(name))
        info = update_host(a, the_motion(name))
        update_device(b, the_motion(name))
        got = [assert_holds(be, new, f"{name} after the {who} form") for be, who in ((a, "host"), (b, "device"))]
        assert R.same_arrays(got[0], got[1])
        assert info["upload_ms"] > 0 and info["device_ms"] > 0 and info["total_ms"] >= info["upload_ms"]
    finally:
        a.release()
        b.release()


# ---------------------------------------------------------------------------------------------- verdict parity

def edited(m, **arrays):
    out = types.SimpleNamespace(**vars(m))
    for key, value in arrays.items():
        setattr(out, key, value)
    return out


def defect(m, kind, at, textured=None):
    """Mesh `m` with one defect at each triangle of `at`: in the topology (rebound by the caller) or in the vertex buffers"""
    idx, pos, nrm, uvp, mat = m.indices.copy(), m.positions.copy(), m.normals.copy(), m.uvp.copy(), m.mat_pos.copy()
    for i in at:
        if kind == "duplicate_index":
            idx[i, 2] = idx[i, 1]
        elif kind == "nan_vertex":
            pos[idx[i, 0], 1] = np.nan
        elif kind == "beyond_2_21":
            pos[idx[i, 2], 0] = np.nextafter(f32(2.0 ** 21), f32(np.inf))
        elif kind == "nan_normal":
            nrm[idx[i, 1], 2] = np.nan
        elif kind == "material_out_of_range":
            mat[i] = 0x7FFFFFFF
        elif kind == "infinite_texture_coordinate":
            uvp[i, 1, 0] = np.inf
            if textured is not None:
                mat[i] = textured
    return edited(m, indices=idx, positions=pos, normals=nrm, uvp=uvp, mat_pos=mat)


DEFECTS = ["duplicate_index", "nan_vertex", "beyond_2_21", "nan_normal", "material_out_of_range", "infinite_texture_coordinate"]
PLACES = {"feat_textured": lambda n: [0, n // 2, n - 1], "tris20k": lambda n: [0, 63, 64, 255, 256, n - 1]}


@pytest.fixture(scope="module")
def pairs():
    """Per base scene two contexts - the new forms' and ptmi_update_triangles' - and the records both hold, kept for the module."""
    made = {}

    def get(name):
        if name not in made:
            sc = R.scene(name)
            made[name] = dict(new=context(sc), old=context(sc), held=R.cached_layout(name, False))
        return made[name]
    yield get
    for p in made.values():
        p["new"].release()
        p["old"].release()


def verdicts(pair, m, what):
    """Bind `m`, update through both new forms, and hold status, message and what the context then holds to
    ptmi_update_triangles of the restated records on the second context.  Returns the common (status, message)."""
    tris = V.restate(m)[0]
    pair["new"].bind_mesh(m)
    want = outcome(lambda: pair["old"].update_triangles(tris))
    for form, update in (("device", update_device), ("host", update_host)):
        got = outcome(lambda: update(pair["new"], m))
        assert got == want, (what, form, got, want)
    a, b = R.read_records(pair["new"], pair["held"]), R.read_records(pair["old"], pair["held"])
    msg = R.describe_difference(a, b, f"{what}: the new forms' context against ptmi_update_triangles'")
    assert msg == "", msg
    if want[0] != 0:
        msg = R.describe_difference(a, pair["held"], f"{what}: after the refusal")
        assert msg == "", msg
    else:
        pair["held"] = dict(a, info=pair["held"]["info"])
    return want


@pytest.mark.parametrize("kind", DEFECTS)
@pytest.mark.parametrize("name", ["feat_textured", "tris20k"])
def test_the_verdict_is_that_of_update_triangles_for_the_assembled_records(pairs, name, kind):
    sc = R.scene(name)
    facts = X.Facts.of(sc, precomputed=True)
    textured = facts.material(True)
    if name == "feat_textured":
        assert textured is not None
    pair = pairs(name)
    base = the_motion(name)
    for at in PLACES[name](len(base.indices)):
        m = defect(base, kind, [at], textured)
        got = verdicts(pair, m, f"{name}: {kind} at {at}")
        # ... and both are what the NumPy restatement of the screen says of the restated records
        codes = X.codes(V.restate(m)[0], facts)
        refused = np.flatnonzero(codes != X.OK)
        if kind == "infinite_texture_coordinate" and textured is None:
            assert len(refused) == 0 and got == (0, "")  # (no material of this scene reads texture coordinates)
            continue
        first = int(refused[0])
        assert got == (X.STATUS[int(codes[first])], X.message((first << 4) | int(codes[first]))), (kind, at, got)
        if name == "tris20k":
            assert first == at  # (no vertex of this mesh is shared: the defect is triangle `at`'s alone)


def test_of_two_defective_triangles_the_first_is_named(pairs):
    pair = pairs("tris20k")
    base = the_motion("tris20k")
    got = verdicts(pair, defect(base, "nan_vertex", [19000, 300]), "two NaN vertices")
    assert got == (UNSUPPORTED, X.message((300 << 4) | X.VERTEX))
    m = defect(defect(base, "nan_vertex", [19000]), "material_out_of_range", [19001])
    got = verdicts(pair, m, "a NaN vertex, then a material out of range")
    assert got == (UNSUPPORTED, X.message((19000 << 4) | X.VERTEX))


# ---------------------------------------------------------------------------------------------- arguments and state

def raw_bind(be, m, edit=None, null=False):
    t, keep = backend.mesh_topology(m)
    if edit:
        edit(t)
    be._check(be._lib.ptmi_bind_mesh(be._ctx, None if null else C.byref(t)))


def raw_update(be, device_form, buffers):
    info = backend.UpdateInfo()
    call = be._lib.ptmi_update_vertices_device if device_form else be._lib.ptmi_update_vertices
    be._check(call(be._ctx, None if buffers is None else C.byref(buffers), C.byref(info)))


def test_every_argument_and_state_refusal_leaves_every_byte():
    sc = R.scene("cornell")
    m = the_motion("cornell")
    old = R.cached_layout("cornell", False)
    nv, nt = len(m.positions), len(m.indices)
    p, n = on_device(m.positions), on_device(m.normals)
    host_p, host_n = np.ascontiguousarray(m.positions), np.ascontiguousarray(m.normals)

    def buffers(device_form, **edits):
        b = backend.VertexBuffers(C.sizeof(backend.VertexBuffers), nv, 12, 12, p.data_ptr() if device_form else host_p.ctypes.data,
                                  n.data_ptr() if device_form else host_n.ctypes.data)
        for key, value in edits.items():
            setattr(b, key, value)
        return b

    be = context(sc)
    try:
        for device_form in (True, False):
            assert outcome(lambda: raw_update(be, device_form, buffers(device_form))) == (STATE, "no mesh is bound (ptmi_bind_mesh)")
        bad_index = m.indices.copy()
        bad_index[7, 2] = nv
        for edit, words in ((lambda t: setattr(t, "struct_size", 56), "topology is NULL or struct_size mismatch (ABI)"),
                            (lambda t: setattr(t, "reserved", 7), "topology.reserved is not 0"),
                            (lambda t: setattr(t, "n_triangles", nt - 1), f"{nt - 1} triangles, the context holds {nt} (the topology is that of the uploaded array)"),
                            (lambda t: setattr(t, "n_vertices", 0), "n_vertices is 0"),
                            (lambda t: setattr(t, "indices", None), "indices is NULL"),
                            (lambda t: setattr(t, "mat_pos", None), "mat_pos is NULL"),
                            (lambda t: setattr(t, "indices", bad_index.ctypes.data), f"triangle 7 corner 2: index {nv}, the mesh has {nv} vertices")):
            assert outcome(lambda: raw_bind(be, m, edit)) == (INVALID_ARGUMENT, words)
        for device_form in (True, False):  # (a refused bind binds nothing)
            assert outcome(lambda: raw_update(be, device_form, buffers(device_form))) == (STATE, "no mesh is bound (ptmi_bind_mesh)")
        assert_holds(be, old, "after the refused binds")
        be.bind_mesh(V.derived("cornell"))
        common = [(None, "vertex buffers are NULL or struct_size mismatch (ABI)"),
                  (dict(struct_size=28), "vertex buffers are NULL or struct_size mismatch (ABI)"),
                  (dict(n_vertices=nv + 1), f"{nv + 1} vertices, the mesh has {nv}"),
                  (dict(position_stride=8), "position_stride is 8 (bytes: at least 12, a multiple of 4)"),
                  (dict(position_stride=18), "position_stride is 18 (bytes: at least 12, a multiple of 4)"),
                  (dict(normal_stride=0), "normal_stride is 0 (bytes: at least 12, a multiple of 4)"),
                  (dict(positions=None), "positions is NULL")]
        for device_form in (True, False):
            for edits, words in common:
                b = None if edits is None else buffers(device_form, **edits)
                assert outcome(lambda: raw_update(be, device_form, b)) == (INVALID_ARGUMENT, words), (device_form, words)
        for edits, words in ((dict(positions=p.data_ptr() + 4), "positions is not 16-byte aligned"),
                             (dict(normals=n.data_ptr() + 8), "normals is not 16-byte aligned")):
            assert outcome(lambda: raw_update(be, True, buffers(True, **edits))) == (INVALID_ARGUMENT, words)
        assert_holds(be, old, "after the refused updates")
        # a bind is scene memory: it goes with ptmi_initialize_memory, and with an unbind
        be.initialize_memory(sc)
        assert outcome(lambda: raw_update(be, True, buffers(True))) == (STATE, "no mesh is bound (ptmi_bind_mesh)")
        be.bind_mesh(V.derived("cornell"))
        be.bind_mesh(V.derived("cornell"))  # (a second bind replaces the first)
        be.bind_mesh(None)
        assert outcome(lambda: raw_update(be, False, buffers(False))) == (STATE, "no mesh is bound (ptmi_bind_mesh)")
        assert_holds(be, old, "after binds and unbinds")
    finally:
        be.release()
    assert bytes_of(p) == host_p.tobytes() and bytes_of(n) == host_n.tobytes()


def test_calls_before_initialize_memory_are_state_errors():
    sc = R.scene("cornell")
    m = V.derived("cornell")
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        with pytest.raises(PtmiError) as e:
            be.bind_mesh(m)
        assert e.value.code == STATE and "ptmi_bind_mesh before ptmi_initialize_memory" in str(e.value)
        for call, who in ((lambda: update_device(be, m), "ptmi_update_vertices_device"), (lambda: update_host(be, m), "ptmi_update_vertices")):
            with pytest.raises(PtmiError) as e:
                call()
            assert e.value.code == STATE and who + " before ptmi_initialize_memory" in str(e.value)
    finally:
        be.release()


def test_deep_chain_27_is_refused_as_a_whole():
    sc = R.scene("deep_chain_27")
    want = R.cached_layout("deep_chain_27", False)
    be = context(sc)
    try:
        be.bind_mesh(V.derived("deep_chain_27"))
        for m in (V.derived("deep_chain_27"), V.moved("deep_chain_27")):
            for update in (update_device, update_host):
                got = outcome(lambda: update(be, m))
                assert got[0] == UNSUPPORTED and "NaN distances" in got[1]
                assert got == outcome(lambda: be.update_triangles(V.restate(m)[0]))
            assert_holds(be, want, "deep_chain_27 after the refused update")
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- strides

@pytest.mark.parametrize("stride", V.STRIDES)
def test_strides_with_nan_in_the_padding_give_the_same_records(stride):
    sc = R.scene("cornell")
    _, new = wanted("cornell")
    be = context(sc)
    try:
        be.bind_mesh(V.derived("cornell"))
        update_device(be, the_motion("cornell"), stride)
        assert_holds(be, new, f"after a device update at stride {stride}")
        be.update_triangles(sc.triangulation)
        update_host(be, the_motion("cornell"), stride)
        assert_holds(be, new, f"after a host update at stride {stride}")
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- context variants

def test_both_listed_devices_hold_the_same_records():
    sc = R.scene("cornell")
    _, new = wanted("cornell")
    be = context(sc, devices=[0, 0])
    try:
        be.bind_mesh(V.derived("cornell"))
        info = update_device(be, the_motion("cornell"))
        got = [assert_holds(be, new, f"listed device {i} after the update", device_index=i) for i in (0, 1)]
        assert got[0]["n_devices"] == 2 and R.same_arrays(got[0], got[1])
        assert info["upload_ms"] > 0  # (the copy to the second listed device)
    finally:
        be.release()


def test_a_vertex_update_under_render_ahead(monkeypatch):
    monkeypatch.setenv("PTMI_RENDER_AHEAD", "2")
    sc = R.scene("cornell")
    _, new = wanted("cornell")
    be = context(sc)
    try:
        be.bind_mesh(V.derived("cornell"))
        for k in range(4):
            be.render(k, 1)
            be.synchronize()
        update_device(be, the_motion("cornell"))
        assert_holds(be, new, "after a vertex update under PTMI_RENDER_AHEAD=2")
        be.render(4, 1)
        assert_holds(be, new, "after one more iteration")
    finally:
        be.release()


def test_records_form_vertex_form_host_records_form_on_one_context():
    sc = R.scene("tris20k")
    tris1 = U.displaced(sc.triangulation, seed=1, amplitude=0.01)
    tris2, want2 = wanted("tris20k")
    tris3 = U.displaced(tris2, seed=3, amplitude=0.01)
    once = U.moved_scene(sc, tris1)
    twice = U.moved_scene(once, tris2)
    wants = [R.layout_in_mode(s, False) for s in (once, twice, U.moved_scene(twice, tris3))]
    be = context(sc)
    try:
        be.bind_mesh(V.derived("tris20k"))
        # (the records form reads a torch tensor of the 336-byte records)
        t = gpu_cases.tensor_on_device(np.frombuffer(bytearray(tris1.tobytes()), f32).reshape(len(tris1), 84))
        be.update_triangles_device(t.data_ptr(), len(tris1))
        assert_holds(be, wants[0], "after the records form")
        update_device(be, the_motion("tris20k"))
        assert_holds(be, wants[1], "after the vertex form")
        be.update_triangles(tris3)
        assert_holds(be, wants[2], "after the host records form")
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- renders

@pytest.mark.parametrize("flags", ARITHMETICS)
def test_render_update_clear_render_equals_a_fresh_context(flags):
    sc = R.scene("cornell")
    tris, _ = wanted("cornell")
    be = context(sc, flags=flags)
    try:
        be.bind_mesh(V.derived("cornell"))
        be.render(0, 3)
        before = state(be)
        update_device(be, the_motion("cornell"))
        assert_same_state(state(be), before)  # the update itself touched nothing that was rendered
        be.clear()
        be.render(0, 3)
        got = state(be)
    finally:
        be.release()
    fresh = context(U.moved_scene(sc, tris), flags=flags)
    try:
        fresh.render(0, 3)
        assert_same_state(got, state(fresh))
    finally:
        fresh.release()
