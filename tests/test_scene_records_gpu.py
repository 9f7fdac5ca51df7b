"""The scene records a context holds on the device, read back and compared word for word.

DESIGN 1b promises that after ptmi_update_triangles a context holds, byte for byte, the records of a fresh upload of the new
triangles with ptmi_bvh_refit's tree.  A render sees the records its rays touch and cannot tell a -0 corner from a +0 one; here
the four arrays every kernel reads - the one array of node and triangle records, tri_ids, the shading records, big_leaves - are
copied back from every listed device (oracle/scene_record_probe.cpp: ptmi_synchronize and four copies, no kernel) and compared
as uint32 words, padding included, no tolerance, no record left out.

Yardstick: build_layout on the host (scene_record_cases.Model.layout: the code the upload runs, pinned by the oracle parities)
for the scene - after an update for (new triangles, ptmi_bvh_refit's tree).  The one word the host cannot compute is u_den[3] of a
DTriPre record in the default arithmetic, which the device writes through v_rcp_f32: it is held to the default-arithmetic
oracle's value of FullKernel.cl:556 for that triangle (pto_triangle_inverse_determinant), not masked.
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend
from gpu_cases import assert_same_state, state
import gpu_cases
import scene_record_cases as R
import scene_update_cases as U

pytestmark = pytest.mark.gpu
W, H = R.W, R.H
DA = backend.FLAG_DEFAULT_ARITHMETIC
INVALID_ARGUMENT, STATE, UNSUPPORTED = -1, -6, -7
ARITHMETICS = [pytest.param(0, id="strict"), pytest.param(DA, id="default")]
RECORD_FORMS = [pytest.param(False, id="precomputed"), pytest.param(True, id="generic")]


@pytest.fixture(scope="module", autouse=True)
def tools():
    gpu_cases.require_probe_tools()


def context(sc, **kw):
    return gpu_cases.context(sc, W, H, **kw)


def record_form(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("PTMI_GENERIC_TRIANGLES", "1")
    else:
        monkeypatch.delenv("PTMI_GENERIC_TRIANGLES", raising=False)


def expected(lay, tris, flags):
    """What a context with `flags` holds for the host layout `lay` of a scene with the triangles `tris`."""
    return R.with_default_arithmetic_denominators(lay, tris) if flags & DA else lay


def assert_holds(be, want, what, device_index=0):
    got = R.read_records(be, want, device_index)
    msg = R.describe_difference(got, want, what)
    assert msg == "", msg
    return got


def child_boxes(lay):
    """(lo, hi, empty) of both children of every node record: float32[n, 2, 3] twice, bool[n, 2]"""
    nodes = lay["recs"][lay["tri_ids"] == R.NO_TRIANGLE]
    f = nodes[:, :12].view(np.float32).reshape(-1, 2, 2, 3)
    return f[:, :, 0], f[:, :, 1], (nodes[:, 12:14] & R.REF_EMPTY) != 0


# ---------------------------------------------------------------------------------------------- A. after upload

UPLOAD_SCENES = ["cornell", "big_leaf", "empty_leaves", "feat_textured", "signed_zero-s0", "tris20k", "deep_chain_27"]
_uploaded = {}


def uploaded_expectation(name, flags, generic):
    key = (name, flags, generic)
    if key not in _uploaded:
        _uploaded[key] = expected(R.cached_layout(name, generic), R.scene(name).triangulation, flags)
    return _uploaded[key]


@pytest.mark.parametrize("generic", RECORD_FORMS)
@pytest.mark.parametrize("flags", ARITHMETICS)
@pytest.mark.parametrize("name", UPLOAD_SCENES)
def test_an_upload_holds_the_host_layout(name, flags, generic, monkeypatch):
    """The upload copies, tri_ids, big_leaves and, in the default arithmetic, the denominator kernel on every record: its tail
    lanes (record counts that are no multiple of 256) and the node records it must leave alone."""
    record_form(monkeypatch, generic)
    want = uploaded_expectation(name, flags, generic)
    host = R.cached_layout(name, generic)
    if name == "big_leaf":
        assert len(want["big_leaves"]) >= 1
    if name == "empty_leaves":
        assert child_boxes(host)[2].any()
    if name == "tris20k" and flags & DA and not generic:
        # (the device word is not the host's: the expectation is a different one for many records, and for no node record)
        changed = np.flatnonzero((want["recs"] != host["recs"]).any(axis=1))
        assert len(changed) > 100 and (host["tri_ids"][changed] != R.NO_TRIANGLE).all()
        assert (np.flatnonzero((want["recs"] != host["recs"]).any(axis=0)) == [R.U_DEN_W]).all()
    be = context(R.scene(name), flags=flags)
    try:
        assert_holds(be, want, f"{name} after ptmi_initialize_memory")
    finally:
        be.release()


def test_the_reader_refuses_what_it_cannot_read():
    sc = R.scene("cornell")
    be = Backend().setup_context(W, H, 4, sc.lightsSize)
    try:
        assert R.record_sizes(be)[0] == STATE  # before ptmi_initialize_memory
        be.initialize_memory(sc)
        rc, sizes = R.record_sizes(be)
        assert rc == R.OK and sizes[5] == 1
        assert R.record_sizes(be, 1)[0] == INVALID_ARGUMENT
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- B. after ptmi_update_triangles

def moved(name):
    return lambda sc: U.moved_triangles(sc, name)


def moved_by(amplitude):
    return lambda sc: U.displaced(sc.triangulation, 7, amplitude=amplitude)


def snapped(seed):
    return lambda sc: R.snapped_to_signed_zero(sc.triangulation, seed)


# scene, flags, generic records, the motion
UPDATE_CASES = {
    # fewer records, triangles and level nodes than one workgroup
    "cornell-strict": ("cornell", 0, False, moved("cornell")),
    "cornell-default": ("cornell", DA, False, moved("cornell")),
    # DBigLeaf ranges; children flagged empty
    "big_leaf": ("big_leaf", 0, False, moved("big_leaf")),
    "empty_leaves": ("empty_leaves", 0, False, moved("empty_leaves")),
    # all twelve UV floats, the three shading normals and both material indices of DShade
    "feat_textured": ("feat_textured", 0, False, moved("feat_textured")),
    "feat_textured-default": ("feat_textured", DA, False, moved("feat_textured")),
    # 4096 triangles (no tail in the shade kernel), levels wider than one workgroup, new zeros of either sign against held ones
    "signed_zero-s0-snapped": ("signed_zero-s0", 0, False, snapped(0)),
    "signed_zero-s1-snapped": ("signed_zero-s1", 0, False, snapped(1)),
    # one node per level, 26 levels: many launches with n = 1 (deep_chain_27 itself cannot be updated: see below)
    "chain_26": ("chain_26", 0, False, moved("chain_26")),
    # levels of thousands of nodes, a 32-lane tail in the shade kernel
    "tris20k-precomputed-strict": ("tris20k", 0, False, moved("tris20k")),
    "tris20k-precomputed-default": ("tris20k", DA, False, moved("tris20k")),
    "tris20k-generic-strict": ("tris20k", 0, True, moved("tris20k")),
    "tris20k-generic-default": ("tris20k", DA, True, moved("tris20k")),
    # every box gets smaller: a keep_sel that kept held values on anything but equality would leave boxes too large
    "tris20k-shrunk": ("tris20k", 0, False, lambda sc: R.shrunk(sc.triangulation)),
    # the exponent range: cornell scaled by 2^-10 and 2^10, triangles, camera and lights alike, the motion scaled with it
    "cornell*2^-10": ("cornell*2^-10", 0, False, moved_by(0.02 * 2.0 ** -10)),
    "cornell*2^10": ("cornell*2^10", 0, False, moved_by(0.02 * 2.0 ** 10)),
    "cornell*2^-10-default": ("cornell*2^-10", DA, False, moved_by(0.02 * 2.0 ** -10)),
    "cornell*2^10-default": ("cornell*2^10", DA, False, moved_by(0.02 * 2.0 ** 10)),
}


def sign_ties_in_leaf_boxes(held, tris):
    """How many corners of the leaf children's boxes in the layout `held` are a zero whose refit from `tris` - the fold of the
    leaf's triangles in record order, of values that compare equal the first wins - is the zero of the OTHER sign: the corners
    keep_sel exists for."""
    count = 0
    ids = held["tri_ids"]
    for rec in held["recs"][ids == R.NO_TRIANGLE]:
        for child in (0, 1):
            ref = int(rec[12 + child])
            n = (ref >> 27) & 7
            if not ref & 0x80000000 or ref & R.REF_EMPTY or n == 7 or n == 0:
                continue
            start = ref & 0x07FFFFFF
            box = tris["AABB"][ids[start:start + n]]
            corners = rec[6 * child:6 * child + 6].view(np.float32)
            for axis in range(3):
                for corner, values, fold in ((corners[axis], box["pMin"][:, axis], np.min), (corners[3 + axis], box["pMax"][:, axis], np.max)):
                    fresh = fold(values)
                    if corner == 0 and fresh == 0:
                        first = values[np.flatnonzero(values == 0)[0]]
                        count += int(np.signbit(first) != np.signbit(corner))
    return count


@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_an_update_holds_the_layout_of_a_fresh_upload(case, monkeypatch):
    """Before the update the old scene's layout, which is not the new one's; after it the new one's in all four arrays, tri_ids
    and big_leaves untouched.  The exponent cases are cornell scaled by 2^-10 and by 2^10, its tree scaled with it (every product
    is exact; ptmi_bvh_create itself refuses to build a tree over boxes of the larger size): screen_update accepts both."""
    name, flags, generic, motion = UPDATE_CASES[case]
    record_form(monkeypatch, generic)
    sc = R.scene(name)
    tris = motion(sc)
    old = uploaded_expectation(name, flags, generic)
    host_new = R.layout_in_mode(U.moved_scene(sc, tris), generic)
    new = expected(host_new, tris, flags)
    lo0, hi0, empty = child_boxes(R.cached_layout(name, generic))
    lo1, hi1, empty1 = child_boxes(host_new)
    assert np.array_equal(empty, empty1)
    if name == "big_leaf":
        assert len(new["big_leaves"]) >= 1
    if name == "empty_leaves":
        assert empty.any() and (lo1[empty] == np.inf).all() and (hi1[empty] == -np.inf).all()
    if name.startswith("signed_zero"):
        assert len(tris) == 4096 and sign_ties_in_leaf_boxes(R.cached_layout(name, generic), tris) > 0
    if case == "tris20k-shrunk":
        assert (lo1[~empty] >= lo0[~empty]).all() and (hi1[~empty] <= hi0[~empty]).all()
        smaller = ((lo1 > lo0) | (hi1 < hi0)).any(axis=2)
        assert smaller[~empty].all(), f"{int((~smaller[~empty]).sum())} boxes did not shrink"
    be = context(sc, flags=flags)
    try:
        before = assert_holds(be, old, f"{case} before the update")
        assert R.describe_difference(before, new) != ""  # (live memory, and the motion changes records)
        assert not np.array_equal(before["recs"], new["recs"])
        if name == "feat_textured":
            assert not np.array_equal(before["shade"], new["shade"])
        info = be.update_triangles(tris)
        after = assert_holds(be, new, f"{case} after ptmi_update_triangles")
    finally:
        be.release()
    assert np.array_equal(after["tri_ids"], before["tri_ids"]) and np.array_equal(after["big_leaves"], before["big_leaves"])
    assert info["levels"] == int(host_new["info"][5])
    if name == "chain_26":
        assert info["levels"] == 26
    if name == "tris20k":
        assert 12 <= info["levels"] <= 20 and len(tris) % 256 == 32


def test_deep_chain_27_is_refused_and_keeps_every_byte():
    """deep_chain_27 (bvh_stress_cases: a tree of more than 22 levels) spans 2^27 units, beyond the 2^21 inside which the
    wavefront kernel's records cannot yield NaN distances: the scene has a ptmi_literal_kernel_reason, and the contract (DESIGN
    1b) has ptmi_update_triangles refuse such a scene as a whole, moved or not.  So its records are pinned after the upload
    (above) and across the refusal; the deep chain that IS updated is chain_26, the same shape inside the range."""
    sc = R.scene("deep_chain_27")
    assert sc.bvhMaxDepth > 22
    want = R.cached_layout("deep_chain_27", False)
    be = context(sc)
    try:
        for tris in (sc.triangulation, U.displaced(sc.triangulation, 7)):
            with pytest.raises(PtmiError) as e:
                be.update_triangles(tris)
            assert e.value.code == UNSUPPORTED and "NaN distances" in str(e.value)
            assert_holds(be, want, "deep_chain_27 after the refused update")
    finally:
        be.release()


@pytest.mark.parametrize("name", ["signed_zero-s0", "signed_zero-s1"])
def test_an_update_with_unchanged_triangles_changes_no_byte(name):
    """The lattice whose boxes hold zeros of both signs, decided by an order the finished tree no longer tells: every refitted
    corner ties with the held one."""
    sc = R.scene(name)
    old = R.cached_layout(name, False)
    assert R.same_arrays(R.layout_in_mode(U.moved_scene(sc, sc.triangulation), False), old)  # (the yardsticks agree)
    lo, hi, empty = child_boxes(old)
    zeros = np.concatenate([lo[~empty].ravel(), hi[~empty].ravel()])
    zeros = zeros[zeros == 0]
    assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    be = context(sc)
    try:
        assert_holds(be, old, f"{name} before the update")
        be.update_triangles(sc.triangulation)
        assert_holds(be, old, f"{name} after an update with the triangles it holds")
    finally:
        be.release()


def test_two_successive_updates_hold_the_layout_of_two_successive_refits():
    sc = R.scene("tris20k")
    tris1 = U.displaced(sc.triangulation, seed=1, amplitude=0.01)
    tris2 = U.displaced(tris1, seed=2, amplitude=0.01)
    once = U.moved_scene(sc, tris1)
    want1, want2 = R.layout_in_mode(once, False), R.layout_in_mode(U.moved_scene(once, tris2), False)
    be = context(sc)
    try:
        be.update_triangles(tris1)
        assert_holds(be, want1, "after the first update")
        be.update_triangles(tris2)
        assert_holds(be, want2, "after the second update")
    finally:
        be.release()


def test_refused_updates_and_a_camera_move_leave_every_byte():
    """Before any update, and again after a good one (when the scratch triangles and the schedule exist)."""
    sc = R.scene("cornell")
    tris = U.moved_triangles(sc, "cornell")
    old, new = R.cached_layout("cornell", False), R.layout_in_mode(U.moved_scene(sc, tris), False)
    be = context(sc)
    try:
        for held, held_scene in ((old, sc), (new, U.moved_scene(sc, tris))):
            for kind in U.BAD_TRIANGLES:
                with pytest.raises(PtmiError) as e:
                    be.update_triangles(U.bad_triangles(held_scene, kind))
                assert e.value.code == (INVALID_ARGUMENT if kind == "wrong_count" else UNSUPPORTED), str(e.value)
                assert_holds(be, held, f"after the refused update ({kind})")
            cam = U.moved_camera(sc)
            be.set_camera(cam.cameraPosition, cam.cameraDirection, cam.cameraRight, cam.cameraUp)
            assert_holds(be, held, "after ptmi_set_camera")
            if held is old:
                be.update_triangles(tris)
                assert_holds(be, new, "after the good update")
    finally:
        be.release()


def test_both_listed_devices_hold_the_same_records():
    sc = R.scene("cornell")
    tris = U.moved_triangles(sc, "cornell")
    old, new = R.cached_layout("cornell", False), R.layout_in_mode(U.moved_scene(sc, tris), False)
    be = context(sc, devices=[0, 0])
    try:
        assert R.record_sizes(be, 2)[0] == INVALID_ARGUMENT
        for want, what in ((old, "after the upload"), (new, "after the update")):
            if want is new:
                be.update_triangles(tris)
            got = [assert_holds(be, want, f"listed device {i} {what}", device_index=i) for i in (0, 1)]
            assert got[0]["n_devices"] == 2 and R.same_arrays(got[0], got[1])
    finally:
        be.release()


def test_an_update_under_render_ahead(monkeypatch):
    """The blocking one-iteration-per-call caller that is rendered ahead of: launches for later iterations are in flight when
    the update arrives."""
    monkeypatch.setenv("PTMI_RENDER_AHEAD", "2")
    sc = R.scene("cornell")
    tris = U.moved_triangles(sc, "cornell")
    new = R.layout_in_mode(U.moved_scene(sc, tris), False)
    be = context(sc)
    try:
        for k in range(4):
            be.render(k, 1)
            be.synchronize()
        be.update_triangles(tris)
        assert_holds(be, new, "after an update under PTMI_RENDER_AHEAD=2")
        be.render(4, 1)
        assert_holds(be, new, "after one more iteration")
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- C. still renderable

def test_the_updated_lattice_renders_like_a_fresh_upload():
    sc = R.scene("signed_zero-s0")
    tris = R.snapped_to_signed_zero(sc.triangulation, 0)
    be = context(sc)
    try:
        be.update_triangles(tris)
        be.render(0, 2)
        got = state(be)
    finally:
        be.release()
    fresh = context(U.moved_scene(sc, tris))
    try:
        fresh.render(0, 2)
        want = state(fresh)
    finally:
        fresh.release()
    assert_same_state(got, want)
