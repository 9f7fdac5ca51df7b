"""ptmi_update_vertices: what can be checked without a GPU.

The record a vertex update derives - the importer's Triangle_Create, steps 1-6 of include/ptmi.h - exists three times: as
csrc/mesh_assemble_common.h (the assemble kernel's and ptmi_assemble_triangles' one function), as the NumPy restatement of
vertex_update_cases.py (one binary32 operation per line) and as scenes.triangle_create, which every scene of this repository was
built with.  Here ptmi_assemble_triangles is held to the restatement word for word, all 84 words, on the unit meshes and on the
derived meshes of four scenes, at rest and moved; the restatement to scenes.triangle_create; and the header as a program of its
own (tests/mesh_assemble_model.cpp, compiled here with g++ -ffp-contract=off -fsanitize=address,undefined) to the restatement
over files of the same meshes.  No comparison is made against a scene's uploaded records: a round trip through an indexed mesh
loses the original winding's last bit of N.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from opencl_pathtracer_amd import PtmiError, backend, scenes, structs as S
import abi_cases
import model_build
import scene_record_cases as R
import vertex_update_cases as V

ROOT = abi_cases.ROOT
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
NAMES = ["ptmi_bind_mesh", "ptmi_update_vertices", "ptmi_update_vertices_device", "ptmi_assemble_triangles"]
SCENES = ["cornell", "feat_textured", "signed_zero-s0", "tris20k"]
INVALID_ARGUMENT = -1
f32 = np.float32

derived, moved = V.derived, V.moved


def every_mesh():
    for name, m in V.UNIT_CASES.items():
        yield name, m
    for name in SCENES:
        yield name, derived(name)
        yield name + " moved", moved(name)


# ---------------------------------------------------------------------------------------------- the ABI

def test_the_four_calls_are_declared_exported_and_bound():
    declared, exported = abi_cases.declared_symbols(), abi_cases.exported_symbols()
    for name in NAMES:
        assert name in declared and name in exported and name in backend.ABI_SYMBOLS, name


def test_the_structs_have_the_layout_of_the_header_and_the_abi_version_stays_4():
    fields = {"ptmi_mesh_topology": backend.MeshTopology, "ptmi_vertex_buffers": backend.VertexBuffers}
    lines = ['VALUE("abi", PTMI_ABI_VERSION);', "SIZE(ptmi_update_info);"]
    for struct, mirror in fields.items():
        lines.append(f"SIZE({struct});")
        lines += [f"OFFSET({struct}, {name});" for name, _ in mirror._fields_]
    v = abi_cases.header_values(lines)
    assert v["abi"] == 4 and v["ptmi_update_info"] == 40 and v["ptmi_mesh_topology"] == 64 and v["ptmi_vertex_buffers"] == 32
    for struct, mirror in fields.items():
        assert C.sizeof(mirror) == v[struct]
        for name, _ in mirror._fields_:
            assert getattr(mirror, name).offset == v[f"{struct}.{name}"], (struct, name)
    assert backend.load_library().ptmi_abi_version() == 4


# ---------------------------------------------------------------------------------------------- the restatement's own promises

def test_the_case_list_keeps_its_promises():
    V.check_the_list()


def test_the_moved_tris20k_reorders_triangles_into_all_six_outcomes():
    rest, went = V.restate(derived("tris20k"))[1], V.restate(moved("tris20k"))[1]
    assert set(went.tolist()) == set(range(V.OUTCOMES))
    assert 0 < int((rest != went).sum()) < len(rest)


def test_the_fallback_to_n_is_taken():
    assert V.restate(V.UNIT_CASES["normal_lengths"])[2].any() and V.restate(V.UNIT_CASES["index_twice"])[2].sum() == 0
    t, _, fallback = V.restate(V.UNIT_CASES["normal_lengths"])
    w = V.words(t)
    for i, k in np.argwhere(fallback):
        assert np.array_equal(w[i, 12 + 4 * k:16 + 4 * k], w[i, 48:52]) and t["N"][i][3] == 1  # N_k is N, w = 1 included


# ---------------------------------------------------------------------------------------------- the host call

def named(name):
    return V.UNIT_CASES[name] if name in V.UNIT_CASES else (moved(name[:-len(" moved")]) if name.endswith(" moved") else derived(name))


@pytest.mark.parametrize("name", list(V.UNIT_CASES) + SCENES + [s + " moved" for s in SCENES])
def test_assemble_triangles_equals_the_restatement(name):
    m = named(name)
    want = V.restate(m)[0]
    msg = V.describe_difference(backend.assemble_triangles(m), want, name)
    assert msg == "", msg
    if m.normals is not None:
        flat = V.with_buffers(m, normals=None)
        msg = V.describe_difference(backend.assemble_triangles(flat), V.restate(flat)[0], name + " without normals")
        assert msg == "", msg


@pytest.mark.parametrize("stride", V.STRIDES)
def test_strides_with_nan_in_every_padding_word(stride):
    for name in ("six_outcomes", "shared_index", "normal_lengths"):
        m = V.UNIT_CASES[name]
        got = backend.assemble_triangles(m, positions=V.padded(m.positions, stride), normals=V.padded(m.normals, stride))
        msg = V.describe_difference(got, V.restate(m)[0], f"{name} at stride {stride}")
        assert msg == "", msg


@pytest.mark.parametrize("name", SCENES)
def test_the_restatement_equals_triangle_create(name):
    for label, m in ((name, derived(name)), (name + " moved", moved(name))):
        p, n = m.positions[m.indices.astype(np.int64)], m.normals[m.indices.astype(np.int64)]
        with np.errstate(all="ignore"):
            theirs = scenes.triangle_create(p[:, 0], p[:, 1], p[:, 2], normals=n, uvp=m.uvp, uvn=m.uvn, mat_pos=m.mat_pos, mat_neg=m.mat_neg)
        theirs["id"] = m.ids
        ours = V.restate(m)[0]
        a, b = V.words(ours), V.words(np.frombuffer(bytearray(theirs.tobytes()), dtype=S.Triangle))
        # (numpy leaves the padding of a struct array it made undefined: compare the fields' words)
        field_words = np.ones(84, bool)
        field_words[[76, 77, 78, 79, 83]] = False  # isEmpty's word is compared below, byte for byte
        differ = np.argwhere((a != b) & field_words)
        assert ours["AABB"]["isEmpty"].tolist() == theirs["AABB"]["isEmpty"].tolist()
        if name != "signed_zero-s0":
            assert len(differ) == 0, (label, differ[:8])
            continue
        # np.minimum / np.maximum may keep the other zero of a tie: the words that differ are box words, and zeros on both sides
        for i, k in differ:
            assert 64 <= k < 76 and {int(a[i, k]), int(b[i, k])} == {0, 0x80000000}, (label, i, k, hex(a[i, k]), hex(b[i, k]))
        print(f"{label}: {len(differ)} box words differ in the sign of a zero")


# ---------------------------------------------------------------------------------------------- refusals of the host call

def test_every_refusal_of_the_host_call():
    lib = backend.load_library()
    m = V.UNIT_CASES["six_outcomes"]
    out = np.zeros(len(m.indices), S.Triangle)

    def call(edit_topology=None, edit_buffers=None, no_topology=False, no_buffers=False, no_out=False):
        t, keep = backend.mesh_topology(m)
        b, keep2 = backend._host_vertex_buffers(m.positions, m.normals)
        if edit_topology:
            edit_topology(t)
        if edit_buffers:
            edit_buffers(b)
        rc = lib.ptmi_assemble_triangles(None if no_topology else C.byref(t), None if no_buffers else C.byref(b),
                                         None if no_out else out.ctypes.data_as(C.c_void_p))
        return rc, lib.ptmi_last_error(None).decode()

    assert call()[0] == 0
    before = out.tobytes()
    bad_index = np.array(m.indices, np.uint32)
    bad_index[4, 1] = 3
    cases = [
        (dict(no_topology=True), "topology is NULL or struct_size mismatch (ABI)"),
        (dict(edit_topology=lambda t: setattr(t, "struct_size", 60)), "topology is NULL or struct_size mismatch (ABI)"),
        (dict(edit_topology=lambda t: setattr(t, "reserved", 1)), "topology.reserved is not 0"),
        (dict(edit_topology=lambda t: setattr(t, "n_vertices", 0)), "n_vertices is 0"),
        (dict(edit_topology=lambda t: setattr(t, "indices", None)), "indices is NULL"),
        (dict(edit_topology=lambda t: setattr(t, "mat_pos", None)), "mat_pos is NULL"),
        (dict(edit_topology=lambda t: setattr(t, "indices", bad_index.ctypes.data)), "triangle 4 corner 1: index 3, the mesh has 3 vertices"),
        (dict(no_buffers=True), "vertex buffers are NULL or struct_size mismatch (ABI)"),
        (dict(edit_buffers=lambda b: setattr(b, "struct_size", 24)), "vertex buffers are NULL or struct_size mismatch (ABI)"),
        (dict(edit_buffers=lambda b: setattr(b, "n_vertices", 4)), "4 vertices, the mesh has 3"),
        (dict(edit_buffers=lambda b: setattr(b, "position_stride", 8)), "position_stride is 8 (bytes: at least 12, a multiple of 4)"),
        (dict(edit_buffers=lambda b: setattr(b, "position_stride", 14)), "position_stride is 14 (bytes: at least 12, a multiple of 4)"),
        (dict(edit_buffers=lambda b: setattr(b, "normal_stride", 18)), "normal_stride is 18 (bytes: at least 12, a multiple of 4)"),
        (dict(edit_buffers=lambda b: setattr(b, "positions", None)), "positions is NULL"),
        (dict(no_out=True), "out is NULL"),
    ]
    for kw, words in cases:
        rc, text = call(**kw)
        assert (rc, text) == (INVALID_ARGUMENT, "ptmi_assemble_triangles: " + words), (words, rc, text)
        assert out.tobytes() == before
    with pytest.raises(PtmiError):
        backend.assemble_triangles(V.mesh(m.positions, [[0, 1, 3]]))
    # no triangles: nothing to refuse, nothing written
    empty = V.mesh(np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32))
    assert len(backend.assemble_triangles(empty)) == 0


def test_a_null_context_is_an_invalid_argument():
    lib = backend.load_library()
    info, b = backend.UpdateInfo(), backend.VertexBuffers()
    t, keep = backend.mesh_topology(V.UNIT_CASES["six_outcomes"])
    assert lib.ptmi_bind_mesh(None, C.byref(t)) == INVALID_ARGUMENT
    for call in (lib.ptmi_update_vertices, lib.ptmi_update_vertices_device):
        assert call(None, C.byref(b), C.byref(info)) == INVALID_ARGUMENT
        assert info.struct_size == 40  # (set before anything is looked at, as ptmi_update_triangles does)
        assert call(None, C.byref(b), None) == INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- mesh_from_triangulation

@pytest.mark.parametrize("name", ["cornell", "feat_textured", "tris20k"])
def test_a_round_trip_through_the_mesh_keeps_vertices_coordinates_and_box(name):
    tris = R.scene(name).triangulation
    m = derived(name)
    assert m.indices.max() < len(m.positions) and len(m.positions) <= 3 * len(tris)
    back = V.restate(m)[0]
    for field in ("S1", "S2", "S3", "UVP1", "UVP2", "UVP3", "UVN1", "UVN2", "UVN3", "materialWithPositiveNormalIndex",
                  "materialWithNegativeNormalIndex", "id"):
        assert np.array_equal(back[field].view(np.uint32), np.ascontiguousarray(tris[field]).view(np.uint32)), field
    for corner in ("pMin", "pMax", "centroid"):
        assert np.array_equal(back["AABB"][corner].view(np.uint32), np.ascontiguousarray(tris["AABB"][corner]).view(np.uint32)), corner
    # N keeps its side everywhere and its value to the last bit or so
    assert (scenes._dot3(back["N"][:, :3], tris["N"][:, :3]) > 0.99).all()


# ---------------------------------------------------------------------------------------------- the header as a program of its own

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    model_build.sanitizer_runtimes_or_skip()
    tmp = tmp_path_factory.mktemp("mesh_assemble")
    exe = model_build.program([os.path.join(ROOT, "tests", "mesh_assemble_model.cpp")], tmp, "mesh_assemble_model",
                              opt=["-O1", "-g"], werror=False, fp_strict=True,
                              sanitize=model_build.SANITIZE, includes=[os.path.join(ROOT, "include"), CSRC])

    def run(blocks):
        """blocks: (mesh, stride) -> the records of every block, one array each"""
        src, dst = str(tmp / "meshes.bin"), str(tmp / "records.bin")
        with open(src, "wb") as f:
            for m, stride in blocks:
                n, nv = len(m.indices), len(m.positions)
                optional = [m.uvp, m.uvn, m.mat_neg, m.ids]
                f.write(np.array([n, nv, stride, 0 if m.normals is None else stride] + [int(x is not None) for x in optional], np.uint32).tobytes())
                f.write(np.ascontiguousarray(m.indices, np.uint32).tobytes())
                for a in (m.positions, m.normals):
                    if a is not None:
                        f.write(V.padded(a, stride).base.tobytes())  # (the rows with their padding)
                for a, dtype in ((m.uvp, f32), (m.uvn, f32), (m.mat_pos, np.uint32), (m.mat_neg, np.uint32), (m.ids, np.uint32)):
                    if a is not None:
                        f.write(np.ascontiguousarray(a, dtype).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        data = np.fromfile(dst, dtype=S.Triangle)
        assert len(data) == sum(len(m.indices) for m, _ in blocks)
        out, at = [], 0
        for m, _ in blocks:
            out.append(data[at:at + len(m.indices)])
            at += len(m.indices)
        return out
    return run


def test_the_header_as_a_program_equals_the_restatement(program):
    blocks, labels = [], []
    for name, m in every_mesh():
        strides = V.STRIDES if name in V.UNIT_CASES else (12,)
        for stride in strides:
            blocks.append((m, stride))
            labels.append(f"{name} at stride {stride}")
            if m.normals is not None and stride == 12:
                blocks.append((V.with_buffers(m, normals=None), stride))
                labels.append(f"{name} without normals")
    for (m, _), label, got in zip(blocks, labels, program(blocks)):
        msg = V.describe_difference(got, V.restate(m)[0], label)
        assert msg == "", msg
