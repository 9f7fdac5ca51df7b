"""ptmi_render_guides without a GPU: the new ABI is held against the header, the entry points validate their arguments, and the
yardstick of the GPU tests (guide_cases.py) checks itself against the yardstick of the ray queries and against the conditions
its scenes have to meet."""
import ctypes as C

import numpy as np
import pytest

from opencl_pathtracer_amd import backend, structs as S
from abi_cases import declared_symbols, exported_symbols, header_values
import guide_cases as G
import ray_query_cases as Q

NEW_SYMBOLS = {"ptmi_render_guides", "ptmi_render_guides_device"}


# ---------------------------------------------------------------------------------------------- ABI

def test_header_binding_list_and_library_agree(built):
    declared = set(declared_symbols())
    assert NEW_SYMBOLS <= declared and declared == set(backend.ABI_SYMBOLS)
    assert NEW_SYMBOLS <= exported_symbols()
    assert backend.load_library().ptmi_abi_version() == 4


LAYOUT = ['VALUE("sizeof", sizeof(ptmi_guides));'] + [
    f'VALUE("{field}", offsetof(ptmi_guides, {field}));' for field in "struct_size reserved albedo normal position hit_count ids".split()]


def test_ctypes_struct_matches_the_header():
    out = header_values(LAYOUT)
    want = {"sizeof": C.sizeof(backend.Guides)}
    want.update({name: getattr(backend.Guides, name).offset for name, _ in backend.Guides._fields_})
    assert out == want
    assert [name for name, _ in backend.Guides._fields_][2:] == list(backend.GUIDE_PLANES) == list(G.PLANES)


def test_argument_validation_needs_no_gpu(built):
    lib = backend.load_library()
    good = backend.Guides(C.sizeof(backend.Guides), 0)
    bad = backend.Guides(C.sizeof(backend.Guides) - 8, 0)
    for call in (lib.ptmi_render_guides, lib.ptmi_render_guides_device):
        assert call(None, 0, 1, C.byref(good)) == -1  # a NULL context
        assert call(None, 0, 1, C.byref(bad)) == -1   # ... and a wrong struct_size with it
        assert call(None, 0, 1, None) == -1
        assert call(None, 0, 0, None) == -1           # (refused whatever the count)


# ---------------------------------------------------------------------------------------------- the yardstick against the ray queries'

@pytest.mark.parametrize("name", ["cornell", "feat_textured"])
def test_yardstick_equals_the_ray_query_walk(built, name):
    """The first hit of Kernel_Main's path (pto_trace_path) == the tree walk of ray_query_cases on the ray this module builds
    from pto_sampler and the camera expression: triangle, point, s and t bit for bit, and the same side."""
    sc = G.scene(name)
    y = G.yardstick(name)
    k = np.arange(96)
    pixels = (k * 1031 + (G.W // 2) * (G.H + 1)) % (G.W * G.H)
    its = (0, 7, 8)
    origins, directions, samples = [], [], []
    for j, p in enumerate(pixels):
        gx, gy, it = int(p % G.W), int(p // G.W), its[j % 3]
        _, d = y.primary_ray(gx, gy, it)
        origins.append(sc.cameraPosition)
        directions.append(d)
        samples.append(y.sample(gx, gy, it))
    rays = np.zeros(len(pixels), S.RAY)
    rays["origin"], rays["direction"], rays["max_squared_distance"] = np.float32(origins), np.float32(directions), np.inf
    want = Q.expected_hits(sc, rays)
    hits = 0
    for s, w in zip(samples, want):
        assert s["hit"] == (w["triangle_id"] != Q.MISS)
        if s["hit"]:
            hits += 1
            assert (s["triangle_id"], s["front"]) == (w["triangle_id"], w["front"])
            assert np.array_equal(np.float32([s["s"], s["t"]]).view(np.uint32), np.float32([w["s"], w["t"]]).view(np.uint32))
            assert np.array_equal(s["point"].view(np.uint32), w["point"].view(np.uint32))
    assert hits >= 40


# ---------------------------------------------------------------------------------------------- the conditions on the scenes

@pytest.mark.parametrize("name", ("cornell",) + G.SCENES + ("feat_two_sided_from_behind",))
def test_scenes_meet_the_yardsticks_conditions(built, name):
    """At most 10 % of a scene's hit samples lack a bit-exact albedo, and every sample lands in the pixel of its work-item (the
    planes are indexed by work-item, the integrator's accumulators by where the sample lands: the same for these samplers)."""
    for sampler in (S.JITTERED, S.UNIFORM):
        y = G.yardstick(name, sampler)
        its = G.iterations_of(name)
        c = y.census(its)
        assert c["excluded"] <= G.MAX_EXCLUDED * c["hits"], (name, c)
        assert c["hits"] + c["misses"] == len(its) * G.W * G.H
        for it in its[:2]:
            for p in range(0, G.W * G.H, 7):
                assert y.lands_in_its_own_pixel(p % G.W, p // G.W, it), (name, sampler, p, it)


def test_feat_textured_has_textured_hits_and_misses(built):
    c = G.yardstick("feat_textured").census(G.iterations_of("feat_textured")[:1])
    assert c["textured_hits"] > 1000 and c["misses"] > 500 and c["excluded"] == 0, c


def test_feat_two_sided_shows_both_sides(built):
    """Both values of `front`, and both materials of a two-sided triangle, are in what the GPU tests compare.  From the scene's
    own camera every primary ray meets its surface from the positive side (measured: 4978 hits of iterations 5 and 6, all front = 1 -
    the sheet's and the wall's normals face that camera, a sphere shows its outside), so the negative sides come from the second
    camera the GPU tests move to with ptmi_set_camera (guide_cases.behind_the_sheet)."""
    sc = G.scene("feat_two_sided")
    fronts, negative_materials = set(), 0
    for name in ("feat_two_sided", "feat_two_sided_from_behind"):
        r = G.yardstick(name).iteration(G.iterations_of(name)[0])
        hit = r["hit"]
        fronts |= {int(v) for v in np.unique(r["ids"][..., 2][hit])}
        tri, mat = r["ids"][..., 0][hit], r["ids"][..., 1][hit]
        pos, neg = sc.triangulation["materialWithPositiveNormalIndex"][tri], sc.triangulation["materialWithNegativeNormalIndex"][tri]
        assert np.array_equal(mat, np.where(r["ids"][..., 2][hit] == 1, pos, neg))
        negative_materials += int(((pos != neg) & (mat == neg)).sum())
    assert fronts == {0, 1} and negative_materials > 100
