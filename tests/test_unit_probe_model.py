"""The function-level differential on the CPU: every group of tests/unit_probe_cases.py through both builds of the oracle, and
the COVERAGE of the committed cases - each comparison a function makes is taken both ways, and at equality where equality can
be reached - so that the GPU leg (test_unit_probe_gpu.py: product == oracle == the reference's own function) cannot pass
without having looked at the boundaries."""
import numpy as np
import pytest

import oracle_ffi as O
import unit_probe_cases as K

f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def libs(built):
    return O.oracle(False), O.oracle(True)


@pytest.fixture(scope="module")
def tri(libs):
    return K.triangle_cases(libs[0])


def test_case_counts(tri):
    for cases in (K.box_cases(), tri[0], K.texture_cases(), K.sky_cases(), K.light_cases(), K.material_cases(), K.sampling_cases(), K.pixel_cases()):
        assert 0 < len(cases) <= 4096


def test_box_coverage(libs):
    cases = K.box_cases()
    for lib in libs:
        decided = K.oracle_box(lib, cases, decider=True)[:, 0]
        hit = K.oracle_box(lib, cases)[:, 0]
        assert np.array_equal(hit == 1, (decided == 9) | (decided == 11))
        inside = K.box_in_ordered_domain(lib, cases)
        assert 2 * inside.sum() >= len(cases) and (~inside).sum() > 0
        for region, name in ((inside, "the ordered domain"), (~inside, "outside it")):
            counts = np.bincount(decided[region], minlength=12)
            # (the isEmpty test and every slab / cross / distance test decides, in both regions; an empty box counts as ordered)
            assert (counts[1:12] > 0).all(), (name, counts)
        # equality with the limit is reached: among consecutive limits the decision flips
        lim = cases.view(f32)[:, 7]
        same_ray = (cases[1:, :7] == cases[:-1, :7]).all(axis=1) & (cases[1:, 8:] == cases[:-1, 8:]).all(axis=1)
        step = same_ray & (cases[1:, 7] == cases[:-1, 7] + 1) & (lim[1:] > 0)
        assert (step & (decided[:-1] == 10) & (decided[1:] == 11)).sum() >= 3
        # ties of the cross tests: a ray through an edge passes `tmin > tymax` (resp. `tymin > tmax`, and the z pairs) as false, and
        # the same ray with ONE origin coordinate one ulp aside is rejected by exactly that test
        one_word = ((cases[1:] != cases[:-1]).sum(axis=1) == 1) & (np.abs(cases[1:, 8:11].astype(np.int64) - cases[:-1, 8:11]).max(axis=1) == 1)
        for test in (4, 5, 7, 8):
            flips = one_word & ((decided[1:] == test) != (decided[:-1] == test)) & ((decided[1:] >= 9) | (decided[:-1] >= 9))
            assert flips.sum() > 0, f"no slab tie on box test {test}"


def test_triangle_coverage(libs, tri):
    cases, n_inside = tri
    safe, equal_w = K.triangle_domains(cases)
    assert 2 * safe.sum() >= len(cases) and 2 * (safe & equal_w).sum() >= len(cases)
    assert (~safe[n_inside:]).all() and len(cases) > n_inside     # the outside block is outside, and not empty
    assert safe[:n_inside].all(), np.flatnonzero(~safe[:n_inside])[:5]  # nothing else is excluded from any comparison
    assert (safe & ~equal_w).sum() > 0
    for lib in libs:
        first = K.oracle_triangle(lib, cases, first_rejection=True)[:, 0]
        out = K.oracle_triangle(lib, cases)
        assert np.array_equal(first == 0, out[:, 0] == 1)
        counts = np.bincount(first[safe], minlength=8)
        assert (counts > 0).all(), dict(zip(["accepted"] + list(K.REJECTIONS.values()), counts))
        acc = safe & (out[:, 0] == 1)
        s, t = out[:, 5].view(f32), out[:, 6].view(f32)
        assert (acc & (s == 0)).sum() > 0 and (acc & (t == 0)).sum() > 0 and (acc & (s + t == 1) & (s > 0) & (t > 0)).sum() > 0
        assert (acc & (out[:, 7] == 1)).sum() > 0 and (acc & (out[:, 7] == 0)).sum() > 0
        # the limit at equality: a hit whose squared distance equals the limit it was given
        assert (acc & (out[:, 8] == cases[:, 24])).sum() > 0
        # the squared distance at the 1e-5 threshold: accepted AT it, accepted at the nearest square above (within 2 ulps), and
        # rejected by that test at the nearest square below (a square of a binary32 reaches the threshold itself, not its neighbours)
        nsd, thr = out[:, 8].view(f32), f32(0.00001)
        fc = cases.view(f32)
        sweep = safe & (fc[:, 16] == 1) & (fc[:, 17] == 1) & (fc[:, 22] == -1) & (fc[:, 14] == 1) & (fc[:, 18] < 0.004) & (fc[:, 18] > 0.003)
        square = fc[:, 18] * fc[:, 18]
        assert (sweep & acc & (nsd == thr)).sum() > 0
        assert (sweep & acc & (nsd > thr) & (nsd <= K.up(thr, 2))).sum() > 0
        assert (sweep & (first == 3) & (square < thr) & (square >= K.down(thr, 2))).sum() > 0
        # |N.d| on either side of 1e-5, both signs
        n_z = cases.view(f32)[:, 14]
        at = np.abs(n_z) == f32(0.00001)
        assert (at & (first == 0)).sum() >= 2 and (safe & (np.abs(n_z) == K.down(f32(0.00001))) & (first == 1)).sum() >= 2


def test_texture_and_sky_indices(libs):
    tex, texels = K.texture_data()
    cases = K.texture_cases()
    for lib in libs:
        out, index = K.oracle_texture(lib, cases)
        lo = cases[:, 2]
        assert ((index >= lo) & (index < lo + cases[:, 0] * cases[:, 1])).all(), "a texel index outside its texture"
        u = cases.view(f32)[:, 3]
        x = (index - lo) % cases[:, 0]
        wrapped_to_one = (u < 0) & (u > -1e-8) & (u != 0)
        assert wrapped_to_one.sum() > 0 and (x[wrapped_to_one] == cases[wrapped_to_one, 0] - 1).all()   # the u < 0 arm giving exactly 1.0
        assert (x[(u == 0) | (u == 1)] == 0).all()   # an exact integer becomes 0
        for w, h in K.TEXTURE_SIZES:   # every corner texel of every texture is read
            sel = (cases[:, 0] == w) & (cases[:, 1] == h)
            got = set((index[sel] - lo[sel]).tolist())
            assert {0, w - 1, (h - 1) * w, w * h - 1} <= got
    sky = K.sky_cases()
    for lib in libs:
        out, face, index = K.oracle_sky(lib, sky)
        counts = np.bincount(face, minlength=7)
        assert (counts > 0).all(), counts          # each face, and the fall-through
        faces = tex[len(K.TEXTURE_SIZES):]
        f = np.where(face == 6, 0, face)
        assert ((index >= faces["offset"][f]) & (index < faces["offset"][f] + faces["width"][f] * faces["height"][f])).all()
        assert len(np.unique(index)) >= 30


def test_light_coverage(libs):
    cases = K.light_cases()
    f = cases.view(f32)
    for lib in libs:
        branch = K.light_branch(lib, cases)       # the oracle's own decision
        counts = np.bincount(branch, minlength=len(K.LIGHT_BRANCHES))
        assert (counts > 0).all(), dict(zip(K.LIGHT_BRANCHES, counts))
        out = K.oracle_light(lib, cases).view(f32)[:, 0]
        assert np.isnan(out[branch == 5]).any()                                     # 0 / 0
        # cos_angle == a cone exactly (the construction of light_cases makes cos_angle = -direction.z): not inside the inner cone at
        # cos_inner, not outside the outer cone at cos_outer, and one ulp decides
        exact = (cases[:, 11] == K.SPOT) & (f[:, 14] == -2) & (f[:, 12] == 0) & (f[:, 13] == 0) & (f[:, 4] == 0) & (f[:, 5] == 0) & (f[:, 6] == -0.75)
        cos_angle = -f[:, 6]
        assert (exact & (f[:, 9] == cos_angle) & (branch == 4)).sum() > 0 and (exact & (f[:, 9] == K.down(cos_angle[exact][0])) & (branch == 2)).sum() > 0
        assert (exact & (f[:, 10] == cos_angle) & (branch == 4)).sum() > 0 and (exact & (f[:, 10] == K.up(cos_angle[exact][0])) & (branch == 3)).sum() > 0
        # p == position normalises a zero vector: the point light divides by a zero squared distance
        at_light = (f[:, 12:16] == f[:, 0:4]).all(axis=1)
        assert (at_light & (branch == 1)).sum() > 0 and (at_light & (branch >= 2) & (branch <= 5)).sum() > 0
        assert np.isnan(out[at_light & (branch == 1) & (f[:, 8] == 0)]).any()       # 0 / 0 * ...
        assert (~np.isfinite(out[at_light & (branch == 1) & (f[:, 8] != 0)])).any()


def test_material_coverage(libs):
    cases = K.material_cases()
    for lib in libs:
        out = K.oracle_material(lib, cases).view(f32)
        water_in = cases[:, 13] == 1
        total = out[:, 2] == 1
        assert (water_in & total).sum() > 0 and (water_in & ~total).sum() > 0 and (~water_in & ~total).sum() > 0
        # consecutive cos1 values straddle the edge of total reflection
        c = cases.view(f32)[:, 6]
        col = water_in & (cases[:, 12] == 0) & (cases.view(f32)[:, 2] == -1) & (c > 0.6) & (c < 0.7)
        flips = np.diff(total[col].astype(int))
        assert len(flips) >= 90 and np.abs(flips).sum() == 1
        assert np.isnan(out[:, 0]).any()                      # sin1 of a cos1 above 1
        flipped = (out[:, 13:17] != cases.view(f32)[:, 8:12]).any(axis=1)
        d = (cases.view(f32)[:, 8:12].astype(np.float64) * cases.view(f32)[:, 4:8]).sum(axis=1)
        assert (flipped & (d == 0)).sum() > 0 and (~flipped & (d > 0)).sum() > 0
        assert set(np.unique(cases[:, 12])) == set(range(6))


def test_sampling_coverage(libs):
    found = K.scanned_seeds()
    assert all(len(found[k]) > 0 for k in range(7)), {K.OCTANTS[k]: len(v) for k, v in found.items()}
    cases = K.sampling_cases()
    seeds = cases[:, 0].view(np.int32)
    for special in (0, 1, -1, 2147483647, -2147483648):
        assert (seeds == special).any()
    z = cases.view(f32)[:, 3]
    for v in K.around(f32(0.9999)):
        assert (z == v).any() and (z == -v).any()
    for lib in libs:
        out = K.oracle_sampling(lib, cases)
        assert ((out[:, 2] == 0) & (out[:, 3] == 1)).sum() > 0 and (out[:, 2] == 1).sum() > 0   # the two seed rules part; pixel (0,0) iteration 0
        # every scanned seed falls, by the ORACLE's own branches, in the class the scan filed it under
        for k, seeds_k in found.items():
            for seed in seeds_k:
                assert K.oracle_octant(lib, seed) == k, (K.OCTANTS[k], seed)
        lib.pto_concentric_sample_disk.argtypes = [O.C.POINTER(O.C.c_int32), O.C.POINTER(O.C.c_float), O.C.POINTER(O.C.c_float)]

        def disk(seed):
            s, dx, dy = O.C.c_int32(seed), O.C.c_float(), O.C.c_float()
            lib.pto_concentric_sample_disk(O.C.byref(s), O.C.byref(dx), O.C.byref(dy))
            return dx.value, dy.value
        for seed in found[4] + found[6]:       # |sx| < 1e-4, alone and with |sy| < 1e-4: theta = 0, r = sy - the sx override wins
            dx, dy = disk(seed)
            assert dy == 0.0 and f32(dx) == f32(np.float64(K.disk_sample(seed)[1]) * 0.999)
        for seed in found[5]:                  # |sy| < 1e-4 alone: theta = 2 (a quarter turn), r = sx
            dx, dy = disk(seed)
            assert abs(dx) < 1e-6 and abs(dy - float(f32(np.float64(K.disk_sample(seed)[0]) * 0.999))) < 1e-6 and dy != 0.0
        # every class is among the committed cases
        classes = {K.oracle_octant(lib, int(v)) for v in np.unique(seeds)}
        assert classes == set(range(7))


def test_pixel_coverage(libs):
    cases = K.pixel_cases()
    assert 0 < len(cases) <= 4096
    assert {(int(w), int(h)) for w, h in cases[:, 2:4]} == set(K.PIXEL_SIZES) and set(cases[:, 5]) == {0, 1, 2}
    f = cases.view(f32)
    for lib in libs:
        out = K.oracle_pixel(lib, cases)
        w, h = cases[:, 2].astype(np.int64), cases[:, 3].astype(np.int64)
        assert (out[:, 3] < w * h).all() and (out[:, 4] < w * h).all()
        px, py = out[:, 4] % w, out[:, 4] // w
        # the clamp: (sx + 0.5) * W == W exactly lands on the last column, for every size; so does the row
        for size in K.PIXEL_SIZES:
            sel = (w == size[0]) & (h == size[1])
            at_x, at_y = sel & ((f[:, 7].astype(np.float64) + 0.5) * w == w), sel & ((f[:, 8].astype(np.float64) + 0.5) * h == h)
            assert at_x.sum() > 0 and (px[at_x] == w[at_x] - 1).all() and at_y.sum() > 0 and (py[at_y] == h[at_y] - 1).all()
            beyond = sel & ((f[:, 7].astype(np.float64) + 0.5) * w > w)
            assert beyond.sum() > 0 and (px[beyond] == w[beyond] - 1).all()
        big = w == 1920
        assert (big & (px == 0)).sum() > 0 and (big & (px == 1919) & (f[:, 7] < 0.5)).sum() > 0   # the last column without the clamp
        # a JITTERED or UNIFORM sample stays in its own pixel; the drawn sample's seed moves only where the sampler draws
        own = cases[:, 5] != K.S.RANDOM
        assert (out[own, 3] == (cases[own, 1] * cases[own, 2] + cases[own, 0])).all()
        assert (out[cases[:, 5] == K.S.UNIFORM, 2] == cases[cases[:, 5] == K.S.UNIFORM, 6]).all()
    ref = K.pixel_reference_cases()
    assert len(ref) == 64 and (ref[:, 0] + 8 * ref[:, 1] == np.arange(64)).all() and (ref[:, 2:4] == 8).all() and (ref[:, 5] == K.S.JITTERED).all()


def test_the_two_arithmetics_share_every_decision(libs, tri):
    """Decisions on lattice inputs do not depend on the arithmetic (ties are exact in both): the coverage above holds for both
    builds because it is the same coverage."""
    box = K.box_cases()
    assert (K.oracle_box(libs[0], box) != K.oracle_box(libs[1], box)).sum() <= len(box) // 100
    a, b = K.oracle_triangle(libs[0], tri[0]), K.oracle_triangle(libs[1], tri[0])
    assert (a[:, 0] != b[:, 0]).sum() <= len(a) // 100
