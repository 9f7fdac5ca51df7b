"""What the decks of stack_depth_cases.py are for, asserted on the CPU for every depth tests/test_stack_depth_gpu.py uses: the
rays it sends and the rays its images start with FILL a traversal stack of as many levels as the tree is deep, nothing asks for
more, the full-stack rays do not all see the same card, and the upload accepts 29 levels and refuses 30.  Conditions on the
inputs, not measurements: nobody has to trust that "the stack was full".  The walk is ray_query_cases.Walker's, whose every
decision is the CPU oracle's; no product kernel runs here.

The fewest distinct closest hits asked of the full-stack rays is 4 - or every card the deck has, for the decks of one and two
levels, which have two and three (the 9 coincident triangles of the big leaf count once: the first of them wins every tie).
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import PtmiError, backend
import ray_query_cases as Q
import stack_depth_cases as K

ERR_LIMIT = -4
ARITHMETICS = pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
DEPTHS = pytest.mark.parametrize("depth", K.DEPTHS)


def assert_full_stack_rays_mean_something(d, ids, most):
    """At least 64 rays hold exactly D entries, none more; their closest hits are at least 4 distinct triangles (or every card
    of a smaller deck), and at least one of them misses everything."""
    full = most == d.depth
    assert int(full.sum()) >= 64 and int(most.max()) == d.depth
    hits = set(ids[full].tolist()) - {Q.MISS}
    assert len(hits) >= min(4, d.depth + 1), hits
    assert int((ids[full] == Q.MISS).sum()) >= 1


def test_the_gpu_tests_use_these_depths():
    assert K.DEPTHS == (1, 2, 15, 16, 22, 23, 28, 29) and K.LIMIT == 30 and max(K.DEPTHS) == K.LIMIT - 1
    assert set(K.SOME_DEPTHS) <= set(K.DEPTHS) and set(K.CALL_DEPTHS) <= set(K.DEPTHS)
    assert (K.W, K.H, K.RAY_DEPTH, K.SPP) == (32, 24, 4, 2)


@DEPTHS
def test_the_deck_is_the_chain_it_claims_to_be(depth):
    d = K.deck(depth)
    bvh, tris = d.scene.bvh, d.scene.triangulation
    assert len(bvh) == 2 * depth + 1 and d.scene.bvhMaxDepth == depth
    for k in range(depth):
        assert not bvh["isLeaf"][2 * k] and bvh["cutAxis"][2 * k] == 0
        assert (bvh["son1Id"][2 * k], bvh["son2Id"][2 * k]) == (2 * k + 1, 2 * k + 2) and bvh["isLeaf"][2 * k + 1]
    assert bvh["isLeaf"][2 * depth]
    leaves = bvh["nbTriangles"][bvh["isLeaf"] != 0]
    assert sorted(leaves.tolist()) == [1] * depth + [K.N_BIG] and len(tris) == depth + K.N_BIG
    assert bvh["nbTriangles"][2 * (depth - 1) + 1] == K.N_BIG  # the leaf pushed last: the top entry of a full stack
    assert not bvh["trianglesAABB"]["isEmpty"].any()
    # cards in the order of the chain: card k near x = 0.5 k, so a ray towards -x meets the rest of the chain first
    x = np.stack([tris["S1"][:, 0], tris["S2"][:, 0], tris["S3"][:, 0]], axis=1)
    for k in range(depth + 1):
        assert (np.abs(x[list(d.leaf_tris[k])] - 0.5 * k) <= 0.03 + 1e-6).all()
    assert d.most_pending == depth
    assert np.abs(np.stack([tris["S1"], tris["S2"], tris["S3"]])).max() < 2.0 ** 21 / 1024


@DEPTHS
@ARITHMETICS
def test_query_rays_fill_the_stack_next_to_rays_that_hold_nothing(depth, da):
    d = K.deck(depth)
    rays, kinds = K.query_rays(d)
    assert len(rays) == K.N_QUERY == 256 and set(kinds) == set("ABCZL")
    ids, most = K.occupancy(d.scene, rays, default_arithmetic=da)
    assert_full_stack_rays_mean_something(d, ids, most)
    assert (most[kinds == "A"] == depth).all()
    assert (most[kinds == "B"] <= 1).all() and (ids[kinds == "B"] != Q.MISS).any()  # towards +x: the leaf first
    assert (most[kinds == "C"] == 0).all() and (ids[kinds == "C"] == Q.MISS).all()
    z = rays[kinds == "Z"]["direction"][:, 0]
    assert (z == 0).all() and np.signbit(z).sum() == len(z) // 2
    if not da:  # (the limits are one ulp below the hits of the strict arithmetic; the other one's may lie an ulp nearer)
        assert (ids[kinds == "L"] == Q.MISS).all()
    for g in range(0, K.N_QUERY, 64):  # every wave of 64 lanes holds full stacks next to empty ones
        assert int((most[g:g + 64] == depth).sum()) >= 16 and int((most[g:g + 64] == 0).sum()) >= 8
        assert (np.diff(np.flatnonzero(most[g:g + 64] == depth)) <= 2).all()
    any_ids, any_most = K.occupancy(d.scene, rays, any_hit=True, default_arithmetic=da)
    assert int((any_most == depth).sum()) >= 64 and int(any_most.max()) == depth


@DEPTHS
def test_primary_rays_fill_the_stack(depth):
    """Both iterations of the image in the strict arithmetic, the first one in the default arithmetic too."""
    d = K.deck(depth)
    for it, da in ((0, False), (1, False), (0, True)):
        ids, most = K.occupancy(d.scene, K.primary_rays(d, it, default_arithmetic=da), default_arithmetic=da)
        assert_full_stack_rays_mean_something(d, ids, most)
        assert (most == depth).all()  # the view lies inside every card's box


@DEPTHS
def test_decks_with_empty_leaves_hold_every_other_entry(depth):
    """A child without triangles is never pushed, by the reference (its flagged box fails the test) or by the kernels (the
    upload stores it as a box that is never hit): the most a ray holds is D less the empty leaves among the first D."""
    d = K.deck(depth, empty_leaves=True)
    bvh = d.scene.bvh
    empty = [k for k in range(depth) if bvh["nbTriangles"][2 * k + 1] == 0]
    assert empty == ([k for k in range(depth) if (depth - 1 - k) % 3 == 0] if depth >= 2 else [])
    assert all(bvh["trianglesAABB"]["isEmpty"][2 * k + 1] == 1 for k in empty)
    assert d.most_pending == depth - len(empty)
    ids, most = K.occupancy(d.scene, K.primary_rays(d))
    assert (most == d.most_pending).all()
    assert len(set(ids.tolist()) - {Q.MISS}) >= min(4, depth + 1 - len(empty)) and (ids == Q.MISS).any()


def test_moved_cards_keep_the_stack_full():
    d = K.moved(29)
    assert not np.array_equal(d.scene.triangulation["S1"], K.deck(29).scene.triangulation["S1"])
    ids, most = K.occupancy(d.scene, K.primary_rays(d))
    assert_full_stack_rays_mean_something(d, ids, most)


def test_the_upload_accepts_29_levels_and_refuses_30():
    for sc in (K.deck(29).scene, K.deck(29, empty_leaves=True).scene, K.moved(29).scene, K.with_stated_depth(K.deck(29), 31)):
        backend.validate_scene(sc, K.W, K.H, K.RAY_DEPTH)
    too_deep = K.deck(K.LIMIT)
    assert len(too_deep.scene.bvh) == 2 * K.LIMIT + 1
    for sc in (too_deep.scene, K.with_stated_depth(too_deep, 5)):  # the depth the layout computes is what counts
        with pytest.raises(PtmiError) as e:
            backend.validate_scene(sc, K.W, K.H, K.RAY_DEPTH)
        assert e.value.code == ERR_LIMIT and "bvh depth 30 >= 30" in str(e.value)
