"""The traversal stacks of every kernel at every tree depth the upload accepts, FULL: the decks of stack_depth_cases.py, whose
rays hold as many pending entries as the tree is deep (tests/test_stack_depth_model.py asserts that on the CPU, ray by ray).

The stack of a traversal kernel lives in LDS with exactly as many levels as the uploaded tree has, and in the wavefront kernel
the words behind the last level are the leaf passes' keys and items.  An off-by-one in the sizing, in a push or in a pop would
not fault: it would overwrite a neighbour's words and change results on deep trees only.  So everything a call leaves behind
is held against the CPU oracle word for word, at the depths where the launch changes (the wait debt at 16, workgroups of 64
lanes from 23 on, the limit of 30) and at the smallest trees:

  ptmi_render         image, sample counts, the three histograms and the counters (gpu_cases.assert_same_state), in both
                      arithmetics, in the plain and the general instantiations, with and without culling code, in the
                      one-path-per-lane kernel (whose stack is a fixed 30 levels: the independent second implementation), and at
                      four depths in the statistics build, with SUPER_SAMPLING, the UNIFORM sampler and generic triangle records;
  ptmi_query_rays     against ray_query_cases.expected_hits, whose records count every box and triangle test: a lost or
                      duplicated entry shows even where the hit does not move;
  ptmi_trace_paths, ptmi_render_guides    against the yardsticks of path_query_cases.py and guide_cases.py;
  the limit           30 levels are refused with PTMI_ERR_LIMIT, and the context goes on to render 29;
  ptmi_update_triangles    moved cards under the same topology.

One oracle render and one set of expected hits per (deck, configuration), shared and left unchanged.
"""
import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, PtmiError, backend, render_scene, structs as S
from gpu_cases import assert_same_state, state
import cases
import gpu_cases
import guide_cases as G
import oracle_ffi as O
import path_query_cases as P
import ray_query_cases as Q
import stack_depth_cases as K

pytestmark = pytest.mark.gpu
W, H, RAY_DEPTH, SPP = K.W, K.H, K.RAY_DEPTH, K.SPP
DA, STATS, ONE_PATH_PER_LANE = backend.FLAG_DEFAULT_ARITHMETIC, backend.FLAG_SCHEDULER_STATS, backend.FLAG_MEGAKERNEL
ERR_LIMIT = -4
ARITHMETICS = pytest.mark.parametrize("da", [False, True], ids=["strict", "default"])
SWITCHES = ("PTMI_LEAF_CULL", "PTMI_GENERIC_SHADING", "PTMI_GENERIC_TRIANGLES", "PTMI_WIDE_WORKGROUPS", "PTMI_QUERY_MAX_BLOCKS")
_hits, _sums, _planes = {}, {}, {}


def lanes_of(depth):
    """The production instantiations over precomputed records: workgroups of 64 lanes from 23 levels on."""
    return 64 if depth >= 23 else 256


def render(d, monkeypatch, da, env=(), flags=0, **context):
    """(gpu_cases.state of a fresh context after SPP iterations, its scheduler statistics); every developer switch unset but `env`"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)
    be = gpu_cases.context(d.scene, W, H, RAY_DEPTH, flags=flags | (DA if da else 0), **context)
    try:
        assert be.literal_kernel_reason() is None  # the ordinary kernels, not the NaN-safe ones
        be.render(0, SPP)
        return state(be), be.scheduler_stats()
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- a. ptmi_render

PRODUCTION = [("plain", ()), ("general", (("PTMI_GENERIC_SHADING", "1"),)), ("no_culling_code", (("PTMI_LEAF_CULL", "0"),)),
              ("culling_forced", (("PTMI_LEAF_CULL", "2"),)), ("general_culling_forced", (("PTMI_GENERIC_SHADING", "1"), ("PTMI_LEAF_CULL", "2")))]


@ARITHMETICS
@pytest.mark.parametrize("depth", K.DEPTHS)
def test_renders_with_a_full_stack_equal_the_oracle(depth, da, monkeypatch):
    d = K.deck(depth)
    want = K.oracle(d, da)
    assert want["counters"]["surface_hits"] > 0 and want["counters"]["shadow_rays"] > 0
    for name, env in PRODUCTION:
        got, grid = render(d, monkeypatch, da, env)
        assert grid["workgroup_lanes"] == lanes_of(depth), (name, grid)
        assert_same_state(got, want)
    got, _ = render(d, monkeypatch, da, flags=ONE_PATH_PER_LANE)
    assert_same_state(got, want)


@ARITHMETICS
@pytest.mark.parametrize("depth", K.DEPTHS)
def test_renders_around_empty_children_equal_the_oracle(depth, da, monkeypatch):
    """Every third leaf without triangles: such a child is tested, counted and never pushed, so the pending entries are the
    leaves between them (stack_depth_cases.py) - under a stack that still has one level per level of the tree."""
    d = K.deck(depth, empty_leaves=True)
    want = K.oracle(d, da)
    for name, env in (PRODUCTION[0], PRODUCTION[3], PRODUCTION[1]):
        got, grid = render(d, monkeypatch, da, env)
        assert grid["workgroup_lanes"] == lanes_of(depth), (name, grid)
        assert_same_state(got, want)
    got, _ = render(d, monkeypatch, da, flags=ONE_PATH_PER_LANE)
    assert_same_state(got, want)


@ARITHMETICS
@pytest.mark.parametrize("depth", K.SOME_DEPTHS)
def test_the_other_instantiations_with_a_full_stack(depth, da, monkeypatch):
    """The statistics build, SUPER_SAMPLING, the UNIFORM sampler (general path logic) and generic triangle records."""
    d = K.deck(depth)
    got, grid = render(d, monkeypatch, da, flags=STATS)
    assert grid["trips_node"] > 0 and grid["leaf_item_violations"] == 0 and grid["workgroup_lanes"] == 256
    assert_same_state(got, K.oracle(d, da))
    got, grid = render(d, monkeypatch, da, super_sampling=True)
    assert grid["workgroup_lanes"] == 256
    assert_same_state(got, K.oracle(d, da, super_sampling=True))
    got, grid = render(d, monkeypatch, da, sampler=S.UNIFORM)
    assert grid["workgroup_lanes"] == lanes_of(depth)
    assert_same_state(got, K.oracle(d, da, sampler=S.UNIFORM))
    got, grid = render(d, monkeypatch, da, (("PTMI_GENERIC_TRIANGLES", "1"),))
    assert grid["workgroup_lanes"] == 256
    assert_same_state(got, K.oracle(d, da))


@ARITHMETICS
@pytest.mark.parametrize("depth", [23, 29])
def test_deep_decks_in_wide_workgroups(depth, da, monkeypatch):
    """PTMI_WIDE_WORKGROUPS=1: the same instantiations in workgroups of 256 lanes, whose level is 1024 bytes and not 256."""
    d = K.deck(depth)
    for env in ((), (("PTMI_GENERIC_SHADING", "1"),)):
        got, grid = render(d, monkeypatch, da, env + (("PTMI_WIDE_WORKGROUPS", "1"),))
        assert grid["workgroup_lanes"] == 256, grid
        assert_same_state(got, K.oracle(d, da))


def test_random_sampler_at_29_levels():
    """The bar of tests/test_parity_gpu.py::test_random_sampler_vs_oracle: counts, counters and the depth histogram are
    exact, the image's per-channel RMS error at most 1e-6 (the samples land in other pixels in another order)."""
    sc = K.deck(29).scene
    color, count, (dep, _, _), counters = render_scene(sc, W, H, RAY_DEPTH, SPP, sampler=S.RANDOM)
    o_color, o_count, (o_dep, _, _), totals = O.oracle_render(sc, W, H, RAY_DEPTH, SPP, sampler=S.RANDOM)
    assert np.array_equal(count, o_count) and counters == totals and np.array_equal(dep, o_dep)
    assert (cases.rms_per_channel(color, count, o_color, o_count) <= 1e-6).all()


# ---------------------------------------------------------------------------------------------- b. ptmi_query_rays

def expected_hits(d, da, any_hit):
    key = (id(d), da, any_hit)
    if key not in _hits:
        with np.errstate(all="ignore"):
            _hits[key] = (Q.expected_hits(d.scene, K.query_rays(d)[0], any_hit, default_arithmetic=da), d)
    return _hits[key][0]


def _tensors(rays):
    import torch
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(len(rays), 12).copy()).cuda()
    d_hits = torch.full((len(rays), 12), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return d_rays, d_hits


QUERY_BLOCK = 256  # lanes of a workgroup of query_rays_kernel and trace_paths_kernel (ptmi_literal_path.hpp: kBlock)


def reused_columns(n):
    """Positions into a batch of n rays, more than QUERY_BLOCK of them: the batch, the batch moved on by one place (the kinds
    alternate, so a full-stack ray lands on the column an empty-stack ray had, and the reverse), and the batch backwards.  On
    ONE workgroup every lane then takes two or three rays in turn, each on the stack column the ray before it left behind."""
    k = np.arange(n)
    order = np.concatenate([k, np.roll(k, -1), k[::-1]])
    assert len(order) > QUERY_BLOCK + n // 2  # (most lanes, at least, take a second ray)
    return order


@ARITHMETICS
@pytest.mark.parametrize("depth", K.DEPTHS)
def test_query_rays_with_full_stacks_next_to_empty_ones(depth, da, monkeypatch):
    """256 rays, in every 64 of which full-stack rays alternate with rays towards +x, rays that miss the root's children, rays
    with d.x = -0.0 and +0.0 and rays limited to an ulp below their hit: host and device form, closest and any hit.  Then 768
    rays (reused_columns) on ONE workgroup of 256 lanes, which loops over them three times: a ray starts on the column a
    full stack, an empty one or an any-hit query that ended early left behind."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    d = K.deck(depth)
    rays = K.query_rays(d)[0]
    order = reused_columns(len(rays))
    assert len(rays) == QUERY_BLOCK and len(order) == 3 * QUERY_BLOCK
    again = rays[order]
    be = gpu_cases.context(d.scene, W, H, RAY_DEPTH, flags=DA if da else 0)
    try:
        for any_hit in (False, True):
            want = expected_hits(d, da, any_hit)
            if not any_hit:
                assert (want["box_tests"] >= 2 * depth).sum() >= 64  # (a walk to the bottom of the chain)
            got = be.query_rays(rays["origin"], rays["direction"], rays["max_squared_distance"], any_hit=any_hit)
            assert not Q.describe_difference(got, want), Q.describe_difference(got, want)
            d_rays, d_hits = _tensors(rays)
            be.query_rays_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), any_hit=any_hit)
            be.synchronize()
            got = np.ascontiguousarray(d_hits.cpu().numpy()).view(S.RAY_HIT).reshape(-1)
            assert not Q.describe_difference(got, want), Q.describe_difference(got, want)
            monkeypatch.setenv("PTMI_QUERY_MAX_BLOCKS", "1")
            got = be.query_rays(again["origin"], again["direction"], again["max_squared_distance"], any_hit=any_hit)
            monkeypatch.delenv("PTMI_QUERY_MAX_BLOCKS")
            assert not Q.describe_difference(got, want[order]), Q.describe_difference(got, want[order])
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- c. ptmi_trace_paths, ptmi_render_guides

@ARITHMETICS
@pytest.mark.parametrize("depth", K.CALL_DEPTHS)
def test_trace_paths_with_full_stacks(depth, da, monkeypatch):
    """The query rays that have no exact zero in their direction (192), twice over in the order of reused_columns' first two
    parts: 384 rays, each under the index of its position, on two workgroups and then on ONE that loops over them."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    d = K.deck(depth)
    rays = K.path_rays(d)
    rays = rays[reused_columns(len(rays))[:2 * len(rays)]]
    assert len(rays) > QUERY_BLOCK
    if (depth, da) not in _sums:
        with np.errstate(all="ignore"):
            _sums[depth, da] = P.Yardstick(d.scene, RAY_DEPTH, S.JITTERED, default_arithmetic=da).sums(rays, n_iterations=2, index_stride=P.STRIDE)
    want = _sums[depth, da]
    assert want["surface_hits"].max() >= 2 and (want["box_tests"] >= 2 * depth).sum() >= 64
    be = gpu_cases.context(d.scene, W, H, RAY_DEPTH, flags=DA if da else 0)
    try:
        got = be.trace_paths(rays["origin"], rays["direction"], n_iterations=2, index_stride=P.STRIDE)
        assert not P.describe_difference(got, want), P.describe_difference(got, want)
        monkeypatch.setenv("PTMI_QUERY_MAX_BLOCKS", "1")
        got = be.trace_paths(rays["origin"], rays["direction"], n_iterations=2, index_stride=P.STRIDE)
        assert not P.describe_difference(got, want), P.describe_difference(got, want)
    finally:
        be.release()


@ARITHMETICS
@pytest.mark.parametrize("depth", K.CALL_DEPTHS)
def test_guides_with_full_stacks(depth, da, monkeypatch):
    """As tests/test_guide_buffers_gpu.py::test_scenes: strict with the JITTERED sampler, default with the UNIFORM one."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    d = K.deck(depth)
    sampler = S.UNIFORM if da else S.JITTERED
    if (depth, da) not in _planes:
        _planes[depth, da] = G.Yardstick(d.scene, W, H, sampler, da).planes(0, 2)
    want, excluded = _planes[depth, da]
    assert not excluded.any() and 0 < (want["hit_count"] > 0).sum() < W * H
    be = gpu_cases.context(d.scene, W, H, RAY_DEPTH, flags=DA if da else 0, sampler=sampler)
    try:
        got = be.render_guides(0, 2)
        assert not G.describe_difference(got, want, excluded), G.describe_difference(got, want, excluded)
    finally:
        be.release()


# ---------------------------------------------------------------------------------------------- d. the limit, e. an update

def test_a_context_refuses_30_levels_and_goes_on_to_render_29(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    too_deep, d = K.deck(K.LIMIT), K.deck(29)
    be = Backend().setup_context(W, H, RAY_DEPTH, d.scene.lightsSize)
    try:
        for sc in (too_deep.scene, K.with_stated_depth(too_deep, 5)):
            with pytest.raises(PtmiError) as e:
                be.initialize_memory(sc)
            assert e.value.code == ERR_LIMIT and "bvh depth 30 >= 30" in str(e.value)
        be.initialize_memory(d.scene)
        be.render(0, SPP)
        assert be.scheduler_stats()["workgroup_lanes"] == 64
        assert_same_state(state(be), K.oracle(d, False))
    finally:
        be.release()


@ARITHMETICS
def test_moved_cards_at_29_levels(da, monkeypatch):
    """ptmi_update_triangles keeps the topology: 29 levels before and after, and the refit boxes still make every level push."""
    d, m = K.deck(29), K.moved(29)
    want = K.oracle(m, da)
    assert not np.array_equal(want["color"], K.oracle(d, da)["color"])  # (the cards did move)
    fresh, _ = render(m, monkeypatch, da)
    assert_same_state(fresh, want)
    be = gpu_cases.context(d.scene, W, H, RAY_DEPTH, flags=DA if da else 0)
    try:
        be.render(0, 1)
        info = be.update_triangles(m.scene.triangulation)
        assert info["levels"] == 29, info
        be.clear()
        be.render(0, SPP)
        assert be.scheduler_stats()["workgroup_lanes"] == 64
        got = state(be)
    finally:
        be.release()
    assert_same_state(got, want)
    assert_same_state(got, fresh)
