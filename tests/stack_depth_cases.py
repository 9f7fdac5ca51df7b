"""A hand-made scene whose rays FILL the traversal stack, and the walk that proves it (test_stack_depth_model.py on the CPU,
test_stack_depth_gpu.py on the GPU).  No product code is changed by any of it.

Every traversal kernel keeps its stack in LDS with exactly as many levels as the uploaded tree is deep, and in the wavefront
kernel the words behind the last level belong to the leaf passes: an off-by-one in the sizing, in a push or in a pop would not
fault, it would render a quietly wrong image on deep trees only.  So the scene is a tree of a chosen depth D in which rays
hold D pending entries, the most a tree of D levels can ask for.

The deck: D + 1 large thin triangles ("cards") stacked along x, card k near x = 0.5 k, every vertex jittered a few hundredths in
x.  A card's vertices lie around a jittered centre of the y-z plane at random angles and radii of 3 to 5 units - random, but
kept only if (rejection sampling, seeded)
  * the card's box holds the whole view of the camera below, with a margin: every camera ray pierces every card's BOX;
  * the card itself covers between a fifth and three fifths of that view, and some of it shows between the three cards in
    front of it: the closest hit varies from ray to ray;
  * the card stays clear of one fixed camera ray, the "hole": the rays around it miss every card.
Materials cycle over the Cornell box's three plain ones, there is one point light and a grey sky.  Every coordinate stays far
below 2^21, so the upload picks the ordinary production kernels.

The tree is written by hand in the shape of scene_record_cases.chain_scene: inner node k is bvh[2k] with cutAxis 0, its son1 the
leaf of card k, its son2 inner node k + 1; the last inner node's son2 is the leaf of card D.  The boxes are ptmi_bvh_refit's.
The reference visits `dir[axis] > 0 ? son1 : son2` first (FullKernel.cl:660-697).  A ray that travels towards -x therefore
descends into the rest of the chain and pushes a leaf on every level: at the bottom it holds D entries, and D is also the depth
scene_layout.cpp computes and the number of levels the kernels' stacks get.  A ray that travels towards +x visits the leaf
first and never holds more than the one inner node behind it.

Options of the builder:
  big_leaf      the card whose leaf is pushed last (card D - 1, the top entry of a full stack) is 9 coincident triangles: one
                leaf of REF_COUNT_BIG or more, whose range comes from the side table;
  empty_leaves  every third leaf, counted down from the one pushed last, holds no triangle (nbTriangles = 0, and ptmi_bvh_refit
                flags its box isEmpty).  The reference's box test refuses a flagged box and the upload stores such a child as
                one that is never hit, so NEITHER side ever pushes it: in this variant the most a ray holds is D less the empty
                leaves among the first D, which `Deck.most_pending` states and the model test asserts.  It is rendered for what
                it does to the entries around the empty children, not for a full stack.
"""
import copy

import numpy as np

from opencl_pathtracer_amd import scenes, structs as S
import path_query_cases as P
import ray_query_cases as Q
import scene_update_cases as U

f32 = np.float32
W, H, RAY_DEPTH, SPP = 32, 24, 4, 2
# the boundaries tests/kernel_choice_model.cpp names - the wait debt changes at 16, the workgroups narrow at 23, the upload
# refuses 30 - and the smallest trees
DEPTHS = (1, 2, 15, 16, 22, 23, 28, 29)
SOME_DEPTHS = (2, 22, 23, 29)  # the further instantiations (statistics, SUPER_SAMPLING, UNIFORM, generic triangle records)
CALL_DEPTHS = (1, 22, 23, 29)  # ptmi_trace_paths and ptmi_render_guides
LIMIT = 30                     # PTMI_BVH_MAX_DEPTH
SPAN = 0.05                    # the camera's right vector: the view is SPAN x SPAN * H / W at unit distance
CAMERA_GAP = 8.0               # from the camera to the nearest card
HOLE = (0.2, -0.15)            # the sample (x, y in [-0.5, 0.5]) of the camera ray every card stays clear of
N_BIG = 9
PATTERN = "ABACAZAL"           # the kinds of 8 consecutive query rays (query_rays)
N_QUERY = 256


# ---------------------------------------------------------------------------------------------- the deck

def _inside(tri, pts):
    """bool[n, m]: point m of `pts` (m, 2) lies inside triangle n of `tri` (n, 3, 2)"""
    a, b, c = tri[:, None, 0], tri[:, None, 1], tri[:, None, 2]
    p = pts[None]

    def side(u, v):
        return (v[..., 0] - u[..., 0]) * (p[..., 1] - u[..., 1]) - (v[..., 1] - u[..., 1]) * (p[..., 0] - u[..., 0])

    s1, s2, s3 = side(a, b), side(b, c), side(c, a)
    return ((s1 > 0) & (s2 > 0) & (s3 > 0)) | ((s1 < 0) & (s2 < 0) & (s3 < 0))


def _card(rs, distance, hidden):
    """The y-z corners (3, 2) of one card `distance` in front of the camera, and which of the 48 rays of an 8 x 6 grid over the
    view it covers: see the module's docstring.  hidden: the grid rays that the three cards in front of this one cover (where
    they leave too little free, less is asked)."""
    half = np.array([0.5 * SPAN * distance, 0.5 * SPAN * distance * H / W])
    gx, gy = np.meshgrid((np.arange(8) + 0.5) / 8 - 0.5, (np.arange(6) + 0.5) / 6 - 0.5)
    view = np.stack([gx.ravel(), gy.ravel()], axis=1) * 2 * half
    hole = np.array(HOLE) * 2 * half
    around = hole + np.array([[0, 0], [1, 1], [1, -1], [-1, 1], [-1, -1]]) * 0.15 * half
    for attempt in range(64):
        n = 2048
        centre = rs.uniform(-0.3, 0.3, (n, 1, 2))
        angle, radius = rs.uniform(0, 2 * np.pi, (n, 3)), rs.uniform(3.0, 5.0, (n, 3))
        tri = centre + np.stack([np.cos(angle), np.sin(angle)], axis=2) * radius[..., None]
        lo, hi = tri.min(axis=1), tri.max(axis=1)
        boxed = ((lo < -(1.5 * half + 0.1)) & (hi > 1.5 * half + 0.1)).all(axis=1)
        covers = _inside(tri, view)
        covered, seen = covers.mean(axis=1), (covers & ~hidden).sum(axis=1)
        clear = ~_inside(tri, around).any(axis=1)
        ok = np.flatnonzero(boxed & clear & (covered >= 0.2) & (covered <= 0.6) & (seen >= (4, 2, 1, 0)[attempt // 16]))
        if len(ok):
            return tri[ok[0]], covers[ok[0]]
    raise AssertionError("no card found")


class Deck:
    """scene: the scenes.Scene with its tree; depth: D; leaf_tris[k]: the triangles of leaf k; most_pending: the entries a ray
    that pierces every box holds at the bottom (D without empty leaves)."""

    def __init__(self, scene, depth, leaf_tris):
        self.scene, self.depth, self.leaf_tris = scene, depth, leaf_tris
        self.most_pending = sum(1 for t in leaf_tris[:depth] if len(t))


_decks = {}


def deck(depth, big_leaf=True, empty_leaves=False):
    """The deck of `depth` levels (built once per set of options; read-only)."""
    key = (depth, big_leaf, empty_leaves)
    if key not in _decks:
        _decks[key] = _build(depth, big_leaf, empty_leaves)
    return _decks[key]


def _build(depth, big_leaf, empty_leaves):
    rs = np.random.default_rng(1000 + depth)
    camera_x = 0.5 * depth + CAMERA_GAP
    last_pushed = depth - 1
    # (a deck of one level keeps both of its cards: an empty one would leave a single triangle to hit)
    empty = {k for k in range(depth) if empty_leaves and depth >= 2 and (last_pushed - k) % 3 == 0}
    big = next(k for k in range(last_pushed, -1, -1) if k not in empty) if big_leaf else -1
    # from the camera's end of the deck backwards (drawn for empty leaves too: the other cards do not depend on the options)
    corners, covers = {}, {}
    for k in range(depth, -1, -1):
        hidden = np.zeros(48, bool)
        for j in range(k + 1, min(k + 4, depth + 1)):
            hidden |= covers[j]
        yz, covers[k] = _card(rs, camera_x - 0.5 * k, hidden)
        corners[k] = np.concatenate([(0.5 * k + rs.uniform(-0.03, 0.03, 3))[:, None], yz], axis=1).astype(f32)
    parts, leaf_tris, first = [], [], 0
    for k in range(depth + 1):
        v = corners[k]
        if k in empty:
            leaf_tris.append(range(first, first))
            continue
        n = N_BIG if k == big else 1
        parts.append(scenes.triangle_create(*(np.tile(v[j], (n, 1)) for j in range(3)), mat_pos=k % 3))
        leaf_tris.append(range(first, first + n))
        first += n
    tris = scenes._concat_tris(parts)
    assert np.abs(np.stack([tris["S1"], tris["S2"], tris["S3"]])).max() < 64  # (far below the 2^21 of the NaN-safe kernels)

    bvh = np.frombuffer(bytearray((2 * depth + 1) * S.Node.itemsize), dtype=S.Node)

    def leaf(node, k):
        bvh["triangleStartIndex"][node], bvh["nbTriangles"][node], bvh["isLeaf"][node] = leaf_tris[k].start, len(leaf_tris[k]), 1

    for k in range(depth):
        bvh["triangleStartIndex"][2 * k], bvh["nbTriangles"][2 * k] = leaf_tris[k].start, len(tris) - leaf_tris[k].start
        bvh["cutAxis"][2 * k] = 0
        bvh["son1Id"][2 * k], bvh["son2Id"][2 * k] = 2 * k + 1, 2 * k + 2
        leaf(2 * k + 1, k)
    leaf(2 * depth, depth)
    rc, msg, bvh = U.bvh_refit(tris, bvh)
    assert rc == 0, msg
    for k in empty:
        assert bvh["trianglesAABB"]["isEmpty"][2 * k + 1] == 1

    base = scenes.cornell_box(W, H)
    sky, texels = scenes.no_sky((200, 200, 200, 255))
    lights = scenes._records([scenes.light_point((camera_x - 2.0, 2.5, 2.0), power=80.0)], S.Light)
    pos, d, r, u = scenes.camera((camera_x, 0.0, 0.0), (-1, 0, 0), (0, SPAN, 0), (0, 0, SPAN * H / W))
    sc = scenes.Scene(tris, lights, base.materiaux, np.zeros(0, S.Texture), texels, sky, pos, d, r, u, bvh=bvh, bvhMaxDepth=depth,
                      name=f"deck{depth}")
    return Deck(sc, depth, leaf_tris)


_moved = {}


def moved(depth):
    """The deck with every vertex displaced by up to 0.02 (scene_update_cases.displaced) under the refit tree: the topology,
    and with it the depth, stays."""
    if depth not in _moved:
        d = deck(depth)
        _moved[depth] = Deck(U.moved_scene(d.scene, U.displaced(d.scene.triangulation, 7)), depth, d.leaf_tris)
    return _moved[depth]


# ---------------------------------------------------------------------------------------------- the walk

class OccupancyWalker(Q.Walker):
    """ray_query_cases.Walker, whose every decision is the CPU oracle's, with a walk that also reports the greatest number of
    pending entries.  An entry is pushed exactly where the reference pushes one (both boxes hit: FullKernel.cl:680-684) - and
    where the kernels push one: a child the upload stores as never hit (an isEmpty box) fails the oracle's box test too."""

    def walk_occupancy(self, origin, direction, limit=np.inf, any_hit=False):
        """(what walk() returns, the greatest number of pending entries): the one walk, listened to through its on_push"""
        pending = [0]
        return self.walk(origin, direction, limit, any_hit, on_push=pending.append), max(pending)


def occupancy(scene, rays, any_hit=False, default_arithmetic=False):
    """(closest-hit triangle ids uint32[n] (Q.MISS: none), most pending entries int[n]) of `rays` on `scene`"""
    w = OccupancyWalker(scene, default_arithmetic)
    ids, most = np.zeros(len(rays), np.uint32), np.zeros(len(rays), np.int64)
    for k, r in enumerate(rays):
        h, most[k] = w.walk_occupancy(r["origin"], r["direction"], r["max_squared_distance"], any_hit)
        ids[k] = h["triangle_id"]
    return ids, most


# ---------------------------------------------------------------------------------------------- the rays

def primary_rays(d, it=0, sampler=S.JITTERED, default_arithmetic=False):
    """The W x H rays Kernel_Main makes for iteration `it` of the deck's image (path_query_cases.camera_rays)."""
    return P.camera_rays(d.scene, W, H, it, sampler, default_arithmetic)


def _view_rays(d, rs, n, towards_minus_x=True):
    """n rays through the camera's view, from the camera's side (towards -x) or from behind card 0 (towards +x): origins a
    little off the axis, directions of several lengths, every 8th one through the hole."""
    camera_x = float(d.scene.cameraPosition[0])
    sx, sy = rs.uniform(-0.5, 0.5, n), rs.uniform(-0.5, 0.5, n)
    sx[::8], sy[::8] = HOLE[0] + rs.uniform(-0.01, 0.01, len(sx[::8])), HOLE[1] + rs.uniform(-0.01, 0.01, len(sy[::8]))
    length = rs.uniform(0.5, 3.0, n)
    if towards_minus_x:
        o = np.stack([np.full(n, camera_x), np.zeros(n), np.zeros(n)], axis=1)
        direction = np.stack([-np.ones(n), SPAN * sx, SPAN * H / W * sy], axis=1) * length[:, None]
    else:
        # the mirror image: from 8 units behind card 0 towards the camera's position, through the same points of the view
        o = np.stack([np.full(n, -CAMERA_GAP), SPAN * sx * (camera_x + CAMERA_GAP), SPAN * H / W * sy * (camera_x + CAMERA_GAP)], axis=1)
        direction = np.stack([np.ones(n), -SPAN * sx, -SPAN * H / W * sy], axis=1) * length[:, None]
    rays = Q.make_rays(o.astype(f32), direction.astype(f32))
    assert (rays["direction"][:, :3] != 0).all()
    return rays


_queries = {}


def query_rays(d):
    """(rays structs.RAY[256], kinds str[256]) - read-only, built once per deck.  Of 8 consecutive rays (PATTERN):
      A  four travel towards -x through the view: they fill the stack (an eighth of them through the hole: they miss);
      B  one travels towards +x through the same view: at most one entry;
      C  one passes far outside the deck: it misses both children of the root;
      Z  one has d.x = -0.0 or +0.0 (in turn) and starts either between two cards or inside the x range of one card's box;
      L  one is a ray of kind A limited to one ulp below its own closest hit (ray_query_cases.limited_rays, strict arithmetic).
    So a lane that holds a full stack sits between lanes that hold none, in every group of 64."""
    key = id(d)
    if key in _queries:
        return _queries[key][:2]
    rs = np.random.default_rng(77 + d.depth)
    sc = d.scene
    camera_x = float(sc.cameraPosition[0])
    n_each = N_QUERY // 8
    a, b = _view_rays(d, rs, 4 * n_each), _view_rays(d, rs, n_each, towards_minus_x=False)
    far = np.stack([np.full(n_each, camera_x), rs.uniform(40, 60, n_each), rs.uniform(-5, 5, n_each)], axis=1)
    c = Q.make_rays(far.astype(f32), (np.array([-1.0, 0.001, 0.002]) * rs.uniform(0.5, 2.0, (n_each, 1))).astype(f32))
    # Z: in the plane x = x0, from 10 units off the axis through it
    phi = rs.uniform(0, 2 * np.pi, n_each)
    k = rs.integers(0, d.depth + 1, n_each)
    leaf_node = np.where(k == d.depth, 2 * d.depth, 2 * k + 1)
    box = sc.bvh["trianglesAABB"][leaf_node]
    x0 = np.where((np.arange(n_each) // 2) % 2 == 0, 0.5 * k + 0.25, 0.5 * (box["pMin"][:, 0] + box["pMax"][:, 0]))
    zero = np.where(np.arange(n_each) % 2 == 0, f32(-0.0), f32(0.0))
    z = Q.make_rays(np.stack([x0, -10 * np.cos(phi), -10 * np.sin(phi)], axis=1).astype(f32),
                    np.stack([zero, np.cos(phi), np.sin(phi)], axis=1).astype(f32))
    assert (np.signbit(z["direction"][0::2, 0])).all() and not np.signbit(z["direction"][1::2, 0]).any()
    # L: further rays of kind A, those that hit
    more = _view_rays(d, rs, 4 * n_each)
    limited = Q.limited_rays(more, Q.expected_hits(sc, more))
    n_hit = len(limited) // 3
    assert n_hit >= n_each
    lim = limited[n_hit:2 * n_hit][:n_each]  # (the middle third: one ulp below)
    rays, kinds = np.zeros(N_QUERY, S.RAY), []
    took = dict(A=0, B=0, C=0, Z=0, L=0)
    source = dict(A=a, B=b, C=c, Z=z, L=lim)
    for i in range(N_QUERY):
        kind = PATTERN[i % 8]
        rays[i] = source[kind][took[kind]]
        took[kind] += 1
        kinds.append(kind)
    rays.setflags(write=False)
    _queries[key] = (rays, np.array(kinds), d)  # (the deck is kept so that its id stays its own)
    return rays, _queries[key][1]


def path_rays(d):
    """The query rays without an exact zero in their direction, unlimited: what ptmi_trace_paths is asked (its yardstick's
    zero-basis camera does not reproduce the sign of a zero)."""
    rays, kinds = query_rays(d)
    out = rays[np.isin(kinds, ["A", "B", "C"])].copy()
    assert (out["direction"][:, :3] != 0).all() and np.isinf(out["max_squared_distance"]).all()
    return out


# ---------------------------------------------------------------------------------------------- the renders' yardstick

_oracle = {}


def oracle(d, default_arithmetic, sampler=S.JITTERED, super_sampling=False):
    """One oracle render of the deck's W x H image (RAY_DEPTH, SPP iterations) per configuration, in the form of
    gpu_cases.state; shared and left unchanged."""
    import oracle_ffi as O
    key = (id(d), default_arithmetic, sampler, super_sampling)
    if key not in _oracle:
        color, count, hists, totals = O.oracle_render(d.scene, W, H, RAY_DEPTH, SPP, sampler=sampler, super_sampling=super_sampling,
                                                      default_arithmetic=default_arithmetic)
        _oracle[key] = (dict(color=color.view(np.uint32).copy(), count=count.copy(), stats=[h.copy() for h in hists], counters=totals), d)
    return _oracle[key][0]


def with_stated_depth(d, stated_depth):
    """The deck's scene with another claim in bvhMaxDepth: the depth that counts is the one the layout computes."""
    sc = copy.copy(d.scene)
    sc.bvhMaxDepth = stated_depth
    return sc
