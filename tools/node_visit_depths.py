#!/usr/bin/env python3
"""At which tree depths the node visits of a scene's queries fall - and how few nodes would have to be served from LDS to catch
a given share of them (why "the top of the BVH from LDS" cannot pay).  CPU only.

Takes a fixed sample of paths (the bounces the oracle traces, as tools/leaf_cull_potential.py does), walks every query of theirs
through scene.bvh near child first as the reference does, and counts the inner nodes whose two child boxes the walk tests, by the
node's depth and per node.  Two approximations, both towards MORE visits near the root, i.e. in favour of an LDS copy of the top:
  * a closest-hit query walks with its FINAL limit - the squared distance of the hit it ends with, infinite on a miss - from the
    start (the reference's limit shrinks to it hit by hit, so it enters some boxes more on the way, which lie deep);
  * a shadow query is not cut at its first accepted triangle.  Its limit is the LINEAR distance to the light, in the squared
    slot, as the reference has it (FullKernel.cl:938).
A box counts as hit when the ray's slab interval is not empty, ends in front of the origin and starts within the limit.

usage: tools/node_visit_depths.py [--scene tris1m] [--width 1920 --height 1080 --depth 10] [--paths 60] [--hottest 255]
"""
import argparse
import json
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opencl_pathtracer_amd import bvh_create, scenes  # noqa: E402
import leaf_cull_cases as K  # noqa: E402
import oracle_ffi as O  # noqa: E402


def walk(nodes, origin, direction, limit, visits):
    """One query through the tree; visits[(node, depth)] += 1 for every inner node whose children are tested."""
    lo, hi, leaf, son1, son2, axis = nodes
    with np.errstate(divide="ignore"):
        inv = 1.0 / direction

    def hit(n):
        t0, t1 = (lo[n] - origin) * inv, (hi[n] - origin) * inv
        near, far = np.nanmax(np.minimum(t0, t1)), np.nanmin(np.maximum(t0, t1))
        return near <= far and far >= 0 and max(near, 0.0) ** 2 <= limit

    stack = [(0, 0)]
    while stack:
        n, depth = stack.pop()
        if leaf[n]:
            continue
        visits[(n, depth)] += 1
        first, second = (son1[n], son2[n]) if direction[axis[n]] > 0 else (son2[n], son1[n])
        for child in (second, first):  # the near child is popped first
            if hit(child):
                stack.append((int(child), depth + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--paths", type=int, default=60)
    ap.add_argument("--hottest", type=int, default=255, help="nodes an LDS copy could hold (64 bytes each)")
    a = ap.parse_args()
    lib = O.oracle(True)
    sc = bvh_create(scenes.build(a.scene, a.width, a.height))
    b = sc.bvh
    nodes = (b["trianglesAABB"]["pMin"][:, :3].astype(np.float64), b["trianglesAABB"]["pMax"][:, :3].astype(np.float64),
             b["isLeaf"] != 0, b["son1Id"], b["son2Id"], b["cutAxis"])
    rs = np.random.default_rng(1)
    visits, n_queries = Counter(), 0
    for _ in range(a.paths):
        x, y = int(rs.integers(0, a.width)), int(rs.integers(0, a.height))
        queries = K.path_queries(lib, sc, a.width, a.height, a.depth, x, y, 0, True)[0]
        for k, (origin, direction, limit, shadow, hit_tri, _bounce) in enumerate(queries):
            if not shadow and hit_tri is not None:
                # the hit point is where the path's next query starts (a shadow ray: exactly; a scattered one: 0.001 off)
                d = np.asarray(queries[k + 1][0], np.float64)[:3] - np.asarray(origin, np.float64)[:3]
                limit = float(d @ d)
            walk(nodes, np.asarray(origin, np.float64)[:3], np.asarray(direction, np.float64)[:3], limit, visits)
            n_queries += 1
    total = sum(visits.values())
    by_depth = Counter()
    for (_, depth), n in visits.items():
        by_depth[depth] += n
    upto = lambda d: sum(n for k, n in by_depth.items() if k <= d) / total
    hottest = sum(n for _, n in visits.most_common(a.hottest)) / total
    print(json.dumps({
        "scene": a.scene, "paths": a.paths, "queries": n_queries, "node_visits": total, "tree_depth": int(sc.bvhMaxDepth),
        "share_of_visits_depth_0_to_3": round(upto(3), 4), "share_of_visits_depth_0_to_7": round(upto(7), 4),
        "share_of_visits_depth_13_and_deeper": round(1 - upto(12), 4),
        "share_by_depth": {str(d): round(by_depth[d] / total, 4) for d in sorted(by_depth)},
        "hottest_nodes": a.hottest, "hottest_nodes_lds_bytes": 64 * a.hottest, "share_of_visits_hottest_nodes": round(hottest, 4),
    }, indent=1))


if __name__ == "__main__":
    main()
