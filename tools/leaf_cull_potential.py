#!/usr/bin/env python3
"""What the leaf culling of csrc/leaf_cull.h can skip on a scene, measured on the CPU with the real rule and certificate.

Walks the queries of a fixed sample of paths (the bounces the oracle traces: pto_trace_path) through build_layout's records with
tests/leaf_cull_model.cpp and tests/leaf_cull_wide_model.cpp, box and triangle decisions from the oracle's exported deciders, and
writes a JSON with
  * leaf visits and triangle tests skipped, split into direct and pushed leaves, closest-hit and shadow queries - what the
    kernel does: the leaves of both tiers of the certificate under the wide rule,
  * the same shares for the tight tier alone under its own rule (`tight_only`: the kernel before the wide tier),
  * the share of leaves that get no certificate, per tier,
  * what the margins and the certificate cost against a zero-margin rule on every ordinary leaf (not a valid rule: the ceiling).

usage: tools/leaf_cull_potential.py [--scene tris1m] [--width 1920 --height 1080 --depth 10] [--paths 400] [--out profiles/...json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opencl_pathtracer_amd import bvh_create, scenes  # noqa: E402
import leaf_cull_cases as K  # noqa: E402
import leaf_cull_wide_cases as KW  # noqa: E402
import oracle_ffi as O  # noqa: E402


def constants(m):
    import ctypes as C
    tight, wide = (C.c_double * 4)(), (C.c_double * 4)()
    m.cull_constants(tight)
    m.wide_constants(wide)
    return [float(x) for x in tight] + [float(x) for x in wide]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tris1m")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--paths", type=int, default=400)
    ap.add_argument("--strict", action="store_true", help="the strict arithmetic instead of the reference's default build")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    da = not a.strict
    m = KW.build_model(tempfile.mkdtemp())
    lib = O.oracle(da)
    sc = bvh_create(scenes.build(a.scene, a.width, a.height))
    lay = K.Layout(m, sc)
    bits, b = KW.check_records(lay), KW.bits(m)
    assert bits["tight_differs"] == bits["wide_differs"] == bits["stray_bits"] == bits["tight_without_wide"] == 0, bits
    rs = np.random.default_rng(1)
    keys = ("queries", "n_tri", "direct", "popped", "direct_culled", "direct_culled_tris", "popped_culled", "popped_culled_tris",
            "direct_uncertified", "ceiling_leaves", "ceiling_tris")
    tot = {kind: dict.fromkeys(keys, 0) for kind in ("closest_hit", "shadow")}
    tight = {kind: dict.fromkeys(keys[1:9], 0) for kind in ("closest_hit", "shadow")}
    for _ in range(a.paths):
        x, y = int(rs.integers(0, a.width)), int(rs.integers(0, a.height))
        for origin, direction, limit, shadow, _hit, _bounce in K.path_queries(lib, sc, a.width, a.height, a.depth, x, y, 0, da)[0]:
            t = tot["shadow" if shadow else "closest_hit"]
            real = KW.walk(lay, lib, origin, direction, limit, shadow, b["mask_7"], True)
            old = KW.walk(lay, lib, origin, direction, limit, shadow, b["mask_7_tight_only"], False)
            ceiling = lay.walk(lib, origin, direction, limit, shadow, 3)
            assert all(real[k] == old[k] == ceiling[k] for k in ("hit", "limit_bits", "n_bbx", "n_tri")), (real, old, ceiling)
            t["queries"] += 1
            for k in keys[1:9]:
                t[k] += real[k]
                tight["shadow" if shadow else "closest_hit"][k] += old[k]
            t["ceiling_leaves"] += ceiling["direct_culled"] + ceiling["popped_culled"]
            t["ceiling_tris"] += ceiling["direct_culled_tris"] + ceiling["popped_culled_tris"]
    lay.free()
    all_tri = sum(t["n_tri"] for t in tot.values())
    share = lambda n: round(n / max(all_tri, 1), 4)
    result = {
        "scene": a.scene, "width": a.width, "height": a.height, "depth": a.depth, "paths": a.paths,
        "arithmetic": "default" if da else "strict", "iteration": 0,
        "leaves": bits["leaves"], "leaves_without_certificate_share": round(1 - bits["wide"] / max(bits["leaves"], 1), 4),
        "triangle_tests": all_tri,
        "skipped_share_direct": share(sum(t["direct_culled_tris"] for t in tot.values())),
        "skipped_share_direct_and_pushed": share(sum(t["direct_culled_tris"] + t["popped_culled_tris"] for t in tot.values())),
        "skipped_share_zero_margin_no_certificate": share(sum(t["ceiling_tris"] for t in tot.values())),
        "by_query_kind": tot,
        "tight_only": {
            "leaves_without_certificate_share": round(1 - bits["tight"] / max(bits["leaves"], 1), 4),
            "skipped_share_direct": share(sum(t["direct_culled_tris"] for t in tight.values())),
            "skipped_share_direct_and_pushed": share(sum(t["direct_culled_tris"] + t["popped_culled_tris"] for t in tight.values())),
            "by_query_kind": tight,
        },
        "constants": dict(zip(("kRel", "kAbs", "kKappaMax", "kEpsAbsMax", "kRelWide", "kAbsWide", "kKappaWideMax", "kEpsAbsWideMax"), constants(m))),
    }
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
