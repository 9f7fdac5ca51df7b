// bvh_build.cpp - host-side binned-SAH BVH build behind ptmi_bvh_create().
//
// Produces the Node[] the integrator consumes, bit-compatible with the
// reference's BVH_Create (Controleur/PathTracer_BVH.cpp:12-37) and its recursive
// BVH_BuildStructure (:109-356).  Every decision at a node - the leaf tests, k1,
// the bin of a centroid, the scans, the SAH, the best split, the children's
// boxes - is made by bvh_build_common.h, the header the device builder and its
// model use, so the three cannot drift apart.  What is the host's own is here:
// the depth-first recursion with pre-order node numbering (left child = parent +
// 1), the Hoare style in-place partition of the triangle array, the depth and
// capacity guards, and the lifetime of the scratch, which decides what a split on
// a skipped axis sees.  tests/test_bvh.py checks equality against the reference
// builder compiled unmodified (oracle/_ref/libref_bvh.so) and against committed
// tree digests.
//
// Host only: no device needed.  Compile with -ffp-contract=off.

#include <algorithm>
#include <climits>
#include <string>
#include <cstring>
#include <vector>

#include "bvh_build_common.h"
#include "ptmi.h"
#include "ptmi_internal.h"

using namespace ptmi_bvh;

namespace {

struct Builder {
    ptmi_triangle* tris;
    ptmi_node* nodes;
    uint32_t size = 0, max_depth = 0, depth = 0;

    // The reference keeps its bins, scans and k1 as function-level statics shared by every recursion level
    // (BVH.cpp:154-161), and a node fills them only for the axes it bins.  When the SAH picks an axis that was skipped at
    // this node (every real cost >= the INT_MAX of a skipped axis), it splits with the k1 and the scans of the last node
    // in depth-first order that binned that axis.  The scans are a function of the bins, so the bins are what is kept:
    // the bins, counts and k1 of an axis are reset only at a node that bins that axis; sah is reset at every node.
    PBox bins[3][kBins];
    int counts[3][kBins];
    float sah[3][kBins - 1];
    double rpart[kBins - 1];
    float k1[3] = { 0, 0, 0 };
    bool failed = false;    // a centroid fell outside its node's bins, or a split left a side empty
    uint32_t capacity = 0;  // nodes the caller's array holds: 2n - 1

    void make_node(uint32_t idx, uint32_t start, uint32_t count, const PBox& tri_box, const PBox& cen_box)
    {
        // BVH_CreateNode, BVH.cpp:42-53 (fields it leaves untouched are zero here)
        ptmi_node& n = nodes[idx];
        std::memset(&n, 0, sizeof n);
        n.triangle_start_index = start;
        n.nb_triangles = count;
        pbox_store(tri_box, &n.triangles_aabb);
        pbox_store(cen_box, &n.centroids_aabb);
    }

    uint32_t make_leaf(uint32_t idx, int why)
    {
        nodes[idx].is_leaf = 1;
        nodes[idx].comments = why;
        if (depth > max_depth) max_depth = depth;
        return idx + 1;
    }

    // BVH_BuildStructure, BVH.cpp:109-356.  Returns the index after the subtree.
    uint32_t build(uint32_t idx)
    {
        ptmi_node* N = &nodes[idx];
        // (boxes whose extents overflow make the cost comparisons meaningless - a split can then leave a side empty and never end;
        // a tree this deep is of no use to the integrator either: PTMI_BVH_MAX_DEPTH)
        if (failed || depth > kMaxBuildDepth) { failed = true; return idx + 1; }

        const ptmi_float4 cmin = N->centroids_aabb.p_min, cmax = N->centroids_aabb.p_max;
        const int early = early_leaf(N->nb_triangles, cmin, cmax);
        if (early >= 0) return make_leaf(idx, early);

        const int first = (int)N->triangle_start_index;
        const int last = first + (int)N->nb_triangles - 1;

        for (int axis = 0; axis < 3; axis++) {
            for (int i = 0; i < kBins - 1; i++) sah[axis][i] = (float)INT_MAX;
            if (!axis_k1(cmin, cmax, axis, &k1[axis])) continue;
            for (int i = 0; i < kBins; i++) {
                // (BoundingBox_Reset: marked empty, its corners and centroid left as the last fold made them)
                PBox& b = bins[axis][i];
                if (b.n) b.centroid = pbox_centroid(b);
                b.n = 0;
                counts[axis][i] = 0;
            }
            const float lo = axis_of(cmin, axis);
            for (int i = first; i <= last; i++) {
                const ptmi_bounding_box& a = tris[i].aabb;
                const float scaled = scaled_pos(k1[axis], axis_of(a.centroid, axis), lo);
                // (the reference ASSERTs triangleBin < const__K, BVH.cpp:199, and indexes out of bounds without it: centroids so
                // far apart that their difference overflows - the entry point below already refuses non-finite ones)
                if (!bin_ok(scaled)) { failed = true; return idx + 1; }
                counts[axis][(int)scaled]++;
                if (!a.is_empty) pbox_unite(bins[axis][(int)scaled], a.p_min, a.p_max, a.centroid);  // (UniteWith skips an empty box)
            }
            axis_sah(bins[axis], counts[axis], rpart, sah[axis]);
        }

        int best_axis, best_index;
        float best_sah;
        best_split(&sah[0][0], &best_axis, &best_index, &best_sah);

        // (BoundingBox_Area of a box marked empty is 0, whatever its corners hold)
        const ptmi_bounding_box& tb = N->triangles_aabb;
        if (tb.is_empty ? kKI * best_sah + kKT > 0.0 : sah_leaf(best_sah, N->nb_triangles, tb.p_min, tb.p_max))
            return make_leaf(idx, PTMI_NODE_BAD_SAH);

        N->cut_axis = (uint32_t)best_axis;

        int left = first, right = last;
        {
            const float lo = axis_of(cmin, best_axis), k = k1[best_axis];
            auto goes = [&](int i) { return goes_left(scaled_pos(k, axis_of(tris[i].aabb.centroid, best_axis), lo), best_index); };
            while (left < right) {
                while (goes(left) && left < right) left++;
                while (!goes(right) && left < right) right--;
                if (left < right) std::swap(tris[left], tris[right]);
            }
        }

        PBox left_cen = pbox_empty(), right_cen = pbox_empty();
        for (int i = first; i < left; i++) pbox_add_point(left_cen, tris[i].aabb.centroid);
        for (int i = last; i >= left; i--) pbox_add_point(right_cen, tris[i].aabb.centroid);

        // taken before recursing: the scratch is shared (BVH.cpp:322-325).  A side that took no box at all (empty boxes
        // alone) is the bin next to the plane as it stands: l2r[index] = bin[index], r2l[index + 1] = bin[index + 1].
        PBox left_tri, right_tri;
        int left_count, right_count;
        split_sides(bins[best_axis], counts[best_axis], best_index, &left_tri, &left_count, &right_tri, &right_count);
        if (left_tri.n == 0) left_tri = bins[best_axis][best_index];
        if (right_tri.n == 0) right_tri = bins[best_axis][best_index + 1];

        // A split always leaves triangles on both sides when the costs are numbers, and the tree then has at most 2n - 1 nodes -
        // what the caller allocated (BVH.cpp:20).  With boxes whose extents overflow it need not: refuse instead of writing past
        // the array (the reference would).
        if (left_count <= 0 || right_count <= 0 || (uint64_t)size + 2 > capacity) { failed = true; return idx + 1; }
        depth++;
        size += 2;

        const uint32_t son1 = idx + 1;
        N->son1_id = son1;
        make_node(son1, (uint32_t)first, (uint32_t)left_count, left_tri, left_cen);
        const uint32_t son2 = build(son1);
        if (failed || son2 >= capacity) { failed = true; depth--; return idx + 1; }
        nodes[idx].son2_id = son2;
        make_node(son2, (uint32_t)(first + left_count), (uint32_t)right_count, right_tri, right_cen);
        const uint32_t next = build(son2);
        depth--;
        return next;
    }
};

}  // namespace

extern "C" int ptmi_bvh_create(ptmi_triangle* triangulation, uint32_t n, ptmi_node* bvh, uint32_t* bvh_size,
                               uint32_t* bvh_max_depth)
{
    if (!triangulation || !bvh || n == 0) {
        ptmi_internal::set_global_error("ptmi_bvh_create: null array or empty triangulation");
        return PTMI_ERR_INVALID_ARGUMENT;
    }
    // The reference's builder has no defined behaviour for boxes that are not numbers (its bin ASSERT fires, BVH.cpp:199; without
    // assertions it writes out of bounds): an error code here.
    const RootFold root = fold_records(triangulation, n, [](uint32_t, const ptmi_bounding_box&) {});
    if (root.refused) {
        ptmi_internal::set_global_error("ptmi_bvh_create: triangle " + std::to_string(root.index) + " has a bounding box that is not finite");
        return PTMI_ERR_BAD_SCENE;
    }
    std::vector<Builder> holder(1);  // ~12 KB of scratch: keep it off the stack
    Builder& b = holder[0];
    b.tris = triangulation;
    b.nodes = bvh;
    b.capacity = 2u * n - 1u;
    b.make_node(0, 0, n, root.tri, root.cen);
    b.size = 1;
    b.build(0);
    if (b.failed) {
        ptmi_internal::set_global_error("ptmi_bvh_create: bounding boxes too large to build a tree from (their extents overflow)");
        return PTMI_ERR_BAD_SCENE;
    }
    if (bvh_size) *bvh_size = b.size;
    if (bvh_max_depth) *bvh_max_depth = b.max_depth;
    return PTMI_OK;
}
