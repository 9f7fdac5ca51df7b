// bvh_build_common.h - the per-node arithmetic of the binned-SAH builder, shared by the host builder (bvh_build.cpp), the
// device builder (bvh_build_device.hip) and its serial model (tests/bvh_device_model.cpp).
//
// Every function here makes the decision the reference's BVH_BuildStructure makes at one node, operation for operation:
// the same float / double mix, the same order of the box unions.  The three builders differ in their schedule only: the
// order in which they visit nodes and combine partial results, and that is what PBox is for:
//
//   std::min<float>(a, b) is (b < a) ? b : a - of values that compare equal (-0 and +0) it keeps the one it saw first.  A
//   fold of boxes in a fixed index order is therefore "the first occurrence of the minimum", which is associative: partial
//   folds of consecutive ranges give the serial result when they are merged in range order (pbox_merge(earlier, later)).
//   That holds for numbers; a NaN stops the serial fold where it stands and would not merge the same way.  The boxes'
//   x, y, z are finite (the entry point refuses others); a NaN w is handed to the host builder (PTMI_BVH_FALLBACK_RECORDS).
//
//   BoundingBox_UniteWith into an empty box copies the other box's centroid, and BoundingBox_AddPoint into an empty box
//   sets centroid = point; only the second addition recomputes it as the midpoint of the corners.  PBox keeps the count of
//   boxes it holds and the centroid of a single one, and pbox_centroid gives what the serial fold would have.
//
// Compile with -ffp-contract=off (host and device): no product or sum here may be fused.
#ifndef PTMI_BVH_BUILD_COMMON_H
#define PTMI_BVH_BUILD_COMMON_H

#include <climits>
#include <cmath>
#include <cstdint>

#include "ptmi_hd.h"
#include "ptmi_scene.h"

namespace ptmi_bvh {

constexpr int kBins = 64;               // const__K
constexpr uint32_t kLeafMaxSize = 4;    // const__leafMaxSize
constexpr float kLeafMinDiag = 0.001f;  // const__leafMinDiagLength
constexpr float kKI = 1.0f;             // const__KI
constexpr float kKT = 0.01f;            // const__KT
constexpr uint32_t kMaxBuildDepth = 8 * PTMI_BVH_MAX_DEPTH;  // deeper than this the host builder refuses the scene
constexpr int kFoldChunks = 256;        // the children's centroid boxes: partial folds per node, merged in order

// std::min<float> / std::max<float>, written as the selects they are (not fminf / v_min_f32: those order -0 below +0)
PTMI_HD float min_sel(float a, float b) { return (b < a) ? b : a; }
PTMI_HD float max_sel(float a, float b) { return (a < b) ? b : a; }
PTMI_HD ptmi_float4 min4(const ptmi_float4& a, const ptmi_float4& b)
{
    return { min_sel(a.x, b.x), min_sel(a.y, b.y), min_sel(a.z, b.z), min_sel(a.w, b.w) };
}
PTMI_HD ptmi_float4 max4(const ptmi_float4& a, const ptmi_float4& b)
{
    return { max_sel(a.x, b.x), max_sel(a.y, b.y), max_sel(a.z, b.z), max_sel(a.w, b.w) };
}
PTMI_HD ptmi_float4 mid4(const ptmi_float4& a, const ptmi_float4& b)
{
    return { (a.x + b.x) / 2, (a.y + b.y) / 2, (a.z + b.z) / 2, (a.w + b.w) / 2 };
}
PTMI_HD float axis_of(const ptmi_float4& v, int axis) { return axis == 0 ? v.x : (axis == 1 ? v.y : v.z); }

// A box being folded: corners, the centroid of the first box it took, and how many boxes (or points) it took.
struct PBox {
    ptmi_float4 p_min, p_max, centroid;
    uint32_t n;
};

PTMI_HD PBox pbox_empty()
{
    PBox b;
    b.p_min = b.p_max = b.centroid = ptmi_float4{ 0, 0, 0, 0 };
    b.n = 0;
    return b;
}

// self.UniteWith(box) for a box that is not empty (self's values win ties: self came first)
PTMI_HD void pbox_unite(PBox& self, const ptmi_float4& p_min, const ptmi_float4& p_max, const ptmi_float4& centroid)
{
    if (self.n == 0) {
        self.p_min = p_min; self.p_max = p_max; self.centroid = centroid; self.n = 1;
        return;
    }
    self.p_min = min4(self.p_min, p_min);
    self.p_max = max4(self.p_max, p_max);
    self.n += 1;
}
PTMI_HD void pbox_add_point(PBox& self, const ptmi_float4& v) { pbox_unite(self, v, v, v); }

// the fold of `first`'s range followed by `second`'s
PTMI_HD ptmi_float4 sel4(bool c, const ptmi_float4& a, const ptmi_float4& b)
{
    return { c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w };
}
PTMI_HD PBox pbox_merge(const PBox& first, const PBox& second)
{
    // (selects rather than early returns: the device keeps the boxes in registers)
    const bool one = first.n == 0 || second.n == 0;
    const bool take_second = first.n == 0;
    PBox r;
    r.p_min = one ? sel4(take_second, second.p_min, first.p_min) : min4(first.p_min, second.p_min);
    r.p_max = one ? sel4(take_second, second.p_max, first.p_max) : max4(first.p_max, second.p_max);
    r.centroid = sel4(take_second, second.centroid, first.centroid);
    r.n = first.n + second.n;
    return r;
}

// the centroid the serial fold leaves: the single box's own, else the midpoint of the corners
PTMI_HD ptmi_float4 pbox_centroid(const PBox& b) { return b.n == 1 ? b.centroid : mid4(b.p_min, b.p_max); }

// A folded box as the BoundingBox the serial fold leaves (the fields only: the caller zeroes the padding).  A box that took
// nothing is marked empty and keeps the corners and centroid it holds, as BoundingBox_Reset does.
PTMI_HD void pbox_store(const PBox& b, ptmi_bounding_box* out)
{
    out->p_min = b.p_min; out->p_max = b.p_max;
    out->centroid = b.n == 0 ? b.centroid : pbox_centroid(b);
    out->is_empty = b.n == 0;
}

// BoundingBox_Area: float products and sums, widened on return
PTMI_HD double half_area(const ptmi_float4& p_min, const ptmi_float4& p_max)
{
    const float dx = p_max.x - p_min.x, dy = p_max.y - p_min.y, dz = p_max.z - p_min.z;
    const float a = dx * dy + dy * dz + dz * dx;
    return a;
}
PTMI_HD double pbox_half_area(const PBox& b) { return b.n == 0 ? 0.0 : half_area(b.p_min, b.p_max); }

// The leaf tests before any binning: PTMI_NODE_LEAF_MAX_SIZE, PTMI_NODE_LEAF_MIN_DIAG, or -1 for "bin this node".
PTMI_HD int early_leaf(uint32_t nb_triangles, const ptmi_float4& cen_min, const ptmi_float4& cen_max)
{
    if (nb_triangles <= kLeafMaxSize) return PTMI_NODE_LEAF_MAX_SIZE;
    const float dx = cen_min.x - cen_max.x, dy = cen_min.y - cen_max.y, dz = cen_min.z - cen_max.z;
    if ((dx * dx) + (dy * dy) + (dz * dz) < kLeafMinDiag) return PTMI_NODE_LEAF_MIN_DIAG;
    return -1;
}

// Per axis: false if the host builder skips the axis at this node (it then keeps k1 and the scans of an earlier node);
// else k1, rounded through double as the host rounds it.
PTMI_HD bool axis_k1(const ptmi_float4& cen_min, const ptmi_float4& cen_max, int axis, float* k1)
{
    const double cut_length = axis_of(cen_max, axis) - axis_of(cen_min, axis);
    if (cut_length < kLeafMinDiag) return false;
    *k1 = (float)((float)kBins * (0.999f) / cut_length);
    return true;
}

// The centroid's scaled position on an axis; the bin is (int) of it, and it must lie in [0, 64) (the host refuses the
// scene otherwise).  A triangle goes to the left child when scaled < best_index + 1 - the host's partition test.
PTMI_HD float scaled_pos(float k1, float c, float lo) { return k1 * (c - lo); }
PTMI_HD bool bin_ok(float scaled) { return scaled >= 0.0f && scaled < (float)kBins; }
PTMI_HD bool goes_left(float scaled, int best_index) { return scaled < (best_index + 1); }

// The SAH of the 63 split planes of one binned axis, with the prefix and suffix scans in the host's order
// (l2r[i] = bin[i] united with l2r[i - 1]; r2l[j] = bin[j] united with r2l[j + 1]).  `rpart` is 63 doubles of scratch.
PTMI_HD void axis_sah(const PBox* bins, const int* counts, double* rpart, float* sah)
{
    PBox acc = bins[kBins - 1];
    int cnt = counts[kBins - 1];
    rpart[kBins - 2] = cnt * pbox_half_area(acc);
    for (int j = kBins - 2; j >= 1; j--) {
        acc = pbox_merge(bins[j], acc);
        cnt += counts[j];
        rpart[j - 1] = cnt * pbox_half_area(acc);
    }
    acc = bins[0];
    cnt = counts[0];
    for (int i = 0; i < kBins - 1; i++) {
        if (i > 0) { acc = pbox_merge(bins[i], acc); cnt += counts[i]; }
        sah[i] = (float)(cnt * pbox_half_area(acc) + rpart[i]);
    }
}

// The children of a split after bin `index`: l2r[index] and r2l[index + 1], boxes and counts, scanned as axis_sah does.
PTMI_HD void split_sides(const PBox* bins, const int* counts, int index, PBox* left, int* left_count, PBox* right, int* right_count)
{
    PBox acc = bins[0];
    int cnt = counts[0];
    for (int i = 1; i <= index; i++) { acc = pbox_merge(bins[i], acc); cnt += counts[i]; }
    *left = acc;
    *left_count = cnt;
    acc = bins[kBins - 1];
    cnt = counts[kBins - 1];
    for (int j = kBins - 2; j >= index + 1; j--) { acc = pbox_merge(bins[j], acc); cnt += counts[j]; }
    *right = acc;
    *right_count = cnt;
}

// The best split: start at sah[0][0], then every axis, i = 1..62, strict <.  `sah` is 3 x 63 (INT_MAX on skipped axes).
PTMI_HD void best_split(const float* sah, int* best_axis, int* best_index, float* best_sah)
{
    int ba = 0, bi = 0;
    float bs = sah[0];
    for (int axis = 0; axis < 3; axis++)
        for (int i = 1; i < kBins - 1; i++)
            if (sah[axis * (kBins - 1) + i] < bs) { ba = axis; bs = sah[axis * (kBins - 1) + i]; bi = i; }
    *best_axis = ba;
    *best_index = bi;
    *best_sah = bs;
}

// Not worth splitting: the host's `KI * best + KT > nbTriangles * area(trianglesAABB)`
PTMI_HD bool sah_leaf(float best_sah, uint32_t nb_triangles, const ptmi_float4& tri_min, const ptmi_float4& tri_max)
{
    return kKI * best_sah + kKT > nb_triangles * half_area(tri_min, tri_max);
}

// The record screen and the root of every builder, in one walk over the triangles in index order (BVH_Create: UniteWith
// into the triangles' box - a box marked empty is skipped -, AddPoint into the centroids').  The walk ends at the first
// record with a non-finite number among the nine the builders read: no builder takes such a scene.  each(i, aabb) is
// called for every record before that.
struct RootFold {
    PBox tri, cen;
    bool refused;    // record `index` is not finite; tri and cen stop short of it
    uint32_t index;
    bool unfolded;   // a record walked is one the device does not fold: a box marked empty, a NaN w
};
template <class Each>
inline RootFold fold_records(const ptmi_triangle* tris, uint32_t n, Each each)
{
    RootFold r = { pbox_empty(), pbox_empty(), false, 0, false };
    for (uint32_t i = 0; i < n; i++) {
        const ptmi_bounding_box& a = tris[i].aabb;
        const float v[9] = { a.p_min.x, a.p_min.y, a.p_min.z, a.p_max.x, a.p_max.y, a.p_max.z, a.centroid.x, a.centroid.y, a.centroid.z };
        for (float f : v)
            if (!std::isfinite(f)) { r.refused = true; r.index = i; return r; }
        if (a.is_empty || std::isnan(a.p_min.w) || std::isnan(a.p_max.w) || std::isnan(a.centroid.w)) r.unfolded = true;
        if (!a.is_empty) pbox_unite(r.tri, a.p_min, a.p_max, a.centroid);
        pbox_add_point(r.cen, a.centroid);
        each(i, a);
    }
    return r;
}

}  // namespace ptmi_bvh

#endif  // PTMI_BVH_BUILD_COMMON_H
