// The serial model of the device builder (opencl_pathtracer_amd/csrc/bvh_build_device.hip): the same level-synchronous
// schedule, the same per-node arithmetic (bvh_build_common.h, the header the kernels use), the same order of folds and
// merges - run on the host, one node after another.  tests/test_bvh_device_model.py compiles it with g++ and checks its
// trees against ptmi_bvh_create, and where it flags a stale split.
//
//   int model_bvh_build_ex(tris, n, nodes, perm, &size, &max_depth, slot_seed, &levels)
//   int model_bvh_build(tris, n, nodes, perm, &size, &max_depth)        (slot_seed 0, levels not reported)
//     0: built - nodes[0 .. size) in pre-order; perm[i] = the input index of the triangle at position i
//     1: a split whose axis was skipped at its node (the host builder uses an earlier node's scans there)
//     2: a condition the host builder refuses the scene for (a box that is not finite, bin out of range, empty side, too deep)
//     3: records the device does not fold (a NaN w, a box marked empty)
// Like the device it stops at the first level that flags anything, a stale split ahead of an error.
//
// slot_seed: on the device a splitting node takes its two child slots from an atomic counter, so the order of a level's
// nodes in the workspace is the order in which their workgroups got there.  slot_seed != 0 visits the open nodes of every
// level in a shuffled order (and so hands out the slots in that order); 0 visits them in slot order.  The output must not
// depend on it: the sizes and pre-order passes below are the device's (k_sizes, k_preorder, k_emit), level by level over
// the slot-indexed arrays.  levels: the number of k_level launches the device makes (ptmi_bvh_build_info.levels).
#include <cstring>
#include <utility>
#include <vector>

#include "bvh_build_common.h"

using namespace ptmi_bvh;

namespace {

struct MNode {
    PBox tri, cen;
    uint32_t start, count, cut_axis, depth;
    int leaf;
    uint32_t child;
};

// the device's fold_centroids: kFoldChunks consecutive chunks, each folded in order, merged in chunk order (tree of pairs)
PBox fold_centroids(const ptmi_float4* cen, const std::vector<uint32_t>& perm, uint32_t lo, uint32_t hi, bool descending)
{
    const uint32_t m = hi - lo + 1, len = (m + kFoldChunks - 1) / kFoldChunks;
    std::vector<PBox> red(kFoldChunks);
    for (uint32_t t = 0; t < (uint32_t)kFoldChunks; t++) {
        PBox acc = pbox_empty();
        for (uint32_t k = t * len; k < m && k < (t + 1) * len; k++)
            pbox_add_point(acc, cen[perm[descending ? hi - k : lo + k]]);
        red[t] = acc;
    }
    for (uint32_t s = 1; s < (uint32_t)kFoldChunks; s *= 2)
        for (uint32_t t = 0; t < (uint32_t)kFoldChunks; t += 2 * s) red[t] = pbox_merge(red[t], red[t + s]);
    return red[0];
}

constexpr uint32_t kThreads = 256;  // k_level's workgroup: the partition ranks positions in batches of this many

// the order in which the open nodes [begin, end) of a level get to their child slots
std::vector<size_t> visit_order(size_t begin, size_t end, uint64_t* rng)
{
    std::vector<size_t> order(end - begin);
    for (size_t i = 0; i < order.size(); i++) order[i] = begin + i;
    if (*rng == 0) return order;
    for (size_t i = order.size(); i > 1; i--) {  // Fisher-Yates on a 64-bit LCG
        *rng = *rng * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(order[i - 1], order[(size_t)((*rng >> 33) % i)]);
    }
    return order;
}

}  // namespace

extern "C" int model_bvh_build_ex(const ptmi_triangle* tris, uint32_t n, ptmi_node* out, uint32_t* perm_out, uint32_t* size_out,
                                  uint32_t* depth_out, uint32_t slot_seed, uint32_t* levels_out)
{
    std::vector<ptmi_float4> pmin(n), pmax(n), cen(n);
    const RootFold fold = fold_records(tris, n, [&](uint32_t i, const ptmi_bounding_box& a) {
        pmin[i] = a.p_min; pmax[i] = a.p_max; cen[i] = a.centroid;
    });
    if (fold.unfolded) return 3;
    if (fold.refused) return 2;
    std::vector<uint32_t> perm(n), scratch(n);
    for (uint32_t i = 0; i < n; i++) perm[i] = i;
    std::vector<MNode> nodes;
    nodes.push_back({ fold.tri, fold.cen, 0, n, 0, 0, -1, 0 });
    uint32_t max_depth = 0;

    uint64_t rng = slot_seed ? 0x9E3779B97F4A7C15ull * slot_seed : 0;
    std::vector<size_t> level_begin{ 0 };
    uint32_t levels = 0;
    size_t begin = 0, end = 1;
    while (begin < end) {
        int flags = 0;
        levels++;
        for (size_t self : visit_order(begin, end, &rng)) {
            MNode N = nodes[self];
            if (N.depth > kMaxBuildDepth) { flags |= 2; continue; }
            const int early = early_leaf(N.count, N.cen.p_min, N.cen.p_max);
            if (early >= 0) {
                nodes[self].leaf = early;
                if (N.depth > max_depth) max_depth = N.depth;
                continue;
            }
            const uint32_t first = N.start, last = N.start + N.count - 1;
            float k1[3] = { 0, 0, 0 }, lo[3];
            bool binned[3];
            PBox bins[3][kBins];
            int counts[3][kBins];
            double rpart[3][kBins - 1];
            float sah[3][kBins - 1];
            bool bad = false;
            for (int a = 0; a < 3; a++) {
                binned[a] = axis_k1(N.cen.p_min, N.cen.p_max, a, &k1[a]);
                lo[a] = axis_of(N.cen.p_min, a);
                for (int b = 0; b < kBins; b++) { bins[a][b] = pbox_empty(); counts[a][b] = 0; }
                if (!binned[a]) {
                    for (int i = 0; i < kBins - 1; i++) sah[a][i] = (float)INT_MAX;
                    continue;
                }
                for (uint32_t p = first; p <= last; p++) {
                    const uint32_t id = perm[p];
                    const float s = scaled_pos(k1[a], axis_of(cen[id], a), lo[a]);
                    if (!bin_ok(s)) { bad = true; break; }
                    pbox_unite(bins[a][(int)s], pmin[id], pmax[id], cen[id]);
                    counts[a][(int)s]++;
                }
                if (bad) break;
                axis_sah(bins[a], counts[a], rpart[a], sah[a]);
            }
            if (bad) { flags |= 2; continue; }
            int axis, index;
            float best;
            best_split(&sah[0][0], &axis, &index, &best);
            if (sah_leaf(best, N.count, N.tri.p_min, N.tri.p_max)) {
                nodes[self].leaf = PTMI_NODE_BAD_SAH;
                if (N.depth > max_depth) max_depth = N.depth;
                continue;
            }
            if (!binned[axis]) { flags |= 1; continue; }
            PBox lt, rt;
            int lc, rc;
            split_sides(bins[axis], counts[axis], index, &lt, &lc, &rt, &rc);
            if (lc <= 0 || rc <= 0 || (uint32_t)lc + (uint32_t)rc != N.count) { flags |= 2; continue; }
            // partition, as k_level ranks it: the positions of the left-going triangles in [mid, last], counted from the end in
            // batches of kThreads ...
            const uint32_t mid = first + (uint32_t)lc, n_right = last - mid + 1, L = (uint32_t)lc;
            uint32_t running = 0;
            for (uint32_t off = 0; off < n_right; off += kThreads) {
                uint32_t total = 0;
                for (uint32_t t = 0; t < kThreads; t++) {
                    const uint32_t k_off = off + t;
                    if (k_off >= n_right) continue;
                    const uint32_t q = last - k_off;
                    if (goes_left(scaled_pos(k1[axis], axis_of(cen[perm[q]], axis), lo[axis]), index)) scratch[first + running + total++] = q;
                }
                running += total;
            }
            const uint32_t pairs = running;
            // ... and the k-th right-going triangle in [first, mid) swaps with the k-th of them
            running = 0;
            for (uint32_t off = 0; off < L; off += kThreads) {
                uint32_t total = 0;
                for (uint32_t t = 0; t < kThreads; t++) {
                    if (off + t >= L) continue;
                    const uint32_t p = first + off + t, id = perm[p];
                    if (goes_left(scaled_pos(k1[axis], axis_of(cen[id], axis), lo[axis]), index)) continue;
                    const uint32_t rank = running + total++;
                    if (rank >= pairs) return 2;
                    const uint32_t q = scratch[first + rank];
                    perm[p] = perm[q];
                    perm[q] = id;
                }
                running += total;
            }
            const PBox lcen = fold_centroids(cen.data(), perm, first, mid - 1, false);
            const PBox rcen = fold_centroids(cen.data(), perm, mid, last, true);
            nodes[self].cut_axis = (uint32_t)axis;
            nodes[self].child = (uint32_t)nodes.size();
            nodes.push_back({ lt, lcen, first, (uint32_t)lc, 0, N.depth + 1, -1, 0 });
            nodes.push_back({ rt, rcen, mid, (uint32_t)rc, 0, N.depth + 1, -1, 0 });
        }
        if (flags & 1) return 1;
        if (flags & 2) return 2;
        begin = end;
        end = nodes.size();
        level_begin.push_back(begin);
    }

    // numbering, level by level over the slot-indexed arrays: subtree sizes from the deepest level up (k_sizes), pre-order
    // numbers from the root down (k_preorder: son1 = parent + 1, son2 = son1 + size(son1))
    const size_t total = nodes.size();
    std::vector<uint32_t> size(total), pre(total);
    for (size_t l = level_begin.size() - 1; l-- > 0;)
        for (size_t i = level_begin[l]; i < level_begin[l + 1]; i++)
            size[i] = nodes[i].leaf >= 0 ? 1u : 1u + size[nodes[i].child] + size[nodes[i].child + 1];
    pre[0] = 0;
    for (size_t l = 0; l + 1 < level_begin.size(); l++)
        for (size_t i = level_begin[l]; i < level_begin[l + 1]; i++)
            if (nodes[i].leaf < 0) {
                pre[nodes[i].child] = pre[i] + 1;
                pre[nodes[i].child + 1] = pre[i] + 1 + size[nodes[i].child];
            }
    for (size_t i = 0; i < total; i++) {
        const MNode& d = nodes[i];
        ptmi_node& o = out[pre[i]];
        std::memset(&o, 0, sizeof o);
        pbox_store(d.tri, &o.triangles_aabb);
        pbox_store(d.cen, &o.centroids_aabb);
        o.triangle_start_index = d.start;
        o.nb_triangles = d.count;
        if (d.leaf >= 0) {
            o.is_leaf = 1;
            o.comments = d.leaf;
        } else {
            o.cut_axis = d.cut_axis;
            o.son1_id = pre[d.child];
            o.son2_id = pre[d.child + 1];
        }
    }
    std::memcpy(perm_out, perm.data(), sizeof(uint32_t) * n);
    *size_out = (uint32_t)total;
    *depth_out = max_depth;
    if (levels_out) *levels_out = levels;
    return 0;
}

extern "C" int model_bvh_build(const ptmi_triangle* tris, uint32_t n, ptmi_node* out, uint32_t* perm_out, uint32_t* size_out,
                               uint32_t* depth_out)
{
    return model_bvh_build_ex(tris, n, out, perm_out, size_out, depth_out, 0, nullptr);
}
