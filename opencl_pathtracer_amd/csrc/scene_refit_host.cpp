// scene_refit_host.cpp - the host side of an in-place scene update (see scene_refit.h).  No device call in this file.
#include "scene_refit.h"

#include <cmath>

#include "scene_layout.h"
#include "scene_refit_common.h"

using namespace ptmi_bvh;

namespace ptmi_internal {

namespace {

int fail(std::string& err, int code, const std::string& msg)
{
    err = msg;
    return code;
}

const char* const kReinitialise = ": an update cannot express that, call ptmi_initialize_memory with the new scene";

}  // namespace

int screen_verdict(uint32_t word, std::string& err)
{
    if (word == ptmi_refit::kScreenAccepted) return PTMI_OK;
    const int rc = screen_refusal(word & 15u, word >> 4, err);
    if (rc == PTMI_ERR_UNSUPPORTED) err += kReinitialise;
    return rc;
}

uint32_t screen_update_word(const UpdateFacts& facts, const ptmi_triangle* triangulation, uint32_t triangulation_size)
{
    for (uint32_t i = 0; i < triangulation_size; i++)
        if (const uint32_t code = ptmi_refit::screen_triangle(triangulation[i], facts.material_is_simple_color.data(),
                                                              (uint32_t)facts.material_is_simple_color.size(), facts.tris_precomputed))
            return ptmi_refit::screen_word(i, code);
    return ptmi_refit::kScreenAccepted;
}

int screen_update(const UpdateFacts& facts, const ptmi_triangle* triangulation, uint32_t triangulation_size, std::string& err)
{
    return screen_verdict(screen_update_word(facts, triangulation, triangulation_size), err);
}

int build_refit_schedule(const DNode* records, const uint32_t* tri_ids, uint32_t n_records, const DBigLeaf* big_leaves,
                         uint32_t n_big_leaves, uint32_t root_ref, uint32_t triangulation_size, RefitSchedule& out, std::string& err)
{
    out.nodes.clear();
    out.first.clear();
    // the triangles behind a leaf reference: 0, or their number; -1 if anything the kernels would index is out of range
    auto leaf_count = [&](uint32_t ref) -> long {
        uint32_t count = ref_leaf_count(ref), start = ref & REF_INDEX_MASK_LEAF;
        if (count == REF_COUNT_BIG) {
            if (start >= n_big_leaves) return -1;
            count = big_leaves[start].count;
            start = big_leaves[start].start;
        }
        if ((uint64_t)start + count > n_records) return -1;
        for (uint32_t k = 0; k < count; k++)
            if (tri_ids[start + k] >= triangulation_size) return -1;  // (a node record's 0xFFFFFFFF included)
        return (long)count;
    };
    const char* const broken = "the uploaded records are inconsistent (refit schedule)";
    if (root_ref & REF_LEAF) {  // a tree of one leaf: no box to refit
        if (leaf_count(root_ref) < 0) return fail(err, PTMI_ERR_INTERNAL, broken);
        out.first.push_back(0);
        return PTMI_OK;
    }
    std::vector<uint8_t> holds(n_records, 0);  // 0: not reached; 1: reached; 2: reached, and triangles lie below
    std::vector<uint32_t> level, next;
    auto reach = [&](uint32_t ref, std::vector<uint32_t>& to) -> bool {
        const uint32_t r = ref & REF_INDEX_MASK_INNER;
        if (r >= n_records || tri_ids[r] != 0xFFFFFFFFu || holds[r]) return false;
        holds[r] = 1;
        to.push_back(r);
        return true;
    };
    if (!reach(root_ref, level)) return fail(err, PTMI_ERR_INTERNAL, broken);
    while (!level.empty()) {
        if (out.levels() >= PTMI_BVH_MAX_DEPTH) return fail(err, PTMI_ERR_INTERNAL, broken);
        out.first.push_back((uint32_t)out.nodes.size());
        out.nodes.insert(out.nodes.end(), level.begin(), level.end());
        next.clear();
        for (uint32_t r : level)
            for (uint32_t ref : {records[r].ref1, records[r].ref2})
                if ((ref & REF_LEAF) ? leaf_count(ref) < 0 : !reach(ref, next)) return fail(err, PTMI_ERR_INTERNAL, broken);
        level.swap(next);
    }
    out.first.push_back((uint32_t)out.nodes.size());
    // bottom-up: is a reference flagged empty exactly where no triangle lies below it?
    auto flag_ok = [&](uint32_t ref) -> int {  // -1: no; else whether triangles lie below
        const bool below = (ref & REF_LEAF) ? leaf_count(ref) > 0 : holds[ref & REF_INDEX_MASK_INNER] == 2;
        return ((ref & REF_EMPTY) != 0) == !below ? (int)below : -1;
    };
    const char* const flags = "the uploaded tree marks a box empty that holds triangles, or the reverse: its flags would change with a refit";
    for (size_t k = out.nodes.size(); k-- > 0;) {
        const uint32_t r = out.nodes[k];
        const int b1 = flag_ok(records[r].ref1), b2 = flag_ok(records[r].ref2);
        if (b1 < 0 || b2 < 0) return fail(err, PTMI_ERR_UNSUPPORTED, std::string(flags) + kReinitialise);
        holds[r] = (b1 || b2) ? 2 : 1;
    }
    if (flag_ok(root_ref) < 0) return fail(err, PTMI_ERR_UNSUPPORTED, std::string(flags) + kReinitialise);
    return PTMI_OK;
}

}  // namespace ptmi_internal

// Host only: the boxes of a tree in the reference's layout from the triangles it indexes, topology untouched.
extern "C" int ptmi_bvh_refit(const ptmi_triangle* triangulation, uint32_t triangulation_size, ptmi_node* bvh, uint32_t bvh_size)
{
    using ptmi_internal::set_global_error;
    if (!triangulation || !bvh || bvh_size == 0) {
        set_global_error("ptmi_bvh_refit: null array or empty bvh");
        return PTMI_ERR_INVALID_ARGUMENT;
    }
    // the walk of build_layout (scene_layout.cpp), with its structural checks; nothing is written before it has ended
    std::vector<uint8_t> seen(bvh_size, 0);
    std::vector<uint32_t> order, todo;
    std::string why;
    auto check_node = [&](uint32_t id) -> bool {
        if (id >= bvh_size) { why = "child index out of range"; return false; }
        if (seen[id]) { why = "node " + std::to_string(id) + " reached twice (cycle or shared subtree)"; return false; }
        seen[id] = 1;
        const ptmi_node& n = bvh[id];
        if (n.is_leaf && (uint64_t)n.triangle_start_index + n.nb_triangles > triangulation_size) { why = "leaf triangle range out of bounds"; return false; }
        return true;
    };
    if (!check_node(0)) {
        set_global_error("ptmi_bvh_refit: bvh[0]: " + why);
        return PTMI_ERR_BAD_SCENE;
    }
    todo.push_back(0);
    while (!todo.empty()) {
        const uint32_t id = todo.back();
        todo.pop_back();
        order.push_back(id);
        const ptmi_node& n = bvh[id];
        if (n.is_leaf) continue;
        if (!check_node(n.son1_id) || !check_node(n.son2_id)) {
            set_global_error("ptmi_bvh_refit: bvh[" + std::to_string(id) + "]: " + why);
            return PTMI_ERR_BAD_SCENE;
        }
        todo.push_back(n.son2_id);
        todo.push_back(n.son1_id);
    }
    // Children first (a node precedes its subtree in `order`).  A stored box and the number of boxes it took are the fold again:
    // the centroid of a fold's first box matters only while the fold holds that one box, and then the stored centroid is it.
    std::vector<uint32_t> taken_tri(bvh_size, 0), taken_cen(bvh_size, 0);
    auto held = [](const ptmi_bounding_box& b, uint32_t taken) {
        PBox p;
        p.p_min = b.p_min; p.p_max = b.p_max; p.centroid = b.centroid; p.n = taken;
        return p;
    };
    for (size_t k = order.size(); k-- > 0;) {
        const uint32_t id = order[k];
        ptmi_node& n = bvh[id];
        // (a box that takes nothing keeps the corners and centroid it holds, as BoundingBox_Reset leaves them)
        PBox tri = held(n.triangles_aabb, 0), cen = held(n.centroids_aabb, 0);
        if (n.is_leaf) {
            const ptmi_triangle* first = triangulation + n.triangle_start_index;
            ptmi_refit::fold_triangles(n.nb_triangles, [first](uint32_t j) -> const ptmi_triangle& { return first[j]; }, &tri, &cen);
        } else {
            const uint32_t a = n.son1_id, b = n.son2_id;
            if (taken_tri[a] + taken_tri[b])
                tri = pbox_merge(held(bvh[a].triangles_aabb, taken_tri[a]), held(bvh[b].triangles_aabb, taken_tri[b]));
            if (taken_cen[a] + taken_cen[b])
                cen = pbox_merge(held(bvh[a].centroids_aabb, taken_cen[a]), held(bvh[b].centroids_aabb, taken_cen[b]));
        }
        // a corner that keeps its value keeps its bits (scene_refit_common.h: keep_sel), the centroid follows the corners
        if (tri.n) { tri.p_min = ptmi_refit::keep4(n.triangles_aabb.p_min, tri.p_min); tri.p_max = ptmi_refit::keep4(n.triangles_aabb.p_max, tri.p_max); }
        if (cen.n) { cen.p_min = ptmi_refit::keep4(n.centroids_aabb.p_min, cen.p_min); cen.p_max = ptmi_refit::keep4(n.centroids_aabb.p_max, cen.p_max); }
        pbox_store(tri, &n.triangles_aabb);
        pbox_store(cen, &n.centroids_aabb);
        taken_tri[id] = tri.n;
        taken_cen[id] = cen.n;
    }
    return PTMI_OK;
}
