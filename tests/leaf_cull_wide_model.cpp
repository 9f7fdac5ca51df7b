// leaf_cull_wide_model.cpp - the wide tier of csrc/leaf_cull.h behind a C interface, beside tests/leaf_cull_model.cpp (which
// keeps the tight tier's): the wide pair's constants, rule and certificate, a serial walk that culls by a chosen set of record
// bits under a chosen rule - what node_step does at every PTMI_LEAF_CULL level, and what the commit before the wide tier did -
// and the cull words of a layout against the tight tier computed afresh.  Compiled by tests/leaf_cull_wide_cases.py into one
// library with leaf_cull_model.cpp and its companions - no HIP.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "leaf_cull.h"
#include "ptmi_internal.h"
#include "scene_layout.h"

using namespace ptmi_internal;

extern "C" {

typedef int (*wide_box_decider)(const ptmi_bounding_box* bb, const float origin[4], const float direction[4], float squared_distance);
typedef int (*wide_tri_decider)(const ptmi_triangle* tri, const float origin[4], const float direction[4], float* squared_distance, float* s,
                                float* t, float point[4]);

void wide_constants(double out[4])
{
    out[0] = ptmi_cull::kRelWide; out[1] = ptmi_cull::kAbsWide; out[2] = ptmi_cull::kKappaWideMax; out[3] = ptmi_cull::kEpsAbsWideMax;
}

// the record bits: child 1, child 2, computed, wide 1, wide 2, wide computed; DScene::leaf_cull's tight-only flag; then the
// record bits a launch looks at, (kernel_cull_mask << kernel_cull_shift), for DScene::leaf_cull = 0, 3, 7, 7 + the flag
void wide_bits(uint32_t out[11])
{
    out[0] = ptmi_cull::kCullChild1; out[1] = ptmi_cull::kCullChild2; out[2] = ptmi_cull::kCullComputed; out[3] = ptmi_cull::kCullWide1;
    out[4] = ptmi_cull::kCullWide2; out[5] = ptmi_cull::kCullWideComputed; out[6] = ptmi_cull::kCullTightOnly;
    const uint32_t levels[4] = {0u, 3u, 7u, 7u | ptmi_cull::kCullTightOnly};
    for (int k = 0; k < 4; k++) out[7 + k] = ptmi_cull::kernel_cull_mask(levels[k]) << ptmi_cull::kernel_cull_shift(levels[k]);
}

int wide_rule(const float lo[3], const float hi[3], const float o[4], float dw, float limit)
{
    return ptmi_cull::leaf_cull_rule_wide(ptmi_cull::box_distance2(lo, hi, o[0], o[1], o[2]), limit, o[0], o[1], o[2], o[3], dw) ? 1 : 0;
}

int wide_triangle_certified(const ptmi_triangle* t, const float lo[3], const float hi[3]) { return ptmi_cull::triangle_certified_wide(*t, lo, hi) ? 1 : 0; }

// One query, node_step's way.  mask: the record bits the walk looks at, one tier's three (wide_bits; the tier's "computed" bit
// in it: the far child of a closest-hit query is judged where it would be pushed); wide: the wide rule instead of the tight one.
// mask = 0 is the plain walk.  out: as cull_walk's (leaf_cull_model.cpp), out[11] = direct leaves the mask does not certify.
int wide_walk(const DNode* recs, const uint32_t* tri_ids, const DBigLeaf* big_leaves, uint32_t root_ref, const ptmi_triangle* tris,
              wide_box_decider box_hit, wide_tri_decider tri_hit, const float o[4], const float d[4], float limit, int shadow, uint32_t mask, int wide,
              uint32_t out[12])
{
    std::memset(out, 0, 12 * sizeof(uint32_t));
    out[0] = 0xFFFFFFFFu;
    std::vector<uint32_t> stack;
    std::vector<uint8_t> mark;
    uint32_t cur = root_ref;
    bool direct = false, marked = false, finished = false;
    const bool may = ptmi_cull::ray_may_cull(o[0], o[1], o[2], o[3], d[3]);
    auto rule = [&](const float lo[3], const float hi[3]) {
        const float d2 = ptmi_cull::box_distance2(lo, hi, o[0], o[1], o[2]);
        return may && (wide ? ptmi_cull::box_is_beyond_wide(d2, limit) : ptmi_cull::box_is_beyond(d2, limit));
    };
    const bool pushed_too = (mask & (ptmi_cull::kCullComputed | ptmi_cull::kCullWideComputed)) != 0u && !shadow;
    while (!finished) {
        bool pop = false;
        if (cur & REF_LEAF) {
            uint32_t start, count;
            leaf_range(cur, big_leaves, &start, &count);
            out[direct ? 4 : 5]++;
            if (marked) {
                out[8]++; out[9] += count; out[3] += count;
            } else {
                for (uint32_t k = 0; k < count && !finished; k++) {
                    float s, t, point[4];
                    out[3]++; out[10]++;
                    if (tri_hit(&tris[tri_ids[start + k]], o, d, &limit, &s, &t, point)) {
                        out[0] = start + k;
                        if (shadow) finished = true;
                    }
                }
            }
            pop = true;
        } else {
            const DNode& n = recs[cur & REF_INDEX_MASK_INNER];
            ptmi_bounding_box b1{}, b2{};
            b1.p_min = {n.lo1[0], n.lo1[1], n.lo1[2], 0}; b1.p_max = {n.hi1[0], n.hi1[1], n.hi1[2], 0}; b1.is_empty = (n.ref1 & REF_EMPTY) ? 1 : 0;
            b2.p_min = {n.lo2[0], n.lo2[1], n.lo2[2], 0}; b2.p_max = {n.hi2[0], n.hi2[1], n.hi2[2], 0}; b2.is_empty = (n.ref2 & REF_EMPTY) ? 1 : 0;
            const bool h1 = box_hit(&b1, o, d, limit) != 0, h2 = box_hit(&b2, o, d, limit) != 0;
            out[2] += 2;
            const bool fwd = d[n.axis] > 0;
            auto certified = [&](bool one) {
                return (n.cull & mask & (one ? ptmi_cull::kCullChild1 | ptmi_cull::kCullWide1 : ptmi_cull::kCullChild2 | ptmi_cull::kCullWide2)) != 0u;
            };
            if (!h1 && !h2) {
                pop = true;
            } else {
                const bool first = fwd ? h1 : !h2;
                if (h1 && h2) {
                    const uint32_t far_ref = fwd ? n.ref2 : n.ref1;
                    const bool far_one = !fwd;
                    mark.push_back(pushed_too && (n.cull & mask & (ptmi_cull::kCullComputed | ptmi_cull::kCullWideComputed)) && (far_ref & REF_LEAF) && certified(far_one) && rule(far_one ? n.lo1 : n.lo2, far_one ? n.hi1 : n.hi2) ? 1 : 0);
                    stack.push_back(far_ref);
                }
                cur = first ? n.ref1 : n.ref2; direct = true; marked = false;
                if (cur & REF_LEAF) {
                    const uint32_t count = ref_leaf_count(cur);
                    if (!certified(first)) out[11]++;
                    if (certified(first) && rule(first ? n.lo1 : n.lo2, first ? n.hi1 : n.hi2)) {
                        out[4]++; out[6]++; out[7] += count; out[3] += count;
                        pop = true;
                    }
                }
            }
        }
        if (pop && !finished) {
            if (stack.empty()) break;
            cur = stack.back(); stack.pop_back();
            direct = false;
            marked = mark.back() != 0;
            mark.pop_back();
        }
    }
    std::memcpy(&out[1], &limit, 4);
    return 0;
}

// The cull words of `n_rec` records (tri_ids[i] == 0xFFFFFFFF: an inner record) against both tiers computed afresh from the
// records' own boxes and `tris` with leaf_is_cullable / leaf_is_cullable_wide:
// out[0] = inner records, out[1] = leaf children (not flagged empty), out[2] = of them with the tight bit, out[3] = with the wide
// bit, out[4] = with the wide bit only, out[5] = records whose low three bits are not kCullComputed + the tight tier afresh,
// out[6] = records whose next three bits are not kCullWideComputed + the wide tier afresh, out[7] = records with a bit outside the six,
// out[8] = tight leaves without the wide bit.
void wide_check_records(const DNode* recs, const uint32_t* tri_ids, uint32_t n_rec, const ptmi_triangle* tris, uint32_t out[9])
{
    std::memset(out, 0, 9 * sizeof(uint32_t));
    for (uint32_t i = 0; i < n_rec; i++) {
        if (tri_ids[i] != 0xFFFFFFFFu) continue;
        const DNode& n = recs[i];
        out[0]++;
        const uint32_t start1 = n.ref1 & REF_INDEX_MASK_LEAF, start2 = n.ref2 & REF_INDEX_MASK_LEAF;
        const auto tri1 = [&](uint32_t k) -> const ptmi_triangle& { return tris[tri_ids[start1 + k]]; };
        const auto tri2 = [&](uint32_t k) -> const ptmi_triangle& { return tris[tri_ids[start2 + k]]; };
        const uint32_t tight = ptmi_cull::kCullComputed | (ptmi_cull::leaf_is_cullable(n.ref1, n.lo1, n.hi1, tri1) ? ptmi_cull::kCullChild1 : 0u) |
                               (ptmi_cull::leaf_is_cullable(n.ref2, n.lo2, n.hi2, tri2) ? ptmi_cull::kCullChild2 : 0u);
        const uint32_t wide = ptmi_cull::kCullWideComputed | (ptmi_cull::leaf_is_cullable_wide(n.ref1, n.lo1, n.hi1, tri1) ? ptmi_cull::kCullWide1 : 0u) |
                              (ptmi_cull::leaf_is_cullable_wide(n.ref2, n.lo2, n.hi2, tri2) ? ptmi_cull::kCullWide2 : 0u);
        if ((n.cull & 7u) != tight) out[5]++;
        if ((n.cull & (7u << ptmi_cull::kCullWideShift)) != wide) out[6]++;
        if (n.cull & ~63u) out[7]++;
        const bool leaf[2] = {(n.ref1 & REF_LEAF) && !(n.ref1 & REF_EMPTY), (n.ref2 & REF_LEAF) && !(n.ref2 & REF_EMPTY)};
        const uint32_t t_bit[2] = {ptmi_cull::kCullChild1, ptmi_cull::kCullChild2}, w_bit[2] = {ptmi_cull::kCullWide1, ptmi_cull::kCullWide2};
        for (int c = 0; c < 2; c++) {
            if (!leaf[c]) continue;
            out[1]++;
            if (n.cull & t_bit[c]) out[2]++;
            if (n.cull & w_bit[c]) out[3]++;
            if ((n.cull & w_bit[c]) && !(n.cull & t_bit[c])) out[4]++;
            if ((n.cull & t_bit[c]) && !(n.cull & w_bit[c])) out[8]++;
        }
    }
}

}  // extern "C"
