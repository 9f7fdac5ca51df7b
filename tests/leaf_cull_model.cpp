// leaf_cull_model.cpp - the rule and the certificate of csrc/leaf_cull.h behind a C interface, and a serial model of one BVH
// query over the records build_layout makes (csrc/scene_layout.cpp), with the wavefront kernel's visit order and its culling.
// Compiled by tests/test_leaf_cull_model.py and tools/leaf_cull_potential.py together with tests/scene_refit_model.cpp (which
// supplies the layout and the serial refit) - no HIP.
//
// The walk takes its box and triangle decisions from the CALLER's functions: the tests pass the oracle's exported deciders
// (pto_bounding_box_intersects, pto_triangle_intersects), so the model decides nothing about geometry itself except whether a
// leaf is culled.
#include <cstdint>
#include <cstring>
#include <vector>

#include "leaf_cull.h"
#include "ptmi_internal.h"
#include "scene_layout.h"

using namespace ptmi_internal;

extern "C" {

typedef int (*box_decider)(const ptmi_bounding_box* bb, const float origin[4], const float direction[4], float squared_distance);
typedef int (*tri_decider)(const ptmi_triangle* tri, const float origin[4], const float direction[4], float* squared_distance, float* s,
                           float* t, float point[4]);

void cull_constants(double out[4]) { out[0] = ptmi_cull::kRel; out[1] = ptmi_cull::kAbs; out[2] = ptmi_cull::kKappaMax; out[3] = ptmi_cull::kEpsAbsMax; }

float cull_box_distance2(const float lo[3], const float hi[3], const float o[3]) { return ptmi_cull::box_distance2(lo, hi, o[0], o[1], o[2]); }

// o: the origin's four components; dw: the direction's fourth
int cull_rule(const float lo[3], const float hi[3], const float o[4], float dw, float limit)
{
    return ptmi_cull::leaf_cull_rule(ptmi_cull::box_distance2(lo, hi, o[0], o[1], o[2]), limit, o[0], o[1], o[2], o[3], dw) ? 1 : 0;
}

// out: eps_abs, kappa (untouched when the triangle gets no bound at all)
int cull_triangle_slack(const ptmi_triangle* t, const float lo[3], const float hi[3], double out[2])
{
    return ptmi_cull::triangle_slack(*t, lo, hi, &out[0], &out[1]) ? 1 : 0;
}

int cull_triangle_certified(const ptmi_triangle* t, const float lo[3], const float hi[3]) { return ptmi_cull::triangle_certified(*t, lo, hi) ? 1 : 0; }

// mode: 0 = every leaf is tested; 1 = direct leaves are culled (what the kernel does); 2 = also far children that satisfy the
// rule when they are pushed (a limit only shrinks during a query); 3 = mode 2 with a zero-margin rule and no certificate (the
// potential the margins are measured against: NOT a valid rule).
// out[0] = hit record (0xFFFFFFFF none), out[1] = bits of the final limit, out[2] = box tests, out[3] = triangle tests counted,
// out[4] = leaves reached directly, out[5] = leaves popped, out[6] = direct leaves culled, out[7] = their triangles,
// out[8] = popped leaves culled (modes 2, 3; in mode 1: that WOULD be), out[9] = their triangles, out[10] = triangles tested,
// out[11] = direct leaves without a certificate
int cull_walk(const DNode* recs, const uint32_t* tri_ids, const DBigLeaf* big_leaves, uint32_t root_ref, const ptmi_triangle* tris,
              box_decider box_hit, tri_decider tri_hit, const float o[4], const float d[4], float limit, int shadow, int mode, uint32_t out[12])
{
    std::memset(out, 0, 12 * sizeof(uint32_t));
    out[0] = 0xFFFFFFFFu;
    std::vector<uint32_t> stack;
    std::vector<uint8_t> mark;  // per stack entry: a leaf that satisfied the rule when it was pushed
    uint32_t cur = root_ref;
    bool direct = false, marked = false;
    auto rule = [&](const float lo[3], const float hi[3]) {
        const float d2 = ptmi_cull::box_distance2(lo, hi, o[0], o[1], o[2]);
        if (mode == 3) return d2 > limit && d2 < 0x1p+90f;
        return ptmi_cull::leaf_cull_rule(d2, limit, o[0], o[1], o[2], o[3], d[3]);
    };
    bool finished = false;
    while (!finished) {
        bool pop = false;
        if (cur & REF_LEAF) {
            uint32_t start, count;
            leaf_range(cur, big_leaves, &start, &count);
            out[direct ? 4 : 5]++;
            if (marked) { out[8]++; out[9] += count; }
            if (marked && mode >= 2) {
                out[3] += count;
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
            auto cullable = [&](bool one) {
                const uint32_t r = one ? n.ref1 : n.ref2;
                if (mode == 3) return (r & REF_LEAF) && !(r & REF_EMPTY) && ref_leaf_count(r) != REF_COUNT_BIG;
                return (n.cull & (one ? ptmi_cull::kCullChild1 : ptmi_cull::kCullChild2)) != 0u;
            };
            if (!h1 && !h2) {
                pop = true;
            } else {
                const bool first = fwd ? h1 : !h2;
                if (h1 && h2) {
                    const uint32_t far_ref = fwd ? n.ref2 : n.ref1;
                    const bool far_one = !fwd;
                    mark.push_back((far_ref & REF_LEAF) && cullable(far_one) && rule(far_one ? n.lo1 : n.lo2, far_one ? n.hi1 : n.hi2) ? 1 : 0);
                    stack.push_back(far_ref);
                }
                cur = first ? n.ref1 : n.ref2; direct = true; marked = false;
                if (cur & REF_LEAF) {
                    const uint32_t count = ref_leaf_count(cur);
                    if (!cullable(first)) out[11]++;
                    if (mode >= 1 && cullable(first) && rule(first ? n.lo1 : n.lo2, first ? n.hi1 : n.hi2)) {
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

// build_layout's cull bits for `scene`: out[0] = inner records, out[1] = of them with kCullComputed, out[2] = leaf children (not
// flagged empty), out[3] = of them cullable, out[4] = inner records whose cull word is not zero.  Returns build_layout's status.
int cull_layout_bits(const ptmi_config* cfg, const ptmi_scene* scene, uint32_t out[5])
{
    Relayout lay;
    std::string err;
    std::memset(out, 0, 5 * sizeof(uint32_t));
    const int rc = build_layout(*cfg, scene, lay, err);
    if (rc != PTMI_OK) return rc;
    for (size_t i = 0; i < lay.recs.size(); i++) {
        if (lay.tri_ids[i] != 0xFFFFFFFFu) continue;
        const DNode& n = *reinterpret_cast<const DNode*>(&lay.recs[i]);
        out[0]++;
        if (n.cull & ptmi_cull::kCullComputed) out[1]++;
        if (n.cull) out[4]++;
        if ((n.ref1 & REF_LEAF) && !(n.ref1 & REF_EMPTY)) { out[2]++; if (n.cull & ptmi_cull::kCullChild1) out[3]++; }
        if ((n.ref2 & REF_LEAF) && !(n.ref2 & REF_EMPTY)) { out[2]++; if (n.cull & ptmi_cull::kCullChild2) out[3]++; }
    }
    return rc;
}

}  // extern "C"
