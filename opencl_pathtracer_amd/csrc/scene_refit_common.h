// scene_refit_common.h - the arithmetic of an in-place scene update, shared by the host (scene_layout.cpp, scene_refit_host.cpp),
// the device (scene_refit.hip) and the serial model of the device schedule (tests/scene_refit_model.cpp).
//
// Three things live here, once:
//   * the screen of a new triangle - why build_layout or an in-place update refuses it, as a small code (ScreenCode) - for the
//     host loops and for the screen kernel of ptmi_update_triangles_device (tests/update_screen_model.cpp runs it on its own),
//     and its material part restated on the DShade record a context keeps (ptmi_update_materials; tests/material_screen_model.cpp);
//   * a triangle's device records (DTri / DTriPre / DShade) as build_layout writes them at upload, so that a record rewritten on
//     the device holds the bytes a fresh upload of the same triangle would;
//   * the refit of a box from the boxes below it: a leaf's box is the fold of its triangles' `aabb` in ascending index order
//     (pbox_unite: of values that compare equal the first one wins), an inner node's is pbox_merge(son1, son2) - son1's range
//     precedes son2's, so the merge is the fold over the whole range (bvh_build_common.h).
//     A corner whose refitted value compares equal to the one the box holds keeps the bits it holds (keep_sel): the only
//     values that compare equal and differ are -0 and +0, and which of the two a builder's box holds was decided by the order
//     in which the builder met them (its bins, its triangles before the partition) - an order the finished tree no longer
//     tells.  So a refit with unchanged triangles changes no byte, and one with moved triangles changes what moved.
//
// Compile with -ffp-contract=off (host and device): the products and sums of the DTriPre record are the kernel's own, fused
// only where fmaf says so.
#ifndef PTMI_SCENE_REFIT_COMMON_H
#define PTMI_SCENE_REFIT_COMMON_H

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "bvh_build_common.h"
#include "leaf_cull.h"
#include "ptmi_internal.h"

namespace ptmi_refit {

using ptmi_bvh::PBox;
using ptmi_internal::DBigLeaf;
using ptmi_internal::DNode;
using ptmi_internal::DShade;
using ptmi_internal::DTri;
using ptmi_internal::DTriPre;

// dot() of the kernels: an fma chain over four components (ptmi_device.hpp)
PTMI_HD float dot4(const float a[4], const float b[4])
{
    return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])));
}

// the edge vectors S2 - S1 and S3 - S1 of the triangle test (FullKernel.cl:528-529)
PTMI_HD void triangle_edges(const ptmi_triangle& t, float u[4], float v[4])
{
    u[0] = t.s2.x - t.s1.x; u[1] = t.s2.y - t.s1.y; u[2] = t.s2.z - t.s1.z; u[3] = t.s2.w - t.s1.w;
    v[0] = t.s3.x - t.s1.x; v[1] = t.s3.y - t.s1.y; v[2] = t.s3.z - t.s1.z; v[3] = t.s3.w - t.s1.w;
}

// The DTriPre form needs the importers' convention of equal w on the three vertices: the edge vectors then have w = +0 exactly.
PTMI_HD bool triangle_keeps_equal_w(const ptmi_triangle& t)
{
    return t.s1.w == t.s2.w && t.s1.w == t.s3.w && std::isfinite(t.s1.w);
}

PTMI_HD void store4(float d[4], const ptmi_float4& v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }

// What the intersection test reads, generic form: the three vertices and the normal.
PTMI_HD void make_tri_record(const ptmi_triangle& t, DTri* d)
{
    store4(d->s1, t.s1); store4(d->s2, t.s2); store4(d->s3, t.s3); store4(d->n, t.n);
}

// The ray-independent part of Triangle_Intersects (FullKernel.cl:528-556) done once: the same operations, the same order, the
// same rounding as the kernel's generic form, with the correctly rounded reciprocal of the strict arithmetic (the default
// arithmetic's reciprocal is a device instruction's: launch_precompute_denominators_da patches u_den[3] afterwards).
PTMI_HD void make_tri_record_pre(const ptmi_triangle& t, DTriPre* p)
{
    const float S1[4] = {t.s1.x, t.s1.y, t.s1.z, t.s1.w}, N[4] = {t.n.x, t.n.y, t.n.z, t.n.w};
    float u[4], v[4];
    triangle_edges(t, u, v);
    const float uv = dot4(u, v), uu = dot4(u, u), vv = dot4(v, v);
    const float denom = 1 / (uv * uv - uu * vv);
    p->n[0] = N[0]; p->n[1] = N[1]; p->n[2] = N[2]; p->n[3] = N[3];
    p->s1d[0] = S1[0]; p->s1d[1] = S1[1]; p->s1d[2] = S1[2]; p->s1d[3] = dot4(N, S1);
    p->u_den[0] = u[0]; p->u_den[1] = u[1]; p->u_den[2] = u[2]; p->u_den[3] = denom;
    p->v_s1w[0] = v[0]; p->v_s1w[1] = v[1]; p->v_s1w[2] = v[2]; p->v_s1w[3] = S1[3];
}

// What only a confirmed surface hit reads.
PTMI_HD void make_shade_record(const ptmi_triangle& t, DShade* s)
{
    store4(s->n1, t.n1); store4(s->n2, t.n2); store4(s->n3, t.n3);
    s->uvp[0] = t.uvp1.x; s->uvp[1] = t.uvp1.y; s->uvp[2] = t.uvp2.x; s->uvp[3] = t.uvp2.y; s->uvp[4] = t.uvp3.x; s->uvp[5] = t.uvp3.y;
    s->uvn[0] = t.uvn1.x; s->uvn[1] = t.uvn1.y; s->uvn[2] = t.uvn2.x; s->uvn[3] = t.uvn2.y; s->uvn[4] = t.uvn3.x; s->uvn[5] = t.uvn3.y;
    s->mat_pos = t.mat_pos;
    s->mat_neg = t.mat_neg;
    s->pad[0] = s->pad[1] = 0;
}

// A material without its host pointer: the record the shading reads (build_layout at upload, ptmi_update_materials in place).
PTMI_HD void make_mat_record(const ptmi_material& m, ptmi_internal::DMat* d)
{
    store4(d->color, m.simple_color);
    d->opacity = m.opacity;
    d->texture_id = m.texture_id;
    d->type = m.type;
    d->is_simple_color = m.is_simple_color ? 1u : 0u;
}

// ---- the screen ------------------------------------------------------------------------------------------------------------

// Why one triangle is refused, as a small code: what build_layout asks of every triangle (scene_layout.cpp: its materials and
// texture coordinates, and whether its record can make a triangle test compute a NaN distance) and what an in-place update
// asks on top (scene_refit.h: screen_update).  One copy for the host loops and for the screen kernel of
// ptmi_update_triangles_device (scene_refit.hip), so that both give one verdict for one record.  The codes are in the order of
// the checks: of a triangle with several defects the smallest one is reported.  Words come from scene_layout.cpp:
// screen_message.
enum ScreenCode : uint32_t {
    kScreenOk = 0,
    kScreenMaterial = 1,   // a material index out of range                                  (PTMI_ERR_BAD_SCENE)
    kScreenTexCoord = 2,   // a textured material, and a texture coordinate not finite or beyond 2^30          (PTMI_ERR_BAD_SCENE)
    kScreenVertex = 3,     // a vertex not finite or beyond 2^21                       (PTMI_ERR_UNSUPPORTED, and all that follow)
    kScreenNormal = 4,     // n, n1, n2 or n3 not finite or beyond 16
    kScreenNoArea = 5,     // a barycentric determinant (cl:556, either arithmetic) zero, not finite, or without a finite reciprocal
    kScreenUnequalW = 6,   // unequal w where the uploaded records are DTriPre
    kScreenEmptyBox = 7,   // aabb marked empty
    kScreenBadBox = 8,     // aabb not finite with pMin <= pMax (the centroid included)
};
// The verdict on a whole array in one word: (index << 4) | code of the first refused triangle (an index is below 2^27), or
// kScreenAccepted.  The smallest word of all refused triangles is the first one's.
constexpr uint32_t kScreenAccepted = 0xFFFFFFFFu;
PTMI_HD uint32_t screen_word(uint32_t index, uint32_t code) { return (index << 4) | code; }

constexpr float kScreenCoord = 2097152.0f, kScreenNormalBound = 16.0f, kScreenTexCoordBound = 1073741824.0f;

PTMI_HD bool within4(const ptmi_float4& v, float bound)
{
    return std::fabs(v.x) <= bound && std::fabs(v.y) <= bound && std::fabs(v.z) <= bound && std::fabs(v.w) <= bound;  // (false for NaN)
}
PTMI_HD bool within2(const ptmi_float2& v, float bound) { return std::fabs(v.x) <= bound && std::fabs(v.y) <= bound; }

// Texture coordinates index texels (header.cl:430-459: u - (int)u, then (uint)(u * (width - 1))): beyond the int range the wrap
// does nothing and the index leaves the texture - in the reference as well, which reads whatever is there.
PTMI_HD uint32_t screen_materials(const ptmi_triangle& t, const uint8_t* material_is_simple_color, uint32_t materiaux_size)
{
    if (t.mat_pos >= materiaux_size || t.mat_neg >= materiaux_size) return kScreenMaterial;
    if (!material_is_simple_color[t.mat_pos] || !material_is_simple_color[t.mat_neg])
        if (!(within2(t.uvp1, kScreenTexCoordBound) && within2(t.uvp2, kScreenTexCoordBound) && within2(t.uvp3, kScreenTexCoordBound) &&
              within2(t.uvn1, kScreenTexCoordBound) && within2(t.uvn2, kScreenTexCoordBound) && within2(t.uvn3, kScreenTexCoordBound)))
            return kScreenTexCoord;
    return kScreenOk;
}

// screen_materials restated on the DShade record of a triangle - what a context still holds of it once the caller's array is
// gone (ptmi_update_materials: a material that turns textured puts the texture coordinates of its triangles to the test they were
// spared at upload).  make_shade_record copies the twelve coordinates and both indices unchanged, so the verdict is the
// triangle's.  The record is taken as its seven 16-byte quads, through quad_at(k): the indices lie in quad 6, the coordinates in
// quads 3, 4 and 5, which are fetched only where one of the two materials is textured under the table given.
struct ShadeQuad {
    uint32_t w[4];
};
constexpr uint32_t kShadeQuadTexCoords = 3, kShadeQuadMaterials = 6;
static_assert(offsetof(DShade, uvp) == 16 * kShadeQuadTexCoords && offsetof(DShade, uvn) + sizeof(DShade::uvn) == 16 * kShadeQuadMaterials &&
              offsetof(DShade, mat_pos) == 16 * kShadeQuadMaterials && offsetof(DShade, mat_neg) == 16 * kShadeQuadMaterials + 4 &&
              sizeof(DShade) == 16 * (kShadeQuadMaterials + 1), "the quads of a DShade record");

PTMI_HD bool quad_within(const ShadeQuad& q, float bound)
{
    float v[4];
    __builtin_memcpy(v, q.w, 16);
    return std::fabs(v[0]) <= bound && std::fabs(v[1]) <= bound && std::fabs(v[2]) <= bound && std::fabs(v[3]) <= bound;  // (false for NaN)
}

template <class QuadAt>
PTMI_HD uint32_t screen_shade_materials(QuadAt quad_at, const uint8_t* material_is_simple_color, uint32_t materiaux_size)
{
    const ShadeQuad m = quad_at(kShadeQuadMaterials);
    const uint32_t mat_pos = m.w[0], mat_neg = m.w[1];
    if (mat_pos >= materiaux_size || mat_neg >= materiaux_size) return kScreenMaterial;
    if (!material_is_simple_color[mat_pos] || !material_is_simple_color[mat_neg]) {
        const ShadeQuad a = quad_at(kShadeQuadTexCoords), b = quad_at(kShadeQuadTexCoords + 1), c = quad_at(kShadeQuadTexCoords + 2);
        if (!(quad_within(a, kScreenTexCoordBound) && quad_within(b, kScreenTexCoordBound) && quad_within(c, kScreenTexCoordBound)))
            return kScreenTexCoord;
    }
    return kScreenOk;
}

// ... on a record in host memory (the model of the tests; the device fetches the quads as 16-byte loads: scene_refit.hip)
inline uint32_t screen_shade_record(const DShade& s, const uint8_t* material_is_simple_color, uint32_t materiaux_size)
{
    const unsigned char* const bytes = reinterpret_cast<const unsigned char*>(&s);
    return screen_shade_materials(
        [bytes](uint32_t k) {
            ShadeQuad q;
            __builtin_memcpy(q.w, bytes + 16 * k, 16);
            return q;
        },
        material_is_simple_color, materiaux_size);
}

PTMI_HD bool determinant_is_usable(float d) { return d != 0.0f && std::isfinite(d) && std::isfinite(1.0f / d); }

// Can this triangle's record make a triangle test compute a NaN distance (scene_layout.cpp: scene_needs_literal_kernel)?
PTMI_HD uint32_t screen_literal(const ptmi_triangle& t)
{
    if (!within4(t.s1, kScreenCoord) || !within4(t.s2, kScreenCoord) || !within4(t.s3, kScreenCoord)) return kScreenVertex;
    if (!within4(t.n, kScreenNormalBound) || !within4(t.n1, kScreenNormalBound) || !within4(t.n2, kScreenNormalBound) ||
        !within4(t.n3, kScreenNormalBound))
        return kScreenNormal;
    float u[4], v[4];
    triangle_edges(t, u, v);
    const float uv = dot4(u, v), uu = dot4(u, u), vv = dot4(v, v);
    // cl:556, strict and default arithmetic
    if (!determinant_is_usable(uv * uv - uu * vv) || !determinant_is_usable(fmaf(uv, uv, -(uu * vv)))) return kScreenNoArea;
    return kScreenOk;
}

PTMI_HD bool box_axis_ok(float lo, float hi, float c) { return std::isfinite(lo) && std::isfinite(hi) && std::isfinite(c) && lo <= hi; }

// The whole screen of one triangle of an update: the first failing check, in the order of the codes.
PTMI_HD uint32_t screen_triangle(const ptmi_triangle& t, const uint8_t* material_is_simple_color, uint32_t materiaux_size, bool tris_precomputed)
{
    if (const uint32_t code = screen_materials(t, material_is_simple_color, materiaux_size)) return code;
    if (const uint32_t code = screen_literal(t)) return code;
    if (tris_precomputed && !triangle_keeps_equal_w(t)) return kScreenUnequalW;
    const ptmi_bounding_box& a = t.aabb;
    if (a.is_empty) return kScreenEmptyBox;
    if (!(box_axis_ok(a.p_min.x, a.p_max.x, a.centroid.x) && box_axis_ok(a.p_min.y, a.p_max.y, a.centroid.y) &&
          box_axis_ok(a.p_min.z, a.p_max.z, a.centroid.z)))
        return kScreenBadBox;
    return kScreenOk;
}

// ---- refit --------------------------------------------------------------------------------------------------------------

// `box` united with the aabb of the triangles tri_at(0), tri_at(1), ... tri_at(count - 1), in that order; boxes marked empty are
// skipped (BoundingBox_UniteWith), and `cen`, if given, takes their centroids as points (BoundingBox_AddPoint takes all).
template <class TriAt>
PTMI_HD void fold_triangles(uint32_t count, TriAt tri_at, PBox* box, PBox* cen)
{
    for (uint32_t k = 0; k < count; k++) {
        const ptmi_bounding_box& a = tri_at(k).aabb;
        if (!a.is_empty) ptmi_bvh::pbox_unite(*box, a.p_min, a.p_max, a.centroid);
        if (cen) ptmi_bvh::pbox_add_point(*cen, a.centroid);
    }
}

// of a refitted value and the held one: the held one where they compare equal (-0 / +0), else the refitted one
PTMI_HD float keep_sel(float held, float fresh) { return fresh == held ? held : fresh; }
PTMI_HD ptmi_float4 keep4(const ptmi_float4& held, const ptmi_float4& fresh)
{
    return { keep_sel(held.x, fresh.x), keep_sel(held.y, fresh.y), keep_sel(held.z, fresh.z), keep_sel(held.w, fresh.w) };
}

PTMI_HD PBox corners_box(const float lo[3], const float hi[3])
{
    PBox b;
    b.p_min = ptmi_float4{lo[0], lo[1], lo[2], 0};
    b.p_max = ptmi_float4{hi[0], hi[1], hi[2], 0};
    b.centroid = ptmi_float4{0, 0, 0, 0};
    b.n = 2;  // (a box of a subtree: its centroid is never asked for, only whether it holds anything)
    return b;
}

// The box of the child behind `ref` of an inner record, from what lies below it in the ONE record array: a leaf's triangles
// (through tri_ids into the caller's new triangulation; a big leaf through big_leaves[]), or the two boxes an inner child's own
// record holds - which the level below has refitted already; lo / hi come in as the corners the record holds and keep their bits
// where the value stays (keep_sel).  `ref` is not flagged empty.  Update refuses triangles whose aabb
// is marked empty, so every triangle counts here and the flags of the references stay what the topology made them.
PTMI_HD void refit_child_box(uint32_t ref, const DNode* nodes, const DBigLeaf* big_leaves, const uint32_t* tri_ids,
                             const ptmi_triangle* tris, float lo[3], float hi[3])
{
    using namespace ptmi_internal;
    PBox b = ptmi_bvh::pbox_empty();
    if (ref & REF_LEAF) {
        uint32_t start, count;
        leaf_range(ref, big_leaves, &start, &count);
        const uint32_t* ids = tri_ids + start;
        for (uint32_t k = 0; k < count; k++) {
            const ptmi_bounding_box& a = tris[ids[k]].aabb;
            ptmi_bvh::pbox_unite(b, a.p_min, a.p_max, a.p_min);
        }
    } else {
        const DNode& c = nodes[ref & REF_INDEX_MASK_INNER];
        const PBox first = (c.ref1 & REF_EMPTY) ? ptmi_bvh::pbox_empty() : corners_box(c.lo1, c.hi1);
        const PBox second = (c.ref2 & REF_EMPTY) ? ptmi_bvh::pbox_empty() : corners_box(c.lo2, c.hi2);
        b = ptmi_bvh::pbox_merge(first, second);
    }
    lo[0] = keep_sel(lo[0], b.p_min.x); lo[1] = keep_sel(lo[1], b.p_min.y); lo[2] = keep_sel(lo[2], b.p_min.z);
    hi[0] = keep_sel(hi[0], b.p_max.x); hi[1] = keep_sel(hi[1], b.p_max.y); hi[2] = keep_sel(hi[2], b.p_max.z);
}

// One inner record of a level pass: both child boxes refitted; a child flagged empty keeps what it holds (the inverted infinite
// box where the boxes are ordered).  Reads records of the level below only, writes `d` only: a level's records can be taken in
// any order.  A record that carries "child is a cullable leaf" bits (leaf_cull.h) gets them again from its new boxes and
// triangles, by the function the upload computed them with: unchanged triangles, unchanged bits.
PTMI_HD void refit_record(DNode* d, const DNode* nodes, const DBigLeaf* big_leaves, const uint32_t* tri_ids, const ptmi_triangle* tris)
{
    if (!(d->ref1 & ptmi_internal::REF_EMPTY)) refit_child_box(d->ref1, nodes, big_leaves, tri_ids, tris, d->lo1, d->hi1);
    if (!(d->ref2 & ptmi_internal::REF_EMPTY)) refit_child_box(d->ref2, nodes, big_leaves, tri_ids, tris, d->lo2, d->hi2);
    if (d->cull & ptmi_cull::kCullComputed)
        d->cull = ptmi_cull::record_cull_bits(*d, [&](uint32_t r) -> const ptmi_triangle& { return tris[tri_ids[r]]; });
}

}  // namespace ptmi_refit

#endif  // PTMI_SCENE_REFIT_COMMON_H
