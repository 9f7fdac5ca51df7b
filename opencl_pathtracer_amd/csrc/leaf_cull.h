// leaf_cull.h - leaves whose triangles cannot be accepted: the rule the wavefront kernel applies per ray and the certificate the
// host (scene_layout.cpp) and the refit (scene_refit_common.h) compute per leaf.  HIP-free: the kernel, the host and the serial
// model of the tests (tests/leaf_cull_model.cpp) compile this one copy.
//
// The reference's box test compares the LINEAR entry parameter with the SQUARED hit distance (FullKernel.cl:135), so a query
// walks on through every box its ray pierces behind the hit it has found, and the walk has to stay: the per-path box-test and
// triangle-test counts are results.  What need not stay is the fetch and the test of a triangle that cannot be accepted.
//
// CLAIM (proof: DESIGN.md 5, "Leaves beyond the closest hit").  Let a leaf's box [lo, hi] and its triangles pass
// leaf_is_cullable(), and let a ray with a finite origin and a direction of length <= 1 + 2^-20 satisfy
// leaf_cull_rule(box_distance2(lo, hi, origin), limit, origin, direction.w).  Then Triangle_Intersects (FullKernel.cl:519-589) as the reference
// computes it in float, in either arithmetic, rejects every triangle of the leaf at that `limit`: acceptance needs a computed
// squared distance nsd <= limit (:537), and an accepted point lies within eps of the box, eps = eps_abs + kappa * D with
// eps_abs <= kEpsAbsMax and kappa <= kKappaMax (what the certificate bounds), so that nsd >= (1 - 8u) ((1 - kappa) D - eps_abs)^2,
// which the rule's two margins put above `limit`.  The state of the query after the leaf is then known without reading a record:
// its triangle count goes up by the leaf's count and nothing else changes.
// The claim holds for any pair of margins (kRel, kAbs) with the gates (kKappaMax, kEpsAbsMax) its two inequalities allow.  There
// are two such tiers, the tight one above and the wide one (leaf_is_cullable_wide, leaf_cull_rule_wide); the kernel applies the
// wide rule to the leaves of both (a tight certificate implies the wide one).
#ifndef PTMI_LEAF_CULL_H
#define PTMI_LEAF_CULL_H

#include <cmath>
#include <cstdint>

#include "ptmi_internal.h"

namespace ptmi_cull {

// ---- the rule -------------------------------------------------------------------------------------------------------------
// D2 > kRel * limit + kAbs, D2 the squared distance from the ray origin to the box.  NOT the ray's entry parameter: for a ray that
// grazes the entry face, a point before the entry lies outside the box by |dir_axis| * dt only.  kRel pays for every error that
// grows with D (kappa), kAbs for the absolute ones (eps_abs).  An origin that is not finite never culls: fmaxf drops a NaN, so the
// rule looks at the origin itself (kMaxOrigin; the wavefront kernel gives up rays from beyond 2^40 before they traverse).
constexpr float kRel = 1.001f, kAbs = 0.01f, kMaxOrigin = 0x1p+41f;
// what the certificate may grant: with eta = (kRel - 1) / 2,  (1 - kappa)^2 (1 - eta) kRel >= 1 + 40u  and  eps_abs^2 / eta <= 0.99 kAbs
constexpr double kKappaMax = 0x1p-13, kEpsAbsMax = 2.0e-3;
// The WIDE pair, the one the kernel applies: the culled leaves lie between the hit distance d and d^2 along the ray (the
// reference compares a linear parameter with a squared distance), so a margin of a per cent in D2 loses next to nothing, and it
// buys a kappa gate 16 times as wide - thin triangles, whose conditioning is what kappa measures, are most of what the tight
// gate refuses (tris1m: 18.1 % of the leaves without a certificate, 1.2 % with this one; profiles/leaf_cull_potential_tris1m.json).
// The same two inequalities with eta = (kRelWide - 1) / 2 = 0.005:  (1 - 2^-9)^2 * 0.995 * 1.01 = 1.00103 >= 1 + 40u  and
// (1.5e-2)^2 / 0.005 = 0.045 <= 0.99 * 0.05 = 0.0495.  kRel <= kRelWide, kAbs <= kAbsWide and both gates are wider: the wide
// rule implies the tight rule and a tight certificate the wide one (a leaf of either tier may be culled under the wide rule).
constexpr float kRelWide = 1.01f, kAbsWide = 0.05f;
constexpr double kKappaWideMax = 0x1p-9, kEpsAbsWideMax = 1.5e-2;

// DNode::cull of an inner record: the children that are cullable leaves, and "this record's bits were computed" (a refit
// recomputes the bits of the records that carry them and leaves the others alone: scene_refit_common.h)
constexpr uint32_t kCullChild1 = 1u, kCullChild2 = 2u, kCullComputed = 4u;
// DScene::leaf_cull, the mask the kernel ANDs a record's bits with: the children it may cull where the step chooses them itself,
// and - in the position of kCullComputed, which every record that carries a child bit has set - "also where it would push them".
constexpr uint32_t kCullPushed = kCullComputed;
// ... and the same three for the wide certificate, kCullWideShift above: the children that are leaves of the wide tier (set
// beside the tight bit where a leaf has both: a tight certificate implies the wide one) and a copy of "computed".  So
// `cull >> kCullWideShift` reads as the three tight bits do, for the wide tier, and the kernel's tests are the same
// instructions whichever tier a launch looks at.
constexpr uint32_t kCullWideShift = 3u;
constexpr uint32_t kCullWide1 = kCullChild1 << kCullWideShift, kCullWide2 = kCullChild2 << kCullWideShift, kCullWideComputed = kCullComputed << kCullWideShift;
// DScene::leaf_cull only: the kernel looks at the tight bits alone (PTMI_LEAF_CULL=3, for A/B runs in one binary)
constexpr uint32_t kCullTightOnly = 64u;
// What a launch hands the kernel, from DScene::leaf_cull: by how much it shifts a record's word down before it ANDs it with the
// three mask bits - the wide tier's bits, which hold the leaves of either tier, unless the scene keeps to the tight one.
constexpr uint32_t kernel_cull_shift(uint32_t scene_leaf_cull) { return (scene_leaf_cull & kCullTightOnly) ? 0u : kCullWideShift; }
constexpr uint32_t kernel_cull_mask(uint32_t scene_leaf_cull) { return scene_leaf_cull & (kCullChild1 | kCullChild2 | kCullPushed); }

PTMI_HD float box_distance2(const float lo[3], const float hi[3], float ox, float oy, float oz)
{
    // max(lo - o, o - hi, 0) per axis: at most one of the two differences is positive (lo <= hi)
    const float dx = fmaxf(fmaxf(lo[0] - ox, ox - hi[0]), 0.0f);
    const float dy = fmaxf(fmaxf(lo[1] - oy, oy - hi[1]), 0.0f);
    const float dz = fmaxf(fmaxf(lo[2] - oz, oz - hi[2]), 0.0f);
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// The same value from the differences a slab test forms anyway: per axis the pair (lo - o, hi - o), in either order.  Their
// median with 0 is lo - o where that is positive, hi - o where that is negative - the exact negation of o - hi, and the sign
// goes in the square - and 0 between: for lo <= hi, box_distance2 bit for bit (tests/test_leaf_cull_slab_distance.py).
// (A NaN difference: whatever the median instruction returns; such a ray does not cull, ray_may_cull.)
PTMI_HD float median_with_zero(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(a, 0.0f, b);
#else
    return fmaxf(fminf(a, b), fminf(fmaxf(a, b), 0.0f));
#endif
}
PTMI_HD float box_distance2_from_slabs(float ax, float bx, float ay, float by, float az, float bz)
{
    const float mx = median_with_zero(ax, bx), my = median_with_zero(ay, by), mz = median_with_zero(az, bz);
    return fmaf(mz, mz, fmaf(my, my, mx * mx));
}

// The part of the rule that is the ray's alone (the kernel evaluates it once, where it sets the ray up).  The origin: above.
// The fourth components: the importers write N.w = 1 (their normalize keeps the w of a cross product of points), so the plane
// of the test is N.xyz . x + x.w = d, and it is the triangle's plane of xyz exactly when the computed point has the vertices'
// w.  Points carry w = 1 and directions w = 0 everywhere but behind a GLASS / WATER reflection (Numerics); a ray of
// another kind never culls (the certificate wants S1.w = 1 of a triangle whose N.w is not zero).
PTMI_HD bool ray_may_cull(float ox, float oy, float oz, float ow, float dw)
{
    return fabsf(ox) + fabsf(oy) + fabsf(oz) <= kMaxOrigin && ow == 1.0f && dw == 0.0f;  // (all false for a NaN)
}
// ... and the part that is the box's
PTMI_HD bool box_is_beyond(float d2, float limit)
{
    return d2 > fmaf(limit, kRel, kAbs);  // (false for a NaN)
}
PTMI_HD bool leaf_cull_rule(float d2, float limit, float ox, float oy, float oz, float ow, float dw)
{
    return box_is_beyond(d2, limit) && ray_may_cull(ox, oy, oz, ow, dw);
}
// the wide pair's (what node_step evaluates, for the leaves of both tiers)
// (the right-hand side by itself: it changes only with the limit, and a node step judges two boxes against it)
PTMI_HD float cull_threshold_wide(float limit)
{
    return fmaf(limit, kRelWide, kAbsWide);
}
PTMI_HD bool box_is_beyond_wide(float d2, float limit)
{
    return d2 > cull_threshold_wide(limit);  // (false for a NaN)
}
// "The record certifies the child AND its box lies beyond" as ONE compare (what the kernel's counting step evaluates per child):
// bit 0 of `certified` becomes the sign of the distance - which is never negative - and -d2 < -threshold is d2 > threshold;
// an uncertified child keeps a key >= 0, which is never below a negated threshold that is not positive.
// PRECONDITION: neg_threshold <= 0 or a NaN, i.e. neg_threshold = -cull_threshold_wide(limit) of a limit that is not negative
// (the kernel's limits are squared distances, a linear distance or +inf; then the threshold is at least kAbsWide).  For a
// limit below -kAbsWide / kRelWide the negated threshold is positive and an UNCERTIFIED child nearer than it would compare
// true: not what this function is for (tests/test_node_step_diet.py pins both sides of that line).
// False for a NaN on either side, as box_is_beyond_wide is.
PTMI_HD bool certified_and_beyond_wide(uint32_t certified, float d2, float neg_threshold)
{
    uint32_t bits;
    __builtin_memcpy(&bits, &d2, sizeof bits);
    bits |= certified << 31;
    float key;
    __builtin_memcpy(&key, &bits, sizeof key);
    return key < neg_threshold;
}
PTMI_HD bool leaf_cull_rule_wide(float d2, float limit, float ox, float oy, float oz, float ow, float dw)
{
    return box_is_beyond_wide(d2, limit) && ray_may_cull(ox, oy, oz, ow, dw);
}

// ---- the certificate (double precision, at upload and in a refit) --------------------------------------------------------------
// What a float-accepted point of THIS triangle can lie outside the box [lo, hi] by: eps <= *eps_abs + *kappa * D for every ray
// the claim speaks of (D: distance of its origin from the box).  False: no bound (the triangle is never certified).
// u = 2^-24.  B = the largest norm of a point of the box, so |origin| <= D + B; an accepted point q has |q - o| <= D (its nsd
// is <= limit < D^2), so every coordinate the test computes is below 2 (D + B).  The terms, in the order of the proof:
//   * q lies off the plane N.x = d by rounding errors below 28 u (D + B + |N.w|) - the division by N.dir does not amplify them;
//     N.w enters d and N.o as one more term each, which cancels up to its rounding, and drops out of N.dir (dir.w = 0) - plus
//     the tilt of N against the true normal times the triangle's size; the one term that grows as the ray grazes the plane, the
//     error of N.dir itself, moves q ALONG the normal by <= 4.1 u |q - o| / |cos|, and the distance of the origin from the
//     plane is |q - o| |cos|: in |q - o|^2 the two cancel to a relative 9 u;
//   * the barycentric test sees w = q - S1, |w| <= 2 D + diam(box), rounded (3 u (D + B)), and computes s, t with absolute
//     errors E_s = e |w| |u| |v|^2 |1/det|, E_t = e |w| |u|^2 |v| |1/det|, e = 10.1 u (three roundings in each of w.u, w.v, four
//     in the numerator: the conditioning 1 / sin^2 of the triangle's angle enters here) from Gram coefficients that are floats
//     themselves: K = (float map) o (true Gram matrix) differs from the identity by dk, computed here from the very floats the
//     kernel uses, in both arithmetics;
//   * so the true barycentrics of an accepted point satisfy s >= -sigma_s, t >= -sigma_t, s + t <= 1 + sigma_s + sigma_t + 2u
//     with sigma = E + 0.025 (E_s + E_t) + 1.25 dk, a triangle whose corners lie within
//     max(sigma_s |u| + sigma_t |v|, (sigma_s + 2 sigma_t) |u| + sigma_t |v|, sigma_s |u| + (2 sigma_s + sigma_t) |v|)
//     of the corners of the true one, whose vertices lie inside the box.
PTMI_HD bool triangle_slack(const ptmi_triangle& t, const float lo[3], const float hi[3], double* eps_abs, double* kappa)
{
    const double u24 = 0x1p-24;
    const float S[3][3] = {{t.s1.x, t.s1.y, t.s1.z}, {t.s2.x, t.s2.y, t.s2.z}, {t.s3.x, t.s3.y, t.s3.z}};
    if (!(t.s1.w == t.s2.w && t.s1.w == t.s3.w && fabsf(t.s1.w) <= 0x1p+20f)) return false;  // edge vectors with w = +0 (DTriPre)
    if (!(t.n.w == 0.0f || (t.s1.w == 1.0f && fabsf(t.n.w) <= 4.0f))) return false;  // the plane is a plane of xyz for the rule's rays
    double B2 = 0;
    for (int k = 0; k < 3; k++) {
        if (!(lo[k] <= hi[k] && fabsf(lo[k]) <= 0x1p+20f && fabsf(hi[k]) <= 0x1p+20f)) return false;  // (false for a NaN)
        for (int j = 0; j < 3; j++)
            if (!(S[j][k] >= lo[k] && S[j][k] <= hi[k])) return false;  // the caller's tree may hold any box
        const double m = fmax(fabs((double)lo[k]), fabs((double)hi[k]));
        B2 += m * m;
    }
    const double B = sqrt(B2);
    // the edge vectors and their Gram coefficients as the kernel computes them (ptmi_device.hpp: tri_test, dot = fma chain)
    const float uf[3] = {S[1][0] - S[0][0], S[1][1] - S[0][1], S[1][2] - S[0][2]}, vf[3] = {S[2][0] - S[0][0], S[2][1] - S[0][1], S[2][2] - S[0][2]};
    const float uv_c = fmaf(uf[2], vf[2], fmaf(uf[1], vf[1], uf[0] * vf[0])), uu_c = fmaf(uf[2], uf[2], fmaf(uf[1], uf[1], uf[0] * uf[0])),
                vv_c = fmaf(vf[2], vf[2], fmaf(vf[1], vf[1], vf[0] * vf[0]));
    // ... and exactly
    const double ud[3] = {uf[0], uf[1], uf[2]}, vd[3] = {vf[0], vf[1], vf[2]};
    const double uu = ud[0] * ud[0] + ud[1] * ud[1] + ud[2] * ud[2], vv = vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2],
                 uv = ud[0] * vd[0] + ud[1] * vd[1] + ud[2] * vd[2];
    const double lu = sqrt(uu), lv = sqrt(vv);
    if (!(lu >= 0x1p-16 && lv >= 0x1p-16)) return false;  // (no product of the test underflows)
    const double cr[3] = {ud[1] * vd[2] - ud[2] * vd[1], ud[2] * vd[0] - ud[0] * vd[2], ud[0] * vd[1] - ud[1] * vd[0]};
    const double area2 = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    if (!(area2 > 0)) return false;
    // the record's normal against the true one
    const double N[3] = {t.n.x, t.n.y, t.n.z};
    const double Nn = (N[0] * cr[0] + N[1] * cr[1] + N[2] * cr[2]) / area2, len_n = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
    if (!(fabs(Nn) >= 0.25 && len_n <= 4.0)) return false;
    const double tan2 = len_n * len_n - Nn * Nn;
    const double tilt = sqrt(tan2 > 0 ? tan2 : 0) / fabs(Nn);
    if (!(tilt <= 0x1p-18)) return false;
    // the reciprocal determinant of the two arithmetics (FullKernel.cl:556; the default one's reciprocal is an instruction's
    // value, within 2 ulp of this one: the 8u below)
    const float det_c[2] = {uv_c * uv_c - uu_c * vv_c, fmaf(uv_c, uv_c, -(uu_c * vv_c))};
    double dk = 0, c_w = 0;  // c_w: the distance of an accepted point from the triangle, per unit of |w|
    for (int m = 0; m < 2; m++) {
        if (!(det_c[m] < 0.0f)) return false;
        const double den = (double)(1.0f / det_c[m]);
        if (!std::isfinite(den)) return false;
        const double k11 = den * ((double)uv_c * uv - (double)vv_c * uu) - 1.0, k12 = den * ((double)uv_c * vv - (double)vv_c * uv);
        const double k21 = den * ((double)uv_c * uu - (double)uu_c * uv), k22 = den * ((double)uv_c * uv - (double)uu_c * vv) - 1.0;
        dk = fmax(dk, fmax(fabs(k11) + fabs(k12), fabs(k21) + fabs(k22)) + 8 * u24);
        const double e = 10.1 * u24 * fabs(den) * (1 + 8 * u24), es = e * lu * lv * lv, et = e * lu * lu * lv;
        const double ss = es + 0.025 * (es + et), st = et + 0.025 * (es + et);
        c_w = fmax(c_w, fmax(ss * lu + st * lv, fmax((ss + 2 * st) * lu + st * lv, ss * lu + (2 * ss + st) * lv)));
    }
    if (!(dk <= 0.01)) return false;
    const double diam = sqrt(((double)hi[0] - lo[0]) * ((double)hi[0] - lo[0]) + ((double)hi[1] - lo[1]) * ((double)hi[1] - lo[1]) +
                             ((double)hi[2] - lo[2]) * ((double)hi[2] - lo[2]));
    *kappa = 0x1p-18 + 2 * c_w;
    *eps_abs = 32 * u24 * (B + fabs((double)t.n.w) / fabs(Nn)) + c_w * diam + (5 * dk + 4 * u24 + 2 * tilt) * (lu + lv);
    return std::isfinite(*kappa) && std::isfinite(*eps_abs);
}

PTMI_HD bool triangle_certified(const ptmi_triangle& t, const float lo[3], const float hi[3])
{
    double eps_abs, kappa;
    return triangle_slack(t, lo, hi, &eps_abs, &kappa) && eps_abs <= kEpsAbsMax && kappa <= kKappaMax;
}

PTMI_HD bool triangle_certified_wide(const ptmi_triangle& t, const float lo[3], const float hi[3])
{
    double eps_abs, kappa;
    return triangle_slack(t, lo, hi, &eps_abs, &kappa) && eps_abs <= kEpsAbsWideMax && kappa <= kKappaWideMax;
}

// Is the child behind `ref`, with the box the record holds for it, a leaf the kernel may cull?  An ordinary leaf (not flagged
// empty, one to six triangles in the reference itself) whose triangles are all certified.  tri_at(k): its k-th triangle.
template <class TriAt>
PTMI_HD bool leaf_is_cullable(uint32_t ref, const float lo[3], const float hi[3], TriAt tri_at)
{
    using namespace ptmi_internal;
    if (!(ref & REF_LEAF) || (ref & REF_EMPTY)) return false;
    const uint32_t count = ref_leaf_count(ref);
    if (count == 0u || count == REF_COUNT_BIG) return false;
    for (uint32_t k = 0; k < count; k++)
        if (!triangle_certified(tri_at(k), lo, hi)) return false;
    return true;
}
// ... under the wide rule?
template <class TriAt>
PTMI_HD bool leaf_is_cullable_wide(uint32_t ref, const float lo[3], const float hi[3], TriAt tri_at)
{
    using namespace ptmi_internal;
    if (!(ref & REF_LEAF) || (ref & REF_EMPTY)) return false;
    const uint32_t count = ref_leaf_count(ref);
    if (count == 0u || count == REF_COUNT_BIG) return false;
    for (uint32_t k = 0; k < count; k++)
        if (!triangle_certified_wide(tri_at(k), lo, hi)) return false;
    return true;
}

// Both answers from one evaluation of each triangle's slack (a refit asks per record): bit 0 = leaf_is_cullable, bit 1 =
// leaf_is_cullable_wide.
template <class TriAt>
PTMI_HD uint32_t leaf_cull_tiers(uint32_t ref, const float lo[3], const float hi[3], TriAt tri_at)
{
    using namespace ptmi_internal;
    if (!(ref & REF_LEAF) || (ref & REF_EMPTY)) return 0u;
    const uint32_t count = ref_leaf_count(ref);
    if (count == 0u || count == REF_COUNT_BIG) return 0u;
    uint32_t tiers = 3u;
    for (uint32_t k = 0; k < count && tiers != 0u; k++) {
        double eps_abs, kappa;
        if (!triangle_slack(tri_at(k), lo, hi, &eps_abs, &kappa)) return 0u;
        if (!(eps_abs <= kEpsAbsMax && kappa <= kKappaMax)) tiers &= ~1u;
        if (!(eps_abs <= kEpsAbsWideMax && kappa <= kKappaWideMax)) tiers &= ~2u;
    }
    return tiers;
}

// DNode::cull of inner record `d`, from the boxes and references it holds; tri_of_record(r): the triangle behind leaf record r.
template <class TriOfRecord>
PTMI_HD uint32_t record_cull_bits(const ptmi_internal::DNode& d, TriOfRecord tri_of_record)
{
    const uint32_t start1 = d.ref1 & ptmi_internal::REF_INDEX_MASK_LEAF, start2 = d.ref2 & ptmi_internal::REF_INDEX_MASK_LEAF;
    uint32_t bits = kCullComputed | kCullWideComputed;
    const uint32_t tiers1 = leaf_cull_tiers(d.ref1, d.lo1, d.hi1, [&](uint32_t k) -> const ptmi_triangle& { return tri_of_record(start1 + k); });
    const uint32_t tiers2 = leaf_cull_tiers(d.ref2, d.lo2, d.hi2, [&](uint32_t k) -> const ptmi_triangle& { return tri_of_record(start2 + k); });
    if (tiers1 & 1u) bits |= kCullChild1;
    if (tiers2 & 1u) bits |= kCullChild2;
    if (tiers1 & 2u) bits |= kCullWide1;
    if (tiers2 & 2u) bits |= kCullWide2;
    return bits;
}

}  // namespace ptmi_cull

#endif  // PTMI_LEAF_CULL_H
