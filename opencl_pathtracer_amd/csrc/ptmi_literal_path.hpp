// ptmi_literal_path.hpp - one path of the reference, its loops as they are written (Kernel_Main, FullKernel.cl:1180-1331):
// the body of the one-path-per-lane kernel (kernels.hip), what the wavefront kernel's launches fall back on for the rare
// path whose closest-hit query accepts a NaN distance (kernel_wavefront.hip: redo_poisoned_kernel), and - from the bounce loop
// on - the path of a ray the caller supplies (path_query.hip).
#pragma once

#include "ptmi_device.hpp"
#include "ptmi_shading.hpp"
#include "render_region.h"

namespace PTMI_DEV_NS {

constexpr int kBlock = 256;
constexpr int kStackDepth = PTMI_BVH_MAX_DEPTH;

struct PathCounters {
    uint32_t bbx, tri;  // numIntersectedBBx / numIntersectedTri of the current path
};

// (A launch's staging slot -> the path's pixel and iteration id: decode_slot, render_region.h.)

// The three statistics atomics of a finished path as the reference issues them (FullKernel.cl:1319-1331).
__device__ __forceinline__ void count_path_in_histograms(const DScene& sc, uint32_t depth, uint32_t bbx, uint32_t tri)
{
    // (as_global: `sc` may itself lie in memory, as the wavefront kernel's cold scene does, and its pointers are generic then)
    atomicAdd(&as_global(sc.hist_depths)[depth], 1u);
    if (bbx < PTMI_MAX_INTERSECTION_NUMBER) atomicAdd(&as_global(sc.hist_bbx)[bbx], 1u);
    if (tri < PTMI_MAX_INTERSECTION_NUMBER) atomicAdd(&as_global(sc.hist_tri)[tri], 1u);
}

// A sample of the RANDOM sampler lands on an arbitrary pixel `off`; the reference races there (:1339-1345), here every update
// is an atomic add.  `super_sampling`: from iteration 1 on also the variance (:1346-1349) - the reference read-modify-writes
// that of a pixel other work-items may be updating too.  As in the reference, a pixel whose first sample arrives after
// iteration 0 divides 0 by 0 here, keeps a NaN variance and is never skipped (:1168: the comparison with NaN is false) - with
// this sampler 29 % of the pixels get no sample in iteration 0, so that quirk decides how many samples a render takes and is
// kept (the staged form guards its one such case instead).
__device__ __forceinline__ void add_random_sample(const DScene& sc, uint32_t off, V4 radiance, bool super_sampling, uint32_t iteration)
{
    // (the atomics return what the accumulators held before: sumBefore / nRayBefore of :1339-1342)
    float* const color = &as_global(sc.image_color)[4 * off];  // (as_global: see count_path_in_histograms)
    const V4 before = v4(atomicAdd(&color[0], radiance.x), atomicAdd(&color[1], radiance.y),
                         atomicAdd(&color[2], radiance.z), atomicAdd(&color[3], radiance.w));
    const float n_before = atomicAdd(&as_global(sc.image_ray_nb)[off], 1.f);
    if (super_sampling) {
        float* const vp = &as_global(sc.image_v)[4 * off];
        if (iteration != 0u) {
            const V4 after = before + radiance;
            const float n_after = n_before + 1.f;
            atomicAdd(&vp[0], (radiance.x - fdiv(before.x, n_before)) * (radiance.x - fdiv(after.x, n_after)));
            atomicAdd(&vp[1], (radiance.y - fdiv(before.y, n_before)) * (radiance.y - fdiv(after.y, n_after)));
            atomicAdd(&vp[2], (radiance.z - fdiv(before.z, n_before)) * (radiance.z - fdiv(after.z, n_after)));
            atomicAdd(&vp[3], (radiance.w - fdiv(before.w, n_before)) * (radiance.w - fdiv(after.w, n_after)));
        }
    }
}

// BVH_IntersectRay (FullKernel.cl:620-702) when ANY_HIT == false,
// BVH_IntersectShadowRay (:705-783) when true.  Same visit order as the
// reference: at an inner node the child on the side the ray comes from
// (dir[cutAxis] > 0 ? son1 : son2) is tested first and descended first, the
// other is pushed; leaf triangles in ascending index with the distance limit
// updated between tests.
// `stack`: the lane's column of a [level][lane] array, kBlock words from one level to the next.
// ORDERED: the 5-comparison box test, for a ray and a scene that allow it (box_hit_ordered: the caller asks).
// Returns whether a triangle was accepted; hit.tri = its RECORD index, `limit` = the squared distance it left.
template <bool ANY_HIT, bool PRE, bool ORDERED>
__device__ __forceinline__ bool walk(const DScene& sc, const Ray& r, float& limit, Hit& hit, PathCounters& pc,
                                     uint32_t* __restrict__ stack)
{
    bool found = false;
    int top = 0;
    uint32_t cur = sc.root_ref;
    for (;;) {
        if (cur & REF_LEAF) {
            uint32_t start, count;
            leaf_range(cur, sc.big_leaves, &start, &count);
            for (uint32_t i = start; i < start + count; i++) {
                pc.tri++;
                const float4* q4 = reinterpret_cast<const float4*>(&sc.tris[i]);
                if (tri_hit_record<PRE>(q4[0], q4[1], q4[2], q4[3], r, limit, hit)) {
                    hit.tri = i;
                    if (ANY_HIT) return true;
                    found = true;
                }
            }
            if (top == 0) break;
            cur = stack[(--top) * kBlock];
        } else {
            const float4* np = reinterpret_cast<const float4*>(&sc.nodes[cur & REF_INDEX_MASK_INNER]);
            const NodeView n = node_view(np[0], np[1], np[2], np[3]);
            const float da = n.axis == 0 ? r.d.x : (n.axis == 1 ? r.d.y : r.d.z);
            const bool fwd = da > 0;
            const bool h1 = ORDERED ? box_hit_ordered(n.lo1, n.hi1, r, limit) : box_hit(n.lo1, n.hi1, (n.ref1 & REF_EMPTY) != 0, r, limit);
            const bool h2 = ORDERED ? box_hit_ordered(n.lo2, n.hi2, r, limit) : box_hit(n.lo2, n.hi2, (n.ref2 & REF_EMPTY) != 0, r, limit);
            pc.bbx += 2;
            const uint32_t near_ref = fwd ? n.ref1 : n.ref2, far_ref = fwd ? n.ref2 : n.ref1;
            const bool near_hit = fwd ? h1 : h2, far_hit = fwd ? h2 : h1;
            if (near_hit) {
                if (far_hit) stack[(top++) * kBlock] = far_ref;
                cur = near_ref;
            } else if (far_hit) {
                cur = far_ref;
            } else {
                if (top == 0) break;
                cur = stack[(--top) * kBlock];
            }
        }
    }
    return found;
}

// A closest-hit query of a ray whose direction is NaN in every component (the scattered ray of a hit on a zero-area
// triangle, whose normal is 0/0): every comparison of the box test and of the triangle test is false, so every non-empty
// box is "hit" and every triangle accepted - the query walks the WHOLE tree in one fixed order and keeps its last triangle
// (seconds for one path on a million triangles, ten times per path).  The upload has walked it once
// (scene_layout.cpp: nan_walk_*): the counts are added and the LAST triangle's test is made for real, which leaves the
// very record, bit for bit, that the walk would leave.
template <bool ANY_HIT>
__device__ __forceinline__ bool nan_walk_applies(const DScene& sc, const Ray& r)
{
    return !ANY_HIT && sc.nan_walk_box_tests != 0xFFFFFFFFu && (r.d.x != r.d.x) & (r.d.y != r.d.y) & (r.d.z != r.d.z);
}
template <bool PRE>
__device__ __forceinline__ bool nan_walk(const DScene& sc, const Ray& r, float& limit, Hit& hit, PathCounters& pc)
{
    pc.bbx += sc.nan_walk_box_tests;
    pc.tri += sc.nan_walk_tri_tests;
    if (sc.nan_walk_last_tri == 0xFFFFFFFFu) return false;
    const float4* q4 = reinterpret_cast<const float4*>(&sc.tris[sc.nan_walk_last_tri]);
    const bool accepted = tri_hit_record<PRE>(q4[0], q4[1], q4[2], q4[3], r, limit, hit);
    hit.tri = sc.nan_walk_last_tri;
    return accepted;
}

// One query of a ray, for every kernel that keeps one ray per lane: the shortcut, else the walk with the 5-comparison box test
// where scene, ray and limit allow it (MAY_ORDER; box_hit_ordered takes the limit as never negative), else the walk with the
// LITERAL box test - the same triangle, bit for bit, whichever is taken.  `limit`: as for walk.
template <bool ANY_HIT, bool PRE, bool MAY_ORDER = true>
__device__ __forceinline__ bool query(const DScene& sc, const Ray& r, float& limit, Hit& hit, PathCounters& pc,
                                      uint32_t* __restrict__ stack)
{
    if (nan_walk_applies<ANY_HIT>(sc, r)) return nan_walk<PRE>(sc, r, limit, hit, pc);
    if (MAY_ORDER && sc.boxes_ordered && ray_slabs_are_ordered(r) && !(limit < 0)) return walk<ANY_HIT, PRE, true>(sc, r, limit, hit, pc, stack);
    return walk<ANY_HIT, PRE, false>(sc, r, limit, hit, pc, stack);
}

// The camera ray of sample (gx, gy, iteration) as Kernel_Main makes it (FullKernel.cl:1208-1215); `seed` is left where the
// path goes on.  (kernel_wavefront.hip, "start the next camera path", keeps a copy that reads the cold scene record.)
__device__ __forceinline__ Ray primary_ray(const DScene& sc, uint32_t gx, uint32_t gy, uint32_t iteration, int& seed,
                                           float& sample_x, float& sample_y)
{
    seed = lcg_seed(gx, gy, sc.width, sc.height, iteration, sc.source_seed != 0);
    draw_sample(sc, gx, gy, iteration, seed, sample_x, sample_y);
    Ray r;
    r.o = v4(sc.cam_pos);
    ray_set_direction(r, mad(v4(sc.cam_up), sample_y, mad(v4(sc.cam_right), sample_x, v4(sc.cam_dir))));  // cl:1213
    return r;
}

// The bounce loop of Kernel_Main (FullKernel.cl:1224-1317) from a ray that has been made and a seed that stands where the path
// goes on: the ONE definition for the render kernel, the wavefront kernel's retraces (both through trace_path) and the paths of
// a caller's own rays (path_query.hip).  Returns the radiance; `depth` = the surface hits, `segments` and `shadows` are added to.
// MAY_ORDER: the queries may take the 5-comparison box test where it applies (`query`); false, the ordered form switched off,
// is what makes these loops the fallback for everything the fast forms cannot express.
template <bool PRE, bool MAY_ORDER = false>
__device__ __forceinline__ V4 trace_path_from(const DScene& sc, Ray r, int seed, uint32_t* __restrict__ stack, uint32_t& depth,
                                              uint32_t& segments, uint32_t& shadows, PathCounters& pc)
{
    V4 radiance = v4(0, 0, 0, 0), transfer = v4(1, 1, 1, 1);
    bool active = true, in_water = false;
    uint32_t reflection = 0;
    pc.bbx = 0;
    pc.tri = 0;

    while (active && reflection < sc.max_depth) {
        Hit hit = no_hit();
        segments++;
        float unlimited = INFINITY;
        if (query<false, PRE, MAY_ORDER>(sc, r, unlimited, hit, pc, stack)) {
            Surface sf;
            load_surface(sc, r, hit, sf);

            // Scene_ComputeDirectIllumination, FullKernel.cl:901-954: every light, every bounce
            V4 direct = v4(0, 0, 0, 0);
            for (uint32_t li = 0; li < sc.n_lights; li++) {
                const ptmi_light light = sc.lights[li];
                const bool directional = light.type == PTMI_LIGHT_DIRECTIONNAL;
                const V4 full = directional ? -v4(light.direction) : v4(light.position) - hit.point;
                Ray lr;
                lr.o = hit.point;
                ray_set_direction(lr, full);
                float light_distance = directional ? INFINITY : length(full);  // linear, :938
                const float brdf = material_brdf(sf.mat.type, -lr.d, sf.Ns, r.d);
                Hit dummy;
                shadows++;
                if (!query<true, PRE, MAY_ORDER>(sc, lr, light_distance, dummy, pc, stack))
                    direct = mad(v4(1, 1, 1, 1) * (light_power_toward(light, hit.point, sf.Ns) * brdf), v4(light.color), direct);  // cl:945
            }

            radiance = radiance + scatter(r, seed, in_water, hit, sf, direct, transfer);
            reflection++;
        } else {
            active = false;
            radiance = mad(sky_color(sc.sky, sc.texels, r.d), transfer, radiance);  // :1281-1288
        }
        if (active) active = path_continues(transfer, reflection, seed, sc.russian_roulette != 0);  // :1296-1314
    }
    depth = reflection;
    return radiance;
}

// One path = one Kernel_Main work-item (FullKernel.cl:1180-1331) up to the
// statistics; returns the radiance and the sample position.
// `stop_criterion_draw`: SUPER_SAMPLING draws one random number for its stop criterion before the path starts (cl:1219-1222,
// from iteration 6 on); a caller that re-traces a path of such a render passes true so that the path's numbers are the same.
template <bool PRE>
__device__ __forceinline__ V4 trace_path(const DScene& sc, uint32_t gx, uint32_t gy, uint32_t iteration,
                                         uint32_t* __restrict__ stack, float& sample_x, float& sample_y,
                                         uint32_t& depth, uint32_t& segments, uint32_t& shadows, PathCounters& pc,
                                         bool stop_criterion_draw = false)
{
    int seed;
    const Ray r = primary_ray(sc, gx, gy, iteration, seed, sample_x, sample_y);
    if (stop_criterion_draw) (void)lcg_random(seed);
    return trace_path_from<PRE>(sc, r, seed, stack, depth, segments, shadows, pc);
}

}  // namespace PTMI_DEV_NS
