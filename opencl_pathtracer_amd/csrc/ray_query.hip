// ray_query.hip - rays the CALLER supplies, traced against the scene a context holds (ptmi_query_rays, ptmi.h).
//
// One query = the reference's BVH_IntersectRay (FullKernel.cl:620-702, PTMI_QUERY_CLOSEST) or BVH_IntersectShadowRay
// (:705-783, PTMI_QUERY_ANY) on a ray made by Ray3D_Create (header.cl:276-295), bit for bit in the arithmetic of the build
// (ptmi_device.hpp).  A query is `query` of ptmi_literal_path.hpp: the loops the integrator's literal path runs, with the
// 5-comparison box test (box_hit_ordered) for a ray whose slabs are ordered, chosen once per ray.  What is this kernel's own:
//   * the LDS traversal stack is sized at launch by the depth of the uploaded tree, not by PTMI_BVH_MAX_DEPTH;
//   * the grid-stride loop over the caller's rays, and the ptmi_ray_hit it writes for each.
// The kernel only READS scene memory: no accumulator, histogram or counter of the context is touched.
#include <hip/hip_runtime.h>

#include "ptmi_literal_path.hpp"

namespace PTMI_DEV_NS {

// rays: 3 x 16 bytes each (ptmi_ray), hits: 3 x 16 bytes each (ptmi_ray_hit); a lane keeps one ray and one column of the stack
template <bool ANY_HIT, bool PRE>
__global__ void __launch_bounds__(kBlock) query_rays_kernel(const DScene sc, const float4* __restrict__ rays,
                                                                 float4* __restrict__ hits, const uint32_t n_rays)
{
    extern __shared__ uint32_t query_stack[];  // [stack_levels][kBlock]
    uint32_t* const stack = &query_stack[threadIdx.x];

    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_rays; i += gridDim.x * kBlock) {
        const float4 in_o = rays[3 * (size_t)i], in_d = rays[3 * (size_t)i + 1], in_l = rays[3 * (size_t)i + 2];
        Ray r;
        r.o = v4(in_o);
        ray_set_direction(r, v4(in_d));
        float limit = in_l.x;
        Hit hit = no_hit();
        PathCounters pc{0, 0};
        const bool found = query<ANY_HIT, PRE>(sc, r, limit, hit, pc, stack);
        float4 out_p = make_float4(0, 0, 0, 0), out_q = make_float4(0, 0, 0, __uint_as_float(0xFFFFFFFFu));
        uint32_t front = 0;
        if (found) {
            out_p = make_float4(hit.point.x, hit.point.y, hit.point.z, hit.point.w);
            out_q = make_float4(limit, hit.s, hit.t, __uint_as_float(sc.tri_ids[hit.tri]));
            front = hit.front ? 1u : 0u;
        }
        hits[3 * (size_t)i] = out_p;
        hits[3 * (size_t)i + 1] = out_q;
        hits[3 * (size_t)i + 2] = make_float4(__uint_as_float(front), __uint_as_float(pc.bbx), __uint_as_float(pc.tri), 0.0f);
    }
}

}  // namespace PTMI_DEV_NS

namespace ptmi_internal {

int PTMI_ARITH(launch_query_rays)(const DScene& sc, bool any_hit, const void* d_rays, void* d_hits, uint32_t n_rays,
                                  uint32_t stack_levels, void* stream, std::string* err)
{
    using namespace PTMI_DEV_NS;
    if (n_rays == 0) return PTMI_OK;
    const bool pre = sc.tris_precomputed != 0;
    const auto kernel = any_hit ? (pre ? query_rays_kernel<true, true> : query_rays_kernel<true, false>)
                                : (pre ? query_rays_kernel<false, true> : query_rays_kernel<false, false>);
    uint32_t blocks = 0;
    size_t lds_bytes = 0;
    if (int rc = stack_kernel_grid(stack_levels, ((uint64_t)n_rays + kBlock - 1) / kBlock, "PTMI_QUERY_MAX_BLOCKS",
                                   "query_rays_kernel", &blocks, &lds_bytes, err))
        return rc;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds_bytes, (hipStream_t)stream, sc,
                       static_cast<const float4*>(d_rays), static_cast<float4*>(d_hits), n_rays);
    return launch_status(hipGetLastError(), "query_rays_kernel", err);
}

}  // namespace ptmi_internal
