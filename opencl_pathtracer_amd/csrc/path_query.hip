// path_query.hip - full paths from rays the CALLER supplies (ptmi_trace_paths, ptmi.h): what light arrives along them.
//
// One path = Kernel_Main's (FullKernel.cl:1180-1331) with its camera ray replaced by the caller's: the seed of the path's index
// (InitializeRandomSeed), the sampler's draws made and discarded, Ray3D_Create of the caller's origin and direction, then the
// bounce loop - `trace_path_from` of ptmi_literal_path.hpp, the one definition the render kernels run - bit for bit in the
// arithmetic of the build.  What is this kernel's own:
//   * the head of the path: index, seed, discarded draws, the caller's ray;
//   * the queries take the 5-comparison box test where scene, ray and limit allow it (`query`, as the ray queries do): the same
//     triangles and the same counts as the literal test, chosen once per query;
//   * the LDS traversal stack is sized at launch by the depth of the uploaded tree, not by PTMI_BVH_MAX_DEPTH;
//   * the grid-stride loop over the caller's rays; a lane owns one ray for ALL its iterations, with the sums in registers.
// The kernel only READS scene memory: no accumulator, histogram or counter of the context is touched.
#include <hip/hip_runtime.h>

#include "ptmi_literal_path.hpp"

namespace PTMI_DEV_NS {

struct PathBatch {
    uint32_t n_rays, first_iteration, n_iterations, first_index, index_stride;
};

// rays: 3 x 16 bytes each (ptmi_ray; the third quad - the distance limit and the reserved words - is not read: Kernel_Main's
// segments start unlimited), sums: 3 x 16 bytes each (ptmi_path_sum); a lane keeps one ray and one column of the stack
template <bool PRE>
__global__ void __launch_bounds__(kBlock) trace_paths_kernel(const DScene sc, const float4* __restrict__ rays,
                                                             float4* __restrict__ sums, const PathBatch b)
{
    extern __shared__ uint32_t path_stack[];  // [stack_levels][kBlock]
    uint32_t* const stack = &path_stack[threadIdx.x];

    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < b.n_rays; i += gridDim.x * kBlock) {
        const float4 in_o = rays[3 * (size_t)i], in_d = rays[3 * (size_t)i + 1];
        Ray r;
        r.o = v4(in_o);
        ray_set_direction(r, v4(in_d));
        V4 sum = v4(0, 0, 0, 0);
        uint32_t n_seg = 0, n_hits = 0, n_shadow = 0;
        unsigned long long n_bbx = 0, n_tri = 0;
        for (uint32_t k = 0; k < b.n_iterations; k++) {
            // index = first_index + i + it * index_stride (mod 2^32): the gx + gy * W + it * W * H of InitializeRandomSeed
            int seed = lcg_seed(b.first_index + i, 0u, b.index_stride, 1u, b.first_iteration + k, sc.source_seed != 0);
            if (sc.sampler != PTMI_SAMPLER_UNIFORM) {  // sampler(), cl:1119-1150: JITTERED and RANDOM draw twice, UNIFORM never
                (void)lcg_random(seed);
                (void)lcg_random(seed);
            }
            uint32_t depth;
            PathCounters pc;
            const V4 radiance = trace_path_from<PRE, true>(sc, r, seed, stack, depth, n_seg, n_shadow, pc);
            sum = sum + radiance;
            n_hits += depth;
            n_bbx += pc.bbx;
            n_tri += pc.tri;
        }
        sums[3 * (size_t)i] = make_float4(sum.x, sum.y, sum.z, sum.w);
        sums[3 * (size_t)i + 1] = make_float4(__uint_as_float(n_seg), __uint_as_float(n_hits), __uint_as_float(n_shadow), 0.0f);
        sums[3 * (size_t)i + 2] = make_float4(__uint_as_float((uint32_t)n_bbx), __uint_as_float((uint32_t)(n_bbx >> 32)),
                                              __uint_as_float((uint32_t)n_tri), __uint_as_float((uint32_t)(n_tri >> 32)));
    }
}

}  // namespace PTMI_DEV_NS

namespace ptmi_internal {

int PTMI_ARITH(launch_trace_paths)(const DScene& sc, const void* d_rays, void* d_sums, uint32_t n_rays, uint32_t first_iteration,
                                   uint32_t n_iterations, uint32_t first_index, uint32_t index_stride, uint32_t stack_levels,
                                   void* stream, std::string* err)
{
    using namespace PTMI_DEV_NS;
    if (n_rays == 0 || n_iterations == 0) return PTMI_OK;
    const auto kernel = sc.tris_precomputed ? trace_paths_kernel<true> : trace_paths_kernel<false>;
    uint32_t blocks = 0;
    size_t lds_bytes = 0;
    if (int rc = stack_kernel_grid(stack_levels, ((uint64_t)n_rays + kBlock - 1) / kBlock, "PTMI_QUERY_MAX_BLOCKS",
                                   "trace_paths_kernel", &blocks, &lds_bytes, err))
        return rc;
    const PathBatch b{n_rays, first_iteration, n_iterations, first_index, index_stride};
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds_bytes, (hipStream_t)stream, sc, static_cast<const float4*>(d_rays),
                       static_cast<float4*>(d_sums), b);
    return launch_status(hipGetLastError(), "trace_paths_kernel", err);
}

}  // namespace ptmi_internal
