// guide_buffers.hip - what the camera sees, per pixel, without rendering it (ptmi_render_guides, ptmi.h): the first segment of
// the paths ptmi_render traces, summed over a range of iterations into albedo / normal / position / hit-count planes, and the
// triangle, material and side of the first iteration's hit.
//
// Nothing of the integrator is restated here.  A primary ray is trace_path's `primary_ray`, its closest hit the ray query's
// `query` (both ptmi_literal_path.hpp); the surface is load_surface's and a miss collects sky_color.  What is this kernel's own:
//   * one lane per pixel and one wave per 8 x 8 tile, as the wavefront kernel lays out its paths, in a grid-stride loop over
//     tiles; the lanes of an edge tile that lie outside the image idle;
//   * a lane runs its iterations one after the other and keeps the four sums in registers, so every plane is written once;
//   * the LDS traversal stack is sized at launch by the depth of the uploaded tree, like the query kernel's.
// The kernel only READS scene memory: no accumulator, histogram or counter of the context is touched.
#include <hip/hip_runtime.h>

#include "ptmi_literal_path.hpp"

namespace PTMI_DEV_NS {

constexpr uint32_t kGuideWaves = kBlock / 64;  // 4 waves = 4 tiles; a lane keeps one pixel and one column of the stack

template <bool PRE>
__global__ void __launch_bounds__(kBlock) guide_kernel(const DScene sc, const DGuides out, const uint32_t first_iteration,
                                                            const uint32_t n_iterations, const uint32_t tiles_x,
                                                            const uint32_t n_tiles)
{
    extern __shared__ uint32_t guide_stack[];  // [stack_levels][kBlock]
    uint32_t* const stack = &guide_stack[threadIdx.x];
    const uint32_t wave = threadIdx.x >> 6, in_tile = threadIdx.x & 63u;

    for (uint32_t tile = blockIdx.x * kGuideWaves + wave; tile < n_tiles; tile += gridDim.x * kGuideWaves) {
        const uint32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const uint32_t gx = tile_x * 8u + (in_tile & 7u), gy = tile_y * 8u + (in_tile >> 3);
        if (gx >= sc.width || gy >= sc.height) continue;  // (no barrier anywhere: a lane may sit a tile out)

        V4 albedo = v4(0, 0, 0, 0), normal = v4(0, 0, 0, 0), position = v4(0, 0, 0, 0);
        float hit_count = 0;
        uint32_t id_triangle = 0xFFFFFFFFu, id_material = 0, id_front = 0;
        for (uint32_t k = 0; k < n_iterations; k++) {
            const uint32_t iteration = first_iteration + k;
            int seed;
            float sample_x, sample_y;
            const Ray r = primary_ray(sc, gx, gy, iteration, seed, sample_x, sample_y);
            float limit = INFINITY;
            Hit hit = no_hit();
            PathCounters pc{0, 0};
            if (query<false, PRE>(sc, r, limit, hit, pc, stack)) {
                Surface sf;
                load_surface(sc, r, hit, sf);
                albedo = albedo + sf.color;
                normal = normal + sf.Ns;
                position = position + hit.point;
                hit_count += 1.f;
                if (k == 0) {
                    id_triangle = sc.tri_ids[hit.tri];
                    const DShade* sh = &sc.shade[id_triangle];
                    id_material = hit.front ? sh->mat_pos : sh->mat_neg;  // the one load_surface shaded
                    id_front = hit.front ? 1u : 0u;
                }
            } else {
                albedo = albedo + sky_color(sc.sky, sc.texels, r.d);  // :1281-1288 with transfer = 1
            }
        }

        const size_t p = (size_t)gy * sc.width + gx;
        if (out.albedo) reinterpret_cast<float4*>(out.albedo)[p] = make_float4(albedo.x, albedo.y, albedo.z, albedo.w);
        if (out.normal) reinterpret_cast<float4*>(out.normal)[p] = make_float4(normal.x, normal.y, normal.z, normal.w);
        if (out.position) reinterpret_cast<float4*>(out.position)[p] = make_float4(position.x, position.y, position.z, position.w);
        if (out.hit_count) out.hit_count[p] = hit_count;
        if (out.ids) reinterpret_cast<uint4*>(out.ids)[p] = make_uint4(id_triangle, id_material, id_front, 0u);
    }
}

}  // namespace PTMI_DEV_NS

namespace ptmi_internal {

int PTMI_ARITH(launch_guides)(const DScene& sc, const DGuides& planes, uint32_t first_iteration, uint32_t n_iterations,
                              uint32_t stack_levels, void* stream, std::string* err)
{
    using namespace PTMI_DEV_NS;
    if (n_iterations == 0 || sc.width == 0 || sc.height == 0) return PTMI_OK;
    const auto kernel = sc.tris_precomputed != 0 ? guide_kernel<true> : guide_kernel<false>;
    const uint32_t tiles_x = (sc.width + 7u) / 8u, tiles_y = (sc.height + 7u) / 8u;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
    if (n_tiles > 0x7FFFFFFFull) {  // (the tile index plus its grid-stride step stays below 2^32)
        if (err) *err = "guide_kernel: the image has too many tiles";
        return PTMI_ERR_INTERNAL;
    }
    uint32_t blocks = 0;
    size_t lds_bytes = 0;
    if (int rc = stack_kernel_grid(stack_levels, (n_tiles + kGuideWaves - 1) / kGuideWaves, "PTMI_GUIDE_MAX_BLOCKS", "guide_kernel",
                                   &blocks, &lds_bytes, err))
        return rc;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds_bytes, (hipStream_t)stream, sc, planes, first_iteration,
                       n_iterations, tiles_x, (uint32_t)n_tiles);
    return launch_status(hipGetLastError(), "guide_kernel", err);
}

}  // namespace ptmi_internal
