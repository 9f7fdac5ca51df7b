// scene_refit.hip - the device side of ptmi_update_triangles: the records of a loaded scene rewritten from a new triangulation
// (see scene_refit.h).  Three streaming kernels, one lane per record / triangle / inner node of a level; every
// value comes from scene_refit_common.h, the header the host's upload path and the serial model (tests/scene_refit_model.cpp)
// compute it from.  No atomics, nothing shared between lanes: a lane reads the caller's triangles and, in a level pass, records
// of the level below (written by an earlier launch), and writes the one record that is its own, as whole 16-byte words.
// In front of them, for ptmi_update_triangles_device alone, the screen kernel: the host's checks of the new triangles, one lane
// per triangle, answered in one word (at most one atomicMin per wave that refuses, none in a good update).  And, for
// ptmi_update_materials, the same protocol over the DShade records the device holds: screen_shade_kernel.
#include <hip/hip_runtime.h>

#include "scene_refit.h"
#include "scene_refit_common.h"

namespace ptmi_internal {

namespace {

constexpr uint32_t kBlock = 256;

// `Words` 16-byte words from a lane's own copy of a record to the record array
template <int Words>
__device__ __forceinline__ void store_words(void* dst, const void* src)
{
    float4* const d = static_cast<float4*>(dst);
    const float4* const s = static_cast<const float4*>(src);
#pragma unroll
    for (int k = 0; k < Words; k++) d[k] = s[k];
}

template <bool Precomputed>
__global__ void __launch_bounds__(kBlock) update_tri_records_kernel(DTri* __restrict__ records, const uint32_t* __restrict__ tri_ids,
                                                                    const uint32_t n_records, const ptmi_triangle* __restrict__ tris,
                                                                    const uint32_t n_tris)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_records) return;
    const uint32_t id = tri_ids[r];
    if (id >= n_tris) return;  // (a node record's 0xFFFFFFFF)
    alignas(16) DTri rec;
    if (Precomputed) ptmi_refit::make_tri_record_pre(tris[id], reinterpret_cast<DTriPre*>(&rec));
    else ptmi_refit::make_tri_record(tris[id], &rec);
    store_words<4>(records + r, &rec);
}

__global__ void __launch_bounds__(kBlock) update_shade_records_kernel(DShade* __restrict__ shade, const ptmi_triangle* __restrict__ tris,
                                                                      const uint32_t n_tris)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_tris) return;
    alignas(16) DShade rec;
    ptmi_refit::make_shade_record(tris[i], &rec);
    store_words<sizeof(DShade) / 16>(shade + i, &rec);
}

// (records: read at the children's indices, written at the lane's own - no __restrict__)
__global__ void __launch_bounds__(kBlock) refit_level_kernel(DNode* records, const uint32_t* __restrict__ level_nodes, const uint32_t n,
                                                             const DBigLeaf* __restrict__ big_leaves, const uint32_t* __restrict__ tri_ids,
                                                             const ptmi_triangle* __restrict__ tris)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    DNode* const mine = records + level_nodes[k];
    alignas(16) DNode d;
    store_words<4>(&d, mine);
    ptmi_refit::refit_record(&d, records, big_leaves, tri_ids, tris);
    store_words<4>(mine, &d);
}

// The screen of ptmi_update_triangles_device: one lane per triangle, one verdict each (scene_refit_common.h: screen_triangle, the
// host loop's own function), and of all refusals the smallest word (index << 4) | code into *verdict, which the host set to
// kScreenAccepted.  A lane's word grows with its lane number, so a wave's smallest is its first refusing lane's: that lane issues
// the wave's one atomic, and a wave without a refusal - every wave of a good update - issues none.  Lanes past n take part in the
// ballot with no refusal and read nothing.
__global__ void __launch_bounds__(kBlock) screen_update_kernel(const ptmi_triangle* __restrict__ tris, const uint32_t n_tris,
                                                               const uint8_t* __restrict__ material_is_simple_color,
                                                               const uint32_t materiaux_size, const uint32_t tris_precomputed,
                                                               uint32_t* __restrict__ verdict)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t code = ptmi_refit::kScreenOk;
    if (i < n_tris) code = ptmi_refit::screen_triangle(tris[i], material_is_simple_color, materiaux_size, tris_precomputed != 0);
    const unsigned long long refusing = __ballot(code != ptmi_refit::kScreenOk);
    if (refusing == 0) return;
    const uint32_t lane = __lane_id();
    if (lane == (uint32_t)__ffsll(refusing) - 1u) atomicMin(verdict, ptmi_refit::screen_word(i, code));
}

// The screen of ptmi_update_materials: one lane per DShade record the context holds (its index is the caller's triangle index),
// the verdict of scene_refit_common.h: screen_shade_materials under the NEW table of plain-colour materials, answered as above.
// A lane fetches the quad with its two material indices and, only where one of them is textured, the three quads of texture
// coordinates: four 16-byte loads at most, 16 of a record's 112 bytes where its materials are plain.  Nothing is written but
// the one word.
__global__ void __launch_bounds__(kBlock) screen_shade_kernel(const DShade* __restrict__ shade, const uint32_t n_tris,
                                                              const uint8_t* __restrict__ material_is_simple_color,
                                                              const uint32_t materiaux_size, uint32_t* __restrict__ verdict)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t code = ptmi_refit::kScreenOk;
    if (i < n_tris) {
        const uint4* const quads = reinterpret_cast<const uint4*>(shade + i);  // (records of 7 x 16 bytes in a hipMalloc'ed array)
        code = ptmi_refit::screen_shade_materials(
            [quads](uint32_t k) {
                const uint4 q = quads[k];
                return ptmi_refit::ShadeQuad{{q.x, q.y, q.z, q.w}};
            },
            material_is_simple_color, materiaux_size);
    }
    const unsigned long long refusing = __ballot(code != ptmi_refit::kScreenOk);
    if (refusing == 0) return;
    const uint32_t lane = __lane_id();
    if (lane == (uint32_t)__ffsll(refusing) - 1u) atomicMin(verdict, ptmi_refit::screen_word(i, code));
}

dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

}  // namespace

int launch_screen_shade(const DShade* shade, uint32_t triangulation_size, const uint8_t* material_is_simple_color, uint32_t materiaux_size,
                        uint32_t* verdict, void* stream, std::string* err)
{
    if (triangulation_size == 0) return PTMI_OK;
    hipLaunchKernelGGL(screen_shade_kernel, grid_for(triangulation_size), dim3(kBlock), 0, (hipStream_t)stream, shade, triangulation_size,
                       material_is_simple_color, materiaux_size, verdict);
    return launch_status(hipGetLastError(), "screen_shade_kernel", err);
}

int launch_screen_update(const ptmi_triangle* triangulation, uint32_t triangulation_size, const uint8_t* material_is_simple_color,
                         uint32_t materiaux_size, bool tris_precomputed, uint32_t* verdict, void* stream, std::string* err)
{
    if (triangulation_size == 0) return PTMI_OK;
    hipLaunchKernelGGL(screen_update_kernel, grid_for(triangulation_size), dim3(kBlock), 0, (hipStream_t)stream, triangulation,
                       triangulation_size, material_is_simple_color, materiaux_size, tris_precomputed ? 1u : 0u, verdict);
    return launch_status(hipGetLastError(), "screen_update_kernel", err);
}

int launch_update_tri_records(DTri* records, const uint32_t* tri_ids, uint32_t n_records, const ptmi_triangle* triangulation,
                              uint32_t triangulation_size, bool tris_precomputed, void* stream, std::string* err)
{
    if (n_records == 0) return PTMI_OK;
    if (tris_precomputed)
        hipLaunchKernelGGL(update_tri_records_kernel<true>, grid_for(n_records), dim3(kBlock), 0, (hipStream_t)stream, records, tri_ids,
                           n_records, triangulation, triangulation_size);
    else
        hipLaunchKernelGGL(update_tri_records_kernel<false>, grid_for(n_records), dim3(kBlock), 0, (hipStream_t)stream, records, tri_ids,
                           n_records, triangulation, triangulation_size);
    return launch_status(hipGetLastError(), "update_tri_records_kernel", err);
}

int launch_update_shade_records(DShade* shade, const ptmi_triangle* triangulation, uint32_t triangulation_size, void* stream, std::string* err)
{
    if (triangulation_size == 0) return PTMI_OK;
    hipLaunchKernelGGL(update_shade_records_kernel, grid_for(triangulation_size), dim3(kBlock), 0, (hipStream_t)stream, shade, triangulation,
                       triangulation_size);
    return launch_status(hipGetLastError(), "update_shade_records_kernel", err);
}

int launch_refit_level(DNode* records, const uint32_t* level_nodes, uint32_t n, const DBigLeaf* big_leaves, const uint32_t* tri_ids,
                       const ptmi_triangle* triangulation, void* stream, std::string* err)
{
    if (n == 0) return PTMI_OK;
    hipLaunchKernelGGL(refit_level_kernel, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, records, level_nodes, n, big_leaves, tri_ids,
                       triangulation);
    return launch_status(hipGetLastError(), "refit_level_kernel", err);
}

}  // namespace ptmi_internal
