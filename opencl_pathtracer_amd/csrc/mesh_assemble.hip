// mesh_assemble.hip - the device side of ptmi_update_vertices: 336-byte ptmi_triangle records assembled from the caller's vertex
// buffers and the topology ptmi_bind_mesh stored (mesh_assemble.h).  One lane per triangle; every value comes from
// mesh_assemble_common.h, the header ptmi_assemble_triangles and tests/mesh_assemble_model.cpp compute it from.  A lane reads
// its row of the topology planes (coalesced 16-byte loads), gathers 9 (with normals 18) floats, and writes the one record that
// is its own as 21 sixteen-byte words.  No atomics, no LDS, nothing shared between lanes.
#include <hip/hip_runtime.h>

#include "mesh_assemble.h"
#include "mesh_assemble_common.h"
#include "ptmi_internal.h"

namespace ptmi_internal {

namespace {

constexpr uint32_t kBlock = 256;

// the sink of mesh_assemble_common.h: word k of the lane's record, one 16-byte store
typedef float Word __attribute__((ext_vector_type(4)));
struct RecordOnDevice {
    Word* words;
    __device__ __forceinline__ void f4(int k, const ptmi_float4& v) const { words[k] = Word{v.x, v.y, v.z, v.w}; }
    __device__ __forceinline__ void u4(int k, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const
    {
        words[k] = Word{__uint_as_float(x), __uint_as_float(y), __uint_as_float(z), __uint_as_float(w)};
    }
};

__global__ void __launch_bounds__(kBlock) assemble_triangles_kernel(const uint4* __restrict__ head, const float4* __restrict__ uv,
                                                                    const uint2* __restrict__ tail, const uint32_t n_tris,
                                                                    const void* __restrict__ positions, const uint32_t position_stride,
                                                                    const void* __restrict__ normals, const uint32_t normal_stride,
                                                                    ptmi_triangle* __restrict__ out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_tris) return;
    const uint4 h = head[i];
    const uint2 t = tail[i];
    ptmi_mesh::Corner c0{}, c1{}, c2{};
    if (uv) {
        const float4 a = uv[i], b = uv[(size_t)n_tris + i], c = uv[2 * (size_t)n_tris + i];
        c0.uvp = {a.x, a.y}; c1.uvp = {a.z, a.w}; c2.uvp = {b.x, b.y};
        c0.uvn = {b.z, b.w}; c1.uvn = {c.x, c.y}; c2.uvn = {c.z, c.w};
    }
    c0.p = ptmi_mesh::fetch3(positions, position_stride, h.x, 1.f);
    c1.p = ptmi_mesh::fetch3(positions, position_stride, h.y, 1.f);
    c2.p = ptmi_mesh::fetch3(positions, position_stride, h.z, 1.f);
    if (normals) {
        c0.m = ptmi_mesh::fetch3(normals, normal_stride, h.x, 0.f);
        c1.m = ptmi_mesh::fetch3(normals, normal_stride, h.y, 0.f);
        c2.m = ptmi_mesh::fetch3(normals, normal_stride, h.z, 0.f);
    }
    ptmi_mesh::assemble_triangle(c0, c1, c2, normals == nullptr, h.w, t.x, t.y, RecordOnDevice{reinterpret_cast<Word*>(out + i)});
}

}  // namespace

int launch_assemble_triangles(const MeshTopologyPlanes& topology, const void* positions, uint32_t position_stride, const void* normals,
                              uint32_t normal_stride, ptmi_triangle* out, void* stream, std::string* err)
{
    const uint32_t n = topology.n_triangles;
    if (n == 0) return PTMI_OK;
    hipLaunchKernelGGL(assemble_triangles_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(topology.head), reinterpret_cast<const float4*>(topology.uv),
                       reinterpret_cast<const uint2*>(topology.tail), n, positions, position_stride, normals, normal_stride, out);
    return launch_status(hipGetLastError(), "assemble_triangles_kernel", err);
}

}  // namespace ptmi_internal
