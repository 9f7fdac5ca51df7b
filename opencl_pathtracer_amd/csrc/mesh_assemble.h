// mesh_assemble.h - ptmi_update_vertices: the topology a context keeps on devices[0] and the launch of mesh_assemble.hip.
// See DESIGN.md 1j.
#pragma once

#include <string>

#include "ptmi.h"

namespace ptmi_internal {

// The bound topology on the device, as planes a wave reads with one 16-byte (tail: 8-byte) load per lane, consecutive lanes
// consecutive addresses:
//   head[i] = {indices[3i], indices[3i+1], indices[3i+2], mat_pos[i]}
//   uv[0][i] = {uvp0, uvp1}, uv[1][i] = {uvp2, uvn0}, uv[2][i] = {uvn1, uvn2}  of triangle i, corners in face order;
//              uv == nullptr where the topology was bound without texture coordinates (all twelve are +0)
//   tail[i] = {mat_neg[i], id[i]}
struct MeshTopologyPlanes {
    const uint32_t* head = nullptr;  // uint4 per triangle
    const float* uv = nullptr;       // 3 planes of float4 per triangle, plane p at uv + 4 * p * n_triangles
    const uint32_t* tail = nullptr;  // uint2 per triangle
    uint32_t n_triangles = 0;
};

// out[i] = mesh_assemble_common.h: assemble_triangle of face i, i < topology.n_triangles, from three floats at
// positions + v * position_stride (and normals + v * normal_stride; normals == nullptr: flat).  Every index of `head` is below
// the vertex count the buffers hold (ptmi_bind_mesh checked it).  Asynchronous on `stream`; reads the buffers, writes `out`.
int launch_assemble_triangles(const MeshTopologyPlanes& topology, const void* positions, uint32_t position_stride, const void* normals,
                              uint32_t normal_stride, ptmi_triangle* out, void* stream, std::string* err);

}  // namespace ptmi_internal
