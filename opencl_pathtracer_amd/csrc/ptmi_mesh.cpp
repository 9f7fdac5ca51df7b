// ptmi_mesh.cpp - triangles of a loaded scene updated from vertex and index buffers: ptmi_bind_mesh stores a topology on
// devices[0], ptmi_update_vertices(_device) assembles the 336-byte records there (mesh_assemble.hip) and hands them to the update
// that exists (ptmi_scene_memory.cpp: update_triangles, device form); ptmi_assemble_triangles is the same function on the host,
// without a context.  See include/ptmi.h for the contract and DESIGN.md 1j.
#include <algorithm>
#include <chrono>
#include <vector>

#include "mesh_assemble.h"
#include "mesh_assemble_common.h"
#include "ptmi_context.h"

using namespace ptmi_internal;

namespace {

// What can be said of a topology without a context (empty: nothing)
std::string topology_refusal(const ptmi_mesh_topology* t)
{
    if (!t || t->struct_size != sizeof(ptmi_mesh_topology)) return "topology is NULL or struct_size mismatch (ABI)";
    if (t->reserved != 0) return "topology.reserved is not 0";
    if (t->n_triangles == 0) return "";
    if (t->n_vertices == 0) return "n_vertices is 0";
    if (!t->indices) return "indices is NULL";
    if (!t->mat_pos) return "mat_pos is NULL";
    for (uint32_t i = 0; i < t->n_triangles; i++)
        for (uint32_t k = 0; k < 3; k++)
            if (t->indices[3 * (size_t)i + k] >= t->n_vertices)
                return "triangle " + std::to_string(i) + " corner " + std::to_string(k) + ": index " +
                       std::to_string(t->indices[3 * (size_t)i + k]) + ", the mesh has " + std::to_string(t->n_vertices) + " vertices";
    return "";
}

std::string stride_refusal(const char* name, uint32_t stride)
{
    if (stride < 12 || stride % 4) return std::string(name) + " is " + std::to_string(stride) + " (bytes: at least 12, a multiple of 4)";
    return "";
}

// ... and of vertex buffers for a mesh of n_vertices.  device_form: the pointers are device addresses, 16-byte aligned
std::string buffers_refusal(const ptmi_vertex_buffers* b, uint32_t n_vertices, bool device_form)
{
    if (b->n_vertices != n_vertices)
        return std::to_string(b->n_vertices) + " vertices, the mesh has " + std::to_string(n_vertices);
    std::string why = stride_refusal("position_stride", b->position_stride);
    if (why.empty() && b->normals) why = stride_refusal("normal_stride", b->normal_stride);
    if (!why.empty()) return why;
    if (!b->positions) return "positions is NULL";
    if (device_form && (reinterpret_cast<uintptr_t>(b->positions) & 15u)) return "positions is not 16-byte aligned";
    if (device_form && (reinterpret_cast<uintptr_t>(b->normals) & 15u)) return "normals is not 16-byte aligned";
    return "";
}

ptmi_mesh::Corner corner_of(const ptmi_mesh_topology& t, const ptmi_vertex_buffers& b, size_t corner)
{
    ptmi_mesh::Corner c{};
    const uint32_t v = t.indices[corner];
    c.p = ptmi_mesh::fetch3(b.positions, b.position_stride, v, 1.f);
    if (b.normals) c.m = ptmi_mesh::fetch3(b.normals, b.normal_stride, v, 0.f);
    if (t.uvp) c.uvp = t.uvp[corner];
    c.uvn = t.uvn ? t.uvn[corner] : c.uvp;
    return c;
}

int update_vertices(ptmi_ctx* ctx, const char* who_is_calling, bool device_form, const ptmi_vertex_buffers* vb, ptmi_update_info* info)
{
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
    const clock::time_point t_call = clock::now();
    const std::string who = who_is_calling, prefix = who + ": ";
    if (info) {
        *info = ptmi_update_info{};
        info->struct_size = sizeof(ptmi_update_info);
    }
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (!vb || vb->struct_size != sizeof(ptmi_vertex_buffers))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + "vertex buffers are NULL or struct_size mismatch (ABI)");
    if (int rc = need_scene(ctx, who)) return rc;
    if (!ctx->have_mesh) return fail(ctx, PTMI_ERR_STATE, prefix + "no mesh is bound (ptmi_bind_mesh)");
    const std::string why = buffers_refusal(vb, ctx->mesh_vertices, device_form);
    if (!why.empty()) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + why);
    if (!ctx->literal_kernel_reason.empty())
        return fail(ctx, PTMI_ERR_UNSUPPORTED, prefix + "the uploaded scene has records that can yield NaN distances (" +
                                               ctx->literal_kernel_reason + "): call ptmi_initialize_memory with the new scene");
    // ---- the vertex buffers on devices[0] (nothing of the scene is written before update_triangles has screened the records)
    DeviceState& lead = ctx->dev[0];
    ON_DEVICE(ctx, lead);
    const uint32_t n = ctx->update.triangulation_size;
    const void *d_positions = vb->positions, *d_normals = vb->normals;
    double upload_ms = 0;
    if (!device_form) {
        // the staging buffer holds n_vertices * stride bytes per attribute; of the caller's memory only what lies up to the last
        // vertex's third float is read (an interleaved buffer ends there)
        const size_t nv = vb->n_vertices;
        const size_t normal_at = (nv * vb->position_stride + 15) & ~(size_t)15;
        const size_t bytes = normal_at + (vb->normals ? nv * vb->normal_stride : 0);
        const size_t position_bytes = nv ? (nv - 1) * vb->position_stride + 12 : 0;
        const size_t normal_bytes = vb->normals && nv ? (nv - 1) * vb->normal_stride + 12 : 0;
        if (bytes > lead.vertex_staging_bytes) {
            // (every earlier call has returned, so nothing is in flight on the buffer that goes)
            if (lead.d_vertex_staging) HIP_TRY(ctx, hipFree(lead.d_vertex_staging));
            lead.d_vertex_staging = nullptr;
            lead.vertex_staging_bytes = 0;
            if (int rc = lazy_device_buffer(ctx, lead.d_vertex_staging, bytes)) return rc;
            lead.vertex_staging_bytes = bytes;
        }
        // blocking copies: the source is pageable host memory
        const clock::time_point t_upload = clock::now();
        HIP_TRY(ctx, hipMemcpy(lead.d_vertex_staging, vb->positions, position_bytes, hipMemcpyHostToDevice));
        if (normal_bytes) HIP_TRY(ctx, hipMemcpy(lead.d_vertex_staging + normal_at, vb->normals, normal_bytes, hipMemcpyHostToDevice));
        upload_ms = ms_since(t_upload);
        d_positions = lead.d_vertex_staging;
        d_normals = vb->normals ? lead.d_vertex_staging + normal_at : nullptr;
    }
    if (!lead.d_update_tris) {
        void* p = nullptr;
        HIP_TRY(ctx, hipMalloc(&p, std::max<size_t>((size_t)n * sizeof(ptmi_triangle), 16)));
        lead.allocations.push_back(p);
        lead.d_update_tris = static_cast<ptmi_triangle*>(p);
    }
    // ---- the records: one kernel on the main stream.  The scratch is read by nothing that is in flight: every update is synchronous
    MeshTopologyPlanes planes;
    planes.n_triangles = n;
    planes.head = reinterpret_cast<const uint32_t*>(lead.d_mesh_topology);
    planes.uv = ctx->mesh_has_uv ? reinterpret_cast<const float*>(lead.d_mesh_topology + (size_t)n * 16) : nullptr;
    planes.tail = reinterpret_cast<const uint32_t*>(lead.d_mesh_topology + (size_t)n * (ctx->mesh_has_uv ? 64 : 16));
    // (timed with HIP events that are read once update_triangles has waited for the stream: no wait of its own)
    hipEvent_t begin = nullptr, end = nullptr;
    HIP_TRY(ctx, hipEventCreate(&begin));
    if (hipEventCreate(&end) != hipSuccess) {
        (void)hipEventDestroy(begin);
        return fail(ctx, PTMI_ERR_HIP, prefix + "hipEventCreate failed");
    }
    std::string err;
    int rc = hipEventRecord(begin, lead.stream) == hipSuccess ? (int)PTMI_OK : (int)PTMI_ERR_HIP;
    if (!rc) rc = launch_assemble_triangles(planes, d_positions, vb->position_stride, d_normals, vb->normal_stride, lead.d_update_tris, lead.stream, &err);
    if (!rc && hipEventRecord(end, lead.stream) != hipSuccess) rc = PTMI_ERR_HIP;
    if (rc) {
        (void)hipStreamSynchronize(lead.stream);  // (the caller's buffers are no longer read when the call returns)
        (void)hipEventDestroy(begin);
        (void)hipEventDestroy(end);
        return fail(ctx, rc, prefix + (err.empty() ? "hipEventRecord failed" : err));
    }
    // ---- screen, records, shading records, refit, the other devices: the update that exists, under this entry point's name.  Its
    // screen waits for the main stream before anything is decided, so the records are whole by then
    rc = update_triangles_on_device(ctx, who_is_calling, lead.d_update_tris, n, info);
    if (rc) (void)hipStreamSynchronize(lead.stream);  // (a refusal has waited already; an error may have come before the wait)
    float assemble_ms = 0;
    const hipError_t e = rc ? hipSuccess : hipEventElapsedTime(&assemble_ms, begin, end);
    (void)hipEventDestroy(begin);
    (void)hipEventDestroy(end);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, PTMI_ERR_HIP, prefix + hipGetErrorString(e));
    if (info) {
        info->upload_ms += upload_ms;
        info->device_ms += assemble_ms;
        info->total_ms = ms_since(t_call);
    }
    return PTMI_OK;
}

}  // namespace

extern "C" {

int ptmi_bind_mesh(ptmi_ctx* ctx, const ptmi_mesh_topology* topology)
{
    const std::string who = "ptmi_bind_mesh", prefix = who + ": ";
    if (int rc = need_scene(ctx, who)) return rc;
    DeviceState& lead = ctx->dev[0];
    if (!topology) {  // unbind
        ON_DEVICE(ctx, lead);
        if (lead.d_mesh_topology) HIP_TRY(ctx, hipFree(lead.d_mesh_topology));
        lead.d_mesh_topology = nullptr;
        ctx->have_mesh = false;
        return PTMI_OK;
    }
    if (topology->struct_size == sizeof(ptmi_mesh_topology) && topology->reserved == 0 && topology->n_triangles != ctx->update.triangulation_size)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + std::to_string(topology->n_triangles) + " triangles, the context holds " +
                                                    std::to_string(ctx->update.triangulation_size) + " (the topology is that of the uploaded array)");
    const std::string why = topology_refusal(topology);
    if (!why.empty()) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + why);
    // the planes of mesh_assemble.h, in one allocation: head | uv (where there are texture coordinates) | tail
    const size_t n = topology->n_triangles;
    const bool has_uv = topology->uvp != nullptr || topology->uvn != nullptr;  // (each has its own default: ptmi.h)
    const size_t uv_at = n * 16, tail_at = n * (has_uv ? 64 : 16), bytes = tail_at + n * 8;
    std::vector<uint32_t> host(std::max<size_t>(bytes, 16) / 4, 0u);
    uint32_t* const head = host.data();
    ptmi_float2* const uv = reinterpret_cast<ptmi_float2*>(host.data() + uv_at / 4);
    uint32_t* const tail = host.data() + tail_at / 4;
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) head[4 * i + k] = topology->indices[3 * i + k];
        head[4 * i + 3] = topology->mat_pos[i];
        tail[2 * i] = topology->mat_neg ? topology->mat_neg[i] : topology->mat_pos[i];
        tail[2 * i + 1] = topology->ids ? topology->ids[i] : (uint32_t)i;
        if (has_uv) {
            // plane p of triangle i: float2 slots 2i, 2i + 1 of the plane; the six pairs in the order uvp0 uvp1 uvp2 uvn0 uvn1 uvn2
            // uvp == NULL: zeros; uvn == NULL: uvp
            ptmi_float2 six[6] = {};
            for (int k = 0; k < 3; k++) {
                if (topology->uvp) six[k] = topology->uvp[3 * i + k];
                six[3 + k] = topology->uvn ? topology->uvn[3 * i + k] : six[k];
            }
            for (int s = 0; s < 6; s++) uv[(size_t)(s / 2) * 2 * n + 2 * i + (s & 1)] = six[s];
        }
    }
    ON_DEVICE(ctx, lead);
    char* fresh = nullptr;
    if (int rc = lazy_device_buffer(ctx, fresh, host.size() * 4)) return rc;
    const hipError_t e = hipMemcpy(fresh, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(fresh);
        return fail(ctx, PTMI_ERR_HIP, prefix + hipGetErrorString(e));
    }
    // a second bind replaces the first (no update is in flight: they are synchronous)
    if (lead.d_mesh_topology) (void)hipFree(lead.d_mesh_topology);
    lead.d_mesh_topology = fresh;
    ctx->have_mesh = true;
    ctx->mesh_vertices = topology->n_vertices;
    ctx->mesh_has_uv = has_uv;
    return PTMI_OK;
}

int ptmi_update_vertices(ptmi_ctx* ctx, const ptmi_vertex_buffers* host, ptmi_update_info* info)
{
    return update_vertices(ctx, "ptmi_update_vertices", false, host, info);
}

int ptmi_update_vertices_device(ptmi_ctx* ctx, const ptmi_vertex_buffers* device, ptmi_update_info* info)
{
    return update_vertices(ctx, "ptmi_update_vertices_device", true, device, info);
}

int ptmi_assemble_triangles(const ptmi_mesh_topology* topology, const ptmi_vertex_buffers* host, ptmi_triangle* out)
{
    const std::string prefix = "ptmi_assemble_triangles: ";
    std::string why = topology_refusal(topology);
    if (why.empty() && (!host || host->struct_size != sizeof(ptmi_vertex_buffers))) why = "vertex buffers are NULL or struct_size mismatch (ABI)";
    if (why.empty() && topology->n_triangles) why = buffers_refusal(host, topology->n_vertices, false);
    if (why.empty() && topology->n_triangles && !out) why = "out is NULL";
    if (!why.empty()) return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, prefix + why);
    for (uint32_t i = 0; i < topology->n_triangles; i++) {
        const size_t c = 3 * (size_t)i;
        ptmi_mesh::assemble_triangle(corner_of(*topology, *host, c), corner_of(*topology, *host, c + 1), corner_of(*topology, *host, c + 2),
                                     host->normals == nullptr, topology->mat_pos[i], topology->mat_neg ? topology->mat_neg[i] : topology->mat_pos[i],
                                     topology->ids ? topology->ids[i] : i, ptmi_mesh::RecordInMemory{out + i});
    }
    return PTMI_OK;
}

}  // extern "C"
