// ptmi_query.cpp - rays of the caller's own against the loaded scene (ray_query.hip): ptmi_query_rays / ptmi_query_rays_device.
// Owns, of ptmi_context.h: the per-context query buffers d_query / h_query / query_cap (freed by ptmi_release); reads the scene.
// Both entry points launch on devices[0]'s MAIN stream and touch nothing but the two ray buffers: the launch streams, the stage
// sets, the schedule and the counters are left alone, so whatever was rendered - or rendered ahead - stays what it was.  The
// calls that rewrite scene records wait for that stream first (quiesce, free_scene_memory; ptmi_set_stream waits for the
// stream it leaves), which covers a device-pointer query still in flight.
#include <algorithm>
#include <cstring>

#include "ptmi_context.h"

using namespace ptmi_internal;

static int query_check(ptmi_ctx* ctx, const char* who, uint32_t kind, const void* rays, uint32_t n_rays, const void* hits)
{
    if (int rc = need_scene(ctx, who)) return rc;
    if (kind != PTMI_QUERY_CLOSEST && kind != PTMI_QUERY_ANY) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown kind " + std::to_string(kind));
    if (n_rays && (!rays || !hits)) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": rays or hits is NULL");
    return PTMI_OK;
}

extern "C" {

int ptmi_query_rays_device(ptmi_ctx* ctx, uint32_t kind, const void* d_rays, uint32_t n_rays, void* d_hits)
{
    if (int rc = query_check(ctx, "ptmi_query_rays_device", kind, d_rays, n_rays, d_hits)) return rc;
    if (n_rays == 0) return PTMI_OK;
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_query_rays_device: the device pointers must be 16-byte aligned");
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    std::string err;
    if (int rc = KERNELS_OF(ctx, launch_query_rays)(d.ds, kind == PTMI_QUERY_ANY, d_rays, d_hits, n_rays, ctx->stack_levels, d.stream, &err))
        return fail(ctx, rc, err);
    return PTMI_OK;
}

int ptmi_query_rays(ptmi_ctx* ctx, uint32_t kind, const ptmi_ray* rays, uint32_t n_rays, ptmi_ray_hit* hits)
{
    if (int rc = query_check(ctx, "ptmi_query_rays", kind, rays, n_rays, hits)) return rc;
    if (n_rays == 0) return PTMI_OK;
    static_assert(sizeof(ptmi_ray) == 48 && sizeof(ptmi_ray_hit) == 48, "ray_query.hip moves both as three 16-byte quads");
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    const size_t bytes = (size_t)n_rays * sizeof(ptmi_ray);
    const bool pinned = ctx->host_is_pinned(hits, bytes);
    if (n_rays > ctx->query_cap) {
        // (every earlier host-array query has returned, so nothing is in flight on the buffers that go)
        if (ctx->d_query) (void)hipFree(ctx->d_query);
        if (ctx->h_query) (void)hipHostFree(ctx->h_query);
        ctx->d_query = ctx->h_query = nullptr;
        ctx->query_cap = 0;
        const size_t cap = std::max<size_t>(n_rays, 1024);
        if (int rc = lazy_device_buffer(ctx, ctx->d_query, 2 * cap * sizeof(ptmi_ray))) return rc;
        ctx->query_cap = cap;
    }
    if (!pinned)
        if (int rc = lazy_pinned_buffer(ctx, ctx->h_query, ctx->query_cap * sizeof(ptmi_ray_hit))) return rc;
    char* const d_rays = ctx->d_query;
    char* const d_hits = ctx->d_query + ctx->query_cap * sizeof(ptmi_ray);
    HIP_TRY(ctx, hipMemcpyAsync(d_rays, rays, bytes, hipMemcpyHostToDevice, d.stream));
    std::string err;
    if (int rc = KERNELS_OF(ctx, launch_query_rays)(d.ds, kind == PTMI_QUERY_ANY, d_rays, d_hits, n_rays, ctx->stack_levels, d.stream, &err))
        return fail(ctx, rc, err);
    HIP_TRY(ctx, hipMemcpyAsync(pinned ? (void*)hits : (void*)ctx->h_query, d_hits, bytes, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    if (!pinned) std::memcpy(hits, ctx->h_query, bytes);
    return PTMI_OK;
}

}  // extern "C"
