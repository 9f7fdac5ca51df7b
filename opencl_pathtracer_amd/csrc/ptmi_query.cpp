// ptmi_query.cpp - rays of the caller's own against the loaded scene (ray_query.hip): ptmi_query_rays / ptmi_query_rays_device.
// Owns, of ptmi_context.h: `query_buffers` (a RoundTrip; the hits come back through land()); reads the scene.
// Both entry points launch on devices[0]'s MAIN stream and touch nothing but the two ray buffers: the launch streams, the stage
// sets, the schedule and the counters are left alone, so whatever was rendered - or rendered ahead - stays what it was.  The
// calls that rewrite scene records wait for that stream first (quiesce, free_scene_memory; ptmi_set_stream waits for the
// stream it leaves), which covers a device-pointer query still in flight.
#include <algorithm>

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
    RoundTrip& q = ctx->query_buffers;  // room for at least 1024 rays, with as many hits behind them in the one device buffer
    const size_t room = std::max<size_t>(n_rays, 1024) * sizeof(ptmi_ray_hit);
    Landing landing[1] = {{hits, nullptr, bytes, 0}};
    if (int rc = q.reserve(ctx, 2 * room, room, needs_landing(ctx, landing))) return rc;
    char* const d_hits = q.d + q.cap;
    landing[0].from = d_hits;
    HIP_TRY(ctx, hipMemcpyAsync(q.d, rays, bytes, hipMemcpyHostToDevice, d.stream));
    std::string err;
    if (int rc = KERNELS_OF(ctx, launch_query_rays)(d.ds, kind == PTMI_QUERY_ANY, q.d, d_hits, n_rays, ctx->stack_levels, d.stream, &err))
        return fail(ctx, rc, err);
    return land(ctx, landing, d.stream, q.h);
}

}  // extern "C"
