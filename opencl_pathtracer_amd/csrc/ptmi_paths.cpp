// ptmi_paths.cpp - full paths from rays of the caller's own (path_query.hip): ptmi_trace_paths / ptmi_trace_paths_device.
// Owns, of ptmi_context.h: `path_buffers` (a RoundTrip; the sums come back through land()); reads the scene.
// As for the ray queries (ptmi_query.cpp), both entry points launch on devices[0]'s MAIN stream and touch nothing but the two
// buffers: the launch streams, the stage sets, the schedule and the counters are left alone, so whatever was rendered - or
// rendered ahead - stays what it was, and the calls that rewrite scene records wait for that stream first.
#include <algorithm>

#include "ptmi_context.h"

using namespace ptmi_internal;

static_assert(sizeof(ptmi_path_params) == 32, "ptmi_path_params");
static_assert(sizeof(ptmi_ray) == 48 && sizeof(ptmi_path_sum) == 48, "path_query.hip moves both as three 16-byte quads");

static int paths_check(ptmi_ctx* ctx, const char* who, const ptmi_path_params* p, const void* rays, uint32_t n_rays, const void* sums)
{
    if (int rc = need_scene(ctx, who)) return rc;
    const std::string name(who);
    if (!p) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, name + ": params is NULL");
    if (p->struct_size != sizeof(ptmi_path_params)) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, name + ": struct_size " + std::to_string(p->struct_size) + " is not sizeof(ptmi_path_params)");
    if (p->reserved[0] | p->reserved[1] | p->reserved[2]) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, name + ": a reserved word is not 0");
    if (p->n_iterations > PTMI_MAX_PATH_ITERATIONS)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, name + ": n_iterations " + std::to_string(p->n_iterations) + " exceeds " + std::to_string(PTMI_MAX_PATH_ITERATIONS) + " (chain calls and add the sums)");
    if (n_rays && p->n_iterations && (!rays || !sums)) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, name + ": rays or sums is NULL");
    return PTMI_OK;
}

static int launch(ptmi_ctx* ctx, DeviceState& d, const ptmi_path_params* p, const void* d_rays, uint32_t n_rays, void* d_sums)
{
    std::string err;
    if (int rc = KERNELS_OF(ctx, launch_trace_paths)(d.ds, d_rays, d_sums, n_rays, p->first_iteration, p->n_iterations, p->first_index,
                                                     p->index_stride, ctx->stack_levels, d.stream, &err))
        return fail(ctx, rc, err);
    return PTMI_OK;
}

extern "C" {

int ptmi_trace_paths_device(ptmi_ctx* ctx, const ptmi_path_params* params, const void* d_rays, uint32_t n_rays, void* d_sums)
{
    if (int rc = paths_check(ctx, "ptmi_trace_paths_device", params, d_rays, n_rays, d_sums)) return rc;
    if (n_rays == 0 || params->n_iterations == 0) return PTMI_OK;
    if (((uintptr_t)d_rays | (uintptr_t)d_sums) & 15u)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_trace_paths_device: the device pointers must be 16-byte aligned");
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    return launch(ctx, d, params, d_rays, n_rays, d_sums);
}

int ptmi_trace_paths(ptmi_ctx* ctx, const ptmi_path_params* params, const ptmi_ray* rays, uint32_t n_rays, ptmi_path_sum* sums)
{
    if (int rc = paths_check(ctx, "ptmi_trace_paths", params, rays, n_rays, sums)) return rc;
    if (n_rays == 0 || params->n_iterations == 0) return PTMI_OK;
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    const size_t bytes = (size_t)n_rays * sizeof(ptmi_ray);
    RoundTrip& q = ctx->path_buffers;  // room for at least 1024 rays, with as many sums behind them in the one device buffer
    const size_t room = std::max<size_t>(n_rays, 1024) * sizeof(ptmi_path_sum);
    Landing landing[1] = {{sums, nullptr, bytes, 0}};
    if (int rc = q.reserve(ctx, 2 * room, room, needs_landing(ctx, landing))) return rc;
    char* const d_sums = q.d + q.cap;
    landing[0].from = d_sums;
    HIP_TRY(ctx, hipMemcpyAsync(q.d, rays, bytes, hipMemcpyHostToDevice, d.stream));
    if (int rc = launch(ctx, d, params, q.d, n_rays, d_sums)) return rc;
    return land(ctx, landing, d.stream, q.h);
}

}  // extern "C"
