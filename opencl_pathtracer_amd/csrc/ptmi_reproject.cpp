// ptmi_reproject.cpp - the image carried across a camera move (reproject.hip): ptmi_reproject_device / ptmi_set_camera_reprojected.
// Owns, of ptmi_context.h: `d_reproject_scratch` and `reproject_gathered`.  The device form is a guide-style call: devices[0],
// the main stream, nothing of the context written.  The host form is ptmi_set_camera (camera_check / camera_write of
// ptmi_scene_memory.cpp) with guide launches, the reprojection and an image write around it: it writes the camera and the
// accumulators, and nothing else.
#include <cmath>

#include "ptmi_context.h"

using namespace ptmi_internal;

namespace {

// The host form's scratch: five float4 planes (normal and position of the previous and of the new camera, the result's sums),
// then three float planes (the two hit counts, the result's counts), each rounded up to 16 bytes so that every plane starts
// 16-byte aligned whatever the pixel count - 92 bytes per pixel and at most 45 more.
constexpr size_t kFloat4Planes = 5, kFloatPlanes = 3;
size_t float_plane_bytes(size_t npix) { return (npix * 4 + 15) & ~(size_t)15; }
size_t scratch_bytes(size_t npix) { return kFloat4Planes * npix * 16 + kFloatPlanes * float_plane_bytes(npix); }

bool good_tolerance(float s) { return std::isfinite(s) && s > 0; }

// what both entry points ask of the context and of the struct
int reproject_check(ptmi_ctx* ctx, const char* who, const ptmi_reproject_params* p, bool host_form)
{
    if (int rc = need_scene(ctx, who)) return rc;
    const std::string w = std::string(who) + ": ";
    if (!p) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the ptmi_reproject_params struct is NULL");
    if (p->struct_size != sizeof(ptmi_reproject_params))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "ptmi_reproject_params.struct_size is " + std::to_string(p->struct_size) + ", not " +
                                                        std::to_string(sizeof(ptmi_reproject_params)));
    if (p->flags) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "unknown flag bits (none is defined)");
    if (p->reserved) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the reserved word must be 0");
    if (!good_tolerance(p->position_tolerance) || !good_tolerance(p->normal_tolerance))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "both tolerances must be finite and greater than 0");
    if (!(p->max_history >= 1)) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "max_history must be at least 1 (+infinity: no cap)");
    if (host_form && (p->guide_iterations == 0 || p->guide_iterations >= (1u << 24)))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "guide_iterations must be at least 1 and below 2^24");
    return PTMI_OK;
}

// The host's part of the contract: the rows that invert the previous camera, in double, each rounded to float once; the squared
// tolerances in float.  Refuses a camera that is not finite or has no inverse.
int job_of(ptmi_ctx* ctx, const char* who, const ptmi_reproject_params& p, const float* cam_pos, const float* cam_dir, const float* cam_right,
           const float* cam_up, ReprojectJob& job)
{
    for (const float* v : {cam_pos, cam_dir, cam_right, cam_up})
        for (int i = 0; i < 3; i++)
            if (!std::isfinite(v[i])) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": the previous camera is not finite");
    const auto cross = [](const double* a, const double* b, double* out) {
        out[0] = a[1] * b[2] - a[2] * b[1];
        out[1] = a[2] * b[0] - a[0] * b[2];
        out[2] = a[0] * b[1] - a[1] * b[0];
    };
    const double dir[3] = {cam_dir[0], cam_dir[1], cam_dir[2]}, right[3] = {cam_right[0], cam_right[1], cam_right[2]},
                 up[3] = {cam_up[0], cam_up[1], cam_up[2]};
    double c[3], c1[3], c2[3];
    cross(right, up, c);
    cross(up, dir, c1);
    cross(dir, right, c2);
    const double det = (dir[0] * c[0] + dir[1] * c[1]) + dir[2] * c[2];
    if (!std::isfinite(det) || det == 0)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": the previous camera's direction, right and up span no volume (det is 0 or not finite)");
    job = ReprojectJob{};
    job.width = ctx->cfg.image_width;
    job.height = ctx->cfg.image_height;
    for (int i = 0; i < 3; i++) {
        job.cam[i] = cam_pos[i];
        job.r0[i] = (float)(c[i] / det);
        job.r1[i] = (float)(c1[i] / det);
        job.r2[i] = (float)(c2[i] / det);
    }
    job.tp = p.position_tolerance * p.position_tolerance;
    job.tn = p.normal_tolerance * p.normal_tolerance;
    job.max_history = p.max_history;
    return PTMI_OK;
}

}  // namespace

extern "C" {

int ptmi_reproject_device(ptmi_ctx* ctx, const ptmi_reproject_params* params, const ptmi_float4 previous_camera[4],
                          const ptmi_guides* previous_guides, const void* d_previous_color, const void* d_previous_ray_nb,
                          const ptmi_guides* current_guides, void* d_out_color, void* d_out_ray_nb)
{
    const char* who = "ptmi_reproject_device";
    if (int rc = reproject_check(ctx, who, params, false)) return rc;
    if (!previous_camera) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": previous_camera is NULL");
    for (const ptmi_guides* g : {previous_guides, current_guides})
        if (!g || g->struct_size != sizeof(ptmi_guides))
            return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": a ptmi_guides struct is NULL or its struct_size is wrong");
    const void* planes[] = {previous_guides->normal, previous_guides->position, previous_guides->hit_count, d_previous_color, d_previous_ray_nb,
                            current_guides->normal,  current_guides->position,  current_guides->hit_count,  d_out_color,      d_out_ray_nb};
    for (const void* p : planes) {
        if (!p)
            return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": normal, position and hit_count of both guides, the previous image's "
                                                        "two planes and the result's two are all needed");
        if ((uintptr_t)p & 15u) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": the device pointers must be 16-byte aligned");
    }
    ReprojectJob job;
    if (int rc = job_of(ctx, who, *params, &previous_camera[0].x, &previous_camera[1].x, &previous_camera[2].x, &previous_camera[3].x, job)) return rc;
    job.prev_normal = previous_guides->normal;
    job.prev_position = previous_guides->position;
    job.prev_hit_count = previous_guides->hit_count;
    job.prev_color = static_cast<const float*>(d_previous_color);
    job.prev_ray_nb = static_cast<const float*>(d_previous_ray_nb);
    job.cur_normal = current_guides->normal;
    job.cur_position = current_guides->position;
    job.cur_hit_count = current_guides->hit_count;
    job.out_color = static_cast<float*>(d_out_color);
    job.out_ray_nb = static_cast<float*>(d_out_ray_nb);
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    std::string err;
    if (int rc = launch_reproject(job, d.stream, &err)) return fail(ctx, rc, err);
    return PTMI_OK;
}

int ptmi_set_camera_reprojected(ptmi_ctx* ctx, const ptmi_float4* position, const ptmi_float4* direction, const ptmi_float4* right,
                                const ptmi_float4* up, const ptmi_reproject_params* params)
{
    const char* who = "ptmi_set_camera_reprojected";
    // ---- everything that can refuse, before the first write to the camera or the accumulators
    if (int rc = reproject_check(ctx, who, params, true)) return rc;
    if (int rc = camera_check(ctx, who, position, direction, right, up)) return rc;
    if (ctx->cfg.sampler == PTMI_SAMPLER_RANDOM)
        return fail(ctx, PTMI_ERR_UNSUPPORTED, std::string(who) + ": the RANDOM sampler's samples land on other pixels than the work-item's (no guides)");
    if (ctx->cfg.super_sampling)
        return fail(ctx, PTMI_ERR_UNSUPPORTED, std::string(who) + ": a super_sampling context's variance accumulator and per-pixel stop decisions "
                                               "cannot be carried over");
    DeviceState& d = ctx->dev[0];
    ReprojectJob job;  // (the previous camera is the one the context holds: d.ds is rewritten below)
    if (int rc = job_of(ctx, who, *params, d.ds.cam_pos, d.ds.cam_dir, d.ds.cam_right, d.ds.cam_up, job)) return rc;
    ON_DEVICE(ctx, d);
    const size_t npix = ctx->npix(), plane = ctx->color_bytes();
    if (int rc = lazy_device_buffer(ctx, ctx->d_reproject_scratch, scratch_bytes(npix))) return rc;
    // [set][normal, position, hit_count]: set 0 of the previous camera, set 1 of the new one
    char* const counts = ctx->d_reproject_scratch + kFloat4Planes * plane;
    float* set[2][3];
    for (int s = 0; s < 2; s++) {
        set[s][0] = reinterpret_cast<float*>(ctx->d_reproject_scratch + (2 * s) * plane);
        set[s][1] = reinterpret_cast<float*>(ctx->d_reproject_scratch + (2 * s + 1) * plane);
        set[s][2] = reinterpret_cast<float*>(counts + s * float_plane_bytes(npix));
    }
    float* const out_color = reinterpret_cast<float*>(ctx->d_reproject_scratch + 4 * plane);
    float* const out_count = reinterpret_cast<float*>(counts + 2 * float_plane_bytes(npix));

    // the image ptmi_read_image would return; several devices: their sum, which the main stream then waits for
    const float *color = d.ds.image_color, *count = d.ds.image_ray_nb;
    if (ctx->n_dev() > 1) {
        if (int rc = snapshot_all(ctx, kInternalSlot)) return rc;
        const float* image = nullptr;
        if (int rc = gather_snapshot(ctx, kInternalSlot, &image)) return rc;
        color = image; count = image + 4 * npix;
        ON_DEVICE(ctx, d);
        if (int rc = lazy_event(ctx, ctx->reproject_gathered)) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->reproject_gathered, d.copy_stream));
        HIP_TRY(ctx, hipStreamWaitEvent(d.stream, ctx->reproject_gathered, 0));
    }
    std::string err;
    const auto guides = [&](float* const* planes) {
        return KERNELS_OF(ctx, launch_guides)(d.ds, DGuides{nullptr, planes[0], planes[1], planes[2], nullptr}, params->guide_first_iteration,
                                              params->guide_iterations, ctx->stack_levels, d.stream, &err);
    };
    if (int rc = guides(set[0])) return fail(ctx, rc, err);

    // ---- the camera (waits for the main stream of every device: the guides above and the gathered image are complete)
    if (int rc = camera_write(ctx, *position, *direction, *right, *up)) return rc;

    ON_DEVICE(ctx, d);
    if (int rc = guides(set[1])) return fail(ctx, rc, err);
    job.prev_normal = set[0][0];
    job.prev_position = set[0][1];
    job.prev_hit_count = set[0][2];
    job.prev_color = color;
    job.prev_ray_nb = count;
    job.cur_normal = set[1][0];
    job.cur_position = set[1][1];
    job.cur_hit_count = set[1][2];
    job.out_color = out_color;
    job.out_ray_nb = out_count;
    if (int rc = launch_reproject(job, d.stream, &err)) return fail(ctx, rc, err);

    // ---- the image, as ptmi_write_image stores one: devices[0] gets it, the other devices' partial sums restart from zero
    HIP_TRY(ctx, hipMemcpyAsync(d.ds.image_color, out_color, plane, hipMemcpyDeviceToDevice, d.stream));
    HIP_TRY(ctx, hipMemcpyAsync(d.ds.image_ray_nb, out_count, ctx->count_bytes(), hipMemcpyDeviceToDevice, d.stream));
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    for (uint32_t k = 1; k < ctx->n_dev(); k++) {
        DeviceState& o = ctx->dev[k];
        ON_DEVICE(ctx, o);
        HIP_TRY(ctx, hipMemsetAsync(o.ds.image_color, 0, plane, o.stream));
        HIP_TRY(ctx, hipMemsetAsync(o.ds.image_ray_nb, 0, ctx->count_bytes(), o.stream));
        HIP_TRY(ctx, hipStreamSynchronize(o.stream));
    }
    ON_DEVICE(ctx, d);
    return PTMI_OK;
}

}  // extern "C"
