// ptmi_denoise.cpp - the filter between the accumulators and the display (denoise.hip): ptmi_denoise / ptmi_denoise_device.
// Owns, of ptmi_context.h: `d_denoise_features`, `denoise_buffers` and `denoise_ordered`; reads the scene (the host form renders its
// guides with the guide launch) and the accumulators.  Like the guide calls (ptmi_guides.cpp) both entry points work on
// devices[0] and write nothing but their own scratch and the caller's result: the launch streams, the stage sets, the schedule,
// the counters and the caller's snapshot slots are left alone.
#include <cmath>

#include "ptmi_context.h"

using namespace ptmi_internal;

namespace {

constexpr uint32_t kKnownFlags = PTMI_DENOISE_DEMODULATE_ALBEDO | PTMI_DENOISE_UNTILED;
constexpr size_t kFeatureBytesPerPixel = 56;  // denoise.hip: e, e, g1 (float4 each), g2 (float2)

bool good_sigma(float s) { return std::isfinite(s) && s > 0; }

// what both entry points ask of the context and of the struct
int denoise_check(ptmi_ctx* ctx, const char* who, const ptmi_denoise_params* p)
{
    if (int rc = need_scene(ctx, who)) return rc;
    const std::string w = std::string(who) + ": ";
    if (!p) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the ptmi_denoise_params struct is NULL");
    if (p->struct_size != sizeof(ptmi_denoise_params))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT,
                    w + "ptmi_denoise_params.struct_size is " + std::to_string(p->struct_size) + ", not " + std::to_string(sizeof(ptmi_denoise_params)));
    if (p->passes > 5) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + std::to_string(p->passes) + " passes: at most 5 (steps 1 to 16)");
    if (p->flags & ~kKnownFlags) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "unknown flag bits");
    if (p->reserved[0] || p->reserved[1]) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the reserved words must be 0");
    if (p->guide_iterations == 0 || p->guide_iterations >= (1u << 24))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "guide_iterations must be at least 1 and below 2^24");
    if (!good_sigma(p->sigma_color) || !good_sigma(p->sigma_normal) || !good_sigma(p->sigma_position))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "every sigma must be finite and greater than 0");
    return PTMI_OK;
}

// the job of one call, but for its pointers: the reciprocals are the host's float operations of the contract
DenoiseJob job_of(const ptmi_ctx* ctx, const ptmi_denoise_params& p)
{
    DenoiseJob job{};
    job.width = ctx->cfg.image_width;
    job.height = ctx->cfg.image_height;
    job.passes = p.passes;
    job.demodulate = (p.flags & PTMI_DENOISE_DEMODULATE_ALBEDO) != 0;
    job.tiled = (p.flags & PTMI_DENOISE_UNTILED) == 0;
    job.guide_iterations = (float)p.guide_iterations;
    const float cc = p.sigma_color * p.sigma_color, nn = p.sigma_normal * p.sigma_normal, pp = p.sigma_position * p.sigma_position;
    for (int k = 0; k < 5; k++) job.inv_c[k] = (float)(1 << (2 * k)) / cc;
    job.inv_n = 1.f / nn;
    job.inv_p = 1.f / pp;
    return job;
}

int launch(ptmi_ctx* ctx, DenoiseJob& job, hipStream_t stream)
{
    if (int rc = lazy_device_buffer(ctx, ctx->d_denoise_features, ctx->npix() * kFeatureBytesPerPixel)) return rc;
    job.features = ctx->d_denoise_features;
    std::string err;
    if (int rc = launch_denoise(job, stream, &err)) return fail(ctx, rc, err);
    return PTMI_OK;
}

}  // namespace

extern "C" {

int ptmi_denoise_device(ptmi_ctx* ctx, const ptmi_denoise_params* params, const ptmi_guides* device_guides, const void* d_image_color,
                        const void* d_image_ray_nb, void* d_image_out)
{
    const char* who = "ptmi_denoise_device";
    if (int rc = denoise_check(ctx, who, params)) return rc;
    if (!device_guides || device_guides->struct_size != sizeof(ptmi_guides))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": the ptmi_guides struct is NULL or its struct_size is wrong");
    const void* planes[] = {device_guides->albedo, device_guides->normal, device_guides->position, device_guides->hit_count, d_image_out};
    for (const void* p : planes)
        if (!p) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": albedo, normal, position, hit_count and the result are all needed");
    if (!d_image_color != !d_image_ray_nb)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": give both image planes, or neither for the context's accumulators");
    for (const void* p : {planes[0], planes[1], planes[2], planes[3], planes[4], d_image_color, d_image_ray_nb})
        if ((uintptr_t)p & 15u) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": the device pointers must be 16-byte aligned");
    if (!d_image_color && ctx->n_dev() != 1)
        return fail(ctx, PTMI_ERR_UNSUPPORTED, std::string(who) + ": a multi-device context has partial sums per device; pass the image planes");
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    DenoiseJob job = job_of(ctx, *params);
    job.color = d_image_color ? static_cast<const float*>(d_image_color) : d.ds.image_color;
    job.ray_nb = d_image_ray_nb ? static_cast<const float*>(d_image_ray_nb) : d.ds.image_ray_nb;
    job.albedo = device_guides->albedo;
    job.normal = device_guides->normal;
    job.position = device_guides->position;
    job.hit_count = device_guides->hit_count;
    job.out = static_cast<float*>(d_image_out);
    return launch(ctx, job, d.stream);
}

int ptmi_denoise(ptmi_ctx* ctx, const ptmi_denoise_params* params, float* image_out)
{
    const char* who = "ptmi_denoise";
    if (int rc = denoise_check(ctx, who, params)) return rc;
    if (!image_out) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": image_out is NULL");
    if (ctx->cfg.sampler == PTMI_SAMPLER_RANDOM)
        return fail(ctx, PTMI_ERR_UNSUPPORTED, std::string(who) + ": the RANDOM sampler's samples land on other pixels than the work-item's (no guides)");
    DeviceState& d = ctx->dev[0];
    const size_t plane = ctx->color_bytes();

    // the image ptmi_read_image would return, and the stream it is ordered on (as ptmi_read_display finds them)
    const float *color = d.ds.image_color, *count = d.ds.image_ray_nb;
    hipStream_t stream = d.stream;
    if (ctx->n_dev() > 1) {
        if (int rc = snapshot_all(ctx, kInternalSlot)) return rc;
        const float* image = nullptr;
        if (int rc = gather_snapshot(ctx, kInternalSlot, &image)) return rc;
        color = image; count = image + 4 * ctx->npix();
        stream = d.copy_stream;
    }
    ON_DEVICE(ctx, d);
    if (stream != d.stream) {  // the scratch may still serve a device-form call on the main stream
        if (int rc = lazy_event(ctx, ctx->denoise_ordered)) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->denoise_ordered, d.stream));
        HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->denoise_ordered, 0));
    }

    // the result, which lands, then albedo | normal | position | hit_count
    const Landing landing[1] = {{image_out, nullptr, plane, 0}};
    RoundTrip& b = ctx->denoise_buffers;
    if (int rc = b.reserve(ctx, 4 * plane + ctx->count_bytes(), plane, needs_landing(ctx, landing))) return rc;
    float* planes[5];
    for (int i = 0; i < 5; i++) planes[i] = reinterpret_cast<float*>(b.d + i * plane);
    std::string err;
    if (int rc = KERNELS_OF(ctx, launch_guides)(d.ds, DGuides{planes[1], planes[2], planes[3], planes[4], nullptr}, params->guide_first_iteration,
                                                params->guide_iterations, ctx->stack_levels, stream, &err))
        return fail(ctx, rc, err);

    DenoiseJob job = job_of(ctx, *params);
    job.color = color;
    job.ray_nb = count;
    job.albedo = planes[1];
    job.normal = planes[2];
    job.position = planes[3];
    job.hit_count = planes[4];
    job.out = planes[0];
    if (int rc = launch(ctx, job, stream)) return rc;
    const Landing items[1] = {{image_out, planes[0], plane, 0}};
    return land(ctx, items, stream, b.h);
}

}  // extern "C"
