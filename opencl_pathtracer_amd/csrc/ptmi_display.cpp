// ptmi_display.cpp - the stage behind the denoiser (display.hip): ptmi_display_table, ptmi_read_display_tonemapped /
// ptmi_display_device and ptmi_luminance_histogram / ptmi_luminance_histogram_device.
// Owns, of ptmi_context.h: `d_luminance`; shares `d_display` with ptmi_read_display (ptmi_readback.cpp), which grows it the same
// way.  Like the denoise calls all four work on devices[0] and write nothing but their own scratch and the caller's result.  The
// device forms need no scratch at all, so the host forms - which wait for their stream before they return, as ptmi_read_display
// does - are the only users of both buffers and need no event between the copy stream and the main stream.
#include <cmath>

#include "ptmi_context.h"

using namespace ptmi_internal;

namespace {

// what the display calls ask of the context and of the struct
int display_check(ptmi_ctx* ctx, const char* who, const ptmi_display_params* p)
{
    if (int rc = need_scene(ctx, who)) return rc;
    const std::string w = std::string(who) + ": ";
    if (!p) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the ptmi_display_params struct is NULL");
    if (p->struct_size != sizeof(ptmi_display_params))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT,
                    w + "ptmi_display_params.struct_size is " + std::to_string(p->struct_size) + ", not " + std::to_string(sizeof(ptmi_display_params)));
    if (p->flags) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "unknown flag bits (none is defined)");
    for (uint32_t r : p->reserved)
        if (r) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the reserved words must be 0");
    if (p->tone > PTMI_TONE_FILMIC) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "unknown tone operator " + std::to_string(p->tone));
    if (p->transfer > PTMI_TRANSFER_GAMMA22) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "unknown transfer function " + std::to_string(p->transfer));
    if (p->format > PTMI_PIXELS_RGBA32) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "unknown pixel format " + std::to_string(p->format));
    const uint64_t width = ctx->cfg.image_width, stride = p->row_stride;
    if (p->format == PTMI_PIXELS_RGBA32 ? stride != 4 * width : (stride < 3 * width || stride > 3 * width + 3))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "row_stride must be 3*W plus 0..3 padding bytes for BGR24, 4*W for RGBA32");
    if (!(std::isfinite(p->exposure) && p->exposure > 0)) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "exposure must be finite and greater than 0");
    if (p->tone == PTMI_TONE_REINHARD && !(p->white > 0))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "white must be greater than 0 (+infinity: plain x / (1 + x))");
    return PTMI_OK;
}

// the planes of a device form: both, the colour alone (means), or neither (the context's accumulators)
int device_planes(ptmi_ctx* ctx, const char* who, const void* d_color, const void* d_count, const void* d_out, const float** color, const float** count)
{
    const std::string w = std::string(who) + ": ";
    if (!d_out) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the result is NULL");
    if (d_count && !d_color) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "a count plane without a sum plane");
    for (const void* p : {d_color, d_count, d_out})
        if ((uintptr_t)p & 15u) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, w + "the device pointers must be 16-byte aligned");
    if (!d_color && ctx->n_dev() != 1)
        return fail(ctx, PTMI_ERR_UNSUPPORTED, w + "a multi-device context has partial sums per device; pass the image planes");
    const DeviceState& d = ctx->dev[0];
    *color = d_color ? static_cast<const float*>(d_color) : d.ds.image_color;
    *count = d_color ? static_cast<const float*>(d_count) : d.ds.image_ray_nb;
    return PTMI_OK;
}

// the image ptmi_read_image would return, and the stream it is ordered on (as ptmi_read_display finds them)
int host_image(ptmi_ctx* ctx, const float** color, const float** count, hipStream_t* stream)
{
    DeviceState& d = ctx->dev[0];
    *color = d.ds.image_color;
    *count = d.ds.image_ray_nb;
    *stream = d.stream;
    if (ctx->n_dev() > 1) {
        if (int rc = snapshot_all(ctx, kInternalSlot)) return rc;
        const float* image = nullptr;
        if (int rc = gather_snapshot(ctx, kInternalSlot, &image)) return rc;
        *color = image;
        *count = image + 4 * ctx->npix();
        *stream = d.copy_stream;
    }
    ON_DEVICE(ctx, d);
    return PTMI_OK;
}

DisplayJob job_of(const ptmi_ctx* ctx, const ptmi_display_params& p)
{
    DisplayJob job{};
    job.width = ctx->cfg.image_width;
    job.height = ctx->cfg.image_height;
    job.row_stride = p.row_stride;
    job.tone = p.tone;
    job.transfer = p.transfer;
    job.format = p.format;
    job.exposure = p.exposure;
    job.w2 = p.white * p.white;  // the host's float operation of the contract
    return job;
}

}  // namespace

extern "C" {

int ptmi_display_table(uint32_t transfer, float table[256])
{
    if (transfer > PTMI_TRANSFER_GAMMA22) return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, "ptmi_display_table: unknown transfer function " + std::to_string(transfer));
    if (!table) return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, "ptmi_display_table: table is NULL");
    std::memcpy(table, display_table(transfer), 256 * sizeof(float));
    return PTMI_OK;
}

int ptmi_display_device(ptmi_ctx* ctx, const ptmi_display_params* params, const void* d_color, const void* d_count, void* d_pixels)
{
    const char* who = "ptmi_display_device";
    if (int rc = display_check(ctx, who, params)) return rc;
    DisplayJob job = job_of(ctx, *params);
    if (int rc = device_planes(ctx, who, d_color, d_count, d_pixels, &job.color, &job.ray_nb)) return rc;
    job.out = static_cast<uint8_t*>(d_pixels);
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    std::string err;
    if (int rc = launch_display_tonemapped(job, d.stream, &err)) return fail(ctx, rc, err);
    return PTMI_OK;
}

int ptmi_read_display_tonemapped(ptmi_ctx* ctx, const ptmi_display_params* params, uint8_t* pixels)
{
    const char* who = "ptmi_read_display_tonemapped";
    if (int rc = display_check(ctx, who, params)) return rc;
    if (!pixels) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": pixels is NULL");
    DisplayJob job = job_of(ctx, *params);
    hipStream_t stream = nullptr;
    if (int rc = host_image(ctx, &job.color, &job.ray_nb, &stream)) return rc;
    const size_t bytes = (size_t)job.height * job.row_stride;
    if (bytes > ctx->display_bytes) {  // (every earlier user of the buffer has waited for its stream)
        if (ctx->d_display) (void)hipFree(ctx->d_display);
        ctx->d_display = nullptr;
        ctx->display_bytes = 0;
        if (int rc = lazy_device_buffer(ctx, ctx->d_display, bytes)) return rc;
        ctx->display_bytes = bytes;
    }
    job.out = ctx->d_display;
    std::string err;
    if (int rc = launch_display_tonemapped(job, stream, &err)) return fail(ctx, rc, err);
    // ptmi_read_display's copy: one DMA straight into `pixels` where the caller has page-locked it (what land() would do with it);
    // into pageable memory the runtime's own staged copy, which measures faster than a landing buffer and a memcpy behind it
    // (0.14 ms against 0.40 ms for the 6.2 MB of 1080p)
    HIP_TRY(ctx, hipMemcpyAsync(pixels, ctx->d_display, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return PTMI_OK;
}

int ptmi_luminance_histogram_device(ptmi_ctx* ctx, const void* d_color, const void* d_count, void* d_histogram)
{
    const char* who = "ptmi_luminance_histogram_device";
    if (int rc = need_scene(ctx, who)) return rc;
    const float *color = nullptr, *count = nullptr;
    if (int rc = device_planes(ctx, who, d_color, d_count, d_histogram, &color, &count)) return rc;
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    std::string err;
    if (int rc = launch_luminance_histogram(color, count, static_cast<uint32_t*>(d_histogram), ctx->npix(), d.stream, &err)) return fail(ctx, rc, err);
    return PTMI_OK;
}

int ptmi_luminance_histogram(ptmi_ctx* ctx, uint32_t histogram[PTMI_LUMINANCE_WORDS])
{
    const char* who = "ptmi_luminance_histogram";
    if (int rc = need_scene(ctx, who)) return rc;
    if (!histogram) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": histogram is NULL");
    const float *color = nullptr, *count = nullptr;
    hipStream_t stream = nullptr;
    if (int rc = host_image(ctx, &color, &count, &stream)) return rc;
    const size_t bytes = PTMI_LUMINANCE_WORDS * sizeof(uint32_t);
    if (int rc = lazy_device_buffer(ctx, ctx->d_luminance, bytes)) return rc;
    std::string err;
    if (int rc = launch_luminance_histogram(color, count, ctx->d_luminance, ctx->npix(), stream, &err)) return fail(ctx, rc, err);
    HIP_TRY(ctx, hipMemcpyAsync(histogram, ctx->d_luminance, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return PTMI_OK;
}

}  // extern "C"
