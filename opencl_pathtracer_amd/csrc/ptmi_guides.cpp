// ptmi_guides.cpp - first-hit guide buffers of the loaded scene (guide_buffers.hip): ptmi_render_guides / ptmi_render_guides_device.
// Owns, of ptmi_context.h: `guide_buffers` (a RoundTrip; the planes come back through land()); reads the scene.  Like the ray
// queries (ptmi_query.cpp), both entry points launch on devices[0]'s MAIN stream and touch nothing but the planes: the launch
// streams, the stage sets, the schedule and the counters are left alone, so whatever was rendered - or rendered ahead - stays
// what it was, and the calls that rewrite scene records wait for that stream first.
#include "ptmi_context.h"

using namespace ptmi_internal;

namespace {

constexpr int kPlanes = 5;

// the five planes of a ptmi_guides in the struct's order, and the bytes each takes per pixel
struct Planes {
    void* p[kPlanes];
    bool any() const { return p[0] || p[1] || p[2] || p[3] || p[4]; }
};
constexpr size_t kBytesPerPixel[kPlanes] = {16, 16, 16, 4, 16};

Planes planes_of(const ptmi_guides& g) { return Planes{{g.albedo, g.normal, g.position, g.hit_count, g.ids}}; }

DGuides device_guides(const Planes& q)
{
    return DGuides{static_cast<float*>(q.p[0]), static_cast<float*>(q.p[1]), static_cast<float*>(q.p[2]), static_cast<float*>(q.p[3]),
                   static_cast<uint32_t*>(q.p[4])};
}

int guides_check(ptmi_ctx* ctx, const char* who, const ptmi_guides* planes)
{
    if (int rc = need_scene(ctx, who)) return rc;
    if (!planes) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": the ptmi_guides struct is NULL");
    if (planes->struct_size != sizeof(ptmi_guides))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": ptmi_guides.struct_size is " + std::to_string(planes->struct_size) +
                                                        ", not " + std::to_string(sizeof(ptmi_guides)));
    if (ctx->cfg.sampler == PTMI_SAMPLER_RANDOM)
        return fail(ctx, PTMI_ERR_UNSUPPORTED, std::string(who) + ": the RANDOM sampler's samples land on other pixels than the work-item's");
    return PTMI_OK;
}

int launch(ptmi_ctx* ctx, DeviceState& d, const Planes& device_planes, uint32_t first_iteration, uint32_t n_iterations)
{
    std::string err;
    if (int rc = KERNELS_OF(ctx, launch_guides)(d.ds, device_guides(device_planes), first_iteration, n_iterations, ctx->stack_levels,
                                                d.stream, &err))
        return fail(ctx, rc, err);
    return PTMI_OK;
}

}  // namespace

extern "C" {

int ptmi_render_guides_device(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations, const ptmi_guides* device_planes)
{
    if (int rc = guides_check(ctx, "ptmi_render_guides_device", device_planes)) return rc;
    const Planes q = planes_of(*device_planes);
    for (void* p : q.p)
        if ((uintptr_t)p & 15u) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_render_guides_device: the device planes must be 16-byte aligned");
    if (n_iterations == 0 || !q.any()) return PTMI_OK;
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    return launch(ctx, d, q, first_iteration, n_iterations);
}

int ptmi_render_guides(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations, const ptmi_guides* host_planes)
{
    if (int rc = guides_check(ctx, "ptmi_render_guides", host_planes)) return rc;
    const Planes host = planes_of(*host_planes);
    if (n_iterations == 0 || !host.any()) return PTMI_OK;
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);

    // the planes asked for, one behind the other in the scratch (each starts on a 16-byte boundary): exactly their bytes
    Landing landing[kPlanes] = {};
    size_t total = 0;
    for (int i = 0; i < kPlanes; i++) {
        if (!host.p[i]) continue;
        landing[i] = Landing{host.p[i], nullptr, ctx->npix() * kBytesPerPixel[i], total};
        total += (landing[i].bytes + 15u) & ~(size_t)15u;
    }
    RoundTrip& g = ctx->guide_buffers;
    if (int rc = g.reserve(ctx, total, total, needs_landing(ctx, landing))) return rc;

    Planes dev{};
    for (int i = 0; i < kPlanes; i++)
        if (host.p[i]) landing[i].from = dev.p[i] = g.d + landing[i].offset;
    if (int rc = launch(ctx, d, dev, first_iteration, n_iterations)) return rc;
    return land(ctx, landing, d.stream, g.h);
}

}  // extern "C"
