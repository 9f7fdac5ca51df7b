// ptmi_readback.cpp - images out of the devices: the HIP side of the snapshot ring (snapshot_ring.h keeps its books), the sum of
// the devices' shares on devices[0] - RCCL, loaded at run time, or peer copies and a sum kernel - and the copies to the host.
// Owns, of ptmi_context.h: the snapshot buffers with their events, d_peer_copy, d_reduced and d_display per scene (allocated
// here on first use, freed by free_scene_memory); peer_copied, h_staging and the RCCL communicators per context.
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <mutex>

#include "ptmi_context.h"

using namespace ptmi_internal;

// Queue, behind everything device `d` has been given so far, a copy of its accumulators for ring slot `slot`: into the buffer
// the slot shows if no other slot shows it too, else into one that no slot shows.  *buffer = where it went.
int ptmi_internal::snapshot_device(ptmi_ctx* ctx, DeviceState& d, uint32_t slot, int* buffer)
{
    ON_DEVICE(ctx, d);
    const int b = d.ring.buffer_for(slot);
    if (b < 0) return fail(ctx, PTMI_ERR_STATE, "snapshot ring: no free buffer");  // (cannot happen: as many buffers as slots)
    if (int rc = lazy_device_buffer(ctx, d.d_snapshot[b], ctx->image_bytes())) return rc;
    if (int rc = lazy_event(ctx, d.snapshot_ready[b])) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d.d_snapshot[b], d.ds.image_color, ctx->color_bytes(), hipMemcpyDeviceToDevice, d.stream));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_snapshot[b] + 4 * ctx->npix(), d.ds.image_ray_nb, ctx->count_bytes(), hipMemcpyDeviceToDevice, d.stream));
    HIP_TRY(ctx, hipEventRecord(d.snapshot_ready[b], d.stream));
    d.ring.written(slot, b);
    if (buffer) *buffer = b;
    return PTMI_OK;
}
int ptmi_internal::snapshot_all(ptmi_ctx* ctx, uint32_t slot)
{
    for (DeviceState& d : ctx->dev)
        if (int rc = snapshot_device(ctx, d, slot)) return rc;
    return PTMI_OK;
}

namespace {

// Device float[4*npix] / float[npix] -> the caller's buffers over devices[0]'s `stream`, then wait for that stream.
int copy_out(ptmi_ctx* ctx, hipStream_t stream, const float* d_color, const float* d_count, float* image_color, float* image_ray_nb)
{
    const Landing items[2] = {{image_color, d_color, ctx->color_bytes(), 0}, {image_ray_nb, d_count, ctx->count_bytes(), ctx->color_bytes()}};
    if (needs_landing(ctx, items))
        if (int rc = lazy_pinned_buffer(ctx, ctx->h_staging, ctx->image_bytes())) return rc;
    return land(ctx, items, stream, reinterpret_cast<char*>(ctx->h_staging));
}

// The same for rectangle `r` of the two planes (ptmi_read_region): ONE strided copy per plane, device pitch = the image's row,
// host rows densely packed - 20 bytes per pixel of the rectangle cross the bus.  Straight into a destination the caller has
// page-locked, otherwise through the context's staging buffer (which holds a whole image: any rectangle fits).
int copy_out_region(ptmi_ctx* ctx, hipStream_t stream, const float* d_color, const float* d_count, const Region& r, float* image_color,
                    float* image_ray_nb)
{
    const size_t W = ctx->cfg.image_width, n = (size_t)r.w * r.h, first = (size_t)r.y * W + r.x;
    struct Plane { void* to; const char* from; size_t texel, offset; };
    const Plane planes[2] = {{image_color, reinterpret_cast<const char*>(d_color) + first * 16, 16, 0},
                             {image_ray_nb, reinterpret_cast<const char*>(d_count) + first * 4, 4, n * 16}};
    bool direct[2];
    for (int k = 0; k < 2; k++) direct[k] = !planes[k].to || ctx->host_is_pinned(planes[k].to, n * planes[k].texel);
    if (!(direct[0] && direct[1]))
        if (int rc = lazy_pinned_buffer(ctx, ctx->h_staging, ctx->image_bytes())) return rc;
    char* const landing = reinterpret_cast<char*>(ctx->h_staging);
    for (int k = 0; k < 2; k++) {
        const Plane& p = planes[k];
        if (p.to)
            HIP_TRY(ctx, hipMemcpy2DAsync(direct[k] ? p.to : landing + p.offset, r.w * p.texel, p.from, W * p.texel, r.w * p.texel, r.h,
                                          hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    for (int k = 0; k < 2; k++)
        if (!direct[k]) std::memcpy(planes[k].to, landing + planes[k].offset, n * planes[k].texel);
    return PTMI_OK;
}

// ---- RCCL, loaded at run time (the library has no link-time dependency on it) --------------------------------------------
// north_star: "samples-per-pixel shard across the GPUs of one node with an RCCL reduce of the framebuffer over xGMI".  One
// process drives all devices of a context, so the communicators come from ncclCommInitAll and the G reduce calls of an image
// are one group.  OPT-IN (PTMI_REDUCE=rccl) until the collective has run on a node with two GPUs: the default sum is peer copies
// + sum_images_kernel, whose order of additions is the device order ptmi.h documents; RCCL's order for more than two devices is
// its algorithm's, so the image's last bits depend on the choice.  PTMI_REDUCE=rccl-always sends even a one-device context
// through a one-rank communicator (how the tests exercise this code on a one-GPU box).  Any failure - library absent or of
// another major version, initialisation refused, a run-time error of ncclReduce / ncclGroupEnd - falls back to the peer path for
// the rest of the context's life (ptmi_rccl_state tells which path a context uses).
struct RcclApi {
    void* lib = nullptr;
    int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
    int (*CommDestroy)(void* comm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Reduce)(const void* send, void* recv, size_t count, int datatype, int op, int root, void* comm, hipStream_t stream) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int* version) = nullptr;
    int version = 0;
    bool ok = false;
};
RcclApi& rccl_api()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.lib) break;
        }
        if (!api.lib) return;
        auto sym = [&](const char* n) { return dlsym(api.lib, n); };
        api.CommInitAll = reinterpret_cast<decltype(api.CommInitAll)>(sym("ncclCommInitAll"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
        api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
        api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
        api.Reduce = reinterpret_cast<decltype(api.Reduce)>(sym("ncclReduce"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
        api.GetVersion = reinterpret_cast<decltype(api.GetVersion)>(sym("ncclGetVersion"));
        // the enum values below are those of the NCCL 2 API (rccl.h of ROCm 7.2 reports 2.2x): another major version is refused
        if (api.GetVersion && api.GetVersion(&api.version) != 0) api.version = 0;
        const int major = api.version >= 10000 ? api.version / 10000 : api.version / 1000;
        api.ok = api.CommInitAll && api.CommDestroy && api.GroupStart && api.GroupEnd && api.Reduce && major == 2;
    });
    return api;
}
constexpr int kNcclFloat32 = 7, kNcclSum = 0;  // rccl.h: ncclDataType_t / ncclRedOp_t

// devices[0]'s ctx->d_reduced = sum over the devices of their share of the image of ring slot `slot`, by ONE ncclReduce per
// device (root = devices[0]), each on its device's copy stream behind that device's snapshot.  PTMI_ERR_UNSUPPORTED = this
// context cannot use RCCL (library absent, a device listed twice, initialisation refused): the caller falls back to peer copies.
int rccl_reduce_snapshots(ptmi_ctx* ctx, uint32_t slot)
{
    if (ctx->rccl_state < 0) return PTMI_ERR_UNSUPPORTED;
    RcclApi& api = rccl_api();
    const int G = (int)ctx->n_dev();
    if (ctx->rccl_state == 0) {
        ctx->rccl_state = -1;
        if (!api.ok) return PTMI_ERR_UNSUPPORTED;
        std::vector<int> devs;
        for (DeviceState& d : ctx->dev) {
            for (int o : devs)
                if (o == d.device) return PTMI_ERR_UNSUPPORTED;  // RCCL wants distinct devices
            devs.push_back(d.device);
        }
        ctx->rccl_comms.assign((size_t)G, nullptr);
        if (api.CommInitAll(ctx->rccl_comms.data(), G, devs.data()) != 0) {
            ctx->rccl_comms.clear();
            (void)hipGetLastError();
            return PTMI_ERR_UNSUPPORTED;
        }
        ctx->rccl_state = 1;
    }
    const size_t count = ctx->npix() * 5;
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        HIP_TRY(ctx, hipStreamWaitEvent(d.copy_stream, d.snapshot_ready[d.ring.shown(slot)], 0));
    }
    int rc = api.GroupStart();
    for (int k = 0; k < G && rc == 0; k++) {
        DeviceState& d = ctx->dev[(size_t)k];
        ON_DEVICE(ctx, d);
        float* send = d.d_snapshot[d.ring.shown(slot)];
        rc = api.Reduce(send, k == 0 ? (void*)ctx->d_reduced : (void*)send, count, kNcclFloat32, kNcclSum, 0, ctx->rccl_comms[(size_t)k], d.copy_stream);
    }
    const int rc_end = api.GroupEnd();
    if (rc == 0) rc = rc_end;
    ON_DEVICE(ctx, ctx->dev[0]);
    if (rc != 0) {
        // a run-time refusal: remember why, never try again in this context, and let the caller sum through peer copies
        ctx->err = std::string("ncclReduce: ") + (api.GetErrorString ? api.GetErrorString(rc) : "error") + " (falling back to peer copies)";
        (void)hipGetLastError();
        ctx->rccl_state = -1;
        return PTMI_ERR_UNSUPPORTED;
    }
    return PTMI_OK;
}

}  // namespace

// The image of ring slot `slot` on devices[0], ordered on dev[0].copy_stream: the slot itself for one device; for several,
// every other device's snapshot copied over (each on its own stream, so the transfers use their own xGMI links at the same
// time) and the sum of all of them, in device order, in ctx->d_reduced.  (ptmi_denoise.cpp gathers through it too.)
int ptmi_internal::gather_snapshot(ptmi_ctx* ctx, uint32_t slot, const float** image)
{
    DeviceState& lead = ctx->dev[0];
    const size_t npix = ctx->npix();
    for (DeviceState& d : ctx->dev)
        if (d.ring.shown(slot) < 0 || !d.snapshot_ready[d.ring.shown(slot)] || !d.d_snapshot[d.ring.shown(slot)])
            return fail(ctx, PTMI_ERR_STATE, "ptmi_read_snapshot of a slot no ptmi_snapshot has filled");
    ON_DEVICE(ctx, lead);
    const int lead_src = lead.ring.shown(slot);
    HIP_TRY(ctx, hipStreamWaitEvent(lead.copy_stream, lead.snapshot_ready[lead_src], 0));
    const int reduce = ptmi_switches::read_switches(ptmi_switches::Moment::kReadback).reduce;
    if (ctx->n_dev() == 1 && reduce != ptmi_switches::kReduceRcclAlways) {
        *image = lead.d_snapshot[lead_src];
        return PTMI_OK;
    }
    if (int rc = lazy_device_buffer(ctx, ctx->d_reduced, ctx->image_bytes())) return rc;
    // Which path: peer copies + the sum kernel in device order, unless the caller opted into the collective (PTMI_REDUCE=rccl /
    // rccl-always, above).  The images of a progressive per-image loop (ptmi_render_snapshots: ONE device's share is new per
    // image) are cheaper through the incremental peer copies anyway, which move 1 / (G - 1) of what a reduce would.
    const bool collective = reduce != 0;
    if (int rc = collective ? rccl_reduce_snapshots(ctx, slot) : (int)PTMI_ERR_UNSUPPORTED) {
        if (rc != PTMI_ERR_UNSUPPORTED) return rc;
        if (ctx->n_dev() == 1) {  // (rccl-always on a box without the library)
            *image = lead.d_snapshot[lead_src];
            return PTMI_OK;
        }
    } else {
        *image = ctx->d_reduced;
        return PTMI_OK;
    }
    // peer copies + one sum kernel (also the path of a context that lists one device several times, which RCCL refuses)
    const float* parts[PTMI_MAX_DEVICES];
    parts[0] = lead.d_snapshot[lead_src];
    // the previous sum must have read the landing buffers before they are overwritten: the peers' copies wait for the lead's
    // copy stream as it stands now
    hipEvent_t& gate = lead.peer_copied;
    if (int rc = lazy_event(ctx, gate)) return rc;
    HIP_TRY(ctx, hipEventRecord(gate, lead.copy_stream));
    for (uint32_t k = 1; k < ctx->n_dev(); k++) {  // on devices[0] (the lead device is current)
        if (int rc = lazy_device_buffer(ctx, ctx->dev[k].d_peer_copy, ctx->image_bytes())) return rc;
        parts[k] = ctx->dev[k].d_peer_copy;
    }
    for (uint32_t k = 1; k < ctx->n_dev(); k++) {  // each peer pushes its snapshot over its own link, on a stream and with an event of its own device
        DeviceState& d = ctx->dev[k];
        const int src = d.ring.shown(slot);
        // ... unless the landing buffer already holds that very snapshot: consecutive images of a G-device render differ in
        // ONE device's share, so an image costs one 41.5 MB peer copy, not G - 1
        if (d.ring.landed(slot)) continue;
        ON_DEVICE(ctx, d);
        if (int rc = lazy_event(ctx, d.peer_copied)) return rc;
        HIP_TRY(ctx, hipStreamWaitEvent(d.copy_stream, gate, 0));
        HIP_TRY(ctx, hipStreamWaitEvent(d.copy_stream, d.snapshot_ready[src], 0));
        HIP_TRY(ctx, hipMemcpyPeerAsync(d.d_peer_copy, lead.device, d.d_snapshot[src], d.device, ctx->image_bytes(), d.copy_stream));
        HIP_TRY(ctx, hipEventRecord(d.peer_copied, d.copy_stream));
        d.ring.land(slot);
    }
    ON_DEVICE(ctx, lead);
    for (uint32_t k = 1; k < ctx->n_dev(); k++)
        if (ctx->dev[k].peer_copied) HIP_TRY(ctx, hipStreamWaitEvent(lead.copy_stream, ctx->dev[k].peer_copied, 0));
    std::string err;
    if (int rc = launch_sum_images(ctx->d_reduced, parts, ctx->n_dev(), npix * 5, lead.copy_stream, &err)) return fail(ctx, rc, err);
    *image = ctx->d_reduced;
    return PTMI_OK;
}

void ptmi_internal::destroy_rccl_communicators(ptmi_ctx* ctx)
{
    for (void* comm : ctx->rccl_comms)
        if (comm) (void)rccl_api().CommDestroy(comm);
    ctx->rccl_comms.clear();
}

extern "C" {

int ptmi_reduce_path(const ptmi_ctx* ctx, int* rccl_state, int* n_communicators, int* nccl_version)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (rccl_state) *rccl_state = ctx->rccl_state;
    if (n_communicators) {
        int n = 0;
        for (void* c : ctx->rccl_comms) n += c != nullptr;
        *n_communicators = n;
    }
    if (nccl_version) *nccl_version = ctx->rccl_state != 0 ? rccl_api().version : 0;  // (never loads the library by itself)
    return PTMI_OK;
}

int ptmi_snapshot(ptmi_ctx* ctx, uint32_t slot)
{
    NEED_SCENE(ctx);
    if (slot >= kUserSlots) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "snapshot slot out of range");
    return snapshot_all(ctx, slot);
}

int ptmi_read_snapshot(ptmi_ctx* ctx, uint32_t slot, float* image_color, float* image_ray_nb)
{
    NEED_SCENE(ctx);
    if (slot >= kRingSlots) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "snapshot slot out of range");
    if (!image_color && !image_ray_nb) {  // wait only: the snapshot has been taken on every device (clFinish of that image)
        for (DeviceState& d : ctx->dev) {
            const int src = d.ring.shown(slot);
            if (src < 0 || !d.snapshot_ready[src]) return fail(ctx, PTMI_ERR_STATE, "ptmi_read_snapshot of a slot no ptmi_snapshot has filled");
            ON_DEVICE(ctx, d);
            HIP_TRY(ctx, hipEventSynchronize(d.snapshot_ready[src]));
        }
        return PTMI_OK;
    }
    const float* image = nullptr;
    if (int rc = gather_snapshot(ctx, slot, &image)) return rc;
    return copy_out(ctx, ctx->dev[0].copy_stream, image, image + 4 * ctx->npix(), image_color, image_ray_nb);
}

int ptmi_read_image(ptmi_ctx* ctx, float* image_color, float* image_ray_nb)
{
    NEED_SCENE(ctx);
    if (ctx->n_dev() == 1) {  // straight from the accumulators, in order on the render stream
        DeviceState& d = ctx->dev[0];
        ON_DEVICE(ctx, d);
        return copy_out(ctx, d.stream, d.ds.image_color, d.ds.image_ray_nb, image_color, image_ray_nb);
    }
    if (int rc = snapshot_all(ctx, kInternalSlot)) return rc;
    return ptmi_read_snapshot(ctx, kInternalSlot, image_color, image_ray_nb);
}

int ptmi_read_region(ptmi_ctx* ctx, const ptmi_region* region, float* image_color, float* image_ray_nb)
{
    NEED_SCENE(ctx);
    if (!region) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_read_region: region is NULL");
    const Region r{region->x, region->y, region->width, region->height};
    std::string why;
    if (!check_region(ctx->cfg.image_width, ctx->cfg.image_height, r, &why)) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_read_region: " + why);
    // an empty rectangle copies nothing but waits like any other: "the region of what ptmi_read_image would return at this moment"
    const bool nothing = region_is_empty(r);
    float* const color = nothing ? nullptr : image_color;
    float* const count = nothing ? nullptr : image_ray_nb;
    if (ctx->n_dev() == 1) {  // straight from the accumulators, in order on the render stream
        DeviceState& d = ctx->dev[0];
        ON_DEVICE(ctx, d);
        return copy_out_region(ctx, d.stream, d.ds.image_color, d.ds.image_ray_nb, r, color, count);
    }
    // several devices: their shares are summed first, as for ptmi_read_image (whole images: the sum is not cut to the rectangle)
    if (int rc = snapshot_all(ctx, kInternalSlot)) return rc;
    const float* image = nullptr;
    if (int rc = gather_snapshot(ctx, kInternalSlot, &image)) return rc;
    ON_DEVICE(ctx, ctx->dev[0]);
    return copy_out_region(ctx, ctx->dev[0].copy_stream, image, image + 4 * ctx->npix(), r, color, count);
}

int ptmi_read_display(ptmi_ctx* ctx, uint8_t* bgr, uint32_t row_stride)
{
    if (!bgr) return PTMI_ERR_INVALID_ARGUMENT;
    NEED_SCENE(ctx);
    const uint32_t w = ctx->cfg.image_width, h = ctx->cfg.image_height;
    if (row_stride < 3u * w || row_stride > 3u * w + 3u)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "row_stride must be 3*W plus 0..3 padding bytes");
    DeviceState& d = ctx->dev[0];
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
    const size_t bytes = (size_t)h * row_stride;
    if (bytes > ctx->display_bytes) {
        if (ctx->d_display) (void)hipFree(ctx->d_display);
        ctx->d_display = nullptr;
        ctx->display_bytes = 0;
        if (int rc = lazy_device_buffer(ctx, ctx->d_display, bytes)) return rc;
        ctx->display_bytes = bytes;
    }
    std::string err;
    if (int rc = launch_display_bgr(color, count, ctx->d_display, w, h, row_stride, stream, &err)) return fail(ctx, rc, err);
    HIP_TRY(ctx, hipMemcpyAsync(bgr, ctx->d_display, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return PTMI_OK;
}

}  // extern "C"
