// ptmi_api.cpp - host side of libptmi.so: the C ABI of include/ptmi.h.  This unit: a context's life cycle (setup, release,
// errors) and the small accessors; the rest of the ABI lies in ptmi_scene_memory.cpp (upload and in-place update),
// ptmi_render.cpp (the launches), ptmi_readback.cpp (snapshots and images), ptmi_query.cpp (ray queries) and ptmi_guides.cpp (first-hit guide buffers).
// Owns, of ptmi_context.h: the per-context state - creates the context with its main and copy streams and destroys everything
// the other units have added to it.
//
// Mirrors the life cycle of the reference backend (Controleur/PathTracer_OpenCL.cpp):
// setup_context -> initialize_memory -> render/read ... -> release, with the
// differences DESIGN.md lists (accumulators are zeroed; a launch covers a range
// of iterations; the scene is validated and re-laid out before upload).
// No CPU fallback exists: without a HIP device nothing here computes.
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "kernel_choice.h"
#include "ptmi_context.h"

using namespace ptmi_internal;

namespace {
std::mutex g_err_mutex;
std::string g_err;  // failures that have no context yet
}  // namespace

void ptmi_internal::set_global_error(const std::string& msg)
{
    std::lock_guard<std::mutex> lock(g_err_mutex);
    g_err = msg;
}

extern "C" {

int ptmi_abi_version(void) { return PTMI_ABI_VERSION; }

int ptmi_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* ptmi_last_error(const ptmi_ctx* ctx)
{
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> lock(g_err_mutex);
    static thread_local std::string copy;
    copy = g_err;
    return copy.c_str();
}

int ptmi_setup_context(ptmi_ctx** out, const ptmi_config* cfg)
{
    if (!out) return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, "ctx out-pointer is NULL");
    *out = nullptr;
    if (!cfg || cfg->struct_size != sizeof(ptmi_config))
        return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, "config is NULL or struct_size mismatch (ABI)");
    if (cfg->image_width == 0 || cfg->image_height == 0 || (uint64_t)cfg->image_width * cfg->image_height > 0x3FFFFFFFull)
        return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, "image size must be in [1, 2^30) pixels");
    if (cfg->sampler > PTMI_SAMPLER_UNIFORM) return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, "unknown sampler");
    if (cfg->lights_size >= PTMI_MAX_LIGHT_SIZE)  // PathTracer.cpp:60-65
        return fail(nullptr, PTMI_ERR_LIMIT, "lights_size >= 30");
    if (cfg->n_devices > PTMI_MAX_DEVICES) return fail(nullptr, PTMI_ERR_INVALID_ARGUMENT, "n_devices > PTMI_MAX_DEVICES");
    if (cfg->super_sampling && (cfg->flags & PTMI_FLAG_MEGAKERNEL))
        return fail(nullptr, PTMI_ERR_UNSUPPORTED, "SUPER_SAMPLING needs the wavefront kernel");

    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(nullptr, PTMI_ERR_NO_DEVICE, "no HIP device available (there is no CPU fallback)");
    std::vector<int> ordinals;
    if (cfg->n_devices <= 1) ordinals.push_back(cfg->n_devices == 1 ? cfg->devices[0] : cfg->device);
    else ordinals.assign(cfg->devices, cfg->devices + cfg->n_devices);
    for (int o : ordinals)
        if (o < 0 || o >= n) return fail(nullptr, PTMI_ERR_NO_DEVICE, "device ordinal out of range");

    ptmi_ctx* ctx = new ptmi_ctx();
    ctx->cfg = *cfg;
    ctx->dev.resize(ordinals.size());
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < ordinals.size() && e == hipSuccess; k++) {
        DeviceState& d = ctx->dev[k];
        d.device = ordinals[k];
        e = hipSetDevice(d.device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.own_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.copy_stream, hipStreamNonBlocking);
        d.stream = d.own_stream;
        if (e == hipSuccess && k > 0 && d.device != ordinals[0]) {
            // direct peer copies over xGMI where the platform allows them (hipMemcpyPeerAsync stages through the host otherwise)
            (void)hipDeviceEnablePeerAccess(ordinals[0], 0);
            (void)hipGetLastError();
        }
    }
    if (e != hipSuccess) {
        const std::string msg = std::string("device/stream setup: ") + hipGetErrorString(e);
        ptmi_release(ctx);
        return fail(nullptr, PTMI_ERR_HIP, msg);
    }
    const ptmi_switches::Switches setup = ptmi_switches::read_switches(ptmi_switches::Moment::kSetup);
    // iterations per launch: at most 16, fewer for very large images (32-bit job ids, staging array <= 4 GiB)
    {
        const uint64_t tiles = (uint64_t)((cfg->image_width + 7u) / 8u) * ((cfg->image_height + 7u) / 8u);
        const uint64_t by_jobs = (cfg->sampler == PTMI_SAMPLER_RANDOM ? 0x7FFFFFF0ull : 0xFFFFFFF0ull) / (tiles * 64u);  // (kernel_wavefront.hip: kGivenUp)
        const uint64_t by_bytes = (4ull << 30) / ((uint64_t)cfg->image_width * cfg->image_height * 20u);
        uint64_t cap = kMaxIterationsPerLaunch;
        if (by_jobs < cap) cap = by_jobs;
        if (by_bytes < cap) cap = by_bytes;
        ctx->iterations_per_launch = cap < 1 ? 1u : (uint32_t)cap;
        // PTMI_ITERATIONS_PER_LAUNCH: a lower cap, so that small images take the launch plans of very large ones (1..32; never higher)
        const int want = setup.iterations_per_launch;
        if (want >= 1 && want <= 32 && (uint32_t)want < ctx->iterations_per_launch) ctx->iterations_per_launch = (uint32_t)want;
    }
    // PTMI_LEAF_CULL - 0: the wavefront kernel fetches and tests the triangles of every leaf it reaches (leaf_cull.h);
    // 1: it culls the leaves a node step chooses itself, 2: also the ones it would push - both in every scene whose records
    // carry the bits, also where choose_upload would not expect it to pay; 3: as 2, but only the leaves of the certificate's tight tier
    ctx->leaf_cull = ptmi_choice::leaf_cull_setting(setup);
    *out = ctx;
    return PTMI_OK;
}

int ptmi_set_stream(ptmi_ctx* ctx, void* hip_stream)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (ctx->n_dev() != 1) return fail(ctx, PTMI_ERR_UNSUPPORTED, "ptmi_set_stream on a multi-device context");
    DeviceState& d = ctx->dev[0];
    ON_DEVICE(ctx, d);
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    if (int rc = fold_events(ctx, d)) return rc;
    d.stream = hip_stream ? (hipStream_t)hip_stream : d.own_stream;
    return PTMI_OK;
}

const char* ptmi_literal_kernel_reason(const ptmi_ctx* ctx)
{
    return ctx && ctx->have_scene && !ctx->literal_kernel_reason.empty() ? ctx->literal_kernel_reason.c_str() : nullptr;
}

int ptmi_synchronize(ptmi_ctx* ctx)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    }
    return PTMI_OK;
}

int ptmi_pin_host_buffer(ptmi_ctx* ctx, void* buffer, size_t bytes)
{
    if (!ctx || !buffer || bytes == 0) return PTMI_ERR_INVALID_ARGUMENT;
    if (ctx->host_is_pinned(buffer, bytes)) return PTMI_OK;
    if (ctx->dev.empty()) return PTMI_ERR_STATE;
    ON_DEVICE(ctx, ctx->dev[0]);
    const hipError_t e = hipHostRegister(buffer, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // not sticky: readbacks into this buffer simply keep using the staging path
        return fail(ctx, PTMI_ERR_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e));
    }
    ctx->pinned_host.push_back({(char*)buffer, bytes});
    return PTMI_OK;
}

int ptmi_unpin_host_buffer(ptmi_ctx* ctx, void* buffer)
{
    if (!ctx || !buffer) return PTMI_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < ctx->pinned_host.size(); i++) {
        if (ctx->pinned_host[i].p != (char*)buffer) continue;
        for (DeviceState& d : ctx->dev) {  // no copy into it may be in flight
            ON_DEVICE(ctx, d);
            HIP_TRY(ctx, hipStreamSynchronize(d.stream));
            if (d.copy_stream) HIP_TRY(ctx, hipStreamSynchronize(d.copy_stream));
        }
        (void)hipHostUnregister(buffer);
        (void)hipGetLastError();
        ctx->pinned_host.erase(ctx->pinned_host.begin() + (long)i);
        return PTMI_OK;
    }
    return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_unpin_host_buffer: not a buffer ptmi_pin_host_buffer has page-locked");
}

int ptmi_read_statistics(ptmi_ctx* ctx, uint32_t* depths, uint32_t* bbx, uint32_t* tri)
{
    NEED_SCENE(ctx);
    const uint32_t nd = ctx->cfg.ray_max_depth + 1;
    const size_t words = ctx->hist_words();
    std::vector<uint32_t> sum(words, 0u), part(words);
    for (DeviceState& d : ctx->dev) {  // histograms are integer sums over the devices
        ON_DEVICE(ctx, d);
        HIP_TRY(ctx, hipMemcpyAsync(part.data(), d.d_hist, words * 4, hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
        for (size_t i = 0; i < words; i++) sum[i] += part[i];
    }
    if (depths) std::memcpy(depths, sum.data(), nd * 4);
    if (bbx) std::memcpy(bbx, sum.data() + nd, PTMI_MAX_INTERSECTION_NUMBER * 4);
    if (tri) std::memcpy(tri, sum.data() + nd + PTMI_MAX_INTERSECTION_NUMBER, PTMI_MAX_INTERSECTION_NUMBER * 4);
    return PTMI_OK;
}

// The head of the three counter getters: the counters of the uploaded scene, summed over the devices.
static int read_counter_block(ptmi_ctx* ctx, const char* entry_point, const void* out, unsigned long long (&total)[C_COUNT])
{
    if (!out) return PTMI_ERR_INVALID_ARGUMENT;
    if (int rc = need_scene(ctx, entry_point)) return rc;
    for (int i = 0; i < C_COUNT; i++) total[i] = 0;
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        unsigned long long h[C_COUNT];
        HIP_TRY(ctx, hipMemcpyAsync(h, d.d_counters, sizeof h, hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
        for (int i = 0; i < C_COUNT; i++) total[i] += h[i];
    }
    return PTMI_OK;
}

int ptmi_get_counters(ptmi_ctx* ctx, ptmi_counters* out)
{
    unsigned long long h[C_COUNT];
    if (int rc = read_counter_block(ctx, __func__, out, h)) return rc;
    out->paths = h[C_PATHS]; out->segments = h[C_SEGMENTS]; out->surface_hits = h[C_HITS];
    out->shadow_rays = h[C_SHADOW]; out->box_tests = h[C_BBX]; out->triangle_tests = h[C_TRI];
    return PTMI_OK;
}

int ptmi_get_scheduler_stats(ptmi_ctx* ctx, ptmi_scheduler_stats* out)
{
    unsigned long long h[C_COUNT];
    if (int rc = read_counter_block(ctx, __func__, out, h)) return rc;
    out->trips_node = h[C_TRIPS_I]; out->lanes_node = h[C_LANES_I];
    out->trips_triangle = h[C_TRIPS_T]; out->lanes_triangle = h[C_LANES_T];
    out->trips_path = h[C_TRIPS_P]; out->lanes_path = h[C_LANES_P];
    out->cycles_path = h[C_CYCLES_P]; out->cycles_loop = h[C_CYCLES_LOOP];
    out->leaf_item_violations = h[C_ITEM_VIOLATIONS];
    out->paths_retraced = h[C_RETRACED];
    out->textured_hits = h[C_TEXTURED_HITS];
    uint32_t lanes = 0, resident = 0;
    KERNELS_OF(ctx, last_wavefront_grid)(ctx->dev[0].device, &lanes, &resident);
    out->workgroup_lanes = lanes;
    out->resident_workgroups = resident;
    return PTMI_OK;
}

int ptmi_get_invariant_checks(ptmi_ctx* ctx, ptmi_invariant_checks* out)
{
    unsigned long long h[C_COUNT];
    if (int rc = read_counter_block(ctx, __func__, out, h)) return rc;
    out->sample_out_of_range = h[C_CHK_SAMPLE]; out->normal_not_facing_ray = h[C_CHK_NORMALS];
    out->negative_direct_radiance = h[C_CHK_RADIANCE]; out->scattered_below_surface = h[C_CHK_HEMISPHERE];
    out->statistics_out_of_range = h[C_CHK_STATS_RANGE];
    out->refraction_undefined_in_reference = h[C_UNDEF_REFRACTION];
    return PTMI_OK;
}

int ptmi_kernel_time(ptmi_ctx* ctx, double* total_ms, uint32_t* n_launches)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    double ms = 0;
    uint32_t n = 0;
    for (DeviceState& d : ctx->dev) {  // summed over the devices: total / launches stays the average launch duration
        if (int rc = fold_events(ctx, d)) return rc;
        ms += d.kernel_ms;
        n += d.kernel_launches;
        d.kernel_ms = 0;
        d.kernel_launches = 0;
    }
    if (total_ms) *total_ms = ms;
    if (n_launches) *n_launches = n;
    return PTMI_OK;
}

int ptmi_device_accumulators(ptmi_ctx* ctx, void** d_color, void** d_count)
{
    NEED_SCENE(ctx);
    if (ctx->n_dev() != 1) return fail(ctx, PTMI_ERR_UNSUPPORTED, "ptmi_device_accumulators on a multi-device context (partial sums)");
    if (d_color) *d_color = ctx->dev[0].ds.image_color;
    if (d_count) *d_count = ctx->dev[0].ds.image_ray_nb;
    return PTMI_OK;
}

int ptmi_device_variance(ptmi_ctx* ctx, void** d_image_v)
{
    if (!d_image_v) return PTMI_ERR_INVALID_ARGUMENT;
    NEED_SCENE(ctx);
    if (ctx->n_dev() != 1) return fail(ctx, PTMI_ERR_UNSUPPORTED, "ptmi_device_variance on a multi-device context (per-device moments)");
    if (!ctx->dev[0].ds.image_v) return fail(ctx, PTMI_ERR_STATE, "no variance accumulator: the context was set up without super_sampling");
    *d_image_v = ctx->dev[0].ds.image_v;
    return PTMI_OK;
}

void ptmi_release(ptmi_ctx* ctx)
{
    if (!ctx) return;
    free_scene_memory(ctx);
    if (!ctx->dev.empty()) (void)hipSetDevice(ctx->dev[0].device);
    ctx->query_buffers.release();
    ctx->path_buffers.release();
    ctx->guide_buffers.release();
    ctx->denoise_buffers.release();
    if (ctx->d_denoise_features) (void)hipFree(ctx->d_denoise_features);
    if (ctx->denoise_ordered) (void)hipEventDestroy(ctx->denoise_ordered);
    if (ctx->d_reproject_scratch) (void)hipFree(ctx->d_reproject_scratch);
    if (ctx->reproject_gathered) (void)hipEventDestroy(ctx->reproject_gathered);
    if (ctx->d_luminance) (void)hipFree(ctx->d_luminance);
    destroy_rccl_communicators(ctx);
    for (auto& r : ctx->pinned_host) (void)hipHostUnregister(r.p);
    (void)hipGetLastError();
    if (ctx->h_staging) (void)hipHostFree(ctx->h_staging);
    for (DeviceState& d : ctx->dev) {
        (void)hipSetDevice(d.device);
        for (auto& ev : d.pending_events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        for (auto& ev : d.free_events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        if (d.peer_copied) (void)hipEventDestroy(d.peer_copied);
        for (int i = 0; i < kStageSets; i++) {
            if (d.rendered[i]) (void)hipEventDestroy(d.rendered[i]);
            if (d.stage_free[i]) (void)hipEventDestroy(d.stage_free[i]);
            if (d.launch_stream[i]) (void)hipStreamDestroy(d.launch_stream[i]);
        }
        if (d.own_stream) (void)hipStreamDestroy(d.own_stream);
        if (d.copy_stream) (void)hipStreamDestroy(d.copy_stream);
    }
    delete ctx;
}

}  // extern "C"

