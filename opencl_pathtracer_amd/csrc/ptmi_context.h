// ptmi_context.h - the state behind a ptmi_ctx, grouped by WHEN IT DIES, and what the host units of libptmi.so share
// (ptmi_api.cpp, ptmi_scene_memory.cpp, ptmi_render.cpp, ptmi_readback.cpp, ptmi_query.cpp, ptmi_paths.cpp, ptmi_guides.cpp, ptmi_denoise.cpp, ptmi_reproject.cpp, ptmi_display.cpp, ptmi_mesh.cpp).  Private: not ABI, never installed.
//
// Two lifetimes.  PER SCENE (DeviceScene, ContextScene): free_scene_memory() frees what the struct owns and assigns a
// value-initialised one, so a new per-scene field needs no line anywhere else.  PER CONTEXT (the members DeviceState and ptmi_ctx
// add): ptmi_release() destroys them.  The per-scene structs are BASES of the per-context ones, so that `d.ds` and
// `ctx->have_scene` read as they always did; scene() names the part that dies with the scene.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ptmi.h"
#include "ptmi_internal.h"
#include "scene_refit.h"
#include "launch_schedule.h"
#include "snapshot_ring.h"

struct ptmi_ctx;

namespace ptmi_internal {

// ---- per scene, on one device: a full scene replica and its own accumulators
struct DeviceScene {
    std::vector<void*> allocations;  // everything below up to d_refit_nodes lies in these
    float* d_color = nullptr;
    float* d_count = nullptr;
    uint32_t* d_hist = nullptr;  // depths | bbx | tri
    unsigned long long* d_counters = nullptr;
    uint32_t* d_job_counter = nullptr;
    DScene ds{};
    DScene* d_scene = nullptr;  // device copy of ds (what the wavefront kernel's path logic reads)
    unsigned long long* d_set_counters[kStageSets] = {};  // [PTMI_COUNTER_SPLITS][C_COUNT] each: one block per call a launch renders for
    DScene* d_scene_set[kStageSets] = {};                 // ds with .counters = the set's block
    // ptmi_update_triangles, allocated by the first update of a scene: the caller's new triangles, and the inner records by
    // level (ContextScene::refit)
    // ptmi_update_triangles_device, devices[0] only, allocated by its first call: what the screen kernel reads of the materials
    // (UpdateFacts::material_is_simple_color) and the word it answers with.  That form reads the caller's buffer in place on
    // devices[0], which then needs no d_update_tris
    uint8_t* d_material_is_simple_color = nullptr;
    uint32_t* d_screen_verdict = nullptr;
    // ptmi_update_materials, devices[0] only, allocated by the first call that screens: the table of plain-colour materials AS
    // THE EDIT WOULD LEAVE IT, which its screen kernel reads (the one above stays the table in force until the edit is accepted)
    uint8_t* d_edited_is_simple_color = nullptr;
    ptmi_triangle* d_update_tris = nullptr;
    uint32_t* d_refit_nodes = nullptr;
    // Staged radiances [iteration][pixel] float4 (+ one statistics word per path) of the launches in flight: the stage sets of
    // launch_schedule.h, which decides what runs on them (`schedule`).  What keeps the results those of sequential launches:
    // the staged values reach the accumulators on the ONE main stream, launch after launch (launch_accumulate_staged), and a
    // set is reused only after its previous launch's values have been added (stage_free) or, if nobody adopted it, after it has
    // ended (rendered).
    float* d_stage[kStageSets] = {};      // owned, each its own allocation
    size_t stage_cap[kStageSets] = {};    // iterations a set holds
    // what the set's next launch waits for: stage_free (adopted) or rendered (dropped).  An ALIAS of an event DeviceState owns
    hipEvent_t reuse_after[kStageSets] = {};
    LaunchSchedule schedule;
    hipEvent_t previous_call_done = nullptr;  // the event behind the previous call's work on the main stream: an ALIAS into the timing pool
    // ptmi_snapshot ring: BUFFERS of float[5*W*H] (colour, then count), allocated on first use, each with the event that says it
    // is filled - owned: a slot of the NEXT scene is empty until ptmi_snapshot fills it.  `ring` says which buffer a slot shows
    float* d_snapshot[kRingSlots] = {};
    hipEvent_t snapshot_ready[kRingSlots] = {};
    SnapshotRing ring;
    float* d_peer_copy = nullptr;  // ON devices[0]: where this device's snapshot lands before the sum (ring.landed_*)
    // ptmi_bind_mesh / ptmi_update_vertices (ptmi_mesh.cpp), devices[0] only, owned: the bound topology as ONE allocation (the
    // planes of mesh_assemble.h: head | uv | tail), replaced by the next bind; and where the host form's vertex buffers land
    // (positions, then normals from the next multiple of 16), grown on demand.  The assembled records go to d_update_tris
    char* d_mesh_topology = nullptr;
    char* d_vertex_staging = nullptr;
    size_t vertex_staging_bytes = 0;
};

// One device's share of a render (one process drives all of them from one host thread: every launch and copy is asynchronous).
struct DeviceState : DeviceScene {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;       // render stream (own_stream unless ptmi_set_stream gave another)
    hipStream_t copy_stream = nullptr;  // devices[0]: readbacks; other devices: their peer copy onto devices[0]
    hipStream_t launch_stream[kStageSets] = {};
    hipEvent_t rendered[kStageSets] = {};    // recorded on launch_stream[i] behind the kernel
    hipEvent_t stage_free[kStageSets] = {};  // recorded on the main stream behind the accumulation
    hipEvent_t peer_copied = nullptr;        // this device's snapshot has landed in d_peer_copy (devices[0]: the gate before the copies)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_events, free_events;  // ptmi_kernel_time: one pair per call
    double kernel_ms = 0;
    uint32_t kernel_launches = 0;

    DeviceScene& scene() { return *this; }
};

// ---- per context: a round trip through devices[0] for host arrays of the caller's (ptmi_query_rays, ptmi_trace_paths, ptmi_render_guides) - a
// device buffer, and a pinned landing buffer of `cap` bytes, allocated only once a result's destination is not page-locked.
// reserve() frees and regrows both when `landing_bytes` exceeds the capacity; ptmi_release frees them.
struct RoundTrip {
    char *d = nullptr, *h = nullptr;
    size_t cap = 0;
    int reserve(ptmi_ctx* ctx, size_t device_bytes, size_t landing_bytes, bool need_landing);
    void release()
    {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        cap = 0;
    }
};

// ---- per scene, on the context
struct ContextScene {
    bool have_scene = false;
    bool accum_bound = false;  // caller-owned accumulators (single device)
    uint32_t stack_levels = PTMI_BVH_MAX_DEPTH;
    // Why the uploaded scene is rendered by the one-path-per-lane kernel although the context did not ask for it (empty: it is
    // not).  See scene_needs_literal_kernel() in scene_layout.cpp.
    std::string literal_kernel_reason;
    // ptmi_update_triangles: what it has to know of the uploaded scene, and the schedule of its refit (made by the first update)
    UpdateFacts update;
    RefitSchedule refit;
    bool have_refit = false;
    // ptmi_bind_mesh: is a topology bound, its vertex count, and whether it came with texture coordinates (the uv planes exist)
    bool have_mesh = false;
    uint32_t mesh_vertices = 0;
    bool mesh_has_uv = false;
    // on devices[0], owned
    float* d_reduced = nullptr;    // sum of the devices' snapshots (n_devices > 1)
    uint8_t* d_display = nullptr;  // the pixels of ptmi_read_display and of ptmi_read_display_tonemapped
    size_t display_bytes = 0;
};

}  // namespace ptmi_internal

struct ptmi_ctx : ptmi_internal::ContextScene {
    ptmi_config cfg{};
    std::vector<ptmi_internal::DeviceState> dev;  // dev[0] = devices[0]: where partial images are summed and read back from
    std::string err;
    uint32_t iterations_per_launch = ptmi_internal::kMaxIterationsPerLaunch;
    int leaf_cull = -1;  // PTMI_LEAF_CULL at set-up: 0 = never cull leaves, 1 = direct leaves / 2 = direct and pushed leaves wherever the records carry bits, 3 = as 2 by the tight tier's bits alone; unset (-1): both, where it can pay
    // RCCL communicators, one per device of the context (single process, ncclCommInitAll): the sum of the devices' partial
    // images is an ncclReduce over xGMI where librccl is present and the devices are distinct (ptmi_readback.cpp)
    std::vector<void*> rccl_comms;
    int rccl_state = 0;  // 0 = not tried, 1 = ready, -1 = unavailable (peer copies + a sum kernel instead)
    // host side of the readbacks
    float* h_staging = nullptr;  // pinned, 5*W*H floats
    struct HostRange { char* p; size_t bytes; };
    std::vector<HostRange> pinned_host;  // caller buffers page-locked by ptmi_pin_host_buffer: readbacks DMA straight into them
    // ptmi_query_rays: rays, and `cap` bytes of hits behind them, on the device; the hits land.  ptmi_trace_paths: the same with
    // sums for hits.  ptmi_render_guides: the planes of one call behind one another, in the same layout on the device and where
    // they land
    ptmi_internal::RoundTrip query_buffers, path_buffers, guide_buffers;
    // ptmi_denoise / ptmi_denoise_device (ptmi_denoise.cpp), on devices[0], allocated by the first call that needs them: the
    // feature planes between the filter's passes, 56 bytes per pixel, for either form; for the host form a round trip of 68 more
    // (the result, which lands, then the guide planes it renders); and the event that orders the host form of a multi-device
    // context, which runs on the copy stream, behind a device-form call in flight on the main stream
    char* d_denoise_features = nullptr;
    ptmi_internal::RoundTrip denoise_buffers;
    hipEvent_t denoise_ordered = nullptr;
    // ptmi_set_camera_reprojected (ptmi_reproject.cpp), on devices[0], allocated by the first call: 92 bytes per pixel - the
    // normal and position planes of the previous and of the new camera and the result's sums (float4 each: 80), then the two hit
    // counts and the result's counts (12), every plane starting 16-byte aligned; and the event behind a multi-device context's
    // gathered image, which the main stream waits for
    char* d_reproject_scratch = nullptr;
    hipEvent_t reproject_gathered = nullptr;
    // ptmi_luminance_histogram (ptmi_display.cpp), on devices[0], allocated by the first call: the 260 words of the host form.
    // (ptmi_read_display_tonemapped shares ContextScene::d_display with ptmi_read_display; the device forms need no scratch.)
    uint32_t* d_luminance = nullptr;

    ptmi_internal::ContextScene& scene() { return *this; }
    uint32_t n_dev() const { return (uint32_t)dev.size(); }
    size_t npix() const { return (size_t)cfg.image_width * cfg.image_height; }
    // the sizes of what is kept per pixel: the colour sum (float4), the sample count (float), and both behind one another - a
    // snapshot buffer, and one staged iteration (radiance float4 + one statistics word per path)
    size_t color_bytes() const { return npix() * 16; }
    size_t count_bytes() const { return npix() * 4; }
    size_t image_bytes() const { return npix() * 20; }
    size_t hist_words() const { return (size_t)cfg.ray_max_depth + 1 + 2 * PTMI_MAX_INTERSECTION_NUMBER; }  // depths | bbx | tri
    // Is [p, p + bytes) inside a buffer the caller has page-locked with ptmi_pin_host_buffer?  Then a readback is one DMA into
    // it; any other destination goes through a pinned staging buffer of the context and a host memcpy.
    bool host_is_pinned(const void* p, size_t bytes) const
    {
        for (const HostRange& r : pinned_host)
            if ((const char*)p >= r.p && (const char*)p + bytes <= r.p + r.bytes) return true;
        return false;
    }
};

namespace ptmi_internal {

inline int fail(ptmi_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    else set_global_error(msg);
    return code;
}

#define HIP_TRY(ctx, expr)                                                                           \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess)                                                                       \
            return fail(ctx, PTMI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)

// every device call is made with the target device current
#define ON_DEVICE(ctx, d) HIP_TRY(ctx, hipSetDevice((d).device))

// the integrator's entry points in the context's arithmetic mode (ptmi_internal.h)
inline bool default_arithmetic(const ptmi_ctx* ctx) { return (ctx->cfg.flags & PTMI_FLAG_DEFAULT_ARITHMETIC) != 0; }
#define KERNELS_OF(ctx, name) (default_arithmetic(ctx) ? name##_da : name)

// The head of an entry point that needs an uploaded scene: `return`s what it has to say about a missing context or scene.
inline int need_scene(ptmi_ctx* ctx, const std::string& entry_point)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    return ctx->have_scene ? (int)PTMI_OK : fail(ctx, PTMI_ERR_STATE, entry_point + " before ptmi_initialize_memory");
}
#define NEED_SCENE(ctx)                                        \
    do {                                                       \
        if (int rc__ = need_scene(ctx, __func__)) return rc__; \
    } while (0)

// Buffers and events made on first use (the right device is current): nothing happens where `p` / `e` exists already.
template <class T>
int lazy_device_buffer(ptmi_ctx* ctx, T*& p, size_t bytes)
{
    void* q = p;
    if (!q) HIP_TRY(ctx, hipMalloc(&q, bytes));
    p = static_cast<T*>(q);
    return PTMI_OK;
}
template <class T>
int lazy_pinned_buffer(ptmi_ctx* ctx, T*& p, size_t bytes)
{
    void* q = p;
    if (!q) HIP_TRY(ctx, hipHostMalloc(&q, bytes, hipHostMallocDefault));
    p = static_cast<T*>(q);
    return PTMI_OK;
}
inline int lazy_event(ptmi_ctx* ctx, hipEvent_t& e)
{
    if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return PTMI_OK;
}

inline int RoundTrip::reserve(ptmi_ctx* ctx, size_t device_bytes, size_t landing_bytes, bool need_landing)
{
    if (landing_bytes > cap) {
        release();  // (every earlier call has returned, so nothing is in flight on the buffers that go)
        if (int rc = lazy_device_buffer(ctx, d, device_bytes)) return rc;
        cap = landing_bytes;
    }
    return need_landing ? lazy_pinned_buffer(ctx, h, cap) : (int)PTMI_OK;
}

// Device memory -> host arrays of the caller's over `stream`: one DMA straight into a destination that is page-locked
// (ptmi_pin_host_buffer), otherwise into `landing` at the item's offset and, after the ONE wait for the stream, a memcpy.
struct Landing {
    void* to;  // nullptr: nothing is asked for
    const void* from;
    size_t bytes, offset;
};
template <size_t N>
bool needs_landing(const ptmi_ctx* ctx, const Landing (&items)[N])
{
    for (const Landing& i : items)
        if (i.to && !ctx->host_is_pinned(i.to, i.bytes)) return true;
    return false;
}
template <size_t N>
int land(ptmi_ctx* ctx, const Landing (&items)[N], hipStream_t stream, char* landing)
{
    bool direct[N];
    for (size_t k = 0; k < N; k++) {
        const Landing& i = items[k];
        direct[k] = !i.to || ctx->host_is_pinned(i.to, i.bytes);
        if (i.to) HIP_TRY(ctx, hipMemcpyAsync(direct[k] ? i.to : landing + i.offset, i.from, i.bytes, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    for (size_t k = 0; k < N; k++)
        if (!direct[k]) std::memcpy(items[k].to, landing + items[k].offset, items[k].bytes);
    return PTMI_OK;
}

// ptmi_scene_memory.cpp
bool one_path_per_lane(const ptmi_ctx* ctx);
void free_scene_memory(ptmi_ctx* ctx);
int quiesce(ptmi_ctx* ctx, DeviceState& d);
// ptmi_set_camera in its two halves (ptmi_set_camera_reprojected does its own work between them): what can refuse - a missing
// context, vector or scene, a camera that would change the kernel instantiation - and the write on every device, behind quiesce()
int camera_check(ptmi_ctx* ctx, const char* who, const ptmi_float4* position, const ptmi_float4* direction, const ptmi_float4* right,
                 const ptmi_float4* up);
int camera_write(ptmi_ctx* ctx, const ptmi_float4& position, const ptmi_float4& direction, const ptmi_float4& right, const ptmi_float4& up);
// ptmi_update_triangles_device under another entry point's name: ptmi_update_vertices, whose records are its own scratch
int update_triangles_on_device(ptmi_ctx* ctx, const char* who, const ptmi_triangle* d_tris, uint32_t triangulation_size, ptmi_update_info* info);
// ptmi_render.cpp
int fold_events(ptmi_ctx* ctx, DeviceState& d);
// ptmi_readback.cpp
int snapshot_device(ptmi_ctx* ctx, DeviceState& d, uint32_t slot, int* buffer = nullptr);
int snapshot_all(ptmi_ctx* ctx, uint32_t slot);
int gather_snapshot(ptmi_ctx* ctx, uint32_t slot, const float** image);
void destroy_rccl_communicators(ptmi_ctx* ctx);

}  // namespace ptmi_internal
