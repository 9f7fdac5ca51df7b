// ptmi_scene_memory.cpp - a scene's life on the devices: upload (ptmi_initialize_memory), the calls that rewrite what was uploaded
// (ptmi_clear, ptmi_bind_accumulators, ptmi_set_camera, ptmi_update_triangles, ptmi_update_materials, ptmi_update_lights,
// ptmi_set_sky, the image and variance writes; ptmi_update_vertices, in ptmi_mesh.cpp, ends in update_triangles here) and the one place
// where it all dies (free_scene_memory).
// Owns the per-scene state of ptmi_context.h: writes DeviceScene / ContextScene at upload and resets them whole; the other units
// only fill the lazily allocated parts (stage sets, snapshot buffers, d_reduced, d_display).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "kernel_choice.h"
#include "ptmi_context.h"
#include "scene_layout.h"
#include "scene_refit_common.h"

using namespace ptmi_internal;
using ptmi_switches::Moment;
using ptmi_switches::read_switches;

// what kernel_choice.h reads of the context
static ptmi_choice::ContextTraits traits_of(const ptmi_ctx* ctx)
{
    return {ctx->cfg.sampler, ctx->cfg.flags, ctx->cfg.super_sampling, ctx->cfg.lights_size, ctx->leaf_cull};
}

bool ptmi_internal::one_path_per_lane(const ptmi_ctx* ctx)
{
    return ptmi_choice::one_path_per_lane(traits_of(ctx), !ctx->literal_kernel_reason.empty(), read_switches(Moment::kKernelKind));
}

// Before the scene memory of device `d` is rewritten: a launch ahead may still be reading it (the stage sets' scene records
// too), so drop them all (and the last call, as every forget does: rendering ahead resumes once the caller has been seen to
// continue again) and wait for their streams, then for the main stream.
int ptmi_internal::quiesce(ptmi_ctx* ctx, DeviceState& d)
{
    ON_DEVICE(ctx, d);
    d.schedule.forget();
    for (int i = 0; i < kStageSets; i++)
        if (d.launch_stream[i]) HIP_TRY(ctx, hipStreamSynchronize(d.launch_stream[i]));
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    return PTMI_OK;
}

// The end of a scene: wait, free what the per-scene structs own, and start over from value-initialised ones.  What they merely
// alias (reuse_after, previous_call_done: events of the context) and what lies inside `allocations` is just forgotten.
void ptmi_internal::free_scene_memory(ptmi_ctx* ctx)
{
    for (DeviceState& d : ctx->dev) {
        // NOT quiesce(): this runs after failures too, so it ignores errors and waits on, and the copy stream may still be
        // reading a snapshot.  The launch streams: after a failure between a launch and the main stream's wait for it
        // (render_on_device) a persistent kernel may still be reading the scene
        (void)hipSetDevice(d.device);
        for (int i = 0; i < kStageSets; i++)
            if (d.launch_stream[i]) (void)hipStreamSynchronize(d.launch_stream[i]);
        (void)hipStreamSynchronize(d.stream);
        if (d.copy_stream) (void)hipStreamSynchronize(d.copy_stream);
        for (void* p : d.allocations) (void)hipFree(p);
        for (float* p : d.d_stage)
            if (p) (void)hipFree(p);
        for (uint32_t k = 0; k < kRingSlots; k++) {
            if (d.d_snapshot[k]) (void)hipFree(d.d_snapshot[k]);
            if (d.snapshot_ready[k]) (void)hipEventDestroy(d.snapshot_ready[k]);
        }
        if (d.d_peer_copy) (void)hipFree(d.d_peer_copy);
        if (d.d_mesh_topology) (void)hipFree(d.d_mesh_topology);
        if (d.d_vertex_staging) (void)hipFree(d.d_vertex_staging);
        d.scene() = DeviceScene{};
    }
    if (!ctx->dev.empty()) (void)hipSetDevice(ctx->dev[0].device);
    if (ctx->d_reduced) (void)hipFree(ctx->d_reduced);
    if (ctx->d_display) (void)hipFree(ctx->d_display);
    ctx->scene() = ContextScene{};
}

namespace {

const float kX2inv[1001] = {
#include "x2inv_table.inc"
};

// Device memory that is freed with the scene.
template <class T>
int scene_alloc(ptmi_ctx* ctx, DeviceState& d, size_t bytes, T*& out)
{
    void* p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, bytes));
    d.allocations.push_back(p);
    out = static_cast<T*>(p);
    return PTMI_OK;
}

template <class T>
int upload(ptmi_ctx* ctx, DeviceState& d, const T* host, size_t count, const T** out)
{
    T* p = nullptr;
    if (int rc = scene_alloc(ctx, d, std::max<size_t>(count * sizeof(T), 16), p)) return rc;  // reference uploads >= 1 byte (OpenCL.cpp:165)
    // blocking copy: the source is pageable host memory
    if (count) HIP_TRY(ctx, hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
    *out = p;
    return PTMI_OK;
}
template <class T>
int upload(ptmi_ctx* ctx, DeviceState& d, const std::vector<T>& host, const T** out)
{
    return upload(ctx, d, host.data(), host.size(), out);
}

// Scene validation + re-layout: scene_layout.cpp (host-only, also behind ptmi_validate_scene).
int build_layout(ptmi_ctx* ctx, const ptmi_scene* sc, Relayout& out)
{
    std::string err;
    const int rc = ptmi_internal::build_layout(ctx->cfg, sc, out, err);
    return rc == PTMI_OK ? rc : fail(ctx, rc, err);
}

// The device copies of d.ds: the context's, and one per stage set whose launches count into the set's own block.
int upload_scene_records(ptmi_ctx* ctx, DeviceState& d)
{
    HIP_TRY(ctx, hipMemcpy(d.d_scene, &d.ds, sizeof(DScene), hipMemcpyHostToDevice));
    for (int i = 0; i < kStageSets; i++) {
        DScene k = d.ds;
        k.counters = d.d_set_counters[i];
        HIP_TRY(ctx, hipMemcpy(d.d_scene_set[i], &k, sizeof(DScene), hipMemcpyHostToDevice));
    }
    return PTMI_OK;
}

// Everything of a scene that lives on one device: the re-laid-out records, the accumulators, the statistics.
int upload_scene(ptmi_ctx* ctx, DeviceState& d, const Relayout& lay, const ptmi_scene* sc)
{
    ON_DEVICE(ctx, d);
    DScene& ds = d.ds;
    ds = DScene{};
    ptmi_choice::choose_upload({lay.tris_precomputed, lay.plain_shading, lay.boxes_ordered, !lay.literal_kernel_reason.empty(), lay.cullable_leaves,
                                lay.recs.size(), lay.nan_walk_box_tests, lay.nan_walk_tri_tests, lay.nan_walk_last_tri},
                               traits_of(ctx), read_switches(Moment::kUpload), ds);
    if (int rc = upload(ctx, d, lay.recs, &ds.tris)) return rc;
    ds.nodes = reinterpret_cast<const DNode*>(ds.tris);  // same array: a reference is an index of 64-byte records
    ds.n_records = (uint32_t)lay.recs.size();
    if (int rc = upload(ctx, d, lay.tri_ids, &ds.tri_ids)) return rc;
    if (default_arithmetic(ctx) && lay.tris_precomputed) {
        // the records' reciprocal determinants in the reference's default arithmetic: a device instruction's values
        std::string err;
        if (int rc = launch_precompute_denominators_da(const_cast<DTri*>(ds.tris), ds.tri_ids, ds.n_records, d.stream, &err))
            return fail(ctx, rc, err);
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    }
    if (int rc = upload(ctx, d, lay.shade, &ds.shade)) return rc;
    if (int rc = upload(ctx, d, lay.mats, &ds.mats)) return rc;
    if (int rc = upload(ctx, d, lay.big_leaves, &ds.big_leaves)) return rc;
    if (int rc = upload(ctx, d, sc->lights, sc->lights_size, &ds.lights)) return rc;
    if (int rc = upload(ctx, d, sc->textures, sc->textures_size, &ds.textures)) return rc;
    if (int rc = upload(ctx, d, sc->textures_data, sc->textures_data_size, &ds.texels)) return rc;

    // counters, then one set of job-queue counters per stage set (256-byte aligned, up to 8 x 1024 dwords apart), then the
    // stage sets' counter blocks and scene records
    constexpr size_t kCounterBlock = ((C_COUNT * 8 + 255) / 256) * 256, kSceneBlock = ((sizeof(DScene) + 255) / 256) * 256;
    constexpr size_t kSetCounterBlock = ((PTMI_COUNTER_SPLITS * C_COUNT * 8 + 255) / 256) * 256;
    constexpr int kSets = kStageSets;
    char *dk = nullptr, *dsc = nullptr;
    if (int rc = scene_alloc(ctx, d, ctx->color_bytes(), d.d_color)) return rc;
    if (int rc = scene_alloc(ctx, d, ctx->count_bytes(), d.d_count)) return rc;
    if (int rc = scene_alloc(ctx, d, ctx->hist_words() * 4, d.d_hist)) return rc;
    if (int rc = scene_alloc(ctx, d, kCounterBlock + 256 + kSets * 8 * 1024 * 4 + kSets * kSetCounterBlock, dk)) return rc;
    if (int rc = scene_alloc(ctx, d, (1 + kSets) * kSceneBlock, dsc)) return rc;
    d.d_scene = (DScene*)dsc;
    d.d_counters = (unsigned long long*)dk;
    d.d_job_counter = (uint32_t*)(dk + kCounterBlock);
    for (int i = 0; i < kSets; i++) {
        d.d_set_counters[i] = (unsigned long long*)(dk + kCounterBlock + kSets * 8 * 1024 * 4 + i * kSetCounterBlock);
        d.d_scene_set[i] = (DScene*)(dsc + (1 + i) * kSceneBlock);
    }

    ds.image_color = d.d_color;
    ds.image_ray_nb = d.d_count;
    const bool hist = !(ctx->cfg.flags & PTMI_FLAG_NO_HISTOGRAMS);
    ds.hist_depths = hist ? d.d_hist : nullptr;
    ds.hist_bbx = hist ? d.d_hist + ctx->cfg.ray_max_depth + 1 : nullptr;
    ds.hist_tri = hist ? d.d_hist + ctx->cfg.ray_max_depth + 1 + PTMI_MAX_INTERSECTION_NUMBER : nullptr;
    ds.counters = d.d_counters;
    if (ds.super_sampling) {
        float* dx = nullptr;
        if (int rc = scene_alloc(ctx, d, ctx->color_bytes(), ds.image_v)) return rc;
        if (int rc = scene_alloc(ctx, d, sizeof kX2inv, dx)) return rc;
        if (int rc = scene_alloc(ctx, d, ctx->count_bytes(), ds.stage_flag)) return rc;
        HIP_TRY(ctx, hipMemcpy(dx, kX2inv, sizeof kX2inv, hipMemcpyHostToDevice));
        ds.x2inv = dx;
    }
    ds.sky = *sc->sky;
    std::memcpy(ds.cam_pos, &sc->camera_position, 16);
    std::memcpy(ds.cam_dir, &sc->camera_direction, 16);
    std::memcpy(ds.cam_right, &sc->camera_right, 16);
    std::memcpy(ds.cam_up, &sc->camera_up, 16);
    ds.root_ref = lay.root_ref;
    ds.width = ctx->cfg.image_width;
    ds.height = ctx->cfg.image_height;
    ds.max_depth = ctx->cfg.ray_max_depth;
    return upload_scene_records(ctx, d);
}

}  // namespace

int ptmi_internal::camera_check(ptmi_ctx* ctx, const char* who, const ptmi_float4* position, const ptmi_float4* direction,
                                const ptmi_float4* right, const ptmi_float4* up)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (!position || !direction || !right || !up) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, std::string(who) + ": a camera vector is NULL");
    if (int rc = need_scene(ctx, who)) return rc;
    const std::string why = camera_needs_literal_kernel(*position, *direction, *right, *up);
    if (!why.empty())
        return fail(ctx, PTMI_ERR_UNSUPPORTED, std::string(who) + ": " + why + ": the kernel instantiation was chosen at upload, call "
                                               "ptmi_initialize_memory with the new camera");
    return PTMI_OK;
}

int ptmi_internal::camera_write(ptmi_ctx* ctx, const ptmi_float4& position, const ptmi_float4& direction, const ptmi_float4& right,
                                const ptmi_float4& up)
{
    for (DeviceState& d : ctx->dev)
        if (int rc = quiesce(ctx, d)) return rc;
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        std::memcpy(d.ds.cam_pos, &position, 16);
        std::memcpy(d.ds.cam_dir, &direction, 16);
        std::memcpy(d.ds.cam_right, &right, 16);
        std::memcpy(d.ds.cam_up, &up, 16);
        if (int rc = upload_scene_records(ctx, d)) return rc;
    }
    return PTMI_OK;
}

namespace {

// The screen of the device form: the checks of screen_update as one kernel over the caller's buffer on devices[0]'s main stream,
// and its one word back.  Nothing of the scene is written.
int screen_update_on_device(ptmi_ctx* ctx, const ptmi_triangle* d_tris, uint32_t n, uint32_t* word)
{
    DeviceState& lead = ctx->dev[0];
    ON_DEVICE(ctx, lead);
    const std::vector<uint8_t>& simple = ctx->update.material_is_simple_color;
    if (!lead.d_material_is_simple_color) {
        uint8_t* p = nullptr;
        if (int rc = scene_alloc(ctx, lead, std::max<size_t>(simple.size(), 16), p)) return rc;
        if (!simple.empty()) HIP_TRY(ctx, hipMemcpy(p, simple.data(), simple.size(), hipMemcpyHostToDevice));
        lead.d_material_is_simple_color = p;
    }
    if (!lead.d_screen_verdict)
        if (int rc = scene_alloc(ctx, lead, 16, lead.d_screen_verdict)) return rc;
    std::string err;
    HIP_TRY(ctx, hipMemsetAsync(lead.d_screen_verdict, 0xFF, 4, lead.stream));  // ptmi_refit::kScreenAccepted
    if (int rc = launch_screen_update(d_tris, n, lead.d_material_is_simple_color, (uint32_t)simple.size(), ctx->update.tris_precomputed,
                                      lead.d_screen_verdict, lead.stream, &err))
        return fail(ctx, rc, err);
    HIP_TRY(ctx, hipMemcpyAsync(word, lead.d_screen_verdict, 4, hipMemcpyDeviceToHost, lead.stream));
    HIP_TRY(ctx, hipStreamSynchronize(lead.stream));
    return PTMI_OK;
}

// ptmi_update_triangles and ptmi_update_triangles_device: `tris` is host memory, or (device_form) memory of devices[0] that the
// kernels read in place there.  The two differ in who applies the screen and in how the triangles reach a device; the schedule,
// the scratch, quiesce and the launches are one.
int update_triangles(ptmi_ctx* ctx, const char* who_is_calling, bool device_form, const ptmi_triangle* tris, uint32_t triangulation_size,
                     ptmi_update_info* info)
{
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
    const clock::time_point t_call = clock::now();
    const std::string who = who_is_calling, prefix = who + ": ";
    if (info) {
        *info = ptmi_update_info{};
        info->struct_size = sizeof(ptmi_update_info);
    }
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (!tris) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + (device_form ? "d_triangulation is NULL" : "triangulation is NULL"));
    if (device_form && (reinterpret_cast<uintptr_t>(tris) & 15u))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + "d_triangulation is not 16-byte aligned");
    if (int rc = need_scene(ctx, who)) return rc;
    if (triangulation_size != ctx->update.triangulation_size)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + std::to_string(triangulation_size) + " triangles, the context holds " +
                                                    std::to_string(ctx->update.triangulation_size) + " (the topology cannot change)");
    if (!ctx->literal_kernel_reason.empty())
        return fail(ctx, PTMI_ERR_UNSUPPORTED, prefix + "the uploaded scene has records that can yield NaN distances (" +
                                               ctx->literal_kernel_reason + "): call ptmi_initialize_memory with the new scene");
    // ---- everything that can refuse, before the first device write
    {
        uint32_t word = ptmi_refit::kScreenAccepted;
        if (device_form) {
            if (int rc = screen_update_on_device(ctx, tris, triangulation_size, &word)) return rc;
        } else {
            word = screen_update_word(ctx->update, tris, triangulation_size);
        }
        std::string err;
        if (int rc = screen_verdict(word, err)) return fail(ctx, rc, prefix + err);
    }
    DeviceState& lead = ctx->dev[0];
    if (!ctx->have_refit) {
        // the schedule of the refit, from the records as they were uploaded (every device holds the same)
        ON_DEVICE(ctx, lead);
        std::vector<DNode> records(lead.ds.n_records);
        std::vector<uint32_t> tri_ids(lead.ds.n_records);
        std::vector<DBigLeaf> big_leaves(ctx->update.n_big_leaves);
        HIP_TRY(ctx, hipStreamSynchronize(lead.stream));
        if (!records.empty()) {
            HIP_TRY(ctx, hipMemcpy(records.data(), lead.ds.nodes, records.size() * sizeof(DNode), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(tri_ids.data(), lead.ds.tri_ids, tri_ids.size() * 4, hipMemcpyDeviceToHost));
        }
        if (!big_leaves.empty())
            HIP_TRY(ctx, hipMemcpy(big_leaves.data(), lead.ds.big_leaves, big_leaves.size() * sizeof(DBigLeaf), hipMemcpyDeviceToHost));
        std::string err;
        if (int rc = build_refit_schedule(records.data(), tri_ids.data(), lead.ds.n_records, big_leaves.data(), ctx->update.n_big_leaves,
                                          lead.ds.root_ref, triangulation_size, ctx->refit, err)) {
            ctx->refit = RefitSchedule();
            return fail(ctx, rc, prefix + err);
        }
        ctx->have_refit = true;
    }
    const size_t tri_bytes = (size_t)triangulation_size * sizeof(ptmi_triangle);
    for (DeviceState& d : ctx->dev) {  // (allocations can refuse too)
        ON_DEVICE(ctx, d);
        const bool in_place = device_form && &d == &lead;  // devices[0] reads the caller's buffer where it is
        if (!d.d_update_tris && !in_place)
            if (int rc = scene_alloc(ctx, d, std::max<size_t>(tri_bytes, 16), d.d_update_tris)) return rc;
        if (!d.d_refit_nodes) {
            uint32_t* p = nullptr;
            if (int rc = scene_alloc(ctx, d, std::max<size_t>(ctx->refit.nodes.size() * 4, 16), p)) return rc;
            if (!ctx->refit.nodes.empty())
                HIP_TRY(ctx, hipMemcpy(p, ctx->refit.nodes.data(), ctx->refit.nodes.size() * 4, hipMemcpyHostToDevice));
            d.d_refit_nodes = p;
        }
    }
    const double validate_ms = ms_since(t_call);
    for (DeviceState& d : ctx->dev)
        if (int rc = quiesce(ctx, d)) return rc;
    // ---- the update: new triangles to the device, then the records, the shading records and the boxes, level by level from the deepest
    double upload_ms = 0, device_ms = 0;
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        const ptmi_triangle* d_tris = d.d_update_tris;
        if (device_form && &d == &lead) {
            d_tris = tris;
        } else if (tri_bytes) {
            // (blocking copies.  The device form's source was last written before the main stream of devices[0] was waited for, in quiesce)
            const clock::time_point t_upload = clock::now();
            if (!device_form) HIP_TRY(ctx, hipMemcpy(d.d_update_tris, tris, tri_bytes, hipMemcpyHostToDevice));
            else if (d.device == lead.device) HIP_TRY(ctx, hipMemcpy(d.d_update_tris, tris, tri_bytes, hipMemcpyDeviceToDevice));
            else HIP_TRY(ctx, hipMemcpyPeer(d.d_update_tris, d.device, tris, lead.device, tri_bytes));
            upload_ms += ms_since(t_upload);
        }
        hipEvent_t begin = nullptr, end = nullptr;
        HIP_TRY(ctx, hipEventCreate(&begin));
        if (hipEventCreate(&end) != hipSuccess) {
            (void)hipEventDestroy(begin);
            return fail(ctx, PTMI_ERR_HIP, prefix + "hipEventCreate failed");
        }
        std::string err;
        int rc = hipEventRecord(begin, d.stream) == hipSuccess ? (int)PTMI_OK : (int)PTMI_ERR_HIP;
        DTri* const records = const_cast<DTri*>(d.ds.tris);
        if (!rc) rc = launch_update_tri_records(records, d.ds.tri_ids, d.ds.n_records, d_tris, triangulation_size, d.ds.tris_precomputed != 0, d.stream, &err);
        if (!rc && default_arithmetic(ctx) && d.ds.tris_precomputed)  // the reciprocal determinants of that arithmetic, as at upload
            rc = launch_precompute_denominators_da(records, d.ds.tri_ids, d.ds.n_records, d.stream, &err);
        if (!rc) rc = launch_update_shade_records(const_cast<DShade*>(d.ds.shade), d_tris, triangulation_size, d.stream, &err);
        for (uint32_t level = ctx->refit.levels(); !rc && level-- > 0;)
            rc = launch_refit_level(const_cast<DNode*>(d.ds.nodes), d.d_refit_nodes + ctx->refit.first[level],
                                    ctx->refit.first[level + 1] - ctx->refit.first[level], d.ds.big_leaves, d.ds.tri_ids, d_tris, d.stream, &err);
        hipError_t e = hipEventRecord(end, d.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, begin, end);
        (void)hipEventDestroy(begin);
        (void)hipEventDestroy(end);
        if (rc) return fail(ctx, rc, prefix + err);
        if (e != hipSuccess) return fail(ctx, PTMI_ERR_HIP, prefix + hipGetErrorString(e));
        device_ms += ms;
    }
    if (info) {
        info->levels = ctx->refit.levels();
        info->upload_ms = upload_ms;
        info->device_ms = device_ms;
        info->validate_ms = validate_ms;
        info->total_ms = ms_since(t_call);
    }
    return PTMI_OK;
}

// DScene::plain_shading as an upload of the scene these facts describe would choose it now (the switch is the upload's)
uint32_t plain_shading_of(const UpdateFacts& facts)
{
    return ptmi_choice::scene_plain_shading(facts.material_type.data(), facts.material_is_simple_color.data(), facts.material_type.size(),
                                            facts.light_type.data(), facts.light_type.size(), read_switches(Moment::kUpload))
               ? 1u
               : 0u;
}

// The screen of ptmi_update_materials: the texture coordinates of the triangles whose materials are textured under `simple`, the
// table as the edit would leave it, read from the DShade records of devices[0] by one kernel on its main stream, and its one
// word back.  Nothing of the scene is written.
int screen_shade_on_device(ptmi_ctx* ctx, const std::vector<uint8_t>& simple, uint32_t* word)
{
    DeviceState& lead = ctx->dev[0];
    ON_DEVICE(ctx, lead);
    if (!lead.d_edited_is_simple_color)
        if (int rc = scene_alloc(ctx, lead, std::max<size_t>(simple.size(), 16), lead.d_edited_is_simple_color)) return rc;
    if (!lead.d_screen_verdict)
        if (int rc = scene_alloc(ctx, lead, 16, lead.d_screen_verdict)) return rc;
    // (in stream order, behind whatever still reads the table; `simple` outlives the wait below)
    HIP_TRY(ctx, hipMemcpyAsync(lead.d_edited_is_simple_color, simple.data(), simple.size(), hipMemcpyHostToDevice, lead.stream));
    std::string err;
    HIP_TRY(ctx, hipMemsetAsync(lead.d_screen_verdict, 0xFF, 4, lead.stream));  // ptmi_refit::kScreenAccepted
    const int rc = launch_screen_shade(lead.ds.shade, ctx->update.triangulation_size, lead.d_edited_is_simple_color, (uint32_t)simple.size(),
                                       lead.d_screen_verdict, lead.stream, &err);
    const hipError_t back = rc ? hipSuccess : hipMemcpyAsync(word, lead.d_screen_verdict, 4, hipMemcpyDeviceToHost, lead.stream);
    HIP_TRY(ctx, hipStreamSynchronize(lead.stream));  // (whatever happened: the copies above read and write the caller's memory)
    if (rc) return fail(ctx, rc, err);
    if (back != hipSuccess) return fail(ctx, PTMI_ERR_HIP, std::string("the screen's word back: ") + hipGetErrorString(back));
    return PTMI_OK;
}

int update_materials(ptmi_ctx* ctx, uint32_t first, const ptmi_material* materiaux, uint32_t n, ptmi_material_update_info* info)
{
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
    const clock::time_point t_call = clock::now();
    const std::string who = "ptmi_update_materials", prefix = who + ": ";
    if (info) {
        *info = ptmi_material_update_info{};
        info->struct_size = sizeof(ptmi_material_update_info);
    }
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (int rc = need_scene(ctx, who)) return rc;
    UpdateFacts& facts = ctx->update;
    const size_t count = facts.material_is_simple_color.size();
    const uint32_t plain_before = ctx->dev[0].ds.plain_shading;
    if (info) info->plain_before = info->plain_after = plain_before;
    if ((uint64_t)first + n > count)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + "materials " + std::to_string(first) + " to " + std::to_string((uint64_t)first + n) +
                                                    ", the context holds " + std::to_string(count) + " (their number cannot change)");
    if (n == 0) return PTMI_OK;
    if (!materiaux) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + "materiaux is NULL");
    // ---- everything that can refuse, before the first device write: build_layout's checks, in its order
    std::string err;
    for (uint32_t k = 0; k < n; k++)
        if (int rc = check_material_texture(materiaux[k], first + k, facts.textures_size, err)) return fail(ctx, rc, prefix + err);
    std::vector<uint8_t> simple = facts.material_is_simple_color;
    bool newly_textured = false;
    for (uint32_t k = 0; k < n; k++) {
        const uint8_t now = materiaux[k].is_simple_color ? 1 : 0;
        if (!now && simple[first + k]) newly_textured = true;
        simple[first + k] = now;
    }
    // Only a material that was a plain colour and is textured now puts coordinates to a test they have not passed: every other
    // triangle's were checked at upload or by the last triangle update, under a table at least as demanding.
    uint32_t screened = 0;
    if (newly_textured && facts.triangulation_size) {
        uint32_t word = ptmi_refit::kScreenAccepted;
        if (int rc = screen_shade_on_device(ctx, simple, &word)) return rc;
        if (int rc = screen_verdict(word, err)) return fail(ctx, rc, prefix + err);
        screened = facts.triangulation_size;
    }
    std::vector<DMat> records(n);
    for (uint32_t k = 0; k < n; k++) ptmi_refit::make_mat_record(materiaux[k], &records[k]);
    const double validate_ms = ms_since(t_call);
    for (DeviceState& d : ctx->dev)
        if (int rc = quiesce(ctx, d)) return rc;
    // ---- the update (the context's facts follow once every device holds it)
    UpdateFacts edited = facts;
    edited.material_is_simple_color = simple;
    for (uint32_t k = 0; k < n; k++) edited.material_type[first + k] = materiaux[k].type;
    const uint32_t plain_after = plain_shading_of(edited);
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        HIP_TRY(ctx, hipMemcpy(const_cast<DMat*>(d.ds.mats) + first, records.data(), n * sizeof(DMat), hipMemcpyHostToDevice));
        d.ds.plain_shading = plain_after;
        if (int rc = upload_scene_records(ctx, d)) return rc;
    }
    // the table ptmi_update_triangles_device screens under follows the edit
    DeviceState& lead = ctx->dev[0];
    if (lead.d_material_is_simple_color) {
        ON_DEVICE(ctx, lead);
        HIP_TRY(ctx, hipMemcpy(lead.d_material_is_simple_color, simple.data(), simple.size(), hipMemcpyHostToDevice));
    }
    facts = std::move(edited);
    if (info) {
        info->screened_triangles = screened;
        info->plain_after = plain_after;
        info->validate_ms = validate_ms;
        info->total_ms = ms_since(t_call);
    }
    return PTMI_OK;
}

}  // namespace

int ptmi_internal::update_triangles_on_device(ptmi_ctx* ctx, const char* who, const ptmi_triangle* d_tris, uint32_t triangulation_size,
                                              ptmi_update_info* info)
{
    return update_triangles(ctx, who, true, d_tris, triangulation_size, info);
}

extern "C" {

int ptmi_update_materials(ptmi_ctx* ctx, uint32_t first, const ptmi_material* materiaux, uint32_t n, ptmi_material_update_info* info)
{
    return update_materials(ctx, first, materiaux, n, info);
}

int ptmi_update_lights(ptmi_ctx* ctx, const ptmi_light* lights, uint32_t lights_size)
{
    const std::string who = "ptmi_update_lights", prefix = who + ": ";
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (int rc = need_scene(ctx, who)) return rc;
    if (lights_size != ctx->cfg.lights_size)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + std::to_string(lights_size) + " lights, config.lights_size is " +
                                                    std::to_string(ctx->cfg.lights_size) + " (LIGHTS_SIZE is baked at setup)");
    if (lights_size && !lights) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + "lights is NULL");
    if (!ctx->literal_kernel_reason.empty())
        return fail(ctx, PTMI_ERR_UNSUPPORTED, prefix + "the uploaded scene has records that can yield NaN distances (" +
                                               ctx->literal_kernel_reason + "): call ptmi_initialize_memory with the new scene");
    const std::string why = lights_need_literal_kernel(lights, lights_size);
    if (!why.empty())
        return fail(ctx, PTMI_ERR_UNSUPPORTED, prefix + why + ": the kernel instantiation was chosen at upload, call "
                                               "ptmi_initialize_memory with the new lights");
    for (DeviceState& d : ctx->dev)
        if (int rc = quiesce(ctx, d)) return rc;
    UpdateFacts edited = ctx->update;
    for (uint32_t i = 0; i < lights_size; i++) edited.light_type[i] = lights[i].type;
    const uint32_t plain = plain_shading_of(edited);
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        if (lights_size)
            HIP_TRY(ctx, hipMemcpy(const_cast<ptmi_light*>(d.ds.lights), lights, (size_t)lights_size * sizeof(ptmi_light), hipMemcpyHostToDevice));
        d.ds.plain_shading = plain;
        if (int rc = upload_scene_records(ctx, d)) return rc;
    }
    ctx->update = std::move(edited);
    return PTMI_OK;
}

int ptmi_set_sky(ptmi_ctx* ctx, const ptmi_sky* sky)
{
    const std::string who = "ptmi_set_sky", prefix = who + ": ";
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (!sky) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, prefix + "sky is NULL");
    if (int rc = need_scene(ctx, who)) return rc;
    std::string err;
    if (int rc = check_sky_textures(*sky, ctx->update.textures_data_size, err)) return fail(ctx, rc, prefix + err);
    for (DeviceState& d : ctx->dev)
        if (int rc = quiesce(ctx, d)) return rc;
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        d.ds.sky = *sky;
        if (int rc = upload_scene_records(ctx, d)) return rc;
    }
    return PTMI_OK;
}

int ptmi_initialize_memory(ptmi_ctx* ctx, const ptmi_scene* sc)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (!sc || sc->struct_size != sizeof(ptmi_scene))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "scene is NULL or struct_size mismatch (ABI)");
    free_scene_memory(ctx);

    Relayout lay;
    if (int rc = build_layout(ctx, sc, lay)) return rc;
    ctx->literal_kernel_reason = lay.literal_kernel_reason;
    if (one_path_per_lane(ctx) && !(ctx->cfg.flags & PTMI_FLAG_MEGAKERNEL) && ctx->cfg.super_sampling) {
        ctx->literal_kernel_reason.clear();
        return fail(ctx, PTMI_ERR_UNSUPPORTED, "SUPER_SAMPLING needs the wavefront kernel, which cannot reproduce the reference on this scene with "
                                               "the RANDOM sampler: " + lay.literal_kernel_reason);
    }
    // a ray holds at most one pending far child per level it has descended
    ctx->stack_levels = lay.max_depth < 1 ? 1 : lay.max_depth;
    ctx->update.triangulation_size = sc->triangulation_size;
    ctx->update.n_big_leaves = (uint32_t)lay.big_leaves.size();
    ctx->update.tris_precomputed = lay.tris_precomputed;
    ctx->update.material_is_simple_color = lay.material_is_simple_color;
    ctx->update.material_type = lay.material_type;
    ctx->update.light_type = lay.light_type;
    ctx->update.textures_size = sc->textures_size;
    ctx->update.textures_data_size = sc->textures_data_size;
    for (DeviceState& d : ctx->dev)
        if (int rc = upload_scene(ctx, d, lay, sc)) {
            const std::string msg = ctx->err;
            free_scene_memory(ctx);
            ctx->err = msg;
            return rc;
        }
    ctx->have_scene = true;
    if (int rc = ptmi_clear(ctx)) return rc;
    return ptmi_synchronize(ctx);
}

int ptmi_clear(ptmi_ctx* ctx)
{
    NEED_SCENE(ctx);
    for (DeviceState& d : ctx->dev) {
        ON_DEVICE(ctx, d);
        // (every launch is followed by its accumulation on the main stream, so main-stream order covers the launch streams)
        HIP_TRY(ctx, hipMemsetAsync(d.ds.image_color, 0, ctx->color_bytes(), d.stream));
        HIP_TRY(ctx, hipMemsetAsync(d.ds.image_ray_nb, 0, ctx->count_bytes(), d.stream));
        HIP_TRY(ctx, hipMemsetAsync(d.d_hist, 0, ctx->hist_words() * 4, d.stream));
        HIP_TRY(ctx, hipMemsetAsync(d.d_counters, 0, C_COUNT * 8, d.stream));
        if (d.ds.image_v) HIP_TRY(ctx, hipMemsetAsync(d.ds.image_v, 0, ctx->color_bytes(), d.stream));
        // a launch queued AFTER this call runs on a launch stream of its own and adds to the counters when it ends: it must
        // not overtake the memsets above
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    }
    return PTMI_OK;
}

int ptmi_write_image(ptmi_ctx* ctx, const float* image_color, const float* image_ray_nb)
{
    NEED_SCENE(ctx);
    const size_t color_bytes = ctx->color_bytes(), count_bytes = ctx->count_bytes();
    // the image goes to devices[0]; the other devices' partial sums restart from zero
    for (uint32_t k = 0; k < ctx->n_dev(); k++) {
        DeviceState& d = ctx->dev[k];
        ON_DEVICE(ctx, d);
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
        if (k == 0) {
            if (image_color) HIP_TRY(ctx, hipMemcpy(d.ds.image_color, image_color, color_bytes, hipMemcpyHostToDevice));
            if (image_ray_nb) HIP_TRY(ctx, hipMemcpy(d.ds.image_ray_nb, image_ray_nb, count_bytes, hipMemcpyHostToDevice));
        } else {
            if (image_color) HIP_TRY(ctx, hipMemset(d.ds.image_color, 0, color_bytes));
            if (image_ray_nb) HIP_TRY(ctx, hipMemset(d.ds.image_ray_nb, 0, count_bytes));
        }
    }
    return PTMI_OK;
}

int ptmi_read_variance(ptmi_ctx* ctx, float* image_v)
{
    if (!image_v) return PTMI_ERR_INVALID_ARGUMENT;
    NEED_SCENE(ctx);
    DeviceState& d0 = ctx->dev[0];
    if (!d0.ds.image_v) return fail(ctx, PTMI_ERR_STATE, "no variance accumulator: the context was set up without super_sampling");
    const size_t npix = ctx->npix(), color_bytes = ctx->color_bytes(), count_bytes = ctx->count_bytes();
    ON_DEVICE(ctx, d0);
    HIP_TRY(ctx, hipMemcpyAsync(image_v, d0.ds.image_v, color_bytes, hipMemcpyDeviceToHost, d0.stream));
    HIP_TRY(ctx, hipStreamSynchronize(d0.stream));
    if (ctx->n_dev() == 1) return PTMI_OK;
    // Several devices: each kept (sum S, count n, imageV = sum of squared deviations M2) of ITS samples.  S and n add; M2
    // does not:  M2 = M2_a + M2_b + (mean_b - mean_a)^2 * n_a * n_b / (n_a + n_b)   (Chan, Golub, LeVeque).  Merged here on
    // the host, device after device, in fp32 with the operation order of distributed.merge_moments.
    std::vector<float> sum(npix * 4), cnt(npix), sb(npix * 4), nb(npix), vb(npix * 4);
    HIP_TRY(ctx, hipMemcpy(sum.data(), d0.ds.image_color, color_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cnt.data(), d0.ds.image_ray_nb, count_bytes, hipMemcpyDeviceToHost));
    for (uint32_t k = 1; k < ctx->n_dev(); k++) {
        DeviceState& d = ctx->dev[k];
        ON_DEVICE(ctx, d);
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
        HIP_TRY(ctx, hipMemcpy(sb.data(), d.ds.image_color, color_bytes, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(nb.data(), d.ds.image_ray_nb, count_bytes, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(vb.data(), d.ds.image_v, color_bytes, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < npix; p++) {
            const float na = cnt[p], nbp = nb[p], n = na + nbp;
            const float sa_ = na > 0 ? na : 1.f, sb_ = nbp > 0 ? nbp : 1.f, sn_ = n > 0 ? n : 1.f;
            const bool both = na > 0 && nbp > 0;
            for (int c = 0; c < 4; c++) {
                const float delta = sb[4 * p + c] / sb_ - sum[4 * p + c] / sa_;
                const float cross = delta * delta * (na * nbp / sn_);
                image_v[4 * p + c] = (image_v[4 * p + c] + vb[4 * p + c]) + (both ? cross : 0.f);
                sum[4 * p + c] = sum[4 * p + c] + sb[4 * p + c];
            }
            cnt[p] = n;
        }
    }
    return PTMI_OK;
}

int ptmi_write_variance(ptmi_ctx* ctx, const float* image_v)
{
    if (!image_v) return PTMI_ERR_INVALID_ARGUMENT;
    NEED_SCENE(ctx);
    if (ctx->n_dev() != 1) return fail(ctx, PTMI_ERR_UNSUPPORTED, "ptmi_write_variance on a multi-device context");
    DeviceState& d = ctx->dev[0];
    if (!d.ds.image_v) return fail(ctx, PTMI_ERR_STATE, "no variance accumulator: the context was set up without super_sampling");
    ON_DEVICE(ctx, d);
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    HIP_TRY(ctx, hipMemcpy(d.ds.image_v, image_v, ctx->color_bytes(), hipMemcpyHostToDevice));
    return PTMI_OK;
}

int ptmi_bind_accumulators(ptmi_ctx* ctx, void* d_color, void* d_count)
{
    NEED_SCENE(ctx);
    if (ctx->n_dev() != 1) return fail(ctx, PTMI_ERR_UNSUPPORTED, "ptmi_bind_accumulators on a multi-device context");
    if ((d_color == nullptr) != (d_count == nullptr))
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "bind both accumulators or neither");
    DeviceState& d = ctx->dev[0];
    if (int rc = quiesce(ctx, d)) return rc;  // (upload_scene_records rewrites the stage sets' scene records)
    d.ds.image_color = d_color ? (float*)d_color : d.d_color;
    d.ds.image_ray_nb = d_count ? (float*)d_count : d.d_count;
    ctx->accum_bound = d_color != nullptr;
    return upload_scene_records(ctx, d);
}

int ptmi_set_camera(ptmi_ctx* ctx, const ptmi_float4* position, const ptmi_float4* direction, const ptmi_float4* right, const ptmi_float4* up)
{
    if (int rc = camera_check(ctx, "ptmi_set_camera", position, direction, right, up)) return rc;
    return camera_write(ctx, *position, *direction, *right, *up);
}

int ptmi_update_triangles(ptmi_ctx* ctx, const ptmi_triangle* triangulation, uint32_t triangulation_size, ptmi_update_info* info)
{
    return update_triangles(ctx, "ptmi_update_triangles", false, triangulation, triangulation_size, info);
}

int ptmi_update_triangles_device(ptmi_ctx* ctx, const void* d_triangulation, uint32_t triangulation_size, ptmi_update_info* info)
{
    return update_triangles(ctx, "ptmi_update_triangles_device", true, static_cast<const ptmi_triangle*>(d_triangulation), triangulation_size, info);
}

}  // extern "C"
