// ptmi_render.cpp - the executor of the launch schedule: ptmi_render / ptmi_render_snapshots cut a call into each device's share,
// and render_on_device issues what launch_schedule.h plans for it - launches on the main stream or on a stage set, adoptions,
// launches ahead of the caller - bracketed by an event pair for ptmi_kernel_time.
// Owns, of ptmi_context.h: the stage sets (d_stage, stage_cap, reuse_after), `schedule` and previous_call_done per scene; the
// launch streams, their events and the timing event pools per context (created here, destroyed by ptmi_release).
#include <algorithm>
#include <cstdlib>

#include "ptmi_context.h"

using namespace ptmi_internal;
using ptmi_switches::Moment;
using ptmi_switches::read_switches;

int ptmi_internal::fold_events(ptmi_ctx* ctx, DeviceState& d)
{
    ON_DEVICE(ctx, d);
    for (auto& ev : d.pending_events) {
        float ms = 0;
        HIP_TRY(ctx, hipEventSynchronize(ev.second));
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ev.first, ev.second));
        d.kernel_ms += ms;
        d.kernel_launches++;
        d.free_events.push_back(ev);
    }
    d.pending_events.clear();
    return PTMI_OK;
}

namespace {

// Iteration ids [first, first + n) that device k of G takes: those congruent to k modulo G.
void device_share(uint32_t first, uint32_t n, uint32_t k, uint32_t G, uint32_t* first_k, uint32_t* n_k)
{
    const uint32_t skip = (k + G - first % G) % G;  // ids to skip from `first` to the first one of class k
    *first_k = first + skip;
    *n_k = skip < n ? (n - skip + G - 1) / G : 0;
}

// The images of `plan` before global iteration k_end that this device has not provided yet (snapshot_ring.h).
int snapshots_up_to(ptmi_ctx* ctx, DeviceState& d, SnapshotPlan& plan, uint32_t k_end)
{
    for (int b = -1; plan.due(k_end); plan.next++) {
        if (!plan.must_copy()) {
            d.ring.point(plan.slot(), plan.last_buffer);
            continue;
        }
        if (int rc = snapshot_device(ctx, d, plan.slot(), &b)) return rc;
        plan.copied(b);
    }
    return PTMI_OK;
}

// The render-ahead switches, read per call (tests switch them between contexts): launches kept in flight AHEAD of a blocking
// caller (PTMI_RENDER_AHEAD, default 2, 0 = never, at most kStageSets - 2: beside them one launch whose calls are coming, and one
// set for a call that finds nothing), and CALLS one of them may render for (PTMI_RENDER_AHEAD_CALLS, default 4).
static_assert(kAheadIterations == PTMI_COUNTER_SPLITS, "a launch ahead counts per call: at most that many calls");  // (stage_sets.h)

// Stage set `set` able to hold `iterations` iterations (radiance float4 + one statistics word per path), or `at_least` where the
// device does not have the memory for that many.  Growing it waits for whatever may still use the old arrays.
int ensure_stage_set(ptmi_ctx* ctx, DeviceState& d, int set, size_t iterations, size_t at_least = 0)
{
    if (d.stage_cap[set] >= iterations) return PTMI_OK;
    // NOT quiesce(): only this set's launches ahead are dropped and only its stream is waited for - the other sets' launches
    // keep running, the scene stays as it is
    d.schedule.forget_set(set);
    if (d.launch_stream[set]) HIP_TRY(ctx, hipStreamSynchronize(d.launch_stream[set]));
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    if (d.d_stage[set]) (void)hipFree(d.d_stage[set]);
    d.d_stage[set] = nullptr;
    d.stage_cap[set] = 0;
    d.reuse_after[set] = nullptr;
    void* p = nullptr;
    if (at_least && at_least < iterations && hipMalloc(&p, iterations * ctx->image_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr, iterations = at_least;
    }
    if (!p) HIP_TRY(ctx, hipMalloc(&p, iterations * ctx->image_bytes()));
    d.d_stage[set] = (float*)p;
    d.stage_cap[set] = iterations;
    return PTMI_OK;
}

// where the statistics words of a set's launches go: staged per path and counted after the launch, unless there is no histogram
// (PTMI_FLAG_NO_HISTOGRAMS) or a depth that does not fit the 6-bit field
uint32_t* stats_of(const ptmi_ctx* ctx, const DeviceState& d, int set)
{
    if (!(d.d_stage[set] && d.ds.hist_depths && ctx->cfg.ray_max_depth < 64)) return nullptr;
    return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(d.d_stage[set]) + d.stage_cap[set] * ctx->color_bytes());
}

// A launch of m iterations from id f: on the main stream into set 0 (`main`; staged or not), or a SHORT one on stage set `set`:
// on the set's own stream, counting into the set's own block - it touches nothing else of the context, whether a call has asked
// for it or not.  `calls` > 1: the launch renders for that many calls of m / calls iterations each, and counts per call.
// `region`: the work-items it traces; its staging slots are numbered over the region (render_region.h), so a set that holds m
// iterations of the whole image holds m of any region.
int launch(ptmi_ctx* ctx, DeviceState& d, bool main, bool staged, int set, uint32_t f, uint32_t m, uint32_t stride, const Region& region,
           bool region_call, uint32_t calls = 1)
{
    hipStream_t st = main ? d.stream : d.launch_stream[set];
    if (d.reuse_after[set]) HIP_TRY(ctx, hipStreamWaitEvent(st, d.reuse_after[set], 0));  // (main: a short launch nobody adopted)
    if (staged && !(d.d_stage[set] && d.stage_cap[set] >= m))  // (a planning bug: refused, never a fault)
        return fail(ctx, PTMI_ERR_INTERNAL, "stage set " + std::to_string(set) + " holds " + std::to_string(d.d_stage[set] ? d.stage_cap[set] : 0) +
                                                " iterations, a launch of " + std::to_string(m) + " was to stage into it");
    DScene k = d.ds;
    if (!main) {
        HIP_TRY(ctx, hipMemsetAsync(d.d_set_counters[set], 0, PTMI_COUNTER_SPLITS * C_COUNT * 8, st));
        k.counters = d.d_set_counters[set];
        k.split_paths = calls > 1 ? (m / calls) * region_pixels(region) : 0u;  // (in staging slots)
    }
    std::string err;
    if (int rc = KERNELS_OF(ctx, launch_render_wavefront)(k, main ? d.d_scene : d.d_scene_set[set], f, m, stride, d.d_job_counter + set * 8 * 1024,
                                                          ctx->stack_levels, d.schedule.call.stats_build, staged ? d.d_stage[set] : nullptr,
                                                          staged ? stats_of(ctx, d, set) : nullptr, region, region_call, st, &err))
        return fail(ctx, rc, err);
    if (main) return PTMI_OK;
    d.reuse_after[set] = d.rendered[set];  // (until the main stream adopts it)
    HIP_TRY(ctx, hipEventRecord(d.rendered[set], st));
    return PTMI_OK;
}

// One device's launches for its share of a ptmi_render call, as d.schedule plans them, bracketed by an event pair for
// ptmi_kernel_time.  `region_call` = nullptr: ptmi_render, the whole image.  A call with a region (ptmi_render_region, the whole
// image included) is planned as one that cannot run ahead: it adopts no launch ahead, the ones in flight are dropped, and none
// is left behind it.
int render_on_device(ptmi_ctx* ctx, DeviceState& d, uint32_t first, uint32_t n, uint32_t stride, SnapshotPlan* plan = nullptr,
                     const Region* region_call = nullptr)
{
    if (n == 0) return plan ? snapshots_up_to(ctx, d, *plan, plan->n) : PTMI_OK;
    ON_DEVICE(ctx, d);
    if (int rc = d.pending_events.size() >= 512 ? fold_events(ctx, d) : PTMI_OK) return rc;
    const bool megakernel = one_path_per_lane(ctx);
    const bool staged = !megakernel && ctx->cfg.sampler != PTMI_SAMPLER_RANDOM;
    // launch streams of their own (for SHORT launches only: long ones side by side get in each other's way): only where the
    // launch neither reads nor writes the accumulators (staged results, no adaptive sampling), on the context's own stream,
    // and unless switched off (PTMI_SERIAL_LAUNCHES: read ONCE per process, unlike every other switch)
    static const bool serial_env = read_switches(Moment::kProcess).serial_launches != 0;
    const ptmi_switches::Switches call = read_switches(Moment::kRenderCall);
    const bool may_overlap = staged && !ctx->cfg.super_sampling && d.stream == d.own_stream && !serial_env;
    // rendering ahead (per device: with G devices each sees every G-th call, stride G): nothing but staged results leaves the
    // kernel (the histograms of very deep paths are atomics inside it), and the caller has not asked for an image per iteration
    const bool ahead_allowed = !plan && !region_call && !(d.ds.hist_depths && ctx->cfg.ray_max_depth >= 64);
    const Region region = region_call ? *region_call : whole_image(ctx->cfg.image_width, ctx->cfg.image_height);
    const StageNeed need = d.schedule.begin({first, n, stride, ctx->iterations_per_launch, ctx->cfg.super_sampling != 0, may_overlap,
                                             ahead_allowed, (uint32_t)ptmi_switches::clamped(call.render_ahead, 2, 0, kStageSets - 2),
                                             (uint32_t)ptmi_switches::clamped(call.render_ahead_calls, PTMI_COUNTER_SPLITS, 1, PTMI_COUNTER_SPLITS),
                                             (ctx->cfg.flags & PTMI_FLAG_SCHEDULER_STATS) != 0});
    if (staged) {
        // staging arrays, grown on demand: room for launches ahead only once they are due, and only where the device has it
        if (int rc = ensure_stage_set(ctx, d, 0, need.set0)) return rc;
        for (int i = need.ahead ? 0 : 1; need.others && i < kStageSets; i++)
            if (int rc = ensure_stage_set(ctx, d, i, std::max(need.ahead, need.others), need.others)) return rc;
        for (int i = 0; i < kStageSets && may_overlap; i++) {
            if (!d.launch_stream[i]) HIP_TRY(ctx, hipStreamCreateWithFlags(&d.launch_stream[i], hipStreamNonBlocking));
            if (int rc = lazy_event(ctx, d.rendered[i])) return rc;
            if (int rc = lazy_event(ctx, d.stage_free[i])) return rc;
        }
    }
    // the event pair stays in the pool until the call has been issued
    if (d.free_events.empty()) d.free_events.push_back({nullptr, nullptr});
    if (!d.free_events.back().first) HIP_TRY(ctx, hipEventCreate(&d.free_events.back().first));
    if (!d.free_events.back().second) HIP_TRY(ctx, hipEventCreate(&d.free_events.back().second));
    const std::pair<hipEvent_t, hipEvent_t> ev = d.free_events.back();
    const size_t nslot = region_pixels(region);  // staging slots of one iteration
    std::string err;
    // both events on the MAIN stream, [previous launch accumulated, this one accumulated]: the intervals tile the time line
    HIP_TRY(ctx, hipEventRecord(ev.first, d.stream));
    if (megakernel) {
        if (int rc = KERNELS_OF(ctx, launch_render)(d.ds, first, n, stride, region, d.stream, &err)) return fail(ctx, rc, err);
    } else {
        for (const Step& s : d.schedule.steps()) {
            if (s.kind != Step::kAdopt)
                if (int rc = launch(ctx, d, s.kind == Step::kMain, staged, s.set, s.first, s.n, stride, region, region_call != nullptr)) return rc;
            if (s.kind != Step::kMain) HIP_TRY(ctx, hipStreamWaitEvent(d.stream, d.rendered[s.set], 0));
            float* const stage = staged ? d.d_stage[s.set] + (size_t)s.part * s.n * nslot * 4 : nullptr;
            uint32_t* const stage_stats = staged && stats_of(ctx, d, s.set) ? stats_of(ctx, d, s.set) + (size_t)s.part * s.n * nslot : nullptr;
            if (!plan) {
                if (int rc = KERNELS_OF(ctx, launch_accumulate_staged)(d.ds, s.first, s.n, stage, stage_stats, true, region, d.stream, &err))
                    return fail(ctx, rc, err);
            } else {
                // one accumulation per iteration, each followed by the snapshots of the global iterations up to it
                for (uint32_t j = 0; j < s.n; j++) {
                    const uint32_t id = s.first + j * stride;
                    if (int rc = snapshots_up_to(ctx, d, *plan, id - plan->first)) return rc;  // images before this device's next own one
                    if (int rc = KERNELS_OF(ctx, launch_accumulate_staged)(d.ds, id, 1, stage + (size_t)j * nslot * 4,
                                                                           stage_stats ? stage_stats + (size_t)j * nslot : nullptr, false, region, d.stream,
                                                                           &err))
                        return fail(ctx, rc, err);
                    plan->changed = true;
                    if (int rc = snapshots_up_to(ctx, d, *plan, id - plan->first + 1)) return rc;
                }
                if (int rc = stage_stats ? KERNELS_OF(ctx, launch_histogram_staged)(d.ds, s.n, stage_stats, region, d.stream, &err) : PTMI_OK)
                    return fail(ctx, rc, err);
            }
            if (s.kind != Step::kMain)
                if (int rc = launch_add_counters(d.d_counters, d.d_set_counters[s.set] + (size_t)s.part * C_COUNT, C_COUNT, d.stream, &err))
                    return fail(ctx, rc, err);
            if (may_overlap) {  // (also behind a launch on the main stream: a later short launch may take set 0)
                d.reuse_after[s.set] = d.stage_free[s.set];
                HIP_TRY(ctx, hipEventRecord(d.stage_free[s.set], d.stream));
            }
        }
        // launches ahead only of a caller that WAITS: one whose previous call was still running keeps the GPU busy by itself
        const bool caller_waits = d.previous_call_done == nullptr || hipEventQuery(d.previous_call_done) == hipSuccess;
        (void)hipGetLastError();  // (hipErrorNotReady is not an error)
        for (const LaunchSchedule::Ahead& a : d.schedule.launches_ahead(caller_waits, d.stage_cap))
            if (int rc = launch(ctx, d, false, true, a.set, a.first, a.n * a.calls, stride, whole_image(ctx->cfg.image_width, ctx->cfg.image_height), false, a.calls))
                return rc;  // (launches ahead render whole images, whatever call leaves them)
    }
    if (int rc = plan ? snapshots_up_to(ctx, d, *plan, plan->n) : PTMI_OK) return rc;  // images after its last own one
    HIP_TRY(ctx, hipEventRecord(ev.second, d.stream));
    d.free_events.pop_back();
    d.pending_events.push_back(ev);
    d.previous_call_done = ev.second;  // (stays valid in the pool: fold_events only moves the pair to free_events)
    d.schedule.commit();
    if (region_call) d.schedule.forget();  // (no pattern of ptmi_render calls continues a region call: the schedule's own "no call to continue")
    return PTMI_OK;
}

}  // namespace

extern "C" {

void ptmi_device_share(uint32_t first_iteration, uint32_t n_iterations, uint32_t k, uint32_t n_devices, uint32_t* first_k,
                       uint32_t* n_k)
{
    uint32_t f = first_iteration, n = 0;
    if (n_devices > 0 && k < n_devices) device_share(first_iteration, n_iterations, k, n_devices, &f, &n);
    if (first_k) *first_k = f;
    if (n_k) *n_k = n;
}

int ptmi_render(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations)
{
    NEED_SCENE(ctx);
    if (n_iterations == 0) return PTMI_OK;
    if ((uint64_t)first_iteration + n_iterations > 0xFFFFFFFFull)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "iteration range overflows 32 bits");
    const uint32_t G = ctx->n_dev();
    for (uint32_t k = 0; k < G; k++) {
        uint32_t first_k, n_k;
        device_share(first_iteration, n_iterations, k, G, &first_k, &n_k);
        if (int rc = render_on_device(ctx, ctx->dev[k], first_k, n_k, G)) return rc;
    }
    return PTMI_OK;
}

int ptmi_render_region(ptmi_ctx* ctx, const ptmi_region* region, uint32_t first_iteration, uint32_t n_iterations)
{
    NEED_SCENE(ctx);
    if (!region) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_render_region: region is NULL");
    const Region r{region->x, region->y, region->width, region->height};
    std::string why;
    if (!check_region(ctx->cfg.image_width, ctx->cfg.image_height, r, &why)) return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_render_region: " + why);
    if ((uint64_t)first_iteration + n_iterations > 0xFFFFFFFFull)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_render_region: iteration range overflows 32 bits");
    if (n_iterations == 0 || region_is_empty(r)) return PTMI_OK;
    // (the whole image goes the same way as any other rectangle: this is the case that proves the two entry points equal)
    const uint32_t G = ctx->n_dev();
    for (uint32_t k = 0; k < G; k++) {
        uint32_t first_k, n_k;
        device_share(first_iteration, n_iterations, k, G, &first_k, &n_k);
        if (int rc = render_on_device(ctx, ctx->dev[k], first_k, n_k, G, nullptr, &r)) return rc;
    }
    return PTMI_OK;
}

int ptmi_render_snapshots(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations, uint32_t first_slot)
{
    NEED_SCENE(ctx);
    if (n_iterations == 0) return PTMI_OK;
    if ((uint64_t)first_iteration + n_iterations > 0xFFFFFFFFull)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "iteration range overflows 32 bits");
    if (n_iterations > kUserSlots || first_slot >= kUserSlots)
        return fail(ctx, PTMI_ERR_INVALID_ARGUMENT, "ptmi_render_snapshots: more iterations than snapshot slots, or slot out of range");
    if (ctx->cfg.super_sampling || ctx->cfg.sampler == PTMI_SAMPLER_RANDOM || (ctx->cfg.flags & PTMI_FLAG_MEGAKERNEL))
        return fail(ctx, PTMI_ERR_UNSUPPORTED, "ptmi_render_snapshots needs staged launches (JITTERED / UNIFORM sampler, wavefront kernel, no "
                                                "super_sampling): call ptmi_render + ptmi_snapshot per iteration instead");
    if (one_path_per_lane(ctx)) {  // a scene that needs the one-path-per-lane kernel: the same images, one launch each
        for (uint32_t k = 0; k < n_iterations; k++) {
            if (int rc = ptmi_render(ctx, first_iteration + k, 1)) return rc;
            if (int rc = snapshot_all(ctx, (first_slot + k) % kUserSlots)) return rc;
        }
        return PTMI_OK;
    }
    const uint32_t G = ctx->n_dev();
    for (uint32_t k = 0; k < G; k++) {
        uint32_t first_k, n_k;
        device_share(first_iteration, n_iterations, k, G, &first_k, &n_k);
        SnapshotPlan plan{first_iteration, n_iterations, first_slot};
        if (int rc = render_on_device(ctx, ctx->dev[k], first_k, n_k, G, &plan)) return rc;
    }
    return PTMI_OK;
}

}  // extern "C"
