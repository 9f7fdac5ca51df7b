// launch_schedule.h - one device's launches for a ptmi_render call: on the main stream, on a stage set (stage_sets.h), adopted
// from a launch that ran AHEAD of the caller, and the launches to keep in flight for the next calls; render_on_device
// (ptmi_render.cpp) issues them.  Pure host code without HIP, played on the CPU by tests/launch_schedule_model.cpp.  Not ABI.
// A short launch touches nothing of the context but its stage set until the main stream ADOPTS it.  So once a caller that waits
// for each call has been seen to come back for the next ids with the same count, every call leaves up to `ahead_depth` launches
// for the next calls in flight, each for up to kAheadIterations / n calls.  A call that asks for something else
// drops them without a trace; their sets are free again once their kernels have ended (the executor's reuse_after events).
#pragma once

#include <algorithm>
#include <cstddef>
#include <deque>
#include <vector>

#include "stage_sets.h"

namespace ptmi_internal {

// One ptmi_render call on one device: ids first, first + stride, ... (n iterations) in launches of at most `cap`, or of one under
// super-sampling (iteration k's stop criterion reads the accumulators after k-1).  may_overlap: short launches get streams and
// sets of their own; ahead_allowed: no snapshot plan and no deep-path histograms; ahead_depth / ahead_calls: PTMI_RENDER_AHEAD /
// PTMI_RENDER_AHEAD_CALLS; stats_build: the statistics build counts per launch, so a launch ahead renders for one call.
struct Call {
    uint32_t first, n, stride, cap;
    bool super_sampling, may_overlap, ahead_allowed;
    uint32_t ahead_depth, ahead_calls;
    bool stats_build;
};

// One launch's worth of a call's ids, in id order: main stream, set 0 | a new short launch on `set` | part `part` of the launch ahead on `set`
struct Step { enum Kind { kMain, kNew, kAdopt } kind; int set; uint32_t first, n, part; };

struct LaunchSchedule {
    // a launch that renders for `calls` calls of n iterations each (ids from `first` on), `taken` of which have adopted their part
    struct Ahead { uint32_t first, n, stride; int set; uint32_t calls, taken; };
    std::deque<Ahead> ahead;  // launches in flight that calls have not (all) asked for yet, oldest first
    uint32_t streak = 0;      // calls in a row that continued where the previous one left off
    uint32_t next_set = 0;
    // the previous call: launches only run ahead of a caller that has been SEEN to continue where it left off (ids first + n,
    // same n), so a caller that jumps around pays nothing
    bool have_last = false;
    uint32_t last_first = 0, last_n = 0, last_stride = 0;
    Call call{};  // the call being planned, and whether it has been committed
    bool committed = true, can_run_ahead = false, continues = false;

    // A new call: what its stage sets must hold.  A call begun and never committed failed: the next one starts from a clean
    // schedule.  Launches ahead of a call that cannot run ahead are forgotten.
    StageNeed begin(const Call& c)
    {
        if (!committed) forget();
        call = c, committed = false;
        can_run_ahead = c.may_overlap && c.ahead_allowed && c.ahead_depth > 0 && c.n < kShortLaunch;
        if (!can_run_ahead) ahead.clear();
        continues = have_last && last_n == c.n && last_stride == c.stride &&
                    (uint64_t)last_first + (uint64_t)c.n * c.stride == (uint64_t)c.first;
        return stage_need(c.n, c.cap, c.may_overlap, can_run_ahead, continues);
    }

    // The call's launches: adopted where a launch ran ahead for its ids, else new.
    std::vector<Step> steps()
    {
        std::vector<Step> out;
        const uint32_t cap = call.super_sampling ? 1u : call.cap;
        for (uint32_t done = 0; done < call.n;) {
            const uint32_t m = min_u32(call.n - done, cap), f = call.first + done * call.stride;
            done += m;
            if (!(call.may_overlap && m < kShortLaunch)) {
                out.push_back({Step::kMain, 0, f, m, 0});
                continue;
            }
            // a launch that ran ahead for these ids?  (the oldest first; anything else the caller did not come back for)
            bool found = false;
            while (can_run_ahead && !ahead.empty() && !found) {
                Ahead& a = ahead.front();
                found = a.n == m && a.stride == call.stride && (uint64_t)a.first + (uint64_t)a.taken * a.n * a.stride == (uint64_t)f;
                if (found) out.push_back({Step::kAdopt, a.set, f, m, a.taken});
                if (!found || ++a.taken == a.calls) ahead.pop_front();
            }
            if (!found) out.push_back({Step::kNew, pick_set(), f, m, 0});
        }
        return out;
    }

    // The launches to keep in flight ahead of the caller, once the call's own are issued.  stage_cap: iterations each set holds.
    std::vector<Ahead> launches_ahead(bool caller_waits, const size_t* stage_cap)
    {
        std::vector<Ahead> out;
        streak = continues ? streak + 1 : 0;
        if (!(can_run_ahead && continues && caller_waits)) return out;
        const uint32_t n = call.n, stride = call.stride;
        uint64_t next = ahead.empty() ? (uint64_t)call.first + (uint64_t)n * stride
                                      : (uint64_t)ahead.back().first + (uint64_t)ahead.back().calls * n * stride;
        // (a launch whose calls have begun to come no longer counts: what replaces it starts as soon as it has ended)
        const int untouched = (int)ahead.size() - (!ahead.empty() && ahead.front().taken != 0u ? 1 : 0);
        for (int have = untouched; have < (int)call.ahead_depth; have++) {
            uint32_t calls = call.stats_build ? 1u : call.ahead_calls;
            if (calls > kAheadIterations / n) calls = kAheadIterations / n;
            if (calls * n > call.cap) calls = call.cap / n;
            if (streak < 4 && calls > (1u << (streak - 1))) calls = 1u << (streak - 1);
            while (calls > 1 && next + ((uint64_t)calls * n - 1) * stride > 0xFFFFFFFFull) calls--;
            if (calls < 1 || next + (uint64_t)(n - 1) * stride > 0xFFFFFFFFull) break;
            const int set = pick_set();
            if ((size_t)n * calls > stage_cap[set]) calls = (uint32_t)(stage_cap[set] / n);
            if (calls < 1) break;
            ahead.push_back({(uint32_t)next, n, stride, set, calls, 0u});
            out.push_back(ahead.back());
            next += (uint64_t)calls * n * stride;
        }
        return out;
    }

    // The call has been issued: the next one may continue it.
    void commit() { committed = true, have_last = true, last_first = call.first, last_n = call.n, last_stride = call.stride; }
    // Nothing runs ahead and there is no call to continue (scene freed, call failed, accumulators re-bound).
    void forget() { ahead.clear(), have_last = false; }
    // The launches ahead on stage set `set` (it is reallocated).
    void forget_set(int set) { ahead.erase(std::remove_if(ahead.begin(), ahead.end(), [set](const Ahead& a) { return a.set == set; }), ahead.end()); }
    // a stage set no launch in flight ahead of the caller holds (there always is one: fewer launches ahead than sets)
    int pick_set()
    {
        for (int tries = 1;; tries++) {
            const int set = (int)(next_set++ % kStageSets);
            if (tries == kStageSets || std::none_of(ahead.begin(), ahead.end(), [set](const Ahead& a) { return a.set == set; })) return set;
        }
    }
};

}  // namespace ptmi_internal
