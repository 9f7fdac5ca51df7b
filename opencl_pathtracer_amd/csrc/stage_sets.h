// stage_sets.h - how large the staging arrays of one ptmi_render call must be (render_on_device, ptmi_render.cpp).
// Pure host code without HIP: tests/stage_sets_model.cpp checks it on the CPU.  Not part of the ABI.
//
// A device stages the radiance and statistics word of every path of a launch in one of kStageSets STAGE SETS (20 bytes per
// pixel and iteration).  A call of n iterations is cut into launches of at most `cap` (the context's iterations per launch,
// which keeps one launch's staging within 4 GiB) and a remainder.  A launch of kShortLaunch or more iterations runs on the main
// stream and stages into set 0; a SHORT one, where the launch streams may overlap, runs on a stream of its own and takes
// whichever set comes next - any of them.  Below a cap of kShortLaunch every launch is short.  A launch AHEAD of the caller (one that renders the next calls
// before they come) is short too, and renders for up to kAheadIterations / n calls, never more than cap iterations.
#pragma once

#include <cstdint>

namespace ptmi_internal {

constexpr int kStageSets = 4;
constexpr uint32_t kShortLaunch = 4;      // launches of fewer iterations run beside their neighbours, on any set
constexpr uint32_t kAheadIterations = 4;  // iterations of a launch ahead at most (calls x iterations per call)

// Iterations the stage sets must hold for one call.
struct StageNeed {
    uint32_t set0;    // set 0: the call's longest launch
    uint32_t others;  // sets 1 .. kStageSets-1 (0: the call has no short launch, set 0 is the only one it uses): its longest short launch
    uint32_t ahead;   // every set, set 0 included, where the device has the memory: launches ahead of the caller (0: none).  A launch
                      // ahead renders for as many calls as its set holds, so where `ahead` cannot be allocated `others` must do
};

inline uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// n: iterations of the call (>= 1); cap: iterations per launch (>= 1); may_overlap: short launches get streams and sets of their
// own; can_run_ahead / continues: launches ahead of the caller are wanted and its calls have been seen to follow one another.
inline StageNeed stage_need(uint32_t n, uint32_t cap, bool may_overlap, bool can_run_ahead, bool continues)
{
    StageNeed need{min_u32(n, cap), 0u, 0u};
    // a launch is short when a full one is (cap < kShortLaunch) or the remainder is; either lands on any set
    const uint32_t rest = n % cap;
    const bool has_short = may_overlap && (min_u32(n, cap) < kShortLaunch || (rest != 0 && rest < kShortLaunch));
    if (!has_short) return need;
    need.others = min_u32(kShortLaunch - 1, cap);  // (no launch of this call exceeds cap: neither may the sets)
    if (can_run_ahead && continues) need.ahead = min_u32(kAheadIterations, cap);
    return need;
}

}  // namespace ptmi_internal
