// kernel_choice.h - which kernel a ptmi_render launch gets: the one-path-per-lane kernel (kernels.hip) or one of the seventeen
// instantiations of render_wavefront_kernel (kernel_wavefront.hip), and with which launch parameters.  HIP-free: the host units,
// kernel_wavefront.hip and the model of the tests (tests/kernel_choice_model.cpp, which plays every combination of the
// inputs) compile this one copy.  Three decisions, each a pure function of plain inputs and the developer switches of its
// moment (dev_switches.h):
//   choose_upload      what ptmi_initialize_memory writes into DScene besides pointers and copies
//   one_path_per_lane  the kernel kind, asked at upload and by every render call
//   choose_wavefront   the template arguments and launch parameters of one wavefront launch; with_instance() then finds
//                      the instantiation, of those that exist (kInstances: the list is written once, here)
#pragma once

#include <cstddef>
#include <cstdint>

#include "dev_switches.h"
#include "leaf_cull.h"
#include "ptmi_internal.h"
#include "trip_choice.h"

namespace ptmi_choice {

using ptmi_internal::DScene;
using ptmi_switches::Switches;

// ---- inputs -----------------------------------------------------------------------------------------------------------------
// what the decisions read of a scene's layout (scene_layout.h: Relayout)
struct LayoutTraits {
    bool tris_precomputed, plain_shading;  // after their switches (below): the layout builds its records by the first
    bool boxes_ordered;
    bool nan_records;  // literal_kernel_reason is not empty: the records can yield NaN distances
    uint32_t cullable_leaves;
    size_t n_records;
    uint32_t nan_walk_box_tests, nan_walk_tri_tests, nan_walk_last_tri;
};
// ... and of the context (ptmi_config, and PTMI_LEAF_CULL as ptmi_setup_context read it: -1 = unset)
struct ContextTraits {
    uint32_t sampler, flags, super_sampling, lights_size;
    int leaf_cull;
};

// ---- at upload ----------------------------------------------------------------------------------------------------------------
// The two traits the layout itself needs while it runs (scene_layout.cpp): what the scene allows, unless switched off.
inline bool tris_precomputed_after_switch(bool scene_allows, const Switches& upload) { return scene_allows && !upload.generic_triangles; }
inline bool plain_shading_after_switch(bool scene_allows, const Switches& upload) { return scene_allows && !upload.generic_shading; }

// DScene::plain_shading of a scene: every material a plain-colour PTMI_MAT_STANDART and every light a PTMI_LIGHT_POINT, unless
// switched off.  One per entry of the arrays: a material's type and whether it is a plain colour, a light's type - what
// build_layout reads off the caller's records (scene_layout.cpp) and what a context keeps of them, so that an edit of the
// materials or the lights (ptmi_update_materials, ptmi_update_lights) asks the upload's own rule again.
inline bool scene_plain_shading(const int32_t* material_type, const uint8_t* material_is_simple_color, size_t n_materials,
                                const int32_t* light_type, size_t n_lights, const Switches& upload)
{
    bool plain = plain_shading_after_switch(true, upload);
    for (size_t i = 0; i < n_materials && plain; i++)
        if (material_type[i] != PTMI_MAT_STANDART || !material_is_simple_color[i]) plain = false;
    for (size_t i = 0; i < n_lights && plain; i++)
        if (light_type[i] != PTMI_LIGHT_POINT) plain = false;
    return plain;
}

// PTMI_LEAF_CULL as the context keeps it: 0, 1, 2 or 3 (anything else reads as 1, as it always did); -1 = unset
inline int leaf_cull_setting(const Switches& setup)
{
    if (setup.leaf_cull == ptmi_switches::kUnset) return -1;
    return setup.leaf_cull == '0' ? 0 : setup.leaf_cull == '2' ? 2 : setup.leaf_cull == '3' ? 3 : 1;
}

// The chosen fields of DScene (the others are pointers, sizes and copies of the configuration: upload_scene).
inline void choose_upload(const LayoutTraits& lay, const ContextTraits& ctx, const Switches& upload, DScene& ds)
{
    ds.super_sampling = ctx.super_sampling ? 1u : 0u;
    ds.n_lights = ctx.lights_size;
    ds.sampler = ctx.sampler;
    ds.russian_roulette = (ctx.flags & PTMI_FLAG_RUSSIAN_ROULETTE) ? 1u : 0u;
    ds.source_seed = (ctx.flags & PTMI_FLAG_SOURCE_SEED) ? 1u : 0u;
    ds.tris_precomputed = lay.tris_precomputed ? 1u : 0u;
    ds.plain_shading = lay.plain_shading ? 1u : 0u;
    ds.wide_records = (lay.n_records > (1u << 26) || upload.wide_records) ? 1u : 0u;
    ds.nan_safe = lay.nan_records ? 1u : 0u;
    ds.nan_walk_box_tests = lay.nan_walk_box_tests; ds.nan_walk_tri_tests = lay.nan_walk_tri_tests; ds.nan_walk_last_tri = lay.nan_walk_last_tri;
    if (upload.walk_nan_rays) ds.nan_walk_box_tests = ds.nan_walk_tri_tests = 0xFFFFFFFFu;
    ds.boxes_ordered = (lay.boxes_ordered && !upload.generic_boxes) ? 1u : 0u;
    // (the records carry cull bits exactly when they are precomputed and their distances are numbers: scene_layout.cpp)
    // The culling instantiation pays two box distances per node step (+47 VALU instructions of 283 in the loop) and gets them back
    // where rays walk through leaves behind their hits: 1M triangles +3.5 %, 4M +10 %; in the Cornell box, where what a ray hits
    // is the last thing along it, nothing is culled and the kernel LOSES 4.5 %.  So a scene of few leaves keeps the
    // kernel without the code.  A threshold, not a prediction: a large scene of closed rooms would still pay for nothing.
    constexpr uint32_t kCullMinLeaves = 1024;
    const bool cull_bits = lay.tris_precomputed && !lay.nan_records;
    const bool cull = ctx.leaf_cull < 0 ? lay.cullable_leaves >= kCullMinLeaves : ctx.leaf_cull != 0;
    // (forced to 1, the kernel culls only the leaves a node step chooses itself - A/B against the pushed ones in one binary;
    // forced to 3, it culls as with 2 but honours the tight certificate alone - A/B against the wide tier.  The gate counts
    // the leaves of either tier: LayoutTraits::cullable_leaves.)
    ds.leaf_cull = (cull && cull_bits) ? (ptmi_cull::kCullChild1 | ptmi_cull::kCullChild2 | (ctx.leaf_cull == 1 ? 0u : ptmi_cull::kCullPushed) |
                                          (ctx.leaf_cull == 3 ? ptmi_cull::kCullTightOnly : 0u))
                                       : 0u;
}

// ---- the kernel kind ----------------------------------------------------------------------------------------------------------
// one path per lane (kernels.hip) instead of the wavefront kernel: asked for, or needed by the scene - records that can yield
// NaN distances rendered with the RANDOM sampler, whose samples are not staged, so that a path the wavefront kernel gives up
// could not be traced again; with the other samplers such a scene runs the wavefront kernel's NANSAFE instantiation
// (PTMI_LITERAL_KERNEL=1: the one-path-per-lane kernel as a whole, as before round 4, for A/B runs)
inline bool one_path_per_lane(const ContextTraits& ctx, bool nan_records, const Switches& kernel_kind)
{
    if ((ctx.flags & PTMI_FLAG_MEGAKERNEL) != 0) return true;
    if (!nan_records) return false;
    return ctx.sampler == PTMI_SAMPLER_RANDOM || kernel_kind.literal_kernel == '1';
}

// ---- one wavefront launch -----------------------------------------------------------------------------------------------------
// kernel_wavefront.hip holds these with the kernel and asserts that they agree
constexpr int kWideBlock = 256, kNarrowBlock = 64;  // lanes per workgroup (kWfBlock, kWfBlockNarrow)
constexpr uint32_t kMaxStackLevels = PTMI_BVH_MAX_DEPTH;
constexpr uint32_t kLdsWordsBesideStack = 1 + 4 + 4;  // per lane: sentinel, closest-hit record, keys and items of the leaf passes

struct WavefrontChoice {
    bool stats, pre, ss, plain, nansafe;  // render_wavefront_kernel's template arguments, in its order ...
    int block;
    bool cull;
    uint32_t stack_levels;  // ... and the launch's: the tree depth, clamped to [1, kMaxStackLevels]
    uint32_t wait_debt;     // DWarm::wait_debt
    size_t lds_bytes;       // dynamic LDS of a workgroup
};

inline uint32_t clamp_levels(uint32_t stack_levels)
{
    if (stack_levels < 1) stack_levels = 1;
    if (stack_levels > kMaxStackLevels) stack_levels = kMaxStackLevels;
    return stack_levels;
}

inline size_t wavefront_lds_bytes(uint32_t stack_levels, int block)
{
    // closest-hit record + sentinel + stack (+ the keys and items of the leaf passes), per lane of the workgroup
    return (size_t)(clamp_levels(stack_levels) + kLdsWordsBesideStack) * block * sizeof(uint32_t);
}

// Which instantiation a launch gets, of those that exist.  The common case (no statistics, no adaptive sampling, records
// that cannot yield NaN distances) pays for none of them; the statistics and SUPER_SAMPLING builds always carry the NaN check
// (two instructions per accepted triangle) and, over precomputed records, the culling code (they mask the bits with a scalar).
// `plain`: see the kernel's PLAIN (it implies precomputed records).  The narrow form (kNarrowBlock lanes): only the production
// instantiations, for trees so deep that the wide workgroup's LDS no longer fits five times into a CU - `five_wide_fit` is
// the device's answer (kernel_wavefront.hip asks it once per device and depth).
inline WavefrontChoice choose_wavefront(const DScene& sc, bool scheduler_stats, uint32_t tree_depth, bool five_wide_fit, const Switches& launch)
{
    WavefrontChoice c{};
    c.stack_levels = clamp_levels(tree_depth);
    c.stats = sc.super_sampling || scheduler_stats;
    c.pre = sc.tris_precomputed != 0;
    c.ss = sc.super_sampling != 0;
    c.plain = sc.tris_precomputed && sc.plain_shading && sc.sampler == PTMI_SAMPLER_JITTERED && !sc.russian_roulette && sc.n_lights == 1 &&
              !sc.super_sampling && !scheduler_stats;
    c.nansafe = c.stats || sc.nan_safe != 0;
    const bool production = !c.nansafe;
    // (the host clears leaf_cull where culling is off or cannot pay: choose_upload)
    c.cull = c.pre && (c.stats || (production && sc.leaf_cull != 0u));
    const bool narrow = !five_wide_fit && !launch.wide_workgroups;  // (PTMI_WIDE_WORKGROUPS: developer switch, A/B runs)
    c.block = production && c.pre && narrow ? kNarrowBlock : kWideBlock;
    // lane-trips of waiting a wave tolerates before it spends a pass on path logic: 768 from tree depth 16 on, below that
    // 512 (general path logic) or 320 (plain scenes: the cheaper a pass, the sooner it pays).  A launch parameter since
    // round 2; the sweeps that chose it, on MI355X (Msamples/s: 1M triangles 1080p depth 22 / Cornell box 1080p d8 depth 5 /
    // material mix 4K d16):
    //   round 2, plain-scene specialisation (first two scenes):  192: - / 6360 / 2193    256: - / 6620 / 2317    320: - / 6670 / 2403
    //                           384: - / 6600 / 2442    512: 960 / 6430 / 2491    640: 963 / 6190 / -    768: 976 / - / -    1024: 959 / - / -
    //   round 2, leaf passes:   512: 885 / 5388 / 2344    768: 895 / 5172 / 2314    1024: 895 / 5121 / 2235
    //   round 1's mixed trips (every traversing lane one step per trip, node or triangle: what leaf passes replaced):
    //                           256: - / 4883 / 1876    384: 733 / - / 1969    512: 740 / 4804 / 1986    768: 742 / 4896 / 1944
    //                           1024: 737 / 4845 / 1872    2048: - / 4840 / 1718
    // (a fixed threshold of 8 waiting lanes instead of a debt measured 474 / 743 with an early build)
    // (Never 0: the kernel asks "is path logic due" as `debt >= bound` alone, trip_choice.h, and a bound of 0 is due with no
    // lane waiting - a wave that runs passes for ever.  Checked here where the bound is made; with_instance refuses a choice
    // whose bound was set to 0 behind this function's back.)
    constexpr uint32_t kWaitDebtDeep = 768, kWaitDebtPlain = 320, kWaitDebtGeneral = 512;
    static_assert(ptmi_trip::wait_debt_bound_is_valid(kWaitDebtDeep) && ptmi_trip::wait_debt_bound_is_valid(kWaitDebtPlain) &&
                  ptmi_trip::wait_debt_bound_is_valid(kWaitDebtGeneral), "trip_choice.h: path_logic_due needs a bound of at least 1");
    c.wait_debt = c.stack_levels >= 16u ? kWaitDebtDeep : (c.plain ? kWaitDebtPlain : kWaitDebtGeneral);
    c.lds_bytes = wavefront_lds_bytes(c.stack_levels, c.block);
    return c;
}

// ---- the instantiations that exist --------------------------------------------------------------------------------------------
// An instantiation is named by the arguments that are ON (wide and everything else off: 0).
enum InstanceBits : unsigned { kStats = 1, kPre = 2, kSs = 4, kPlain = 8, kNanSafe = 16, kNarrow = 32, kCull = 64 };

template <unsigned BITS>
struct Instance {
    static constexpr unsigned bits = BITS;
    static constexpr bool stats = (BITS & kStats) != 0, pre = (BITS & kPre) != 0, ss = (BITS & kSs) != 0, plain = (BITS & kPlain) != 0,
                          nansafe = (BITS & kNanSafe) != 0, cull = (BITS & kCull) != 0;
    static constexpr int block = (BITS & kNarrow) ? kNarrowBlock : kWideBlock;
};

inline unsigned instance_bits(const WavefrontChoice& c)
{
    return (c.stats ? kStats : 0u) | (c.pre ? kPre : 0u) | (c.ss ? kSs : 0u) | (c.plain ? kPlain : 0u) | (c.nansafe ? kNanSafe : 0u) |
           (c.block == kNarrowBlock ? kNarrow : 0u) | (c.cull ? kCull : 0u);
}

template <unsigned... BITS>
struct InstanceList {
    static constexpr unsigned bits[sizeof...(BITS)] = {BITS...};
};
// THE list: every render_wavefront_kernel<...> the library holds is here, and a launch can get no other.
using Instances = InstanceList<
    0u,  // production, generic triangle records
    kPre,  // production, general shading
    kPre | kNarrow,
    kPre | kCull,
    kPre | kNarrow | kCull,
    kPre | kPlain,  // production, plain: the common case, BASELINE's untextured scenes among them
    kPre | kPlain | kNarrow,
    kPre | kPlain | kCull,
    kPre | kPlain | kNarrow | kCull,
    kNanSafe,  // records that can yield NaN distances
    kPre | kNanSafe,
    kPre | kPlain | kNanSafe,
    kStats | kNanSafe,  // scheduler statistics
    kStats | kPre | kNanSafe | kCull,
    kStats | kSs | kNanSafe,  // SUPER_SAMPLING
    kStats | kPre | kSs | kNanSafe | kCull>;

template <class F, unsigned... BITS>
bool with_instance_of(unsigned bits, F&& f, InstanceList<BITS...>)
{
    return ((bits == BITS ? (f(Instance<BITS>{}), true) : false) || ...);
}
// Calls f(Instance<...>{}) for the instantiation `c` names and returns true; false - and no call - where the list does not
// hold it, or the choice carries a wait-debt bound the kernel cannot run with (trip_choice.h): the caller's error, never a
// neighbouring instantiation.
template <class F>
bool with_instance(const WavefrontChoice& c, F&& f)
{
    if (c.block != kWideBlock && c.block != kNarrowBlock) return false;
    if (!ptmi_trip::wait_debt_bound_is_valid(c.wait_debt)) return false;
    return with_instance_of(instance_bits(c), f, Instances{});
}

}  // namespace ptmi_choice
