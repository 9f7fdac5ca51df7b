// kernel_choice_model.cpp - plays csrc/kernel_choice.h over every combination of its inputs (tests/test_kernel_choice_model.py
// compares the lines with the rules of the commit before the header existed).  No HIP, no device.  The developer switches are
// the process's environment, read through csrc/dev_switches.h at each decision's own moment, as the library reads them.
//   list     the instantiations the header holds, one line of seven template arguments each
//   switches the reader's table: name, parse, moment
//   upload   choose_upload over the layout traits the big table keeps fixed
//   table    upload -> kernel kind -> wavefront choice -> dispatch, one line per combination
#include <cstdio>
#include <cstring>

#include "kernel_choice.h"

using namespace ptmi_choice;
using ptmi_switches::Moment;
using ptmi_switches::read_switches;

namespace {

constexpr uint32_t kWalkBoxes = 11, kWalkTris = 22, kWalkLast = 33;

void print_upload(const DScene& ds)
{
    std::printf(" | %u %u %u %u %u %u %u %u %u", ds.tris_precomputed, ds.plain_shading, ds.wide_records, ds.boxes_ordered, ds.nan_safe,
                ds.nan_walk_box_tests, ds.nan_walk_tri_tests, ds.nan_walk_last_tri, ds.leaf_cull);
}

struct PrintInstance {
    template <class I>
    void operator()(I) const
    {
        std::printf("%d %d %d %d %d %d %d", (int)I::stats, (int)I::pre, (int)I::ss, (int)I::plain, (int)I::nansafe, I::block, (int)I::cull);
    }
};

template <unsigned... BITS>
void list(InstanceList<BITS...>)
{
    const PrintInstance print;
    ((print(Instance<BITS>{}), std::printf("\n")), ...);
}

DScene uploaded(bool nan, bool pre, bool plain, bool boxes, size_t n_records, uint32_t leaves, const ContextTraits& ctx)
{
    // the layout's part of the upload moment (scene_layout.cpp), then upload_scene's
    const ptmi_switches::Switches layout = read_switches(Moment::kUpload);
    const LayoutTraits lay{tris_precomputed_after_switch(pre, layout), plain_shading_after_switch(plain, layout), boxes, nan, leaves, n_records,
                           kWalkBoxes, kWalkTris, kWalkLast};
    DScene ds{};
    choose_upload(lay, ctx, read_switches(Moment::kUpload), ds);
    return ds;
}

}  // namespace

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "list")) {
        list(Instances{});
        return 0;
    }
    if (!std::strcmp(mode, "switches")) {
        for (const ptmi_switches::SwitchRow& row : ptmi_switches::kSwitchTable) std::printf("%s %d %d\n", row.name, (int)row.parse, (int)row.moment);
        return 0;
    }
    const int leaf_cull = leaf_cull_setting(read_switches(Moment::kSetup));  // as ptmi_setup_context keeps it
    const uint32_t leaves_of[3] = {0, 1023, 1024};
    if (!std::strcmp(mode, "upload")) {
        const size_t records_of[3] = {1, (size_t)1 << 26, ((size_t)1 << 26) + 1};
        for (int i = 0; i < 2 * 2 * 2 * 2 * 3 * 3; i++) {
            const bool nan = i & 1, pre = i & 2, plain = i & 4, boxes = i & 8;
            const int r = (i >> 4) % 3, l = (i >> 4) / 3;
            const ContextTraits ctx{PTMI_SAMPLER_JITTERED, 0u, 0u, 1u, leaf_cull};
            std::printf("%d %d %d %d %d %d %d", leaf_cull, (int)nan, (int)pre, (int)plain, (int)boxes, r, (int)leaves_of[l]);
            print_upload(uploaded(nan, pre, plain, boxes, records_of[r], leaves_of[l], ctx));
            std::printf("\n");
        }
        return 0;
    }
    if (std::strcmp(mode, "table")) return 2;
    const uint32_t samplers[3] = {PTMI_SAMPLER_JITTERED, PTMI_SAMPLER_UNIFORM, PTMI_SAMPLER_RANDOM};
    const uint32_t depths[7] = {1, 15, 16, 22, 23, PTMI_BVH_MAX_DEPTH, PTMI_BVH_MAX_DEPTH + 1};
    for (int bits = 0; bits < 128; bits++)
        for (int s = 0; s < 3; s++)
            for (uint32_t lights = 1; lights <= 2; lights++)
                for (uint32_t leaves : leaves_of)
                    for (uint32_t depth : depths)
                        for (int fit = 0; fit < 2; fit++) {
                            const bool ss = bits & 1, stats = bits & 2, nan = bits & 4, pre = bits & 8, plain = bits & 16, rr = bits & 32, mega = bits & 64;
                            const uint32_t flags = (rr ? PTMI_FLAG_RUSSIAN_ROULETTE : 0u) | (mega ? PTMI_FLAG_MEGAKERNEL : 0u);
                            const ContextTraits ctx{samplers[s], flags, ss ? 1u : 0u, lights, leaf_cull};
                            std::printf("%d %d %d %d %d %d %d %d %u %d %u %u %d", leaf_cull, (int)ss, (int)stats, (int)nan, (int)pre, (int)plain, s, (int)rr,
                                        lights, (int)mega, leaves, depth, fit);
                            const DScene ds = uploaded(nan, pre, plain, true, 1000, leaves, ctx);
                            print_upload(ds);
                            std::printf(" | %d", (int)one_path_per_lane(ctx, nan, read_switches(Moment::kKernelKind)));
                            const WavefrontChoice c = choose_wavefront(ds, stats, depth, fit != 0, read_switches(Moment::kLaunch));
                            std::printf(" | %d %d %d %d %d %d %d %u %u %zu | ", (int)c.stats, (int)c.pre, (int)c.ss, (int)c.plain, (int)c.nansafe, c.block,
                                        (int)c.cull, c.stack_levels, c.wait_debt, c.lds_bytes);
                            if (!with_instance(c, PrintInstance{})) std::printf("none");
                            std::printf("\n");
                        }
    // a choice the list does not hold is refused, not mapped onto a neighbour
    WavefrontChoice odd{};
    odd.plain = true;  // PLAIN without PRE
    odd.block = kWideBlock;
    WavefrontChoice odd_block{};
    odd_block.block = 128;
    std::printf("refused %d %d\n", (int)!with_instance(odd, PrintInstance{}), (int)!with_instance(odd_block, PrintInstance{}));
    return 0;
}
