// Plays ptmi_render calls through opencl_pathtracer_amd/csrc/launch_schedule.h for tests/test_launch_schedule_model.py, with the
// stage sets allocated as render_on_device allocates them.
//
//   launch_schedule_model table MAX_CAP   every cap 1..MAX_CAP, n 1..3*cap+5, may_overlap / ahead_allowed / continues, the sets
//                                         allocated with and without room for launches ahead, and every set the round robin
//                                         can start at: one line per call
//   launch_schedule_model play            call sequences from stdin, one line per event:
//       ctx CAP SUPER_SAMPLING DEPTH CALLS STATS_BUILD                          a new device
//       call FIRST N STRIDE MAY_OVERLAP AHEAD_ALLOWED CALLER_WAITS SMALL_ONLY FAILS  SMALL_ONLY: bit i = set i gets only the small
//                                                                               size; FAILS: the call fails once issued
//       forget                                                                  scene freed, accumulators re-bound
//     each call prints "need", "caps" (after allocation), "held" (the sets of the launches ahead after its own launches), its
//     "step"s, its launches "ahead" and "end".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "launch_schedule.h"

using namespace ptmi_internal;

namespace {

struct Device {
    LaunchSchedule s;
    size_t cap[kStageSets] = {};

    // ensure_stage_set: a set that grows loses its launches ahead; `small_only`: the large size cannot be allocated
    bool ensure(int set, size_t iterations, bool fails)
    {
        if (cap[set] >= iterations) return true;
        s.forget_set(set);
        cap[set] = fails ? 0 : iterations;
        return !fails;
    }
    void allocate(const StageNeed& need, unsigned small_only)
    {
        ensure(0, need.set0, false);
        for (int i = need.ahead ? 0 : 1; need.others && i < kStageSets; i++) {
            const size_t small = need.others, large = need.ahead > small ? need.ahead : small;
            if (!ensure(i, large, large > small && (small_only >> i & 1u))) ensure(i, small, false);
        }
    }
};

std::string render(Device& d, const Call& c, bool caller_waits, unsigned small_only, bool fails)
{
    std::string out;
    char buf[160];
    const StageNeed need = d.s.begin(c);
    std::snprintf(buf, sizeof buf, "need %u %u %u\n", need.set0, need.others, need.ahead);
    out += buf;
    d.allocate(need, small_only);
    std::snprintf(buf, sizeof buf, "caps %zu %zu %zu %zu\n", d.cap[0], d.cap[1], d.cap[2], d.cap[3]);
    out += buf;
    const std::vector<Step> steps = d.s.steps();
    out += "held";
    for (const LaunchSchedule::Ahead& a : d.s.ahead) out += " " + std::to_string(a.set);
    out += "\n";
    for (const Step& st : steps) {
        std::snprintf(buf, sizeof buf, "step %c %d %u %u %u\n", "MNA"[st.kind], st.set, st.first, st.n, st.part);
        out += buf;
    }
    for (const LaunchSchedule::Ahead& a : d.s.launches_ahead(caller_waits, d.cap)) {
        std::snprintf(buf, sizeof buf, "ahead %d %u %u %u\n", a.set, a.first, a.n, a.calls);
        out += buf;
    }
    if (!fails) d.s.commit();  // (a call that fails is never committed)
    return out + "end\n";
}

int table(unsigned max_cap)
{
    for (unsigned cap = 1; cap <= max_cap; cap++)
        for (unsigned n = 1; n <= 3 * cap + 5; n++)
            for (int flags = 0; flags < 8; flags++)
                for (int room = 0; room < 2; room++)
                    for (int start = 0; start < kStageSets; start++) {
                        const bool may_overlap = flags & 1, ahead_allowed = flags & 2, continues = flags & 4;
                        Device d;
                        d.s.next_set = (uint32_t)start;
                        if (continues) {  // a caller that has come back often enough for launches ahead of the most calls
                            d.s.have_last = true, d.s.last_first = 0, d.s.last_n = n, d.s.last_stride = 1, d.s.streak = 3;
                        }
                        const Call c{continues ? n : 0u, n, 1, cap, false, may_overlap, ahead_allowed, 2, kAheadIterations, false};
                        std::printf("key %u %u %d %d %d %d %d\n%s", cap, n, (int)may_overlap, (int)ahead_allowed, (int)continues, room,
                                    start, render(d, c, true, room ? 0u : 0xFu, false).c_str());
                    }
    return 0;
}

int play()
{
    Device d;
    Call c{};
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned a[8] = {};
        if (std::sscanf(line, "ctx %u %u %u %u %u", &a[0], &a[1], &a[2], &a[3], &a[4]) == 5) {
            d = Device{};
            c = Call{0, 0, 0, a[0], a[1] != 0, false, false, a[2], a[3], a[4] != 0};
            std::printf("ctx\n");
        } else if (std::sscanf(line, "call %u %u %u %u %u %u %u %u", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) == 8) {
            c.first = a[0], c.n = a[1], c.stride = a[2], c.may_overlap = a[3] != 0, c.ahead_allowed = a[4] != 0;
            std::fputs(render(d, c, a[5] != 0, a[6], a[7] != 0).c_str(), stdout);
        } else if (std::strncmp(line, "forget", 6) == 0) {
            d.s.forget();
            std::printf("forget\n");
        } else {
            std::fprintf(stderr, "bad line: %s", line);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "table") == 0) return table(argc > 2 ? (unsigned)std::atoi(argv[2]) : 32u);
    if (argc > 1 && std::strcmp(argv[1], "play") == 0) return play();
    std::fprintf(stderr, "usage: %s table [MAX_CAP] | play < events\n", argv[0]);
    return 2;
}
