// The stage-set rule of opencl_pathtracer_amd/csrc/stage_sets.h, tabulated for tests/test_stage_sets_model.py:
// one line "cap n may_overlap can_run_ahead continues set0 others ahead" per call, for every cap 1..max_cap, n 1..3*cap+5 and
// every combination of the three flags.
#include <cstdio>
#include <cstdlib>

#include "stage_sets.h"

int main(int argc, char** argv)
{
    const unsigned max_cap = argc > 1 ? (unsigned)std::atoi(argv[1]) : 32u;
    for (unsigned cap = 1; cap <= max_cap; cap++)
        for (unsigned n = 1; n <= 3 * cap + 5; n++)
            for (int flags = 0; flags < 8; flags++) {
                const bool may_overlap = flags & 1, can_run_ahead = flags & 2, continues = flags & 4;
                const ptmi_internal::StageNeed s = ptmi_internal::stage_need(n, cap, may_overlap, can_run_ahead, continues);
                std::printf("%u %u %d %d %d %u %u %u\n", cap, n, (int)may_overlap, (int)can_run_ahead, (int)continues, s.set0, s.others,
                            s.ahead);
            }
    return 0;
}
