// trip_choice_model.cpp - csrc/trip_choice.h played on the CPU against the forms the wavefront kernel had before the header
// (tests/test_trip_choice_model.py).  The `spec_*` functions are those forms, copied: the specification.
//   choice    every (n_t, n_i, n_p) with n_t + n_i + n_p <= 64, every bound of BOUNDS, every debt the loop can hold
//   masks     any_lane over lane masks
//   sequence  random runs of surveys from a reset debt: the sequence leave / pass / step
//   bound     a wait-debt bound of 0 is refused where the bound is made (kernel_choice.h)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "kernel_choice.h"
#include "trip_choice.h"

using namespace ptmi_internal;

constexpr int kLeafLanes = 19, kLeafRatio = 2;  // PTMI_WF_LEAF_LANES, PTMI_WF_LEAF_RATIO (kernel_wavefront.hip)
static const int BOUNDS[] = {1, 64, 320, 512, 768};

// ---- the loop's predicates as the kernel wrote them -----------------------------------------------------------------------
static bool spec_path_logic_due(int n_p, int wait_debt, int bound) { return n_p > 0 && wait_debt >= bound; }
static bool spec_nothing_traverses(int n_t, int n_i) { return n_t == 0 && n_i == 0; }
static bool spec_pass_is_due(int n_t, int n_i) { return n_t >= kLeafLanes || (n_t > 0 && 3 * n_t >= kLeafRatio * n_i); }
static bool spec_any_lane(unsigned long long b_t, unsigned long long b_n, unsigned long long b_dead)
{
    const unsigned long long m_t = b_t, m_i = b_n & ~b_t, m_p = ~(b_t | b_n | b_dead);
    return (m_t | m_i | m_p) != 0ull;
}

enum Choice { kLeave = 0, kPass = 1, kStep = 2 };
static Choice spec_choice(int n_t, int n_i, int n_p, int debt, int bound)
{
    if (spec_path_logic_due(n_p, debt, bound) || spec_nothing_traverses(n_t, n_i)) return kLeave;
    return spec_pass_is_due(n_t, n_i) ? kPass : kStep;
}
static Choice new_choice(int n_t, int n_i, int debt, int bound)
{
    if (ptmi_trip::path_logic_due(debt, bound) || spec_nothing_traverses(n_t, n_i)) return kLeave;  // (the second clause: unchanged in the kernel)
    return ptmi_trip::pass_is_due<kLeafLanes, kLeafRatio>(n_t, n_i) ? kPass : kStep;
}

static int run_choice()
{
    long long states = 0, bad = 0;
    for (int bound : BOUNDS)
        for (int n_t = 0; n_t <= 64; n_t++)
            for (int n_i = 0; n_t + n_i <= 64; n_i++)
                for (int n_p = 0; n_t + n_i + n_p <= 64; n_p++)
                    // the debt as it is asked, right behind `wait_debt += n_p`.  What the loop can hold: the debt before this
                    // survey was below the bound (the loop leaves on the first trip that finds it there, and a pass zeroes it)
                    for (int debt = n_p; debt <= bound + 64; debt++) {
                        if (debt - n_p >= bound) continue;
                        states++;
                        if (spec_choice(n_t, n_i, n_p, debt, bound) != new_choice(n_t, n_i, debt, bound)) {
                            if (bad++ < 10) std::printf("differs: bound %d n_t %d n_i %d n_p %d debt %d\n", bound, n_t, n_i, n_p, debt);
                        }
                    }
    std::printf("choice states %lld bad %lld\n", states, bad);
    return bad != 0;
}

static int run_masks()
{
    std::mt19937_64 rng(7);
    long long n = 0, bad = 0;
    auto one = [&](unsigned long long b_t, unsigned long long b_n, unsigned long long b_dead) {
        n++;
        if (spec_any_lane(b_t, b_n, b_dead) != ptmi_trip::any_lane(b_t, b_n, b_dead)) bad++;
    };
    const unsigned long long edge[] = {0ull, ~0ull, 1ull, 1ull << 63, 0xFFFFFFFFull, ~0ull << 32};
    for (auto a : edge) for (auto b : edge) for (auto c : edge) one(a, b, c);
    for (int i = 0; i < 200000; i++) {
        unsigned long long a = rng(), b = rng(), c = rng();
        if (i & 1) { a &= rng() & rng(); b &= rng() & rng(); c |= rng() | rng(); }  // (mostly dead waves)
        if (i & 2) { a &= ~c; b &= ~c; }                                            // (as the kernel has them: a dead lane holds neither)
        one(a, b, c);
        one(0ull, 0ull, c | ~(rng() & rng() & rng() & rng() & rng() & rng()));
    }
    std::printf("masks cases %lld bad %lld\n", n, bad);
    return bad != 0;
}

// One wave's life as the kernel's loop nest runs it: survey; leave when no lane is left; trips until the loop leaves; the debt
// zeroed; a pass; survey again.  `surveys` is what each survey() counts, the same list for both forms.
struct Survey { int n_t, n_i, n_p; };
template <class ChoiceFn>
static std::vector<int> play(const std::vector<Survey>& surveys, int bound, ChoiceFn&& choice)
{
    std::vector<int> out;
    int debt = 0;
    for (const Survey& s : surveys) {
        debt += s.n_p;
        const Choice c = choice(s, debt, bound);
        out.push_back((int)c);
        if (c == kLeave) debt = 0;  // (wait_debt = 0 in front of the pass: the next survey is the first trip after it)
    }
    return out;
}

static int run_sequence()
{
    std::mt19937 rng(11);
    long long surveys_played = 0, bad = 0;
    long long kinds[3] = {0, 0, 0};
    for (int bound : BOUNDS)
        for (int run = 0; run < 400; run++) {
            std::vector<Survey> list;
            const int mood = run % 4;  // 0: anything, 1: few waiting lanes (long runs of trips), 2: mostly leaves, 3: draining wave
            for (int k = 0; k < 600; k++) {
                int live = mood == 3 ? (int)(rng() % 8u) : 64 - (int)(rng() % 9u);
                int n_p = mood == 1 ? (int)(rng() % 3u) : (int)(rng() % (unsigned)(live + 1));
                if (n_p > live) n_p = live;
                int rest = live - n_p;
                int n_t = mood == 2 ? rest - (int)(rng() % (unsigned)(rest / 4 + 1)) : (int)(rng() % (unsigned)(rest + 1));
                list.push_back(Survey{n_t, rest - n_t, n_p});
            }
            const std::vector<int> a = play(list, bound, [](const Survey& s, int debt, int b) { return spec_choice(s.n_t, s.n_i, s.n_p, debt, b); });
            const std::vector<int> b = play(list, bound, [](const Survey& s, int debt, int bd) { return new_choice(s.n_t, s.n_i, debt, bd); });
            surveys_played += (long long)list.size();
            for (size_t k = 0; k < a.size(); k++) {
                kinds[a[k]]++;
                if (a[k] != b[k]) bad++;
            }
        }
    std::printf("sequence surveys %lld leave %lld pass %lld step %lld bad %lld\n", surveys_played, kinds[0], kinds[1], kinds[2], bad);
    return bad != 0;
}

struct Nothing {
    template <class I>
    void operator()(I) const {}
};
static int run_bound()
{
    using namespace ptmi_choice;
    DScene ds{};
    ds.tris_precomputed = 1;
    WavefrontChoice c = choose_wavefront(ds, false, 22, true, ptmi_switches::Switches{});
    const bool runs = with_instance(c, Nothing{});
    const uint32_t made = c.wait_debt;
    c.wait_debt = 0;
    const bool refused = !with_instance(c, Nothing{});
    std::printf("bound made %u runs %d zero_refused %d zero_valid %d one_valid %d\n", made, (int)runs, (int)refused,
                (int)ptmi_trip::wait_debt_bound_is_valid(0), (int)ptmi_trip::wait_debt_bound_is_valid(1));
    return !(runs && refused);
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "choice")) return run_choice();
    if (!std::strcmp(mode, "masks")) return run_masks();
    if (!std::strcmp(mode, "sequence")) return run_sequence();
    if (!std::strcmp(mode, "bound")) return run_bound();
    std::fprintf(stderr, "usage: trip_choice_model choice|masks|sequence|bound\n");
    return 2;
}
