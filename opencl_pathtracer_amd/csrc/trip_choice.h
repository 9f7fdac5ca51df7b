// trip_choice.h - what the next trip of the wavefront kernel's traversal loop is.
// HIP-free: kernel_wavefront.hip and the model of the tests (tests/trip_choice_model.cpp, which holds the forms the kernel had
// before this header as the specification and plays both over every state the loop can hold) compile this one copy.
//
// The choice, from what survey() counts of a wave's 64 lanes - n_t wait at a leaf with triangles pending, n_i stand at an inner
// node, n_p wait for path logic (dead lanes are none of the three) - and the wave's wait debt:
//   leave the loop for a path-logic pass  when path logic is due or nothing traverses,
//   else a leaf pass                      when a pass is due,
//   else a node trip.
// Each predicate is the former one under the conditions the loop guarantees where it is asked; the conditions stand beside it.
#pragma once

#include <cstdint>

#include "ptmi_hd.h"

namespace ptmi_trip {

// The smallest wait-debt bound a launch may carry (kernel_choice.h: choose_wavefront makes the bound, with_instance refuses a
// choice below this).  path_logic_due() rests on it: with a bound of 0 a wave none of whose lanes waits would run path-logic
// passes for ever.
constexpr uint32_t kMinWaitDebtBound = 1;
constexpr bool wait_debt_bound_is_valid(uint32_t bound) { return bound >= kMinWaitDebtBound; }

// Path logic is due.  Was `n_p > 0 && wait_debt >= bound`.  The debt is zeroed before every pass, grows by n_p in survey() and
// is asked right behind it; the loop leaves on the first trip that finds it at the bound.  So, bound >= 1, a debt at the bound
// was below it before this trip's n_p was added: n_p > 0 follows.
PTMI_HD constexpr bool path_logic_due(int wait_debt, int bound) { return wait_debt >= bound; }

// "Nothing traverses" stays in the kernel as it was, `n_t == 0 && n_i == 0`, in the loop's own lambda.  Two forms lost by count:
// from the OR of the survey's two ballots, `(b_t | b_n) == 0`, three scalar instructions fewer - and the compiler rotates the
// loop around it: the node step's record loads then issue in the order 16, 0, 48, 32 with vmcnt(2) as their first wait, a full
// vector-memory wait stands in front of them and the node trip has ten vector instructions more (tests/test_node_step_waits.py
// pins the order and the waits).  And the unchanged expression moved into a function of this header: inlined early, it
// reaches the same rotated loop, in every instantiation.

// Some lane is not dead for good.  Was `(m_t | m_i | m_p) != 0` with m_p = ~(b_t | b_n | b_dead).
PTMI_HD constexpr bool any_lane(unsigned long long b_t, unsigned long long b_n, unsigned long long b_dead)
{
    return ((b_t | b_n) | ~(b_t | b_n | b_dead)) != 0ull;
}

// A leaf pass is due: kLeafLanes lanes wait at a leaf, or the waiting triangles (three a lane) are kLeafRatio times as many as
// the lanes left at inner nodes.  Was `n_t >= kLeafLanes || (n_t > 0 && 3 * n_t >= kLeafRatio * n_i)`.  Asked only where
// something traverses (n_t + n_i > 0): there `3 * n_t >= kLeafRatio * n_i` with n_t == 0 would need n_i == 0, so n_t > 0
// follows, and both clauses are one compare against the smaller right side.
template <int kLeafLanes, int kLeafRatio>
PTMI_HD constexpr bool pass_is_due(int n_t, int n_i)
{
    static_assert(kLeafLanes >= 1 && kLeafRatio >= 1, "a pass without a waiting lane");
    const int ratio = kLeafRatio * n_i;
    return 3 * n_t >= (ratio < 3 * kLeafLanes ? ratio : 3 * kLeafLanes);
}

}  // namespace ptmi_trip
