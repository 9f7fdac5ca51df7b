"""The stage sets of a ptmi_render call, planned on the host (csrc/stage_sets.h), checked without a GPU.

render_on_device cuts a call of n iterations into launches of at most `cap` (the context's iterations per launch) and a
remainder.  A launch of fewer than four iterations, where launches may overlap, runs on a stream of its own and stages into
whichever of the four stage sets comes next; any other launch stages into set 0.  A launch AHEAD of a caller that comes back
for one short call after the other renders for up to four iterations' worth of calls, never more than cap, on any set.
tests/stage_sets_model.cpp tabulates the rule for every cap 1..32, n 1..3 cap + 5 and every combination of its three flags;
this file cuts each call into launches as render_on_device does and checks that every launch fits every set it can land on,
that no set is sized beyond the cap (the cap keeps one launch's staging within 4 GiB), and that from a cap of four on the rule
is the one it replaced.  It also checks that the replaced rule fails these checks below a cap of four: sets 1..3 stayed
unallocated where every launch of a call is short, and a short launch then staged into a null array.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "stage_sets_model.cpp")
K_SHORT, K_AHEAD, K_SETS, MAX_CAP = 4, 4, 4, 32


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{(cap, n, may_overlap, can_run_ahead, continues): (set0, others, ahead)} from stage_need()"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    exe = str(tmp_path_factory.mktemp("stage_sets") / "stage_sets_model")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "opencl_pathtracer_amd", "csrc"), MODEL_SRC, "-o", exe], check=True)
    out = subprocess.run([exe, str(MAX_CAP)], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        cap, n, mo, ra, co, set0, others, ahead = map(int, line.split())
        rows[cap, n, bool(mo), bool(ra), bool(co)] = (set0, others, ahead)
    return rows


def old_rule(cap, n, may_overlap, can_run_ahead, continues):
    """What render_on_device allocated before stage_sets.h: sets 1..3 only where the REMAINDER n % cap was short."""
    rest = n % cap
    if may_overlap and rest != 0 and rest < K_SHORT:
        return min(n, cap), K_SHORT - 1, (K_AHEAD if can_run_ahead and continues else 0)
    return min(n, cap), 0, 0


def held(need, room_for_ahead):
    """What each set holds after the call's allocations (from nothing; they only ever grow): set 0 the longest launch, the
    others the longest short one; every set the launches ahead where the device has room for them, else the short size."""
    set0, others, ahead = need
    sets = [set0] + [0] * (K_SETS - 1)
    if others:
        size = max(ahead, others) if room_for_ahead else others
        for i in range(0 if ahead else 1, K_SETS):
            sets[i] = max(sets[i], size)
    return sets


def launches(n, cap):
    done = 0
    while done < n:
        m = min(n - done, cap)
        yield m
        done += m


def violations(key, need):
    cap, n, may_overlap, can_run_ahead, continues = key
    out = []
    if max(need) > cap:
        out.append(f"a set sized {max(need)} iterations beyond the cap {cap}")
    for room in (True, False):
        sets = held(need, room)
        for m in launches(n, cap):
            for s in (range(K_SETS) if may_overlap and m < K_SHORT else [0]):
                if sets[s] < m:
                    out.append(f"a launch of {m} may land on set {s}, which holds {sets[s]}")
        # a launch ahead, as long as render_on_device would make it before it looks at the set (the product only runs ahead of
        # calls of fewer than four iterations on launch streams of their own: can_run_ahead implies both)
        if can_run_ahead and continues and may_overlap and n < K_SHORT:
            calls = K_AHEAD // n
            if calls * n > cap:
                calls = cap // n
            if calls >= 1:
                want = calls * n if room else n  # (without room: as many calls as the set holds, at least one)
                for s in range(K_SETS):
                    if sets[s] < want:
                        out.append(f"a launch ahead of {calls} x {n} lands on set {s}, which holds {sets[s]}")
    return out


def keys():
    for cap in range(1, MAX_CAP + 1):
        for n in range(1, 3 * cap + 6):
            for flags in range(8):
                yield cap, n, bool(flags & 1), bool(flags & 2), bool(flags & 4)


def test_the_table_is_complete(table):
    assert sorted(table) == sorted(keys())


def test_every_launch_fits_every_set_it_can_land_on(table):
    bad = {key: v for key in keys() if (v := violations(key, table[key]))}
    assert not bad, f"{len(bad)} calls, e.g. " + "; ".join(f"{k}: {v[0]}" for k, v in list(bad.items())[:6])


def test_calls_without_a_short_launch_use_set_0_alone(table):
    for key in keys():
        cap, n, may_overlap = key[:3]
        short = may_overlap and any(m < K_SHORT for m in launches(n, cap))
        assert (table[key][1] != 0) == short, key
        assert table[key][2] == 0 or short, key


def test_unchanged_from_a_cap_of_four_on(table):
    """The 1080p paths (cap 32) and every other cap >= 4 allocate what they did."""
    for key in keys():
        if key[0] >= K_SHORT:
            assert table[key] == old_rule(*key), key


def test_the_old_rule_fails_below_a_cap_of_four():
    """The checks above catch the rule stage_sets.h replaced, at every cap below four and at no other."""
    for cap in range(1, MAX_CAP + 1):
        bad = [key for key in keys() if key[0] == cap and violations(key, old_rule(*key))]
        assert bool(bad) == (cap < K_SHORT), cap
    # the calls of the issue: cap 3, a call of 3 (its one launch may take set 1, never allocated); cap 2, a call of 4 (two
    # short launches); cap 1, any call
    for key in ((3, 3, True, False, False), (2, 4, True, False, False), (1, 1, True, False, False), (1, 1, True, True, True)):
        assert any("which holds 0" in v for v in violations(key, old_rule(*key))), key
    # ... and where it did allocate below a cap of four, it sized the sets beyond the cap
    assert any("beyond the cap" in v for v in violations((2, 3, True, True, True), old_rule(2, 3, True, True, True)))
