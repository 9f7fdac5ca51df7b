"""The launches of ptmi_render calls, planned on the host (csrc/launch_schedule.h, csrc/stage_sets.h), checked without a GPU.

render_on_device cuts a call of n iterations into launches of at most `cap` (the context's iterations per launch) and a
remainder.  A launch of fewer than four iterations, where launches may overlap, runs on a stream of its own and stages into
whichever of the four stage sets comes next; any other launch stages into set 0.  A launch AHEAD of a caller that comes back
for one short call after the other renders for up to four iterations' worth of calls, never more than cap, on any set.
tests/launch_schedule_model.cpp plays calls through the header and allocates the sets as render_on_device does.

This file checks, from what the scheduler decided:
- stage_need() for every cap 1..32, n 1..3 cap + 5 and every combination of its flags: every launch and launch ahead fits every
  set it can land on, no set is sized beyond the cap (the cap keeps one launch's staging within 4 GiB), and from a cap of four
  on the rule is the one it replaced.  The replaced rule fails these checks below a cap of four: sets 1..3 stayed unallocated
  where every launch of a call is short, and a short launch then staged into a null array.
- that the scheduler decides what render_on_device decided before the scheduler was taken out of it (ParentDevice below, a
  transcription), call for call, on the sequences of test_render_ahead_gpu.py and on a few thousand random ones;
- invariants of those decisions: every id rendered once and in order, an adopted part is what its launch rendered for that
  call, no new launch on a set a launch ahead holds, launches ahead within min(4, cap) iterations and 32-bit ids, and only
  ahead of a caller that continues and waits.
"""
import os
import random
import subprocess

import pytest

import model_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "launch_schedule_model.cpp")
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
K_SHORT, K_AHEAD, K_SETS, MAX_CAP = 4, 4, 4, 32
U32 = 0xFFFFFFFF


def _compile(tmp, sanitize=()):
    return model_build.program([MODEL_SRC], tmp, "launch_schedule_model", opt="-O1", werror=True, sanitize=sanitize, includes=[CSRC])


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("launch_schedule"))


def parse_calls(out):
    """driver output -> list of events: "ctx" | "forget" | dict(need, caps, held, steps, ahead)"""
    events, cur = [], None
    for line in out.splitlines():
        w = line.split()
        if w[0] in ("ctx", "forget"):
            events.append(w[0])
        elif w[0] == "key":
            cur = {"key": tuple(map(int, w[1:]))}
        elif w[0] == "need":
            cur = {**(cur or {}), "need": tuple(map(int, w[1:])), "steps": [], "ahead": []}
        elif w[0] == "caps":
            cur["caps"] = list(map(int, w[1:]))
        elif w[0] == "held":
            cur["held"] = list(map(int, w[1:]))
        elif w[0] == "step":
            cur["steps"].append((w[1], *map(int, w[2:])))
        elif w[0] == "ahead":
            cur["ahead"].append(tuple(map(int, w[1:])))
        elif w[0] == "end":
            events.append(cur)
            cur = None
    return events


# ---------------------------------------------------------------------------------------------------------------------------
# stage_need() over every cap, n and flag combination

@pytest.fixture(scope="module")
def table(model):
    """[(key, call)] for every (cap, n, may_overlap, ahead_allowed, continues, room, start set)"""
    out = subprocess.run([model, "table", str(MAX_CAP)], check=True, capture_output=True, text=True).stdout
    return [(c["key"], c) for c in parse_calls(out)]


@pytest.fixture(scope="module")
def needs(table):
    """{(cap, n, may_overlap, can_run_ahead, continues): (set0, others, ahead)} from stage_need(), as render_on_device calls it"""
    rows = {}
    for key, c in table:
        cap, n, mo, allowed, co = key[:5]
        k = (cap, n, bool(mo), bool(mo and allowed and n < K_SHORT), bool(co))
        assert rows.setdefault(k, c["need"]) == c["need"], k
    return rows


def stage_need(cap, n, may_overlap, can_run_ahead, continues):
    """stage_need() as the parent commit has it (csrc/stage_sets.h, unchanged)"""
    rest = n % cap
    if not (may_overlap and (min(n, cap) < K_SHORT or 0 < rest < K_SHORT)):
        return min(n, cap), 0, 0
    return min(n, cap), min(K_SHORT - 1, cap), (min(K_AHEAD, cap) if can_run_ahead and continues else 0)


def old_rule(cap, n, may_overlap, can_run_ahead, continues):
    """What render_on_device allocated before stage_need(): sets 1..3 only where the REMAINDER n % cap was short."""
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


def violations(call, need, cap, room):
    """The scheduler's launches of one call against the sets `need` allocates: (set, iterations) of every launch and launch ahead."""
    out = []
    if max(need) > cap:
        out.append(f"a set sized {max(need)} iterations beyond the cap {cap}")
    sets = held(need, room)
    for kind, s, first, m, part in call["steps"]:
        if sets[s] < m:
            out.append(f"a launch of {m} lands on set {s}, which holds {sets[s]}")
    for s, first, n, calls in call["ahead"]:
        if sets[s] < n * calls:
            out.append(f"a launch ahead of {calls} x {n} lands on set {s}, which holds {sets[s]}")
    return out


def test_the_table_is_complete(table, needs):
    keys = {(cap, n, bool(f & 1), bool(f & 2), bool(f & 4), room, start) for cap in range(1, MAX_CAP + 1) for n in range(1, 3 * cap + 6)
            for f in range(8) for room in (0, 1) for start in range(K_SETS)}
    assert {(k[0], k[1], bool(k[2]), bool(k[3]), bool(k[4]), k[5], k[6]) for k, _ in table} == keys and len(table) == len(keys)
    for k, need in needs.items():
        assert need == stage_need(*k), k


def test_every_launch_fits_every_set_it_can_land_on(table):
    """Every start of the round robin: a short launch lands on every set in turn.  The sets the driver allocated are the ones
    held() derives from the need, and every launch the scheduler made fits them."""
    bad = {}
    for key, c in table:
        cap, room = key[0], key[5]
        assert c["caps"] == held(c["need"], room), key
        if v := violations(c, c["need"], cap, room):
            bad[key] = v
    assert not bad, f"{len(bad)} calls, e.g. " + "; ".join(f"{k}: {v[0]}" for k, v in list(bad.items())[:6])
    # ... and launches ahead were made: at every cap, of as many calls as fit (four iterations, never more than the cap)
    most = {}
    for key, c in table:
        for s, first, n, calls in c["ahead"]:
            most[key[0]] = max(most.get(key[0], 0), n * calls)
    assert most == {cap: min(K_AHEAD, cap) for cap in range(1, MAX_CAP + 1)}
    # ... in every call that asks for room ahead and whose n fits a launch, with room and without: as many calls as the set holds
    # (with room min(4, cap) iterations' worth, without it the short size's worth), so that no allocation stops them silently
    for key, c in table:
        cap, n, room = key[0], key[1], key[5]
        if c["need"][2] and n <= cap:
            holds = min(K_AHEAD, cap) if room else min(K_SHORT - 1, cap)
            assert c["ahead"] and all(a_n * calls == holds // n * n for s, f, a_n, calls in c["ahead"]), (key, c)


def test_calls_without_a_short_launch_use_set_0_alone(needs):
    for key, need in needs.items():
        cap, n, may_overlap = key[:3]
        short = may_overlap and any(m < K_SHORT for m in launches(n, cap))
        assert (need[1] != 0) == short, key
        assert need[2] == 0 or short, key


def test_unchanged_from_a_cap_of_four_on(needs):
    """The 1080p paths (cap 32) and every other cap >= 4 allocate what they did."""
    for key, need in needs.items():
        if key[0] >= K_SHORT:
            assert need == old_rule(*key), key


def test_the_old_rule_fails_below_a_cap_of_four(table):
    """The checks above catch the rule stage_need() replaced, at every cap below four and at no other."""
    bad = {}
    for key, c in table:
        cap, n, mo, allowed, co, room, start = key
        old = old_rule(cap, n, bool(mo), bool(mo and allowed and n < K_SHORT), bool(co))
        if v := violations(c, old, cap, room):
            bad.setdefault(cap, []).append((key, v))
    assert sorted(bad) == [1, 2, 3]
    # the calls of the issue: cap 3, a call of 3 (its one launch may take set 1, never allocated); cap 2, a call of 4 (two
    # short launches); cap 1, any call
    for want in ((3, 3, 1, 0, 0), (2, 4, 1, 0, 0), (1, 1, 1, 0, 0), (1, 1, 1, 1, 1)):
        assert any(k[:5] == want and any("which holds 0" in x for x in v) for k, v in bad[want[0]]), want
    # ... and where it did allocate below a cap of four, it sized the sets beyond the cap
    assert any(k[:5] == (2, 3, 1, 1, 1) and any("beyond the cap" in x for x in v) for k, v in bad[2])


# ---------------------------------------------------------------------------------------------------------------------------
# call sequences: the scheduler against the parent commit's render_on_device

class ParentDevice:
    """The decisions of render_on_device as the parent commit made them (ptmi_api.cpp, DeviceState::ahead / streak / next_set /
    have_last), with the stage sets allocated as it allocated them.  A failed call and a re-binding forget what ran ahead and the
    last call, as free_scene_memory did."""

    def __init__(self, cap, super_sampling, depth, calls, stats_build):
        self.cap, self.ss, self.depth, self.calls_env, self.stats = cap, super_sampling, depth, calls, stats_build
        self.ahead = []  # [first, n, stride, set, calls, taken]
        self.streak = self.next_set = 0
        self.last = None
        self.stage_cap = [0] * K_SETS

    def forget(self):
        self.ahead.clear()
        self.last = None

    def pick_set(self):
        s = 0
        for _ in range(K_SETS):
            s = self.next_set % K_SETS
            self.next_set += 1
            if not any(a[3] == s for a in self.ahead):
                break
        return s

    def ensure(self, s, iterations, fails):
        if self.stage_cap[s] >= iterations:
            return True
        self.ahead = [a for a in self.ahead if a[3] != s]
        self.stage_cap[s] = 0 if fails else iterations
        return not fails

    def render(self, first, n, stride, may_overlap, ahead_allowed, caller_waits, small_only, fails):
        can_run_ahead = may_overlap and self.depth > 0 and ahead_allowed and n < K_SHORT
        if not can_run_ahead:
            self.ahead.clear()
        continues = self.last is not None and self.last[1] == n and self.last[2] == stride and self.last[0] + n * stride == first
        need = stage_need(self.cap, n, may_overlap, can_run_ahead, continues)
        out = ["need %d %d %d" % need]
        self.ensure(0, need[0], False)
        if need[1]:
            for i in range(0 if need[2] else 1, K_SETS):
                small, large = need[1], max(need[2], need[1])
                if not self.ensure(i, large, large > small and (small_only >> i) & 1):
                    self.ensure(i, small, False)
        out.append("caps %d %d %d %d" % tuple(self.stage_cap))
        steps = []
        done = 0
        while done < n:
            cap = 1 if self.ss else self.cap
            m = min(n - done, cap)
            f = first + done * stride
            if may_overlap and m < K_SHORT:
                found = False
                s = part = 0
                while can_run_ahead and self.ahead and not found:
                    a = self.ahead[0]
                    found = a[1] == m and a[2] == stride and a[0] + a[5] * a[1] * a[2] == f
                    s, part = a[3], a[5]
                    if not found:
                        self.ahead.pop(0)
                    else:
                        a[5] += 1
                        if a[5] == a[4]:
                            self.ahead.pop(0)
                if found:
                    steps.append("step A %d %d %d %d" % (s, f, m, part))
                else:
                    steps.append("step N %d %d %d 0" % (self.pick_set(), f, m))
            else:
                steps.append("step M 0 %d %d 0" % (f, m))
            done += m
        out.append(" ".join(["held"] + [str(a[3]) for a in self.ahead]))
        out += steps
        self.streak = self.streak + 1 if continues else 0
        if can_run_ahead and continues and caller_waits:
            nxt = first + n * stride if not self.ahead else self.ahead[-1][0] + self.ahead[-1][4] * n * stride
            untouched = len(self.ahead) - (1 if self.ahead and self.ahead[0][5] != 0 else 0)
            for _ in range(untouched, self.depth):
                calls = 1 if self.stats else self.calls_env
                if calls > K_AHEAD // n:
                    calls = K_AHEAD // n
                if calls * n > self.cap:
                    calls = self.cap // n
                if self.streak < 4 and calls > (1 << (self.streak - 1)):
                    calls = 1 << (self.streak - 1)
                while calls > 1 and nxt + (calls * n - 1) * stride > U32:
                    calls -= 1
                if calls < 1 or nxt + (n - 1) * stride > U32:
                    break
                s = self.pick_set()
                if n * calls > self.stage_cap[s]:
                    calls = self.stage_cap[s] // n
                if calls < 1:
                    break
                out.append("ahead %d %d %d %d" % (s, nxt, n, calls))
                self.ahead.append([nxt, n, stride, s, calls, 0])
                nxt += calls * n * stride
        if fails:
            self.forget()
        else:
            self.last = (first, n, stride)
        return out + ["end"]


def play_parent(lines):
    out, dev = [], None
    for line in lines:
        w = line.split()
        if w[0] == "ctx":
            dev = ParentDevice(*map(int, w[1:]))
            out.append("ctx")
        elif w[0] == "forget":
            dev.forget()
            out.append("forget")
        else:
            out += dev.render(*map(int, w[1:]))
    return out


def device_share(first, n, k, G):
    skip = (k + G - first % G) % G
    return first + skip, ((n - skip + G - 1) // G if skip < n else 0)


def gpu_test_sequences():
    """test_render_ahead_gpu.SEQUENCES as each device of a 1-3 device context sees them: a blocking caller (caller_waits)."""
    from test_render_ahead_gpu import SEQUENCES
    lines = []
    for name, seq in SEQUENCES.items():
        for G in (1, 2, 3):
            for depth in (0, 1, 2):  # (render_ahead_depth() clamps 3 to 2)
                for calls in (1, 2, 3, 4):
                    for k in range(G):
                        lines.append(f"ctx 32 0 {depth} {calls} 0")
                        for c in seq:
                            if c[0] != "render":
                                continue
                            f, m = device_share(c[1], c[2], k, G)
                            if m:
                                lines.append(f"call {f} {m} {G} 1 1 1 0 0")
    return lines


def random_sequences(seed, count):
    rng = random.Random(seed)
    lines = []
    for _ in range(count):
        cap = rng.choice([1, 2, 3, 4, 5, 8, 32, rng.randint(1, 32)])
        lines.append(f"ctx {cap} {int(rng.random() < 0.05)} {rng.randint(0, 2)} {rng.randint(1, 4)} {int(rng.random() < 0.15)}")
        stride = rng.randint(1, 3)
        first = rng.choice([0, rng.randint(0, 1000), U32 - rng.randint(0, 40)])
        n = rng.choice([1, 1, 1, 2, 3])
        last = None  # (first, n) of the call before
        for _ in range(rng.randint(5, 60)):
            r = rng.random()
            if r < 0.04:
                lines.append("forget")
                continue
            if r < 0.10:
                first = rng.randint(0, 2000)  # a jump
            elif r < 0.14:
                first = U32 - rng.randint(0, 40)  # near the end of the ids
            elif r < 0.20:
                pass  # a repeat
            elif r < 0.26:
                n = rng.choice([1, 2, 3, 4, 5, rng.randint(1, 70)])
            elif r < 0.28:
                stride = rng.randint(1, 3)
                if last and rng.random() < 0.7:
                    first, n = last[0] + last[1] * stride, last[1]  # where the new stride would continue the call before
            if first + (n - 1) * stride > U32:
                first = rng.randint(0, 1000)
            lines.append(f"call {first} {n} {stride} {int(rng.random() < 0.9)} {int(rng.random() < 0.9)} "
                         f"{int(rng.random() < 0.8)} {rng.randrange(16) if rng.random() < 0.15 else 0} {int(rng.random() < 0.03)}")
            last = (first, n)
            if rng.random() < 0.9 and first + (2 * n - 1) * stride <= U32:
                first += n * stride  # in order
    return lines


SEQUENCE_SETS = {"gpu_tests": gpu_test_sequences, "random": lambda: random_sequences(20261016, 3000)}


@pytest.fixture(scope="module", params=list(SEQUENCE_SETS))
def played(request, model):
    lines = SEQUENCE_SETS[request.param]()
    out = subprocess.run([model, "play"], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    return lines, out


def test_the_scheduler_decides_what_render_on_device_decided(played):
    lines, out = played
    got, want = out.splitlines(), play_parent(lines)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"output line {i}: scheduler {g!r}, parent commit {w!r}"


def test_invariants_of_the_schedule(played):
    lines, out = played
    events = parse_calls(out)
    inputs = [ln.split() for ln in lines]
    assert len(events) == len(inputs)
    launched_ahead, last, cap, n_ahead = {}, None, None, 0
    for inp, ev in zip(inputs, events):
        if inp[0] == "ctx":
            cap, last, launched_ahead = int(inp[1]), None, {}
            continue
        if inp[0] == "forget":
            last, launched_ahead = None, {}
            continue
        first, n, stride, mo, allowed, waits, small_only, fails = map(int, inp[1:])
        # every id of the call rendered once, in order
        ids = [s[2] + k * stride for s in ev["steps"] for k in range(s[3])]
        assert ids == [first + k * stride for k in range(n)], (inp, ev)
        held_sets = set(ev["held"])
        for kind, s, f, m, part in ev["steps"]:
            if kind == "A":
                # an adopted part is exactly the ids that launch rendered for this call
                a_first, a_n, a_calls, taken = launched_ahead[s]
                assert part < a_calls and part not in taken and a_n == m and f == a_first + part * a_n * stride, (inp, ev)
                taken.add(part)
            else:
                launched_ahead.pop(s, None)
                if kind == "N":
                    assert s not in held_sets, (inp, ev)
        continues = last is not None and last == (first - n * stride, n, stride)
        assert not ev["ahead"] or (continues and waits), (inp, ev)
        for s, f, a_n, calls in ev["ahead"]:
            # no new launch on a set a pending launch ahead holds
            assert s not in held_sets, (inp, ev)
            held_sets.add(s)
            assert a_n == n and 1 <= calls and a_n * calls <= min(K_AHEAD, cap) and f + (a_n * calls - 1) * stride <= U32, (inp, ev)
            launched_ahead[s] = (f, a_n, calls, set())
            n_ahead += 1
        last = None if fails else (first, n, stride)
        if fails:
            launched_ahead = {}
    assert n_ahead > 0  # (the sequences do run ahead)


def test_model_under_sanitizers(tmp_path):
    """The driver compiled with -fsanitize=address,undefined, over the table of small caps and the random sequences."""
    model_build.sanitizer_runtimes_or_skip()
    exe = _compile(tmp_path, ["-g", *model_build.SANITIZE])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1"}
    r = subprocess.run([exe, "table", "8"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.count("end\n") > 0, r.stderr[-3000:]
    lines = random_sequences(7, 500)
    r = subprocess.run([exe, "play"], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.splitlines() == play_parent(lines), r.stderr[-3000:]
