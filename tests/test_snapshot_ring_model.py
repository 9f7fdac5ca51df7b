"""The bookkeeping of the ptmi_snapshot ring (csrc/snapshot_ring.h), checked without a GPU.

Every device of a context keeps as many snapshot BUFFERS as the ring has slots, and for every slot the buffer it shows.  A
snapshot copies the accumulators into a buffer; the images of a ptmi_render_snapshots call during which a device's accumulators
did not change all point at ONE copy; and a device other than devices[0] sends a snapshot to its landing buffer on devices[0]
only if that buffer does not hold it already.  tests/snapshot_ring_model.cpp plays calls through the header the way
snapshot_device, snapshots_up_to / render_on_device and gather_snapshot do, without the HIP calls.

This file gives the accumulators of a device a VERSION (every accumulation makes a new one) and lets a copy stamp its buffer with
the version it copied.  Over random sequences of snapshots, bursts on 1, 2 and 3 devices, renders, reads of slots and of the
image (the library's own slot) and scene resets, with six slots in use and with the whole ring (the two sizes of
test_api_fuzz_gpu.py), it checks from what the header decided:
 (a) every filled slot shows a buffer stamped with the version that was current when its snapshot was queued;
 (b) a buffer that two or more slots show is never written;
 (c) the choice of a buffer never fails;
 (d) buffer_refs[b] is the number of slots that show b, after every event;
 (e) a peer copy is skipped only where the landing buffer's stamp equals the source's;
and that the decisions are those of the code before the ring was taken out of ptmi_api.cpp (ParentDevice, a transcription),
event for event.  The same sequences run once more through the model built with -fsanitize=address,undefined.
"""
import os
import random
import subprocess
from collections import Counter

import pytest

import model_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "snapshot_ring_model.cpp")
INCLUDES = [os.path.join(ROOT, "opencl_pathtracer_amd", "csrc"), os.path.join(ROOT, "include")]
RING = 65  # PTMI_MAX_SNAPSHOT_SLOTS
USER_SLOTS = RING - 1
INTERNAL = RING - 1


def _compile(tmp, sanitize=()):
    return model_build.program([MODEL_SRC], tmp, "snapshot_ring_model", opt="-O1", werror=True, sanitize=sanitize, includes=INCLUDES)


def device_share(first, n, k, G):
    skip = (k + G - first % G) % G
    return first + skip, ((n - skip + G - 1) // G if skip < n else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the parent commit's code

class ParentDevice:
    """DeviceState's ring fields with point_slot, the buffer choice of snapshot_device, SnapshotPlan / snapshots_up_to as
    render_on_device drove them, the skip of gather_snapshot and the reset of free_scene_memory, as the parent commit had them
    in ptmi_api.cpp."""

    def __init__(self, k):
        self.k = k
        self.source_slot = [-1] * RING
        self.buffer_refs = [0] * RING
        self.snapshot_gen = [0] * RING
        self.landed_slot, self.landed_gen = -1, 0

    def point_slot(self, slot, b):
        if self.source_slot[slot] >= 0:
            self.buffer_refs[self.source_slot[slot]] -= 1
        self.source_slot[slot] = b
        if b >= 0:
            self.buffer_refs[b] += 1

    def snapshot_device(self, slot, out):
        b = self.source_slot[slot]
        if b < 0 or self.buffer_refs[b] > 1:
            b = slot if self.buffer_refs[slot] == 0 else -1
            k = 0
            while b < 0 and k < RING:
                if self.buffer_refs[k] == 0:
                    b = k
                k += 1
            if b < 0:
                out.append(f"nobuffer {self.k} {slot}")
                return None
        self.point_slot(slot, b)
        self.snapshot_gen[b] += 1
        out.append(f"copy {self.k} {slot} {b}")
        return b

    def burst(self, first, n, first_slot, G, out):
        plan = {"next": 0, "last_slot": -1, "changed": True}

        def snapshots_up_to(k_end):
            while plan["next"] < k_end and plan["next"] < n:
                slot = (first_slot + plan["next"]) % USER_SLOTS
                if plan["changed"] or plan["last_slot"] < 0:
                    b = self.snapshot_device(slot, out)
                    if b is None:
                        return
                    plan["last_slot"], plan["changed"] = b, False
                else:
                    self.point_slot(slot, plan["last_slot"])
                    out.append(f"point {self.k} {slot} {plan['last_slot']}")
                plan["next"] += 1

        first_k, n_k = device_share(first, n, self.k, G)
        for j in range(n_k):
            i = first_k + j * G
            snapshots_up_to(i - first)
            out.append(f"acc {self.k}")
            plan["changed"] = True
            snapshots_up_to(i - first + 1)
        snapshots_up_to(n)

    def peer(self, slot, out):
        src = self.source_slot[slot]
        skip = self.landed_slot == src and self.landed_gen == self.snapshot_gen[src]
        if not skip:
            self.landed_slot, self.landed_gen = src, self.snapshot_gen[src]
        out.append(f"peer {self.k} {slot} {src} {'skip' if skip else 'send'}")

    def reset(self):
        for k in range(RING):
            self.source_slot[k], self.buffer_refs[k] = -1, 0
        self.landed_slot = -1

    def state(self):
        shows = "".join(f" {s}:{b}" for s, b in enumerate(self.source_slot) if b >= 0)
        refs = "".join(f" {b}:{r}" for b, r in enumerate(self.buffer_refs) if r != 0)
        return f"state {self.k} |{shows} |{refs}"


def play_parent(lines):
    out, dev = [], []
    for line in lines:
        out.append(line)
        w = line.split()
        a = list(map(int, w[1:]))
        if w[0] == "ctx":
            dev = [ParentDevice(k) for k in range(a[0])]
        elif w[0] == "render":
            out += [f"acc {d.k}" for d in dev if device_share(a[0], a[1], d.k, len(dev))[1]]
        elif w[0] == "snapshot":
            for d in dev:
                d.snapshot_device(a[0], out)
        elif w[0] == "burst":
            for d in dev:
                d.burst(a[0], a[1], a[2], len(dev), out)
        elif w[0] == "read":
            if any(d.source_slot[a[0]] < 0 for d in dev):
                out.append("unfilled")
            else:
                for d in dev[1:]:
                    d.peer(a[0], out)
        elif w[0] == "reset":
            for d in dev:
                d.reset()
        out += [d.state() for d in dev]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# sequences

def random_sequences(seed, count):
    rng = random.Random(seed)
    lines = []
    for i in range(count):
        G = rng.choice([1, 2, 3])
        few = 6 if i % 2 == 0 else USER_SLOTS  # (six slots: snapshots overwrite each other, and what lazy copies point to, all the time)
        lines.append(f"ctx {G}")
        filled = set()
        for _ in range(rng.randint(10, 60)):
            r = rng.random()
            if r < 0.25:
                lines.append(f"render {rng.randint(0, 1000)} {rng.choice([1, 1, 1, 2, 3, 7])}")
            elif r < 0.45:
                slot = rng.randrange(few)
                lines.append(f"snapshot {slot}")
                filled.add(slot)
            elif r < 0.70:
                n = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 16, rng.randint(1, USER_SLOTS), USER_SLOTS])
                first, slot = rng.randint(0, 1000), rng.randrange(few)
                lines.append(f"burst {first} {n} {slot}")
                filled |= {(slot + k) % USER_SLOTS for k in range(n)}
            elif r < 0.88:
                slot = rng.choice(sorted(filled)) if filled and rng.random() < 0.9 else rng.randrange(USER_SLOTS)
                lines.append(f"read {slot}")
            elif r < 0.97:
                if G > 1:  # ptmi_read_image / ptmi_read_display: the library's own slot
                    lines += [f"snapshot {INTERNAL}", f"read {INTERNAL}"]
            else:
                lines.append("reset")
                filled = set()
    return lines


SEQUENCES = random_sequences(20261018, 400)


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("snapshot_ring"))
    return subprocess.run([exe], input="\n".join(SEQUENCES) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()


@pytest.fixture(scope="module")
def parent():
    return play_parent(SEQUENCES)


def test_the_ring_decides_what_ptmi_api_decided(played, parent):
    want = parent
    assert len(played) == len(want)
    for i, (g, w) in enumerate(zip(played, want)):
        assert g == w, f"output line {i}: snapshot_ring.h {g!r}, parent commit {w!r}"


class Stamps:
    """One device's accumulators and buffers as the test sees them: versions and stamps."""

    def __init__(self, version):
        self.version = version  # of the accumulators; never reused, not even after a reset
        self.stamp = {}         # buffer -> the version copied into it
        self.shows = {}         # slot -> buffer
        self.want = {}          # slot -> the version current when its snapshot was queued
        self.landed = None      # the stamp of what the landing buffer holds


def test_invariants_of_the_ring(played):
    dev, n_points, n_skips, n_sends, n_shared_rewrites = [], 0, 0, 0, 0
    for i, line in enumerate(played):
        w = line.split()
        where = f"output line {i}: {line!r}"
        if w[0] == "ctx":
            dev = [Stamps(1000 * k) for k in range(int(w[1]))]
        elif w[0] == "reset":
            dev = [Stamps(d.version + 1) for d in dev]
        elif w[0] == "acc":
            dev[int(w[1])].version += 1
        elif w[0] == "nobuffer":
            pytest.fail("(c) no buffer for a snapshot, " + where)
        elif w[0] in ("copy", "point"):
            d, slot, b = dev[int(w[1])], int(w[2]), int(w[3])
            assert 0 <= b < RING, where
            if w[0] == "copy":
                others = [s for s, sb in d.shows.items() if sb == b and s != slot]
                assert not others, f"(b) buffer {b} is written while slots {others} show it, " + where
                n_shared_rewrites += d.shows.get(slot, b) != b  # (the slot left a buffer it shared, or its own was taken)
                d.stamp[b] = d.version
            else:
                n_points += 1
            d.shows[slot], d.want[slot] = b, d.version
        elif w[0] == "peer":
            d, slot, b = dev[int(w[1])], int(w[2]), int(w[3])
            assert d.shows[slot] == b, where
            if w[4] == "skip":
                assert d.landed is not None and d.landed == d.stamp[b], f"(e) skipped: the landing buffer holds {d.landed}, the source {d.stamp[b]}, " + where
                n_skips += 1
            else:
                d.landed = d.stamp[b]
                n_sends += 1
        elif w[0] == "state":
            d = dev[int(w[1])]
            shows_txt, refs_txt = line.split("|")[1:]
            shows = {int(s): int(b) for s, b in (x.split(":") for x in shows_txt.split())}
            refs = {int(b): int(r) for b, r in (x.split(":") for x in refs_txt.split())}
            assert shows == d.shows, where
            assert refs == dict(Counter(d.shows.values())), "(d) buffer_refs, " + where
            for slot, b in d.shows.items():
                assert d.stamp[b] == d.want[slot], f"(a) slot {slot} shows version {d.stamp[b]}, queued at {d.want[slot]}, " + where
    # the sequences do reach the cases the ring exists for
    assert n_points > 1000 and n_skips > 100 and n_sends > 100 and n_shared_rewrites > 100


def test_model_under_sanitizers(tmp_path, parent):
    """The model compiled with -fsanitize=address,undefined as a program of its own, over the same sequences."""
    model_build.sanitizer_runtimes_or_skip()
    exe = _compile(tmp_path, ["-g", *model_build.SANITIZE])
    r = subprocess.run([exe], input="\n".join(SEQUENCES) + "\n", capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and r.stdout.splitlines() == parent, r.stderr[-3000:]
