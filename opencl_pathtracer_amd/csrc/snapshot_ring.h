// snapshot_ring.h - the bookkeeping of one device's ptmi_snapshot ring: which BUFFER each ring slot shows, which buffer a new
// snapshot goes to, and what the landing buffer on devices[0] already holds.  snapshot_device / gather_snapshot (ptmi_readback.cpp)
// and snapshots_up_to (ptmi_render.cpp) do the HIP side: allocate, copy, record, wait.  Pure host code without HIP, played on the
// CPU by tests/snapshot_ring_model.cpp.  Not ABI.
// A device's share of the image of ring slot s lives in slot s's own buffer when its accumulators changed with that image, else
// in the buffer of the last image that changed them (a device of a G-device render changes with every G-th image only, so
// ptmi_render_snapshots copies 41.5 MB per OWN iteration instead of per image).  A buffer several slots show is never written: a
// new snapshot for one of them goes to a buffer no slot shows (there always is one: as many buffers as slots) and the others keep
// showing what they showed (tests/test_api_fuzz_gpu.py).
#pragma once

#include <cstdint>

#include "ptmi.h"

namespace ptmi_internal {

constexpr uint32_t kRingSlots = PTMI_MAX_SNAPSHOT_SLOTS;
constexpr uint32_t kUserSlots = kRingSlots - 1;     // the last slot is the library's own:
constexpr uint32_t kInternalSlot = kRingSlots - 1;  // ptmi_read_image / ptmi_read_display of a multi-device context

struct SnapshotRing {
    int source_slot[kRingSlots];         // the buffer ring slot s shows; -1 = the slot has never been filled
    int buffer_refs[kRingSlots] = {};    // slots that show buffer b
    uint32_t snapshot_gen[kRingSlots] = {};  // bumped by every copy into buffer b
    // what this device's landing buffer on devices[0] holds: (buffer, generation) - a peer sends only what has changed
    int landed_buffer = -1;
    uint32_t landed_gen = 0;
    SnapshotRing() { for (int& s : source_slot) s = -1; }

    int shown(uint32_t slot) const { return source_slot[slot]; }

    // Make ring slot `slot` show buffer `b` (-1: nothing).
    void point(uint32_t slot, int b)
    {
        if (source_slot[slot] >= 0) buffer_refs[source_slot[slot]]--;
        source_slot[slot] = b;
        if (b >= 0) buffer_refs[b]++;
    }

    // Where a new snapshot for `slot` goes: the buffer the slot shows if no other slot shows it too, else one that no slot shows
    // (its own, as long as nobody else has taken it).  -1 cannot happen: as many buffers as slots.
    int buffer_for(uint32_t slot) const
    {
        int b = source_slot[slot];
        if (b >= 0 && buffer_refs[b] <= 1) return b;
        b = buffer_refs[slot] == 0 ? (int)slot : -1;
        for (int k = 0; b < 0 && k < (int)kRingSlots; k++)
            if (buffer_refs[k] == 0) b = k;
        return b;
    }

    // A copy of the accumulators into buffer `b` has been queued for `slot`.
    void written(uint32_t slot, int b)
    {
        point(slot, b);
        snapshot_gen[b]++;
    }

    // Does the landing buffer already hold what `slot` shows?  Consecutive images of a G-device render differ in ONE device's
    // share, so an image costs one peer copy, not G - 1.
    bool landed(uint32_t slot) const { return landed_buffer == source_slot[slot] && landed_gen == snapshot_gen[source_slot[slot]]; }
    void land(uint32_t slot) { landed_buffer = source_slot[slot], landed_gen = snapshot_gen[landed_buffer]; }
};

// ptmi_render_snapshots: an image after EVERY iteration of the call although the iterations share launches.  Global iteration
// first + k (k < n) goes to slot (first_slot + k) % kUserSlots.  A device's share of image k is whatever it has accumulated by
// then (its own ids up to first + k): it COPIES its accumulators only when they have changed since its last copy of this call -
// once per own iteration, plus once at the start of the call (so that every image of a call is served from buffers of that call: a
// caller may be overwriting the previous call's) - and lets the other images of the call point at that copy.
struct SnapshotPlan {
    uint32_t first, n, first_slot;
    uint32_t next = 0;     // next global k to provide on this device
    int last_buffer = -1;  // this device's latest copy of this call: the BUFFER it went to
    bool changed = true;   // accumulators changed since (or no copy of this call yet)

    bool due(uint32_t k_end) const { return next < k_end && next < n; }  // an image before k_end is still to be provided
    uint32_t slot() const { return (first_slot + next) % kUserSlots; }   // ... for this ring slot
    bool must_copy() const { return changed || last_buffer < 0; }        // ... by a copy; else by pointing at last_buffer
    void copied(int b) { last_buffer = b, changed = false; }
};

}  // namespace ptmi_internal
