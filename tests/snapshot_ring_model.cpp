// Plays snapshots, bursts and reads through opencl_pathtracer_amd/csrc/snapshot_ring.h for tests/test_snapshot_ring_model.py: the
// ring's decisions as snapshot_device, snapshots_up_to / render_on_device and gather_snapshot take them, without the HIP calls.
//
//   snapshot_ring_model < events      one line per event:
//       ctx G                  a new context of G devices
//       render FIRST N         ptmi_render: the accumulators of every device with a share of the ids change
//       snapshot SLOT          ptmi_snapshot
//       burst FIRST N SLOT     ptmi_render_snapshots
//       read SLOT              ptmi_read_snapshot (SLOT 64 after "snapshot 64": ptmi_read_image of a multi-device context)
//       reset                  ptmi_initialize_memory: the scene's state is value-initialised
//     each event is echoed, followed by its decisions - "acc K" (device K accumulated an iteration), "copy K SLOT B" (its
//     accumulators copied into buffer B for SLOT), "point K SLOT B", "nobuffer K SLOT", "unfilled", "peer K SLOT B send|skip" -
//     and by the header's state per device: "state K | SLOT:B ... | B:REFS ..." (filled slots, referenced buffers).
#include <cstdio>
#include <cstring>
#include <vector>

#include "snapshot_ring.h"

using namespace ptmi_internal;

namespace {

// device_share of ptmi_render.cpp: the ids [first, first + n) that device k of G takes
void device_share(uint32_t first, uint32_t n, uint32_t k, uint32_t G, uint32_t* first_k, uint32_t* n_k)
{
    const uint32_t skip = (k + G - first % G) % G;
    *first_k = first + skip;
    *n_k = skip < n ? (n - skip + G - 1) / G : 0;
}

struct Device {
    uint32_t k;
    SnapshotRing ring;

    // snapshot_device
    int snapshot(uint32_t slot)
    {
        const int b = ring.buffer_for(slot);
        if (b < 0) {
            std::printf("nobuffer %u %u\n", k, slot);
            return b;
        }
        ring.written(slot, b);
        std::printf("copy %u %u %d\n", k, slot, b);
        return b;
    }
    // snapshots_up_to
    void up_to(SnapshotPlan& plan, uint32_t k_end)
    {
        for (; plan.due(k_end); plan.next++) {
            if (!plan.must_copy()) {
                ring.point(plan.slot(), plan.last_buffer);
                std::printf("point %u %u %d\n", k, plan.slot(), plan.last_buffer);
                continue;
            }
            const int b = snapshot(plan.slot());
            if (b < 0) return;
            plan.copied(b);
        }
    }
    // render_on_device with a plan: one accumulation per own iteration, each between the images before and up to it
    void burst(uint32_t first, uint32_t n, uint32_t first_slot, uint32_t G)
    {
        uint32_t first_k, n_k;
        device_share(first, n, k, G, &first_k, &n_k);
        SnapshotPlan plan{first, n, first_slot};
        for (uint32_t j = 0; j < n_k; j++) {
            const uint32_t id = first_k + j * G;
            up_to(plan, id - plan.first);
            std::printf("acc %u\n", k);
            plan.changed = true;
            up_to(plan, id - plan.first + 1);
        }
        up_to(plan, plan.n);
    }
    void print_state() const
    {
        std::printf("state %u |", k);
        for (uint32_t s = 0; s < kRingSlots; s++)
            if (ring.shown(s) >= 0) std::printf(" %u:%d", s, ring.shown(s));
        std::printf(" |");
        for (uint32_t b = 0; b < kRingSlots; b++)
            if (ring.buffer_refs[b] != 0) std::printf(" %u:%d", b, ring.buffer_refs[b]);
        std::printf("\n");
    }
};

// gather_snapshot: every device must have filled the slot; then each peer sends what the landing buffer does not hold yet
void read(std::vector<Device>& dev, uint32_t slot)
{
    for (const Device& d : dev)
        if (d.ring.shown(slot) < 0) {
            std::printf("unfilled\n");
            return;
        }
    for (size_t k = 1; k < dev.size(); k++) {
        const bool skip = dev[k].ring.landed(slot);
        if (!skip) dev[k].ring.land(slot);
        std::printf("peer %zu %u %d %s\n", k, slot, dev[k].ring.shown(slot), skip ? "skip" : "send");
    }
}

}  // namespace

int main()
{
    std::vector<Device> dev;
    char line[128];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned a[3] = {};
        std::fputs(line, stdout);
        if (std::sscanf(line, "ctx %u", &a[0]) == 1 && a[0] >= 1 && a[0] <= PTMI_MAX_DEVICES) {
            dev.clear();
            for (uint32_t k = 0; k < a[0]; k++) dev.push_back(Device{k, SnapshotRing{}});
        } else if (std::sscanf(line, "render %u %u", &a[0], &a[1]) == 2) {
            for (Device& d : dev) {
                uint32_t first_k, n_k;
                device_share(a[0], a[1], d.k, (uint32_t)dev.size(), &first_k, &n_k);
                if (n_k) std::printf("acc %u\n", d.k);
            }
        } else if (std::sscanf(line, "snapshot %u", &a[0]) == 1 && a[0] < kRingSlots) {
            for (Device& d : dev) d.snapshot(a[0]);
        } else if (std::sscanf(line, "burst %u %u %u", &a[0], &a[1], &a[2]) == 3 && a[1] <= kUserSlots && a[2] < kUserSlots) {
            for (Device& d : dev) d.burst(a[0], a[1], a[2], (uint32_t)dev.size());
        } else if (std::sscanf(line, "read %u", &a[0]) == 1 && a[0] < kRingSlots) {
            read(dev, a[0]);
        } else if (std::strncmp(line, "reset", 5) == 0) {
            for (Device& d : dev) d.ring = SnapshotRing{};
        } else {
            std::fprintf(stderr, "bad line: %s", line);
            return 1;
        }
        for (const Device& d : dev) d.print_state();
    }
    return 0;
}
