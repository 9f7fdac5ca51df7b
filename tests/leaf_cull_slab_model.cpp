// leaf_cull_slab_model.cpp - csrc/leaf_cull.h's two box distances side by side behind a C interface: box_distance2, which the
// proof of the culling speaks of, and box_distance2_from_slabs, which the kernel's box tests evaluate on the differences they
// form anyway.  Compiled by tests/test_leaf_cull_slab_distance.py with g++ (-ffp-contract=off, as the library is) - no HIP.
#include <cstdint>
#include <cstring>

#include "leaf_cull.h"

namespace {
uint32_t bits(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
}  // namespace

extern "C" {

uint32_t slab_box_distance2_bits(const float lo[3], const float hi[3], const float o[3]) { return bits(ptmi_cull::box_distance2(lo, hi, o[0], o[1], o[2])); }

// The slab form as a box test feeds it: per axis the pair (near - o, far - o), each difference rounded by itself.
// order: bit k set = axis k hands over (hi - o, lo - o), as a ray does whose direction component k is not positive.
uint32_t slab_from_slabs_bits(const float lo[3], const float hi[3], const float o[3], int order)
{
    float a[3], b[3];
    for (int k = 0; k < 3; k++) {
        const bool swapped = ((order >> k) & 1) != 0;
        a[k] = (swapped ? hi[k] : lo[k]) - o[k];
        b[k] = (swapped ? lo[k] : hi[k]) - o[k];
    }
    return bits(ptmi_cull::box_distance2_from_slabs(a[0], b[0], a[1], b[1], a[2], b[2]));
}

// n boxes and origins (3 floats each): how many of the n x 8 (box, order) pairs differ in a bit; *first = the first such box
uint32_t slab_count_differences(uint32_t n, const float* lo, const float* hi, const float* o, uint32_t* first)
{
    uint32_t differ = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t want = slab_box_distance2_bits(lo + 3 * i, hi + 3 * i, o + 3 * i);
        for (int order = 0; order < 8; order++)
            if (slab_from_slabs_bits(lo + 3 * i, hi + 3 * i, o + 3 * i, order) != want) {
                if (differ == 0) *first = i;
                differ++;
            }
    }
    return differ;
}

}  // extern "C"
