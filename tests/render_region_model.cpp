// render_region_model.cpp - csrc/render_region.h played on the CPU (tests/test_render_region_model.py): for images and regions
// given on the command line or enumerated here, with n iterations per launch,
//   - slot -> (gx, gy, it) -> slot is the identity,
//   - the slots of a launch are exactly 0 .. w * h * n - 1,
//   - the pixels they name are exactly the region's (region_pixel: the accumulate kernels' mapping),
//   - the 8 x 8 tile cover from the region's origin reaches every pixel of the region once and no pixel outside it,
// and check_region's verdicts.  Prints one line of counts; the first violation ends the program with a message and status 1.
//   render_region_model every W H STEP K   the regions of a W x H image whose number is K modulo STEP (STEP 1, K 0: all of them), n = 1, 3, 32
//   render_region_model sample W H N SEED  N seeded regions of a W x H image, n = 1, 3, 32
//   render_region_model check              check_region
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "render_region.h"

using namespace ptmi_internal;

static void fail(const char* what, const Region& r, uint32_t W, uint32_t H, uint32_t n, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0)
{
    std::printf("FAILED %s: image %u x %u region (%u, %u, %u, %u) n %u at (%u, %u, %u)\n", what, W, H, r.x, r.y, r.w, r.h, n, a, b, c);
    std::exit(1);
}

struct Checker {
    uint32_t W, H;
    std::vector<uint32_t> slot_seen, pixel_seen;
    uint32_t stamp = 0;
    unsigned long long regions = 0, paths = 0, tiles = 0;
    Checker(uint32_t w, uint32_t h) : W(w), H(h), slot_seen((size_t)w * h * 32, 0u), pixel_seen((size_t)w * h, 0u) {}

    void launch(const Region& r, uint32_t n)
    {
        std::string why;
        if (!check_region(W, H, r, &why)) fail("check_region refuses a region inside the image", r, W, H, n);
        const uint32_t first = 7u, stride = 3u, per_it = region_pixels(r);
        stamp++;
        for (uint32_t it = 0; it < n; it++)
            for (uint32_t gy = r.y; gy < r.y + r.h; gy++)
                for (uint32_t gx = r.x; gx < r.x + r.w; gx++) {
                    const uint32_t slot = region_slot(r.w, r.h, gx - r.x, gy - r.y, it);
                    if (slot >= per_it * n) fail("slot beyond the launch's", r, W, H, n, gx, gy, it);
                    if (slot_seen[slot] == stamp) fail("slot named twice", r, W, H, n, gx, gy, it);
                    slot_seen[slot] = stamp;
                    uint32_t dx, dy, id;
                    decode_slot(slot, r, first, stride, dx, dy, id);
                    if (dx != gx || dy != gy || id != first + it * stride) fail("decode_slot is not the inverse", r, W, H, n, gx, gy, it);
                    if (region_pixel(r, slot - it * per_it, W) != gy * W + gx) fail("region_pixel names another pixel", r, W, H, n, gx, gy, it);
                    paths++;
                }
        // (per_it * n distinct slots, all below per_it * n: exactly 0 .. per_it * n - 1)
    }

    void cover(const Region& r)
    {
        stamp++;
        const uint32_t tiles_x = region_tiles_x(r.w), n_tiles = region_tiles(r);
        uint32_t reached = 0;
        for (uint32_t tile = 0; tile < n_tiles; tile++)
            for (uint32_t in_tile = 0; in_tile < 64u; in_tile++) {
                uint32_t rx, ry;
                if (!region_tile_pixel(r.w, r.h, tiles_x, tile, in_tile, rx, ry)) continue;
                const uint32_t gx = r.x + rx, gy = r.y + ry;
                if (gx < r.x || gx >= r.x + r.w || gy < r.y || gy >= r.y + r.h || gx >= W || gy >= H) fail("tile pixel outside the region", r, W, H, 0, gx, gy, tile);
                if (pixel_seen[(size_t)gy * W + gx] == stamp) fail("pixel reached twice", r, W, H, 0, gx, gy, tile);
                pixel_seen[(size_t)gy * W + gx] = stamp;
                reached++;
            }
        if (reached != region_pixels(r)) fail("tile cover misses pixels", r, W, H, 0, reached);
        tiles += n_tiles;
    }

    void region(const Region& r)
    {
        cover(r);
        for (uint32_t n : {1u, 3u, 32u}) launch(r, n);
        regions++;
    }
};

static int run_check()
{
    struct Case { uint32_t W, H; Region r; bool ok; };
    const Case cases[] = {
        {43, 29, {0, 0, 43, 29}, true},   {43, 29, {1, 0, 43, 29}, false}, {43, 29, {0, 1, 43, 29}, false}, {43, 29, {42, 28, 1, 1}, true},
        {43, 29, {42, 28, 2, 1}, false},  {43, 29, {42, 28, 1, 2}, false}, {43, 29, {0xFFFFFFFFu, 0, 2, 1}, false},
        {43, 29, {0, 0xFFFFFFFFu, 1, 2}, false}, {43, 29, {0, 0, 0xFFFFFFFFu, 1}, false}, {43, 29, {2, 0, 0xFFFFFFFFu, 1}, false},
        // empty regions are accepted, on the far edge too
        {43, 29, {5, 5, 0, 3}, true},     {43, 29, {5, 5, 3, 0}, true},    {43, 29, {43, 29, 0, 0}, true},  {43, 29, {44, 0, 0, 0}, false},
        {1, 1, {0, 0, 1, 1}, true},       {1, 1, {0, 0, 2, 1}, false},     {0xFFFFFFFFu, 1, {0xFFFFFFFEu, 0, 1, 1}, true},
        {0xFFFFFFFFu, 1, {0xFFFFFFFEu, 0, 2, 1}, false},
    };
    int n = 0;
    for (const Case& c : cases) {
        std::string why;
        const bool ok = check_region(c.W, c.H, c.r, &why);
        if (ok != c.ok || (ok != why.empty())) {
            std::printf("FAILED check_region(%u, %u, (%u, %u, %u, %u)) = %d, message '%s'\n", c.W, c.H, c.r.x, c.r.y, c.r.w, c.r.h, (int)ok, why.c_str());
            return 1;
        }
        if (!check_region(c.W, c.H, c.r, nullptr) != !ok) return 1;  // (no message asked for)
        n++;
    }
    if (!region_is_empty(Region{1, 1, 0, 5}) || !region_is_empty(Region{1, 1, 5, 0}) || region_is_empty(Region{0, 0, 1, 1})) return 1;
    const Region whole = whole_image(43, 29);
    if (whole.x != 0 || whole.y != 0 || whole.w != 43 || whole.h != 29 || region_tiles(whole) != 6u * 4u) return 1;
    std::printf("ok check %d\n", n);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "check")) return run_check();
    if (argc == 6 && !std::strcmp(argv[1], "every")) {
        const uint32_t W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]), step = (uint32_t)std::atoi(argv[4]);
        const uint32_t offset = (uint32_t)std::atoi(argv[5]);
        if (step < 1 || offset >= step) return 2;
        Checker c(W, H);
        unsigned long long k = 0;
        for (uint32_t x = 0; x < W; x++)
            for (uint32_t y = 0; y < H; y++)
                for (uint32_t w = 1; x + w <= W; w++)
                    for (uint32_t h = 1; y + h <= H; h++)
                        if (k++ % step == offset) c.region(Region{x, y, w, h});
        std::printf("ok every %llu regions %llu paths %llu tiles\n", c.regions, c.paths, c.tiles);
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "sample")) {
        const uint32_t W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]), N = (uint32_t)std::atoi(argv[4]);
        uint32_t s = (uint32_t)std::atoi(argv[5]) * 2654435761u + 1u;
        auto next = [&s](uint32_t below) { s = s * 1664525u + 1013904223u; return (uint32_t)(((unsigned long long)(s >> 8) * below) >> 24); };
        Checker c(W, H);
        c.region(whole_image(W, H));
        {  // (the scalar form of decode_slot, as the wavefront kernel calls it)
            uint32_t gx, gy, id;
            decode_slot(2u * W * H + (H - 1u) * W + (W - 1u), 0u, 0u, W, W * H, 5u, 2u, gx, gy, id);
            if (gx != W - 1u || gy != H - 1u || id != 9u) fail("the scalar decode_slot", whole_image(W, H), W, H, 3);
        }
        for (uint32_t i = 0; i < N; i++) {
            const uint32_t x = next(W), y = next(H);
            c.region(Region{x, y, 1u + next(W - x), 1u + next(H - y)});
        }
        std::printf("ok sample %llu regions %llu paths %llu tiles\n", c.regions, c.paths, c.tiles);
        return 0;
    }
    std::printf("usage: render_region_model every W H STEP K | sample W H N SEED | check\n");
    return 2;
}
