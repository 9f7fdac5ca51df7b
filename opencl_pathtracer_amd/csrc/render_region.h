// render_region.h - the rectangle of the image a launch renders (ptmi_render_region; ptmi_render passes the whole image): the
// Region type, the check of a caller's rectangle, the job hand-out's tile cover and the mapping between a launch's staging
// slots and (pixel, iteration).  HIP-free when g++ compiles it: the kernels (kernel_wavefront.hip, kernels.hip), the launch code
// (ptmi_render.cpp) and the model of the tests (tests/render_region_model.cpp) compile this one copy.  Not ABI.
//
// SLOTS ARE REGION-RELATIVE.  A launch of n iterations over region (x, y, w, h) writes the staging slots
//     slot = it_local * (w * h) + (gy - y) * w + (gx - x),      it_local < n, (gx, gy) inside the region,
// which are exactly 0 .. w * h * n - 1.  Every kernel behind a launch that scans slots (redo_poisoned_kernel,
// histogram_staged_kernel, the accumulate kernels) scans that range and nothing else, so THE INVARIANT holds by construction:
// no kernel behind a launch reads a slot the launch did not write - a stale marker of an earlier, larger launch lies at a slot
// number the scan never reaches.  Only the accumulate kernels turn a slot into an image pixel (region_pixel).  The seed and the
// sample of a path keep the FULL image's width and height: a region selects work-items, it does not renumber them.
#pragma once

#include <cstdint>
#include <string>

#include "ptmi_hd.h"

namespace ptmi_internal {

struct Region {
    uint32_t x, y, w, h;  // pixels [x, x + w) x [y, y + h) of the image, row 0 first
};

PTMI_HD Region whole_image(uint32_t width, uint32_t height) { return Region{0u, 0u, width, height}; }
PTMI_HD bool region_is_empty(const Region& r) { return r.w == 0u || r.h == 0u; }
PTMI_HD uint32_t region_pixels(const Region& r) { return r.w * r.h; }

// A caller's rectangle against a width x height image: inside it, in 64 bits (x = 0xFFFFFFFF, w = 2 does not wrap to 1).  An
// empty rectangle is accepted wherever its origin lies inside or on the far edge.
inline bool check_region(uint32_t width, uint32_t height, const Region& r, std::string* err)
{
    if ((uint64_t)r.x + r.w <= (uint64_t)width && (uint64_t)r.y + r.h <= (uint64_t)height) return true;
    if (err)
        *err = "region (" + std::to_string(r.x) + ", " + std::to_string(r.y) + ", " + std::to_string(r.w) + ", " + std::to_string(r.h) +
               ") does not lie inside the " + std::to_string(width) + " x " + std::to_string(height) + " image";
    return false;
}

// The three expressions of the mapping, as macros: the functions below return them, and the wavefront kernel writes them into
// its hand-out in place (kernel_wavefront.hip) - called through functions with reference results, its instantiations for the
// whole image no longer compiled to the code their pinned figures were read off (profiles/render_region_ab.txt).  So the model
// of the tests and the hot kernel still run ONE copy of the text.
#define PTMI_REGION_TILE_RX(tile, tiles_x, in_tile) (((tile) % (tiles_x)) * 8u + ((in_tile) & 7u))
#define PTMI_REGION_TILE_RY(tile, tiles_x, in_tile) (((tile) / (tiles_x)) * 8u + ((in_tile) >> 3))
#define PTMI_REGION_SLOT(w, h, rx, ry, it_local) ((it_local) * ((w) * (h)) + (ry) * (w) + (rx))

// ---- the job hand-out: 8 x 8 tiles from the region's own origin --------------------------------------------------------------
PTMI_HD uint32_t region_tiles_x(uint32_t w) { return (w + 7u) >> 3; }
PTMI_HD uint32_t region_tiles(const Region& r) { return region_tiles_x(r.w) * ((r.h + 7u) >> 3); }
// lane `in_tile` (< 64) of tile `tile` (< region_tiles): its pixel RELATIVE to the region's origin; false = the pixel lies
// beyond the region's right or bottom edge (an edge tile) and is nobody's job
PTMI_HD bool region_tile_pixel(uint32_t w, uint32_t h, uint32_t tiles_x, uint32_t tile, uint32_t in_tile, uint32_t& rx, uint32_t& ry)
{
    rx = PTMI_REGION_TILE_RX(tile, tiles_x, in_tile);
    ry = PTMI_REGION_TILE_RY(tile, tiles_x, in_tile);
    return rx < w && ry < h;
}

// ---- slots ----------------------------------------------------------------------------------------------------------------------
// (rx, ry): relative to the region's origin
PTMI_HD uint32_t region_slot(uint32_t w, uint32_t h, uint32_t rx, uint32_t ry, uint32_t it_local) { return PTMI_REGION_SLOT(w, h, rx, ry, it_local); }
// ... and its inverse plus the origin: the path's pixel in the image and its iteration id (ids of a launch: first_iteration +
// it_local * iteration_stride)
// (the wavefront kernel keeps the region as scalars: x, y, w and n = w * h)
PTMI_HD void decode_slot(uint32_t slot, uint32_t x, uint32_t y, uint32_t w, uint32_t n, uint32_t first_iteration, uint32_t iteration_stride,
                         uint32_t& gx, uint32_t& gy, uint32_t& iteration)
{
    const uint32_t it_local = slot / n, pixel = slot - it_local * n;
    gy = pixel / w;
    gx = pixel - gy * w;
    gx += x;
    gy += y;
    iteration = first_iteration + it_local * iteration_stride;
}
PTMI_HD void decode_slot(uint32_t slot, const Region& r, uint32_t first_iteration, uint32_t iteration_stride, uint32_t& gx, uint32_t& gy,
                         uint32_t& iteration)
{
    decode_slot(slot, r.x, r.y, r.w, r.w * r.h, first_iteration, iteration_stride, gx, gy, iteration);
}
// slot q (< w * h) of one iteration -> the pixel's index in a width-wide image
PTMI_HD uint32_t region_pixel(const Region& r, uint32_t q, uint32_t width)
{
    const uint32_t ry = q / r.w;
    return (r.y + ry) * width + r.x + (q - ry * r.w);
}

}  // namespace ptmi_internal
