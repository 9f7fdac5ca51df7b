// display.hip - accumulators -> displayed pixels on the device.
//
// What the reference shows and saves after every image is produced on the host from the two float buffers it has just
// read back (41.5 MB at 1080p, PathTracer_OpenCL.cpp:97-98): ConvertRGBAToBMPBuffer, Alone/PathTracer_bitmap.cpp:237-286.
// The same quantisation here, on the device, so that a viewer only has to fetch 3 bytes per pixel (6.2 MB at 1080p):
//   pixel = (int) min(sum * 255.f / n, 255.f) per channel, `min` being the Windows macro a < b ? a : b (a NaN from 0/0
//   on a never-sampled pixel shows as 255); a negative red sum marks the pixel pure red (:262 tests .x three times);
//   bytes in B, G, R order, rows padded to a multiple of 4 and zero-filled, image row 0 first.
#include <hip/hip_runtime.h>

#include "ptmi_internal.h"

namespace ptmi_dev {

__device__ __forceinline__ uint32_t display_channel(float sum, float n)
{
    const float v = sum * 255.f / n;  // IEEE multiply, then IEEE divide (no contraction, no reciprocal)
    const float m = v < 255.f ? v : 255.f;
    return (uint32_t)(int)m & 0xFFu;  // (BYTE)(int)
}

__global__ void __launch_bounds__(256) display_bgr_kernel(const float* __restrict__ image_color, const float* __restrict__ image_ray_nb,
                                                          uint8_t* __restrict__ out, const uint32_t width, const uint32_t height,
                                                          const uint32_t row_stride)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= height) return;
    uint8_t* row = out + (size_t)y * row_stride;
    if (x < width) {
        const size_t p = (size_t)y * width + x;
        const float4 c = reinterpret_cast<const float4*>(image_color)[p];
        const float n = image_ray_nb[p];
        uint32_t r = 255u, g = 0u, b = 0u;
        if (!(c.x < 0)) {
            r = display_channel(c.x, n);
            g = display_channel(c.y, n);
            b = display_channel(c.z, n);
        }
        row[3 * x + 0] = (uint8_t)b;
        row[3 * x + 1] = (uint8_t)g;
        row[3 * x + 2] = (uint8_t)r;
    }
    // padding bytes of the scanline (memset 0 in the reference)
    if (x < row_stride - 3u * width) row[3u * width + x] = 0;
}

// ---- the display stage (ptmi.h "displaying an image"): exposure, tone operator, transfer function, 8 bits --------------------
// Any sum-and-count pair or any mean plane.  The arithmetic is the contract ptmi.h states, the same in both arithmetic modes:
// one IEEE operation per written operation (-ffp-contract=off, `/` correctly rounded, denormals kept) and no transcendental -
// the transfer function is a table of 256 thresholds (display_tables.inc), the byte the largest k with T[k] <= t, found by eight
// branch-free steps in a copy of the table in LDS.  tests/display_cases.py restates it in NumPy and the GPU tests hold every
// byte to that.
static const float display_tables_host[3][256] = {
#include "display_tables.inc"
};
__device__ const float display_tables[3][256] = {
#include "display_tables.inc"
};

struct TonemapArgs {
    const float4* color;
    const float* ray_nb;  // nullptr: `color` holds means
    uint8_t* out;
    uint32_t width, height, row_stride, groups;  // groups: lanes per row (BGR24: four pixels each)
    uint32_t tone, transfer;
    float exposure, w2;
    bool counts_by_four;  // BGR24: a lane's four counts lie on a 16-byte boundary (the width a multiple of 4, the plane aligned)
};

// steps 1 to 4 for one pixel, from its colour and (sum form) its count: its bytes as r | g << 8 | b << 16
__device__ __forceinline__ uint32_t display_pixel(const TonemapArgs& a, const float* T, const float4 c, const float n)
{
    float m[3] = {c.x, c.y, c.z};
    if (a.ray_nb) {
        const bool sampled = n > 0;
        for (int i = 0; i < 3; i++) m[i] = sampled ? m[i] / n : 0.f;
    }
    uint32_t rgb = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float x = m[i] * a.exposure;
        if (!(x > 0)) x = 0;
        float t = x;
        if (a.tone == PTMI_TONE_REINHARD) t = (x * (1.f + x / a.w2)) / (1.f + x);
        else if (a.tone == PTMI_TONE_FILMIC) t = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
        t = t < 1.f ? t : 1.f;  // (a NaN becomes 1)
        uint32_t k = 0;         // T[0] = 0 <= t
#pragma unroll
        for (uint32_t step = 128; step; step >>= 1) k += T[k + step] <= t ? step : 0u;
        rgb |= k << (8 * i);
    }
    return rgb;
}

// BGR24: a lane takes four pixels of one row, twelve bytes, and stores them as three dwords where the rows are dword aligned
// and the four pixels exist; the ragged last group of a row, and rows of a stride that is no multiple of 4, store bytes.  The
// lane of a row's last group zero-fills the row's padding.
__global__ void __launch_bounds__(256) display_tonemap_bgr24_kernel(const TonemapArgs a)
{
    __shared__ float T[256];
    T[threadIdx.x] = display_tables[a.transfer][threadIdx.x];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.height * a.groups) return;
    const uint32_t y = (uint32_t)(i / a.groups), g = (uint32_t)(i % a.groups), x0 = 4u * g;
    const uint32_t n = a.width - x0 < 4u ? a.width - x0 : 4u;
    const size_t p0 = (size_t)y * a.width + x0;
    float count[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.ray_nb) {
        if (a.counts_by_four) {
            const float4 q = *reinterpret_cast<const float4*>(a.ray_nb + p0);
            count[0] = q.x; count[1] = q.y; count[2] = q.z; count[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (k < n) count[k] = a.ray_nb[p0 + k];
        }
    }
    uint32_t v[4] = {0, 0, 0, 0};  // b | g << 8 | r << 16
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        if (k < n) {
            const uint32_t rgb = display_pixel(a, T, a.color[p0 + k], count[k]);
            v[k] = (rgb >> 16) | (rgb & 0xFF00u) | ((rgb & 0xFFu) << 16);
        }
    uint8_t* row = a.out + (size_t)y * a.row_stride;
    if (n == 4 && !(a.row_stride & 3u)) {
        uint32_t* d = reinterpret_cast<uint32_t*>(row + 12u * g);
        d[0] = v[0] | (v[1] << 24);
        d[1] = (v[1] >> 8) | (v[2] << 16);
        d[2] = (v[2] >> 16) | (v[3] << 8);
    } else {
        for (uint32_t k = 0; k < n; k++) {
            row[3u * (x0 + k) + 0] = (uint8_t)v[k];
            row[3u * (x0 + k) + 1] = (uint8_t)(v[k] >> 8);
            row[3u * (x0 + k) + 2] = (uint8_t)(v[k] >> 16);
        }
    }
    if (g == a.groups - 1)
        for (uint32_t b = 3u * a.width; b < a.row_stride; b++) row[b] = 0;
}

// RGBA32: a lane takes one pixel, one dword
__global__ void __launch_bounds__(256) display_tonemap_rgba32_kernel(const TonemapArgs a)
{
    __shared__ float T[256];
    T[threadIdx.x] = display_tables[a.transfer][threadIdx.x];
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)a.height * a.width) return;
    reinterpret_cast<uint32_t*>(a.out)[p] = display_pixel(a, T, a.color[p], a.ray_nb ? a.ray_nb[p] : 0.f) | 0xFF000000u;
}

// The luminance histogram of the means (step 1), in quarter-octave bins read off the float's bits: a workgroup counts in LDS,
// then adds its non-zero words to memory.  Integer counts: no order shows.
__global__ void __launch_bounds__(256) luminance_histogram_kernel(const float4* __restrict__ color, const float* __restrict__ ray_nb,
                                                                  uint32_t* __restrict__ histogram, const size_t n_pixels)
{
    __shared__ uint32_t bins[PTMI_LUMINANCE_WORDS];
    for (uint32_t w = threadIdx.x; w < PTMI_LUMINANCE_WORDS; w += 256) bins[w] = 0;
    __syncthreads();
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pixels; p += (size_t)gridDim.x * 256) {
        const float4 c = color[p];
        float m[3] = {c.x, c.y, c.z};
        if (ray_nb) {
            const float n = ray_nb[p];
            const bool sampled = n > 0;
            for (int i = 0; i < 3; i++) m[i] = sampled ? m[i] / n : 0.f;
        }
        const float Y = (0.2126f * m[0] + 0.7152f * m[1]) + 0.0722f * m[2];
        uint32_t word = 256;  // !(Y > 0): black, negative, NaN, never sampled
        if (Y > 0) {
            const int bin = (int)(__float_as_uint(Y) >> 21) - 380;
            word = __float_as_uint(Y) == 0x7F800000u ? 257u : (uint32_t)(bin < 0 ? 0 : bin > 255 ? 255 : bin);
        }
        atomicAdd(&bins[word], 1u);
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < PTMI_LUMINANCE_WORDS; w += 256)
        if (bins[w]) atomicAdd(&histogram[w], bins[w]);
}

// Sum of the partial accumulators of the devices that shared a render, in device order (deterministic; the single-device
// image differs from it only by the order of these float additions).
struct ImageParts {
    const float* p[PTMI_MAX_DEVICES];
};
__global__ void __launch_bounds__(256) sum_images_kernel(float* __restrict__ out, const ImageParts parts, const uint32_t n_parts,
                                                         const size_t n_quads, const uint32_t n_tail)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == n_quads) {  // the floats behind the last whole quad (an image of an odd number of pixels: 5 floats each), in the same order
        for (uint32_t j = 0; j < n_tail; j++) {
            float s = parts.p[0][4 * n_quads + j];
            for (uint32_t k = 1; k < n_parts; k++) s = s + parts.p[k][4 * n_quads + j];
            out[4 * n_quads + j] = s;
        }
    }
    if (i >= n_quads) return;
    float4 s = reinterpret_cast<const float4*>(parts.p[0])[i];
    for (uint32_t k = 1; k < n_parts; k++) {
        const float4 v = reinterpret_cast<const float4*>(parts.p[k])[i];
        s.x = s.x + v.x; s.y = s.y + v.y; s.z = s.z + v.z; s.w = s.w + v.w;
    }
    reinterpret_cast<float4*>(out)[i] = s;
}

}  // namespace ptmi_dev

namespace ptmi_dev {
// dst[i] += src[i]: the counter block of a launch that ran on a stage set of its own, added when the main stream adopts it
__global__ void add_counters_kernel(unsigned long long* __restrict__ dst, const unsigned long long* __restrict__ src, uint32_t n)
{
    const uint32_t i = threadIdx.x;
    if (i < n) dst[i] += src[i];
}
}  // namespace ptmi_dev

namespace ptmi_internal {

int launch_add_counters(unsigned long long* dst, const unsigned long long* src, uint32_t n, void* stream, std::string* err)
{
    hipLaunchKernelGGL(ptmi_dev::add_counters_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dst, src, n);
    return launch_status(hipGetLastError(), "add_counters_kernel", err);
}

int launch_sum_images(float* out, const float* const* parts, uint32_t n_parts, size_t n_floats, void* stream, std::string* err)
{
    if (n_parts == 0 || n_parts > PTMI_MAX_DEVICES) {
        if (err) *err = "launch_sum_images: bad part count";
        return PTMI_ERR_INVALID_ARGUMENT;
    }
    ptmi_dev::ImageParts ip{};
    for (uint32_t k = 0; k < n_parts; k++) ip.p[k] = parts[k];
    const size_t n_quads = n_floats / 4;
    const uint32_t n_tail = (uint32_t)(n_floats & 3u);  // (every buffer comes from hipMalloc: the quads are aligned)
    hipLaunchKernelGGL(ptmi_dev::sum_images_kernel, dim3((unsigned)((n_quads + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, ip,
                       n_parts, n_quads, n_tail);
    return launch_status(hipGetLastError(), "sum_images_kernel", err);
}

int launch_display_bgr(const float* image_color, const float* image_ray_nb, uint8_t* out, uint32_t width, uint32_t height,
                       uint32_t row_stride, void* stream, std::string* err)
{
    const dim3 grid((width + 255u) / 256u, height), block(256);
    hipLaunchKernelGGL(ptmi_dev::display_bgr_kernel, grid, block, 0, (hipStream_t)stream, image_color, image_ray_nb, out, width,
                       height, row_stride);
    return launch_status(hipGetLastError(), "display_bgr_kernel", err);
}

const float* display_table(uint32_t transfer) { return ptmi_dev::display_tables_host[transfer]; }

int launch_display_tonemapped(const DisplayJob& job, void* stream, std::string* err)
{
    const bool rgba = job.format == PTMI_PIXELS_RGBA32;
    ptmi_dev::TonemapArgs a{};
    a.color = reinterpret_cast<const float4*>(job.color);
    a.ray_nb = job.ray_nb;
    a.out = job.out;
    a.width = job.width;
    a.height = job.height;
    a.row_stride = job.row_stride;
    a.groups = rgba ? job.width : (job.width + 3u) / 4u;
    a.tone = job.tone;
    a.transfer = job.transfer;
    a.exposure = job.exposure;
    a.w2 = job.w2;
    a.counts_by_four = !(job.width & 3u) && !((uintptr_t)job.ray_nb & 15u);  // (bound accumulators may lie anywhere)
    const size_t blocks = ((size_t)job.height * a.groups + 255) / 256;
    if (job.transfer > PTMI_TRANSFER_GAMMA22 || blocks == 0 || blocks > 0x7FFFFFFFu) {
        if (err) *err = "launch_display_tonemapped: unknown transfer function, or an image of no or too many workgroups";
        return PTMI_ERR_INTERNAL;
    }
    if (rgba) hipLaunchKernelGGL(ptmi_dev::display_tonemap_rgba32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ptmi_dev::display_tonemap_bgr24_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status(hipGetLastError(), "display_tonemap_kernel", err);
}

int launch_luminance_histogram(const float* color, const float* ray_nb, uint32_t* histogram, size_t n_pixels, void* stream, std::string* err)
{
    const hipError_t e = hipMemsetAsync(histogram, 0, PTMI_LUMINANCE_WORDS * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return launch_status(e, "luminance_histogram_kernel (zeroing)", err);
    // at most 1024 workgroups, each in a grid-stride loop: at most 1024 x 260 adds to memory however large the image
    const size_t wanted = (n_pixels + 255) / 256;
    const unsigned blocks = (unsigned)(wanted < 1 ? 1 : wanted > 1024 ? 1024 : wanted);
    hipLaunchKernelGGL(ptmi_dev::luminance_histogram_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(color), ray_nb, histogram, n_pixels);
    return launch_status(hipGetLastError(), "luminance_histogram_kernel", err);
}

}  // namespace ptmi_internal
