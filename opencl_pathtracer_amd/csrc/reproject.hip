// reproject.hip - the accumulated image of the previous camera, resampled under the camera of now (ptmi_reproject_device,
// ptmi_set_camera_reprojected).
//
// A pixel's world-space point (the current position plane) is projected into the previous camera; the four previous pixels
// around where it lands are blended bilinearly, each taken only where the previous position and normal planes say it saw the
// same surface and its own value is a finite mean.  The arithmetic is the contract of ptmi.h / DESIGN 1g: every operation below
// is ONE IEEE binary32 operation in the written order (the build line has -ffp-contract=off, `/` is the correctly rounded
// division, denormals are kept), no transcendental - tests/reproject_cases.py restates it in NumPy and the GPU tests compare
// word for word.  One arithmetic for both context modes: compiled once.
//
// One lane per pixel and one wave per 8 x 8 tile, in a grid-stride loop over tiles (the guide kernel's layout): under a mild
// camera move the footprint of a tile in the previous frame is about a tile again, so a wave's four gathers fall into a few
// 128-byte lines of each previous plane.  No LDS (the footprint is not known before the projection), no atomics; every plane is
// written once, by vector stores, and a tap's coordinates are checked against the image before anything of it is fetched.
#include <hip/hip_runtime.h>

#include "ptmi_internal.h"

namespace ptmi_dev {

struct ReprojectArgs {
    const float4* prev_normal;
    const float4* prev_position;
    const float* prev_hit_count;
    const float4* prev_color;
    const float* prev_ray_nb;
    const float4* cur_normal;
    const float4* cur_position;
    const float* cur_hit_count;
    float4* out_color;
    float* out_ray_nb;
    uint32_t width, height, tiles_x, n_tiles;
    float3 cam, r0, r1, r2;
    float tp, tn, max_history, Wf, Hf;
};

__device__ __forceinline__ float rp_dot3(const float3 a, const float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float3 rp_sub(const float3 a, const float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 rp_mean(const float4 s, const float n) { return make_float3(s.x / n, s.y / n, s.z / n); }

constexpr uint32_t kReprojectBlock = 256, kReprojectWaves = kReprojectBlock / 64;  // 4 waves = 4 tiles

__global__ void __launch_bounds__(kReprojectBlock) reproject_kernel(const ReprojectArgs a)
{
    const uint32_t wave = threadIdx.x >> 6, in_tile = threadIdx.x & 63u;
    for (uint32_t tile = blockIdx.x * kReprojectWaves + wave; tile < a.n_tiles; tile += gridDim.x * kReprojectWaves) {
        const uint32_t tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
        const uint32_t gx = tile_x * 8u + (in_tile & 7u), gy = tile_y * 8u + (in_tile >> 3);
        if (gx >= a.width || gy >= a.height) continue;  // (no barrier anywhere: a lane may sit a tile out)
        const size_t p = (size_t)gy * a.width + gx;

        float sw = 0.f, sn = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        const float h = a.cur_hit_count[p];
        if (h > 0) {
            const float3 P = rp_mean(a.cur_position[p], h), N = rp_mean(a.cur_normal[p], h);
            const float3 v = rp_sub(P, a.cam);
            const float t = rp_dot3(a.r0, v), ca = rp_dot3(a.r1, v), cb = rp_dot3(a.r2, v);
            const float u = (ca / t + 0.5f) * a.Wf - 0.5f, w_ = (cb / t + 0.5f) * a.Hf - 0.5f;
            if (t > 0 && u > -1.f && u < a.Wf && w_ > -1.f && w_ < a.Hf) {  // (a NaN fails)
                const float x0 = floorf(u), fx = u - x0, y0 = floorf(w_), fy = w_ - y0;
                const float lim = a.tp * rp_dot3(v, v);
                const float gx1 = 1.f - fx, gy1 = 1.f - fy;
                const float weight[4] = {gx1 * gy1, fx * gy1, gx1 * fy, fx * fy};
                const int ix = (int)x0, iy = (int)y0;  // -1 .. W-1, -1 .. H-1: exact
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int qx = ix + (k & 1), qy = iy + (k >> 1);
                    if (qx < 0 || qx >= (int)a.width || qy < 0 || qy >= (int)a.height) continue;
                    const float w = weight[k];
                    if (!(w > 0)) continue;
                    const size_t q = (size_t)qy * a.width + (size_t)qx;
                    const float hq = a.prev_hit_count[q];
                    if (!(hq > 0)) continue;
                    const float nq = a.prev_ray_nb[q];
                    if (!(nq > 0)) continue;
                    const float3 dP = rp_sub(rp_mean(a.prev_position[q], hq), P);
                    if (!(rp_dot3(dP, dP) <= lim)) continue;
                    const float3 dN = rp_sub(rp_mean(a.prev_normal[q], hq), N);
                    if (!(rp_dot3(dN, dN) <= a.tn)) continue;
                    const float4 c = a.prev_color[q];
                    const float m0 = c.x / nq, m1 = c.y / nq, m2 = c.z / nq, m3 = c.w / nq;
                    if (!(m0 - m0 == 0 && m1 - m1 == 0 && m2 - m2 == 0 && m3 - m3 == 0)) continue;
                    sw = sw + w;
                    s0 = s0 + w * m0;
                    s1 = s1 + w * m1;
                    s2 = s2 + w * m2;
                    s3 = s3 + w * m3;
                    sn = sn + w * nq;
                }
            }
        }
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        float n = 0.f;
        if (sw > 0) {
            const float mean_n = sn / sw;
            const float kept = floorf(mean_n < a.max_history ? mean_n : a.max_history);
            if (kept >= 1.f) {
                n = kept;
                out = make_float4((s0 / sw) * n, (s1 / sw) * n, (s2 / sw) * n, (s3 / sw) * n);
            }
        }
        a.out_color[p] = out;
        a.out_ray_nb[p] = n;
    }
}

}  // namespace ptmi_dev

namespace ptmi_internal {

int launch_reproject(const ReprojectJob& job, void* stream, std::string* err)
{
    using namespace ptmi_dev;
    const uint32_t tiles_x = (job.width + 7u) / 8u, tiles_y = (job.height + 7u) / 8u;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
    // (the tile index plus its grid-stride step stays below 2^32; a tap's coordinates are ints)
    if (n_tiles == 0 || n_tiles > 0x7FFFFFFFull || job.width > 0x7FFFFFFFu || job.height > 0x7FFFFFFFu) {
        if (err) *err = "reproject_kernel: an empty image, or one with too many tiles";
        return PTMI_ERR_INTERNAL;
    }
    ReprojectArgs a{};
    a.prev_normal = reinterpret_cast<const float4*>(job.prev_normal);
    a.prev_position = reinterpret_cast<const float4*>(job.prev_position);
    a.prev_hit_count = job.prev_hit_count;
    a.prev_color = reinterpret_cast<const float4*>(job.prev_color);
    a.prev_ray_nb = job.prev_ray_nb;
    a.cur_normal = reinterpret_cast<const float4*>(job.cur_normal);
    a.cur_position = reinterpret_cast<const float4*>(job.cur_position);
    a.cur_hit_count = job.cur_hit_count;
    a.out_color = reinterpret_cast<float4*>(job.out_color);
    a.out_ray_nb = job.out_ray_nb;
    a.width = job.width;
    a.height = job.height;
    a.tiles_x = tiles_x;
    a.n_tiles = (uint32_t)n_tiles;
    a.cam = make_float3(job.cam[0], job.cam[1], job.cam[2]);
    a.r0 = make_float3(job.r0[0], job.r0[1], job.r0[2]);
    a.r1 = make_float3(job.r1[0], job.r1[1], job.r1[2]);
    a.r2 = make_float3(job.r2[0], job.r2[1], job.r2[2]);
    a.tp = job.tp;
    a.tn = job.tn;
    a.max_history = job.max_history;
    a.Wf = (float)job.width;
    a.Hf = (float)job.height;
    // as many workgroups as the device holds at once (8 of four waves per CU, 256 CUs); the loop takes the rest
    constexpr uint64_t kMaxBlocks = 2048;
    const uint64_t wanted = (n_tiles + kReprojectWaves - 1) / kReprojectWaves;
    hipLaunchKernelGGL(reproject_kernel, dim3((unsigned)(wanted > kMaxBlocks ? kMaxBlocks : wanted)), dim3(kReprojectBlock), 0,
                       (hipStream_t)stream, a);
    return launch_status(hipGetLastError(), "reproject_kernel", err);
}

}  // namespace ptmi_internal
