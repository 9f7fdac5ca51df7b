// denoise.hip - accumulators + first-hit guide planes -> a filtered mean image, on the device (ptmi_denoise, ptmi_denoise_device).
//
// An edge-avoiding a-trous wavelet filter: a 5 x 5 B3-spline footprint at steps 1, 2, 4, 8, 16, every tap weighted down by its
// distance from the centre in colour, shading normal and position, and never taken across the hit mask.  The arithmetic is the
// contract of ptmi.h / DESIGN 1e: every operation below is ONE IEEE binary32 operation in the written order (the build line has
// -ffp-contract=off, `/` is the correctly rounded division, denormals are kept), no transcendental - tests/denoise_cases.py
// restates it in NumPy and the GPU tests compare word for word.  One arithmetic for both context modes: compiled once.
//
// Per pixel, between the passes (56 bytes; the context's d_denoise_features):
//   e  float4  (e.xyz, hit ? 1 : 0)   the filtered value; two planes that ping-pong
//   g1 float4  (nrm.xyz, pos.x)       written by the prepass, read by every pass
//   g2 float2  (pos.y, pos.z)
// The divisor d (the clamped albedo, or 1) is needed at a pixel's own position only, before the first pass and after the last:
// both ends compute it from the albedo plane with the same expression instead of carrying it through the passes.
#include <hip/hip_runtime.h>

#include "ptmi_internal.h"

namespace ptmi_dev {

struct DenoisePlanes {
    const float4* color;      // sum plane
    const float* ray_nb;      // count plane
    const float4* albedo;     // guide sums over G iterations
    const float4* normal;
    const float4* position;
    const float* hit_count;
    float G;                  // (float)guide_iterations
    uint32_t demodulate;
};

// d of the contract: a = albedo / G per channel, d_c = a_c > 1e-3f ? a_c : 1e-3f (a NaN albedo gives 1e-3); 1 without the flag
__device__ __forceinline__ float3 denoise_divisor(const DenoisePlanes& in, size_t p)
{
    if (!in.demodulate) return make_float3(1.f, 1.f, 1.f);
    const float4 s = in.albedo[p];
    const float ax = s.x / in.G, ay = s.y / in.G, az = s.z / in.G;
    return make_float3(ax > 1e-3f ? ax : 1e-3f, ay > 1e-3f ? ay : 1e-3f, az > 1e-3f ? az : 1e-3f);
}

// One lane per pixel, p linear (lanes contiguous along a row).  `out` != nullptr: passes == 0, the image leaves here.
__global__ void __launch_bounds__(256) denoise_prepass_kernel(const DenoisePlanes in, float4* __restrict__ e0, float4* __restrict__ g1,
                                                              float2* __restrict__ g2, float4* __restrict__ out, const size_t npix)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float4 c = in.color[p];
    const float n = in.ray_nb[p];
    float mx = 0.f, my = 0.f, mz = 0.f;
    if (n > 0) { mx = c.x / n; my = c.y / n; mz = c.z / n; }
    const float3 d = denoise_divisor(in, p);
    const float ex = mx / d.x, ey = my / d.y, ez = mz / d.z;
    if (out) {
        out[p] = make_float4(ex * d.x, ey * d.y, ez * d.z, n);
        return;
    }
    const float h = in.hit_count[p];
    const bool hit = h > 0;
    float4 nr = make_float4(0.f, 0.f, 0.f, 0.f), ps = nr;
    if (hit) {
        const float4 a = in.normal[p], b = in.position[p];
        nr = make_float4(a.x / h, a.y / h, a.z / h, 0.f);
        ps = make_float4(b.x / h, b.y / h, b.z / h, 0.f);
    }
    e0[p] = make_float4(ex, ey, ez, hit ? 1.f : 0.f);
    g1[p] = make_float4(nr.x, nr.y, nr.z, ps.x);
    g2[p] = make_float2(ps.y, ps.z);
}

struct DenoisePass {
    const float4* e_in;
    const float4* g1;
    const float2* g2;
    float4* e_out;         // the other e plane; the last pass: the image
    uint32_t width, height;
    int step;              // 1 << k
    float inv_c, inv_n, inv_p;
    uint32_t last;         // fuse the re-modulation: e_out[p] = (e * d, n)
};

__device__ __forceinline__ float dot3(float x, float y, float z) { return (x * x + y * y) + z * z; }

// The 25 taps of pixel (x, y), dy outer and dx inner, from wherever `fetch(qx, qy, e, g1, g2)` reads an in-image pixel's
// features.  Every tap is bounds-checked here, before it is fetched.
template <class Fetch>
__device__ __forceinline__ float4 denoise_taps(const DenoisePass& a, const int x, const int y, const float4 ep, const float4 g1p,
                                               const float2 g2p, Fetch fetch)
{
    constexpr float B[3] = {0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + a.step * dx, qy = y + a.step * dy;
            if (qx < 0 || qx >= (int)a.width || qy < 0 || qy >= (int)a.height) continue;
            float4 eq, g1q;
            float2 g2q;
            fetch(qx, qy, eq, g1q, g2q);
            if (eq.w != ep.w) continue;  // the hit mask
            const float b = B[dy < 0 ? -dy : dy] * B[dx < 0 ? -dx : dx];
            const float xc = dot3(eq.x - ep.x, eq.y - ep.y, eq.z - ep.z) * a.inv_c;
            const float xn = dot3(g1q.x - g1p.x, g1q.y - g1p.y, g1q.z - g1p.z) * a.inv_n;
            const float xp = dot3(g1q.w - g1p.w, g2q.x - g2p.x, g2q.y - g2p.y) * a.inv_p;
            const float w = b / (((1.f + xc) * (1.f + xn)) * (1.f + xp));
            if (!(w > 0)) continue;  // a NaN anywhere, or b / inf
            sw = sw + w;
            sx = sx + w * eq.x;
            sy = sy + w * eq.y;
            sz = sz + w * eq.z;
        }
    }
    if (sw > 0) return make_float4(sx / sw, sy / sw, sz / sw, ep.w);
    return ep;
}

__device__ __forceinline__ void denoise_store(const DenoisePass& a, const DenoisePlanes& in, const size_t p, const float4 e)
{
    if (a.last) {
        const float3 d = denoise_divisor(in, p);
        a.e_out[p] = make_float4(e.x * d.x, e.y * d.y, e.z * d.z, in.ray_nb[p]);
    } else {
        a.e_out[p] = e;
    }
}

// Direct form (any step): workgroups of 64 x 4 pixels, a wave = 64 pixels of one row, so the wave's reads for one (dx, dy) are
// one contiguous row segment.
__global__ void __launch_bounds__(256) denoise_atrous_kernel(const DenoisePass a, const DenoisePlanes in)
{
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const float4 e = denoise_taps(a, x, y, a.e_in[p], a.g1[p], a.g2[p], [&](int qx, int qy, float4& eq, float4& g1q, float2& g2q) {
        const size_t q = (size_t)qy * a.width + (size_t)qx;
        eq = a.e_in[q];
        g1q = a.g1[q];
        g2q = a.g2[q];
    });
    denoise_store(a, in, p, e);
}

// Tiled form (step S = 1 or 2, where the footprints of neighbouring lanes overlap almost entirely): a 32 x 8 tile and its halo
// of 2 S pixels staged in LDS once per workgroup - (32 + 4 S) x (8 + 4 S) pixels of 40 bytes, 25.6 KB at S = 2.  A halo pixel
// outside the image is stored as zeros and never read: the taps are bounds-checked against the image, as in the direct form.
template <int S>
__global__ void __launch_bounds__(256) denoise_atrous_tiled_kernel(const DenoisePass a, const DenoisePlanes in)
{
    constexpr int R = 2 * S, TW = 32 + 2 * R, TH = 8 + 2 * R;
    __shared__ float4 s_e[TW * TH];
    __shared__ float4 s_g1[TW * TH];
    __shared__ float2 s_g2[TW * TH];
    const int x0 = (int)(blockIdx.x * 32u), y0 = (int)(blockIdx.y * 8u);
    for (int i = (int)(threadIdx.y * 32u + threadIdx.x); i < TW * TH; i += 256) {
        const int gx = x0 - R + i % TW, gy = y0 - R + i / TW;
        float4 e = make_float4(0.f, 0.f, 0.f, 0.f), g1 = e;
        float2 g2 = make_float2(0.f, 0.f);
        if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height) {
            const size_t q = (size_t)gy * a.width + (size_t)gx;
            e = a.e_in[q];
            g1 = a.g1[q];
            g2 = a.g2[q];
        }
        s_e[i] = e;
        s_g1[i] = g1;
        s_g2[i] = g2;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= (int)a.width || y >= (int)a.height) return;
    const int c = ((int)threadIdx.y + R) * TW + (int)threadIdx.x + R;
    const float4 e = denoise_taps(a, x, y, s_e[c], s_g1[c], s_g2[c], [&](int qx, int qy, float4& eq, float4& g1q, float2& g2q) {
        const int i = (qy - y0 + R) * TW + (qx - x0 + R);  // |q - p| <= R per axis: inside the staged tile
        eq = s_e[i];
        g1q = s_g1[i];
        g2q = s_g2[i];
    });
    denoise_store(a, in, (size_t)y * a.width + (size_t)x, e);
}

}  // namespace ptmi_dev

namespace ptmi_internal {

int launch_denoise(const DenoiseJob& job, void* stream, std::string* err)
{
    const hipStream_t s = (hipStream_t)stream;
    const size_t npix = (size_t)job.width * job.height;
    if (npix == 0 || job.passes > 5 || job.height > 4u * 65535u || job.width > 0x7FFFFFFFu - 64u) {
        if (err) *err = "launch_denoise: an empty image, more than 5 passes, or more rows or columns than the grid holds";
        return PTMI_ERR_INTERNAL;
    }
    const ptmi_dev::DenoisePlanes in{reinterpret_cast<const float4*>(job.color),  job.ray_nb,
                                     reinterpret_cast<const float4*>(job.albedo), reinterpret_cast<const float4*>(job.normal),
                                     reinterpret_cast<const float4*>(job.position), job.hit_count,
                                     job.guide_iterations, job.demodulate ? 1u : 0u};
    float4* e[2] = {reinterpret_cast<float4*>(job.features), reinterpret_cast<float4*>(job.features) + npix};
    float4* g1 = e[1] + npix;
    float2* g2 = reinterpret_cast<float2*>(g1 + npix);
    float4* out = reinterpret_cast<float4*>(job.out);
    hipLaunchKernelGGL(ptmi_dev::denoise_prepass_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, in, e[0], g1, g2,
                       job.passes == 0 ? out : nullptr, npix);
    if (int rc = launch_status(hipGetLastError(), "denoise_prepass_kernel", err)) return rc;
    for (uint32_t k = 0; k < job.passes; k++) {
        const bool last = k + 1 == job.passes;
        const ptmi_dev::DenoisePass a{e[k & 1], g1, g2, last ? out : e[(k + 1) & 1], job.width, job.height, 1 << k,
                                      job.inv_c[k], job.inv_n, job.inv_p, last ? 1u : 0u};
        if (k < 2 && job.tiled) {
            const dim3 grid((job.width + 31u) / 32u, (job.height + 7u) / 8u), block(32, 8);
            if (k == 0) hipLaunchKernelGGL(ptmi_dev::denoise_atrous_tiled_kernel<1>, grid, block, 0, s, a, in);
            else hipLaunchKernelGGL(ptmi_dev::denoise_atrous_tiled_kernel<2>, grid, block, 0, s, a, in);
        } else {
            const dim3 grid((job.width + 63u) / 64u, (job.height + 3u) / 4u), block(64, 4);
            hipLaunchKernelGGL(ptmi_dev::denoise_atrous_kernel, grid, block, 0, s, a, in);
        }
        if (int rc = launch_status(hipGetLastError(), "denoise_atrous_kernel", err)) return rc;
    }
    return PTMI_OK;
}

}  // namespace ptmi_internal
