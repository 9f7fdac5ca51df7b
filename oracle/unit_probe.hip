// unit_probe.hip - TEST INFRASTRUCTURE: the product's device functions (ptmi_device.hpp) called one at a time on chosen inputs.
//
// tests/test_unit_probe_gpu.py holds every function here to the CPU oracle's export of the same reference function and to the
// reference's own function (oracle/ref_unit_probe.cl), word for word, on the boundary inputs of tests/unit_probe_cases.py.
// One lane per case; a case is a fixed number of 32-bit words in and out (the layouts are stated once, in unit_probe_cases.py,
// and repeated in the comments of the kernels below).
// Compiled twice (oracle/Makefile, target probe), once per arithmetic mode as the product's own Makefile does: the entry points
// of the default-arithmetic unit carry the suffix _da.  Groups: box, triangle, texture, sky, light, material, sampling, pixel.
// Into oracle/build/libunit_probe.so; never linked by the product.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ptmi_shading.hpp"
#include "scene_refit_common.h"

namespace PTMI_DEV_NS {
namespace unit_probe {

__device__ __forceinline__ float f_of(uint32_t w) { return __uint_as_float(w); }
__device__ __forceinline__ uint32_t u_of(float f) { return __float_as_uint(f); }
__device__ __forceinline__ V4 v4w(const uint32_t* w) { return v4(f_of(w[0]), f_of(w[1]), f_of(w[2]), f_of(w[3])); }
__device__ __forceinline__ void put4(uint32_t* w, V4 v) { w[0] = u_of(v.x); w[1] = u_of(v.y); w[2] = u_of(v.z); w[3] = u_of(v.w); }

// in  [16]: lo.xyz, hi.xyz, isEmpty, limit, origin[4], direction[4]
// out [3] : box_hit, box_hit_ordered, ray_slabs_are_ordered
__global__ void box_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 16 * (size_t)i;
    float lo[3] = {f_of(w[0]), f_of(w[1]), f_of(w[2])}, hi[3] = {f_of(w[3]), f_of(w[4]), f_of(w[5])};
    const bool empty = w[6] != 0;
    const float limit = f_of(w[7]);
    Ray r;
    r.o = v4w(w + 8);
    ray_set_direction(r, v4w(w + 12));
    out[3 * (size_t)i + 0] = box_hit(lo, hi, empty, r, limit) ? 1u : 0u;
    // the ordered form tests no flag: it reads an empty box as the upload stores it (scene_layout.cpp: build_layout's last pass)
    if (empty) for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    out[3 * (size_t)i + 1] = box_hit_ordered(lo, hi, r, limit) ? 1u : 0u;
    out[3 * (size_t)i + 2] = ray_slabs_are_ordered(r) ? 1u : 0u;
}

// one form's result: accepted, q[4], s, t, front, the limit afterwards, 0 - all zero but the limit when the triangle is rejected
__device__ __forceinline__ void put_tri(uint32_t* o, bool acc, V4 q, float s, float t, bool front, float limit)
{
    for (int k = 0; k < 10; k++) o[k] = 0;
    o[8] = u_of(limit);
    if (acc) {
        o[0] = 1u;
        put4(o + 1, q);
        o[5] = u_of(s);
        o[6] = u_of(t);
        o[7] = front ? 1u : 0u;
    }
}

// in  [28]: S1[4], S2[4], S3[4], N[4], origin[4], direction[4], limit, 3 unused
// rec [n] : the DTri record of each case, pre [n]: its DTriPre record - both written by the host with the product's own
//           record functions (scene_refit_common.h)
// out [40]: put_tri of tri_hit, tri_hit_pre, tri_test<false>, tri_test<true>
__global__ void triangle_kernel(const uint32_t* __restrict__ in, const DTri* __restrict__ rec, DTriPre* __restrict__ pre,
                                uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 28 * (size_t)i;
    uint32_t* o = out + 40 * (size_t)i;
    Ray r;
    r.o = v4w(w + 16);
    ray_set_direction(r, v4w(w + 20));
    const float limit0 = f_of(w[24]);
    if (kDefaultArithmetic) {
        // the default arithmetic's reciprocal determinant is a device instruction's: patched into the uploaded record as
        // kernel_wavefront.hip's precompute_denominators_kernel does (this lane owns pre[i])
        pre[i].u_den[3] = pre_record_denominator(pre[i]);
    }
    const float4* g = reinterpret_cast<const float4*>(&rec[i]);
    const float4* p = reinterpret_cast<const float4*>(&pre[i]);
    {
        Hit h;
        float limit = limit0;
        const bool acc = tri_hit(&rec[i], r, limit, h);
        put_tri(o, acc, h.point, h.s, h.t, h.front, limit);
    }
    {
        Hit h;
        float limit = limit0;
        const bool acc = tri_hit_record<true>(p[0], p[1], p[2], p[3], r, limit, h);
        put_tri(o + 10, acc, h.point, h.s, h.t, h.front, limit);
    }
    // tri_test with the quads in the order kernel_wavefront.hip hands them over (kE1, kL0, kL1 there)
    put_tri(o + 20, false, v4(0, 0, 0, 0), 0, 0, false, limit0);
    tri_test<false>(g[0], g[3], [&](float4& l0, float4& l1) { l0 = g[1]; l1 = g[2]; }, r, limit0,
                    [&](const V4& q, float, float s, float t, bool front, float nsd) { put_tri(o + 20, true, q, s, t, front, nsd); });
    put_tri(o + 30, false, v4(0, 0, 0, 0), 0, 0, false, limit0);
    tri_test<true>(p[0], p[1], [&](float4& l0, float4& l1) { l0 = p[2]; l1 = p[3]; }, r, limit0,
                   [&](const V4& q, float, float s, float t, bool front, float nsd) { put_tri(o + 30, true, q, s, t, front, nsd); });
}

// in  [6]: width, height, offset, u, v, unused;  texels: the texture data;  out [4]: the colour
__global__ void texture_kernel(const uint32_t* __restrict__ in, const ptmi_uchar4* __restrict__ texels, uint32_t* __restrict__ out,
                               uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 6 * (size_t)i;
    ptmi_texture tex;
    tex.width = w[0]; tex.height = w[1]; tex.offset = w[2];
    put4(out + 4 * (size_t)i, texture_pixel(tex, texels, f_of(w[3]), f_of(w[4])));
}

// in  [6]: direction[4], cosRotationAngle, sinRotationAngle;  faces: six ptmi_texture;  out [4]: the colour
__global__ void sky_kernel(const uint32_t* __restrict__ in, const ptmi_texture* __restrict__ faces, const ptmi_uchar4* __restrict__ texels,
                           uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 6 * (size_t)i;
    ptmi_sky sky;
    for (int f = 0; f < 6; f++) sky.sky_textures[f] = faces[f];
    sky.ground_scale = sky.exposant_factor_x = sky.exposant_factor_y = 0;
    sky.cos_rotation_angle = f_of(w[4]);
    sky.sin_rotation_angle = f_of(w[5]);
    put4(out + 4 * (size_t)i, sky_color(sky, texels, v4w(w)));
}

// in  [20]: position[4], direction[4], power, cosInner, cosOuter, type, p[4], N[4];  out [1]
__global__ void light_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 20 * (size_t)i;
    ptmi_light l;
    l.position = ptmi_float4{f_of(w[0]), f_of(w[1]), f_of(w[2]), f_of(w[3])};
    l.direction = ptmi_float4{f_of(w[4]), f_of(w[5]), f_of(w[6]), f_of(w[7])};
    l.color = ptmi_float4{1, 1, 1, 1};
    l.power = f_of(w[8]); l.cos_inner = f_of(w[9]); l.cos_outer = f_of(w[10]); l.type = (int32_t)w[11];
    out[i] = u_of(light_power_toward(l, v4w(w + 12), v4w(w + 16)));
}

// in  [16]: incident[4], N[4], reflected[4], material type, isInWater, 2 unused
// out [20]: glass fraction, varnish fraction, water fraction, water refraction[4], water factor, brdf, reflection[4],
//           put_in_same_hemisphere(reflected, N)[4], 3 unused.  The water refraction and factor stay zero on total reflection
//           (the reference returns before it writes them, FullKernel.cl:237).
__global__ void material_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 16 * (size_t)i;
    uint32_t* o = out + 20 * (size_t)i;
    const V4 inc = v4w(w), N = v4w(w + 4), refl = v4w(w + 8);
    const int type = (int)w[12];
    const bool in_water = w[13] != 0;
    for (int k = 0; k < 20; k++) o[k] = 0;
    // the three calls as ptmi_shading.hpp: scatter_direction makes them
    constexpr DivC by_n_glass = make_divc(kNGlass);
    o[0] = u_of(fresnel_fraction(1, kNGlass, by_n_glass, -dot(inc, N), inc, N, nullptr));
    o[1] = u_of(fresnel_varnish(inc, N));
    const float n1 = in_water ? kNWater : 1.f, n2 = in_water ? 1.f : kNWater;
    V4 refracted = v4(0, 0, 0, 0);
    bool total = false;
    o[2] = u_of(fresnel_fraction(n1, n2, n2, -dot(inc, N), inc, N, &refracted, &total));
    if (!total) {
        put4(o + 3, refracted);
        o[7] = u_of(fdiv(n2 * n2, n1 * n1));  // cl:251, as scatter_direction
    }
    o[8] = u_of(material_brdf(type, inc, N, refl));
    put4(o + 9, reflect_about(inc, N));
    put4(o + 13, put_in_same_hemisphere(refl, N));
}

// in  [12]: seed, N[4], gx, gy, width, height, iteration, 2 unused
// out [12]: lcg_random's value, the seed after it, lcg_seed (the compiler's rule), lcg_seed (the source's rule),
//           cosine_sample_hemisphere(seed, N)[4], the seed after it, 3 unused
__global__ void sampling_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 12 * (size_t)i;
    uint32_t* o = out + 12 * (size_t)i;
    for (int k = 0; k < 12; k++) o[k] = 0;
    int seed = (int)w[0];
    o[0] = u_of(lcg_random(seed));
    o[1] = (uint32_t)seed;
    o[2] = (uint32_t)lcg_seed(w[5], w[6], w[7], w[8], w[9], false);
    o[3] = (uint32_t)lcg_seed(w[5], w[6], w[7], w[8], w[9], true);
    seed = (int)w[0];
    put4(o + 4, cosine_sample_hemisphere(seed, v4w(w + 1)));
    o[8] = (uint32_t)seed;
}

struct PixelScene {
    uint32_t width, height, sampler;
};

// in  [10]: gx, gy, width, height, iteration, sampler, seed, sx, sy, unused
// out [5] : draw_sample's sx, sy, the seed after it, sample_pixel of that sample, sample_pixel of the (sx, sy) given in the case
__global__ void pixel_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = in + 10 * (size_t)i;
    uint32_t* o = out + 5 * (size_t)i;
    const PixelScene sc{w[2], w[3], w[5]};
    int seed = (int)w[6];
    float sx, sy;
    draw_sample(sc, w[0], w[1], w[4], seed, sx, sy);
    o[0] = u_of(sx);
    o[1] = u_of(sy);
    o[2] = (uint32_t)seed;
    o[3] = sample_pixel(sc, sx, sy);
    o[4] = sample_pixel(sc, f_of(w[7]), f_of(w[8]));
}

// ---- host side ----------------------------------------------------------------------------------------------------------

struct DeviceBuffer {
    void* p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    // a copy of `bytes` host bytes (at least one word is allocated, so that a kernel always gets a valid pointer)
    int upload(const void* host, size_t bytes)
    {
        if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) return -1;
        if (bytes && host && hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return -2;
        return 0;
    }
    int zeroed(size_t bytes)
    {
        if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) return -1;
        return hipMemset(p, 0, bytes ? bytes : 4) == hipSuccess ? 0 : -2;
    }
};

inline int finish(uint32_t* out, const DeviceBuffer& d_out, size_t out_bytes)
{
    if (hipGetLastError() != hipSuccess) return -3;
    if (hipDeviceSynchronize() != hipSuccess) return -4;
    return hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -5;
}

inline dim3 grid_of(uint32_t n) { return dim3((n + 63u) / 64u); }

}  // namespace unit_probe
}  // namespace PTMI_DEV_NS

using namespace PTMI_DEV_NS::unit_probe;
using ptmi_internal::DTri;
using ptmi_internal::DTriPre;

extern "C" int PTMI_ARITH(unit_probe_box)(const uint32_t* in, uint32_t n, uint32_t* out)
{
    DeviceBuffer d_in, d_out;
    if (d_in.upload(in, (size_t)n * 16 * 4) || d_out.zeroed((size_t)n * 3 * 4)) return -1;
    hipLaunchKernelGGL(box_kernel, grid_of(n), dim3(64), 0, 0, (const uint32_t*)d_in.p, (uint32_t*)d_out.p, n);
    return finish(out, d_out, (size_t)n * 3 * 4);
}

extern "C" int PTMI_ARITH(unit_probe_triangle)(const uint32_t* in, uint32_t n, uint32_t* out)
{
    std::vector<DTri> rec(n);
    std::vector<DTriPre> pre(n);
    for (uint32_t i = 0; i < n; i++) {
        ptmi_triangle t;
        std::memset(&t, 0, sizeof t);
        std::memcpy(&t.s1, in + 28 * (size_t)i, 16);
        std::memcpy(&t.s2, in + 28 * (size_t)i + 4, 16);
        std::memcpy(&t.s3, in + 28 * (size_t)i + 8, 16);
        std::memcpy(&t.n, in + 28 * (size_t)i + 12, 16);
        ptmi_refit::make_tri_record(t, &rec[i]);
        ptmi_refit::make_tri_record_pre(t, &pre[i]);
    }
    DeviceBuffer d_in, d_rec, d_pre, d_out;
    if (d_in.upload(in, (size_t)n * 28 * 4) || d_rec.upload(rec.data(), (size_t)n * sizeof(DTri)) ||
        d_pre.upload(pre.data(), (size_t)n * sizeof(DTriPre)) || d_out.zeroed((size_t)n * 40 * 4))
        return -1;
    hipLaunchKernelGGL(triangle_kernel, grid_of(n), dim3(64), 0, 0, (const uint32_t*)d_in.p, (const DTri*)d_rec.p, (DTriPre*)d_pre.p,
                       (uint32_t*)d_out.p, n);
    return finish(out, d_out, (size_t)n * 40 * 4);
}

extern "C" int PTMI_ARITH(unit_probe_texture)(const uint32_t* in, uint32_t n, const void* texels, uint32_t n_texels, uint32_t* out)
{
    DeviceBuffer d_in, d_tex, d_out;
    if (d_in.upload(in, (size_t)n * 6 * 4) || d_tex.upload(texels, (size_t)n_texels * 4) || d_out.zeroed((size_t)n * 4 * 4)) return -1;
    hipLaunchKernelGGL(texture_kernel, grid_of(n), dim3(64), 0, 0, (const uint32_t*)d_in.p, (const ptmi_uchar4*)d_tex.p, (uint32_t*)d_out.p, n);
    return finish(out, d_out, (size_t)n * 4 * 4);
}

extern "C" int PTMI_ARITH(unit_probe_sky)(const uint32_t* in, uint32_t n, const void* faces, const void* texels, uint32_t n_texels,
                                          uint32_t* out)
{
    DeviceBuffer d_in, d_faces, d_tex, d_out;
    if (d_in.upload(in, (size_t)n * 6 * 4) || d_faces.upload(faces, 6 * sizeof(ptmi_texture)) || d_tex.upload(texels, (size_t)n_texels * 4) ||
        d_out.zeroed((size_t)n * 4 * 4))
        return -1;
    hipLaunchKernelGGL(sky_kernel, grid_of(n), dim3(64), 0, 0, (const uint32_t*)d_in.p, (const ptmi_texture*)d_faces.p,
                       (const ptmi_uchar4*)d_tex.p, (uint32_t*)d_out.p, n);
    return finish(out, d_out, (size_t)n * 4 * 4);
}

#define UNIT_PROBE_PLAIN_ENTRY(name, kernel, in_words, out_words)                                                                \
    extern "C" int PTMI_ARITH(name)(const uint32_t* in, uint32_t n, uint32_t* out)                                              \
    {                                                                                                                            \
        DeviceBuffer d_in, d_out;                                                                                                \
        if (d_in.upload(in, (size_t)n * (in_words) * 4) || d_out.zeroed((size_t)n * (out_words) * 4)) return -1;                 \
        hipLaunchKernelGGL(kernel, grid_of(n), dim3(64), 0, 0, (const uint32_t*)d_in.p, (uint32_t*)d_out.p, n);                  \
        return finish(out, d_out, (size_t)n * (out_words) * 4);                                                                  \
    }
UNIT_PROBE_PLAIN_ENTRY(unit_probe_light, light_kernel, 20, 1)
UNIT_PROBE_PLAIN_ENTRY(unit_probe_material, material_kernel, 16, 20)
UNIT_PROBE_PLAIN_ENTRY(unit_probe_sampling, sampling_kernel, 12, 12)
UNIT_PROBE_PLAIN_ENTRY(unit_probe_pixel, pixel_kernel, 10, 5)

#if !PTMI_DEFAULT_ARITHMETIC
// The reference's own functions: kernel `name` of the code object at `hsaco_path` (oracle/ref_unit_probe.cl compiled with the
// reference's kernel file), one work-item per case.  Its arguments are (in, out, n) followed by as many of aux0, aux1 as are
// not null - kernelParams, so that the runtime fills the OpenCL kernel's hidden arguments (as device_math_probe.hip).
// image_8x8: one 8 x 8 work-group instead (n == 64), for the functions that read the work-item's pixel from its global id.
extern "C" int unit_probe_reference(const char* hsaco_path, const char* name, const uint32_t* in, uint32_t in_words, uint32_t n,
                                    uint32_t* out, uint32_t out_words, const void* aux0, uint32_t aux0_bytes, const void* aux1,
                                    uint32_t aux1_bytes, uint32_t image_8x8)
{
    DeviceBuffer d_in, d_out, d_aux0, d_aux1;
    if (d_in.upload(in, (size_t)n * in_words * 4) || d_out.zeroed((size_t)n * out_words * 4)) return -1;
    if (aux0 && d_aux0.upload(aux0, aux0_bytes)) return -1;
    if (aux1 && d_aux1.upload(aux1, aux1_bytes)) return -1;
    hipModule_t mod;
    hipFunction_t fn;
    if (hipModuleLoad(&mod, hsaco_path) != hipSuccess) return -6;
    if (hipModuleGetFunction(&fn, mod, name) != hipSuccess) { (void)hipModuleUnload(mod); return -7; }
    void* args[5] = {&d_in.p, &d_out.p, &n, &d_aux0.p, &d_aux1.p};
    int rc = 0;
    if (image_8x8 && n != 64) rc = -9;
    else if (hipModuleLaunchKernel(fn, image_8x8 ? 1 : (n + 63u) / 64u, 1, 1, image_8x8 ? 8 : 64, image_8x8 ? 8 : 1, 1, 0, nullptr, args,
                                   nullptr) != hipSuccess)
        rc = -8;
    if (rc == 0) rc = finish(out, d_out, (size_t)n * out_words * 4);
    (void)hipModuleUnload(mod);
    return rc;
}
#endif
