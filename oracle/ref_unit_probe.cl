// ref_unit_probe.cl - TEST INFRASTRUCTURE: the reference's own functions called one at a time.
//
// Our own text: the reference's kernel file is included where it lies (oracle/Makefile passes -I<reference>/Kernel and the -D
// values Kernel_Main needs), and the kernels below call its functions by name on the cases of tests/unit_probe_cases.py -
// one work-item per case, the word layouts of oracle/unit_probe.hip.  Built by `make -C oracle ref` into
// oracle/_ref/ref_unit_probe.hsaco (the reference's default arithmetic) and ref_unit_probe.strict.hsaco; launched by
// unit_probe_reference (unit_probe.hip).  Functions that take the whole scene (KERNEL_GLOBAL_VAR_DECLARATION) are not probed.
#include "PathTracer_FullKernel.cl"

inline float4 ld4(__global const uint* w) { return (float4)(as_float(w[0]), as_float(w[1]), as_float(w[2]), as_float(w[3])); }
inline void st4(__global uint* w, float4 v) { w[0] = as_uint(v.x); w[1] = as_uint(v.y); w[2] = as_uint(v.z); w[3] = as_uint(v.w); }

// in [16]: lo.xyz, hi.xyz, isEmpty, limit, origin[4], direction[4];  out [1]
__kernel void unit_box(__global const uint* in, __global uint* out, uint n)
{
    const uint i = get_global_id(0);
    if (i >= n) return;
    __global const uint* w = in + 16 * (size_t)i;
    BoundingBox bb;
    bb.pMin = (float4)(as_float(w[0]), as_float(w[1]), as_float(w[2]), 0.0f);
    bb.pMax = (float4)(as_float(w[3]), as_float(w[4]), as_float(w[5]), 0.0f);
    bb.centroid = (float4)(0.0f);
    bb.isEmpty = w[6] != 0;
    const float4 o = ld4(w + 8), d = ld4(w + 12);
    Ray3D r;
    Ray3D_Create(&r, &o, &d, false);
    out[i] = BoundingBox_Intersects(&bb, &r, as_float(w[7])) ? 1u : 0u;
}

// in [28]: S1, S2, S3, N, origin, direction, limit, 3 unused;  materials: two plain-colour materials (0: positive side, 1: negative)
// out [10]: accepted, q[4], s, t, positive side, the limit afterwards, 0
__kernel void unit_triangle(__global const uint* in, __global uint* out, uint n, __global const Material* materials)
{
    const uint i = get_global_id(0);
    if (i >= n) return;
    __global const uint* w = in + 28 * (size_t)i;
    __global uint* o = out + 10 * (size_t)i;
    Triangle t;
    t.S1 = ld4(w); t.S2 = ld4(w + 4); t.S3 = ld4(w + 8); t.N = ld4(w + 12);
    t.N1 = t.N2 = t.N3 = t.N;
    t.UVP1 = t.UVP2 = t.UVP3 = t.UVN1 = t.UVN2 = t.UVN3 = (float2)(0.0f);
    t.materialWithPositiveNormalIndex = 0;
    t.materialWithNegativeNormalIndex = 1;
    t.id = 0;
    const float4 org = ld4(w + 16), dir = ld4(w + 20);
    Ray3D r;
    Ray3D_Create(&r, &org, &dir, false);
    float limit = as_float(w[24]);
    const bool acc = Triangle_Intersects((__global const Texture*)materials, materials, (__global const uchar4*)materials, &t, &r, &limit);
    for (int k = 0; k < 10; k++) o[k] = 0;
    o[8] = as_uint(limit);
    if (acc) {
        o[0] = 1u;
        st4(o + 1, r.intersectionPoint);
        o[5] = as_uint(r.s);
        o[6] = as_uint(r.t);
        o[7] = r.intersectedMaterialId == 0 ? 1u : 0u;
    }
}

// in [6]: width, height, offset, u, v, unused;  out [4]
__kernel void unit_texture(__global const uint* in, __global uint* out, uint n, __global const uchar4* texels, __global Texture* scratch)
{
    const uint i = get_global_id(0);
    if (i >= n) return;
    __global const uint* w = in + 6 * (size_t)i;
    // Texture_GetPixelColorValue takes its texture from global memory: one scratch record per case
    scratch[i].width = w[0]; scratch[i].height = w[1]; scratch[i].offset = w[2];
    st4(out + 4 * (size_t)i, Texture_GetPixelColorValue(&scratch[i], texels, as_float(w[3]), as_float(w[4])));
}

// in [6]: direction[4], cosRotationAngle, sinRotationAngle;  skies: one Sky per case (the six faces + the case's rotation,
// written by the host);  out [4]
__kernel void unit_sky(__global const uint* in, __global uint* out, uint n, __global const uchar4* texels, __global const Sky* skies)
{
    const uint i = get_global_id(0);
    if (i >= n) return;
    const float4 d = ld4(in + 6 * (size_t)i);
    st4(out + 4 * (size_t)i, Sky_GetColorValue(&skies[i], texels, &d));
}

// in [20]: position, direction, power, cosInner, cosOuter, type, p, N;  out [1]
__kernel void unit_light(__global const uint* in, __global uint* out, uint n)
{
    const uint i = get_global_id(0);
    if (i >= n) return;
    __global const uint* w = in + 20 * (size_t)i;
    Light l;
    l.position = ld4(w); l.direction = ld4(w + 4); l.color = (float4)(1.0f);
    l.power = as_float(w[8]); l.cosOfInnerFallOffAngle = as_float(w[9]); l.cosOfOuterFallOffAngle = as_float(w[10]);
    l.type = (LightType)w[11];
    const float4 p = ld4(w + 12), N = ld4(w + 16);
    out[i] = as_uint(Light_PowerToward(&l, &p, &N));
}

// in [16]: incident, N, reflected, material type, isInWater, 2 unused;  out [20]: as unit_probe.hip's material_kernel
__kernel void unit_material(__global const uint* in, __global uint* out, uint n)
{
    const uint i = get_global_id(0);
    if (i >= n) return;
    __global const uint* w = in + 16 * (size_t)i;
    __global uint* o = out + 20 * (size_t)i;
    const float4 inc = ld4(w), N = ld4(w + 4), refl = ld4(w + 8);
    Material m;
    m.simpleColor = (float4)(1.0f); m.textureName = 0; m.opacity = 0; m.textureId = 0; m.isSimpleColor = true; m.hasAlphaMap = false;
    for (int k = 0; k < 20; k++) o[k] = 0;
    m.type = MAT_GLASS;
    o[0] = as_uint(Material_FresnelGlassReflectionFraction(&m, &inc, &N));
    m.type = MAT_VARNHISHED;
    float4 unused = (float4)(0.0f);
    o[1] = as_uint(Material_FresnelVarnishReflectionFraction(&m, &inc, &N, false, &unused));
    m.type = MAT_WATER;
    float4 refracted = (float4)(0.0f);
    float factor = 0.0f;
    o[2] = as_uint(Material_FresnelWaterReflectionFraction(&m, &inc, &N, w[13] != 0, &refracted, &factor));
    st4(o + 3, refracted);
    o[7] = as_uint(factor);
    m.type = (MaterialType)w[12];
    o[8] = as_uint(Material_BRDF(&m, &inc, &N, &refl));
    st4(o + 9, Material_FresnelReflection(&m, &inc, &N));
    float4 v = refl;
    Vector_PutInSameHemisphereAs(&v, &N);
    st4(o + 13, v);
}

// in [12]: seed, N[4], 7 unused here;  out [12]: random(), the seed after it, 0, 0, Material_CosineSampleHemisphere[4], the seed after it
__kernel void unit_sampling(__global const uint* in, __global uint* out, uint n)
{
    const uint i = get_global_id(0);
    if (i >= n) return;
    __global const uint* w = in + 12 * (size_t)i;
    __global uint* o = out + 12 * (size_t)i;
    for (int k = 0; k < 12; k++) o[k] = 0;
    int seed = (int)w[0];
    o[0] = as_uint(random(&seed));
    o[1] = (uint)seed;
    seed = (int)w[0];
    const float4 N = ld4(w + 1);
    st4(o + 4, Material_CosineSampleHemisphere(&seed, &N));
    o[8] = (uint)seed;
}

// One 8 x 8 work-group: the work-item IS pixel (gx, gy) of the 8 x 8 JITTERED image this file is compiled for, case gy * 8 + gx.
// in [10]: gx, gy, 8, 8, iteration, sampler, seed, 3 unused here;  out [5]: sampler()'s x, y, the seed after it, 0, 0
__kernel void unit_pixel(__global const uint* in, __global uint* out, uint n)
{
    const uint i = get_global_id(1) * 8 + get_global_id(0);
    if (i >= n) return;
    __global const uint* w = in + 10 * (size_t)i;
    __global uint* o = out + 5 * (size_t)i;
    int seed = (int)w[6];
    Ray3D r;
    const float2 s = sampler(&r, &seed, w[4]);
    o[0] = as_uint(s.x); o[1] = as_uint(s.y); o[2] = (uint)seed; o[3] = 0; o[4] = 0;
}
