// mesh_assemble_common.h - one 336-byte ptmi_triangle from the three corners of an indexed face: the importer's Triangle_Create
// (Maya/PathTracer_MayaImporter.cpp:943-1047) as ONE function for the host (ptmi_assemble_triangles), the assemble kernel of
// ptmi_update_vertices (mesh_assemble.hip) and the program of the tests (tests/mesh_assemble_model.cpp).  include/ptmi.h states
// the contract; DESIGN.md 1j the layout around it.
//
// Every operation below is one IEEE binary32 operation in the written order.  Compile with -ffp-contract=off and without
// fast-math (host and device): `/` and sqrtf are then the correctly rounded ones, and denormals are kept.  The arithmetic is the
// HOST importer's, so it is the same in both arithmetic modes of a context.
#ifndef PTMI_MESH_ASSEMBLE_COMMON_H
#define PTMI_MESH_ASSEMBLE_COMMON_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "ptmi_hd.h"
#include "ptmi_scene.h"

namespace ptmi_mesh {

// What a face brings per corner, in the face's own winding: the point (w = 1), the vertex normal as given (w = 0; unused where
// the mesh is flat) and the two texture coordinates.
struct Corner {
    ptmi_float4 p, m;
    ptmi_float2 uvp, uvn;
};

PTMI_HD float dot3(const ptmi_float4& a, const ptmi_float4& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// std::min / std::max of the reference's BoundingBox_Create (Structs.h:197-205): of two values that compare equal the FIRST
PTMI_HD float min_first(float a, float b) { return b < a ? b : a; }
PTMI_HD float max_first(float a, float b) { return a < b ? b : a; }
PTMI_HD ptmi_float4 min4(const ptmi_float4& a, const ptmi_float4& b)
{
    return {min_first(a.x, b.x), min_first(a.y, b.y), min_first(a.z, b.z), min_first(a.w, b.w)};
}
PTMI_HD ptmi_float4 max4(const ptmi_float4& a, const ptmi_float4& b)
{
    return {max_first(a.x, b.x), max_first(a.y, b.y), max_first(a.z, b.z), max_first(a.w, b.w)};
}

// Vector_LexLessThan (PathTracer_Utils.h:151)
PTMI_HD bool lex_less(const ptmi_float4& a, const ptmi_float4& b)
{
    return (a.x < b.x) || ((a.x == b.x) && (a.y < b.y)) || ((a.x == b.x) && (a.y == b.y) && (a.z < b.z));
}

// :1030-1036 - a vertex normal shorter than one half gives way to N (which carries w = 1), any other is divided by its length in
// all four components
PTMI_HD ptmi_float4 shading_normal(const ptmi_float4& m, const ptmi_float4& N)
{
    const float l = sqrtf(dot3(m, m));
    if (l < 0.5f) return N;
    return {m.x / l, m.y / l, m.z / l, m.w / l};
}

// Where a record goes, as its 21 sixteen-byte words in ascending order (ptmi_scene.h: s1 s2 s3 | n1 n2 n3 | t1..bt3 | n |
// uvp1 uvp2 | uvp3 uvn1 | uvn2 uvn3 | pMin | pMax | centroid | isEmpty and padding | mat_pos mat_neg id padding): a sink has
// f4(k, value) for a word of floats and u4(k, x, y, z, w) for a word of integers.  The record is never an object of the
// function, so that a lane of the kernel keeps it in registers.  This one writes a record in host memory.
struct RecordInMemory {
    ptmi_triangle* t;
    void f4(int k, const ptmi_float4& v) const { std::memcpy(reinterpret_cast<char*>(t) + 16 * k, &v, 16); }
    void u4(int k, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const
    {
        const uint32_t v[4] = {x, y, z, w};
        std::memcpy(reinterpret_cast<char*>(t) + 16 * k, v, 16);
    }
};

// Triangle_Create of the face (c0, c1, c2) into `sink`.  flat: the mesh has no normal buffer and every corner's normal is
// (N.xyz, 0).  All 336 bytes are written: T1..BT3 are +0 (the integrator never reads them), every padding byte is 0.
template <class Sink>
PTMI_HD void assemble_triangle(Corner c0, Corner c1, Corner c2, bool flat, uint32_t mat_pos, uint32_t mat_neg, uint32_t id, const Sink& sink)
{
    // BoundingBox_Create, all four components
    const ptmi_float4 lo = min4(min4(c0.p, c1.p), c2.p), hi = max4(max4(c0.p, c1.p), c2.p);
    const ptmi_float4 centroid = {(lo.x + hi.x) / 2.f, (lo.y + hi.y) / 2.f, (lo.z + hi.z) / 2.f, (lo.w + hi.w) / 2.f};
    // N = normalize(cross(s2 - s1, s3 - s1)) in the face's winding; the host's normalize leaves w, which is 1
    const float e1x = c1.p.x - c0.p.x, e1y = c1.p.y - c0.p.y, e1z = c1.p.z - c0.p.z;
    const float e2x = c2.p.x - c0.p.x, e2y = c2.p.y - c0.p.y, e2z = c2.p.z - c0.p.z;
    const ptmi_float4 c = {e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x, 0.f};
    const float l = sqrtf(dot3(c, c));
    const ptmi_float4 N = {c.x / l, c.y / l, c.z / l, 1.f};
    if (flat) c0.m = c1.m = c2.m = {N.x, N.y, N.z, 0.f};
    // the cascade of :961-1020, its six outcomes as written there: (a, b, d) = the corners as S1, S2, S3
    Corner a, b, d;
    if (lex_less(c0.p, c1.p)) {
        if (lex_less(c1.p, c2.p)) { a = c0; b = c1; d = c2; }
        else if (lex_less(c0.p, c2.p)) { a = c0; b = c2; d = c1; }
        else { a = c2; b = c0; d = c1; }
    } else {
        if (lex_less(c0.p, c2.p)) { a = c1; b = c0; d = c2; }
        else if (lex_less(c1.p, c2.p)) { a = c1; b = c2; d = c0; }
        else { a = c2; b = c1; d = c0; }
    }
    const ptmi_float4 zero = {0.f, 0.f, 0.f, 0.f};
    sink.f4(0, a.p); sink.f4(1, b.p); sink.f4(2, d.p);
    sink.f4(3, shading_normal(a.m, N)); sink.f4(4, shading_normal(b.m, N)); sink.f4(5, shading_normal(d.m, N));
    for (int k = 6; k < 12; k++) sink.f4(k, zero);
    sink.f4(12, N);
    sink.f4(13, {a.uvp.x, a.uvp.y, b.uvp.x, b.uvp.y});
    sink.f4(14, {d.uvp.x, d.uvp.y, a.uvn.x, a.uvn.y});
    sink.f4(15, {b.uvn.x, b.uvn.y, d.uvn.x, d.uvn.y});
    sink.f4(16, lo); sink.f4(17, hi); sink.f4(18, centroid);
    sink.u4(19, 0u, 0u, 0u, 0u);  // isEmpty = 0 and the box's padding
    sink.u4(20, mat_pos, mat_neg, id, 0u);
}

static_assert(sizeof(ptmi_triangle) == 21 * 16 && offsetof(ptmi_triangle, n1) == 3 * 16 && offsetof(ptmi_triangle, t1) == 6 * 16 &&
              offsetof(ptmi_triangle, n) == 12 * 16 && offsetof(ptmi_triangle, uvp1) == 13 * 16 && offsetof(ptmi_triangle, uvp3) == 14 * 16 &&
              offsetof(ptmi_triangle, uvn2) == 15 * 16 && offsetof(ptmi_triangle, aabb) == 16 * 16 && offsetof(ptmi_triangle, mat_pos) == 20 * 16 &&
              offsetof(ptmi_triangle, id) == 20 * 16 + 8, "the 21 words of assemble_triangle");

// A vertex attribute of the caller's buffers: three floats at base + v * stride (stride a multiple of 4, so the floats are
// aligned); whatever else the stride holds is never read.
PTMI_HD ptmi_float4 fetch3(const void* base, uint32_t stride, uint32_t v, float w)
{
    const float* const f = reinterpret_cast<const float*>(static_cast<const char*>(base) + (size_t)v * stride);
    return {f[0], f[1], f[2], w};
}

}  // namespace ptmi_mesh

#endif  // PTMI_MESH_ASSEMBLE_COMMON_H
