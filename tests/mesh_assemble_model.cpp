// mesh_assemble_model.cpp - csrc/mesh_assemble_common.h as a program of its own: the function the assemble kernel of
// ptmi_update_vertices and ptmi_assemble_triangles run, over files of meshes.  tests/test_mesh_assemble_model.py compiles it
// with g++ -ffp-contract=off -fno-fast-math -fsanitize=address,undefined and holds what it writes to the NumPy restatement of
// tests/vertex_update_cases.py.
//
//   mesh_assemble_model <in> <out>
// <in>: blocks, each 8 words (n_triangles, n_vertices, position_stride, normal_stride or 0 for a flat mesh, has_uvp, has_uvn,
// has_mat_neg, has_ids), then indices[3n], positions (n_vertices * position_stride bytes), normals, uvp[3n], uvn[3n],
// mat_pos[n], mat_neg[n], ids[n] - the optional ones only where the header says so.  <out>: the 336-byte records, block after
// block.  Every array is copied into an allocation of exactly its size, so that a read past one is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mesh_assemble_common.h"

namespace {

struct Block {
    std::unique_ptr<char[]> bytes;
    size_t size = 0;
    template <class T>
    const T* as() const { return reinterpret_cast<const T*>(bytes.get()); }
};

bool read_exact(FILE* f, size_t size, Block& b)
{
    b.bytes.reset(new char[size ? size : 1]);
    b.size = size;
    return size == 0 || std::fread(b.bytes.get(), 1, size, f) == size;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t h[8];
    while (std::fread(h, 4, 8, in) == 8) {
        const uint32_t n = h[0], n_vertices = h[1], position_stride = h[2], normal_stride = h[3];
        Block indices, positions, normals, uvp, uvn, mat_pos, mat_neg, ids;
        bool ok = read_exact(in, (size_t)n * 12, indices) && read_exact(in, (size_t)n_vertices * position_stride, positions);
        ok = ok && read_exact(in, (size_t)n_vertices * normal_stride, normals);
        ok = ok && read_exact(in, h[4] ? (size_t)n * 24 : 0, uvp) && read_exact(in, h[5] ? (size_t)n * 24 : 0, uvn);
        ok = ok && read_exact(in, (size_t)n * 4, mat_pos) && read_exact(in, h[6] ? (size_t)n * 4 : 0, mat_neg);
        ok = ok && read_exact(in, h[7] ? (size_t)n * 4 : 0, ids);
        if (!ok) return 3;
        std::vector<ptmi_triangle> records(n);
        for (uint32_t i = 0; i < n; i++) {
            ptmi_mesh::Corner c[3] = {};
            for (int k = 0; k < 3; k++) {
                const uint32_t v = indices.as<uint32_t>()[3 * i + k];
                if (v >= n_vertices) return 4;
                c[k].p = ptmi_mesh::fetch3(positions.bytes.get(), position_stride, v, 1.f);
                if (normal_stride) c[k].m = ptmi_mesh::fetch3(normals.bytes.get(), normal_stride, v, 0.f);
                if (h[4]) c[k].uvp = uvp.as<ptmi_float2>()[3 * i + k];
                c[k].uvn = h[5] ? uvn.as<ptmi_float2>()[3 * i + k] : c[k].uvp;
            }
            const uint32_t mp = mat_pos.as<uint32_t>()[i];
            ptmi_mesh::assemble_triangle(c[0], c[1], c[2], normal_stride == 0, mp, h[6] ? mat_neg.as<uint32_t>()[i] : mp,
                                         h[7] ? ids.as<uint32_t>()[i] : i, ptmi_mesh::RecordInMemory{&records[i]});
        }
        if (n && std::fwrite(records.data(), sizeof(ptmi_triangle), n, out) != n) return 5;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 5;
}
