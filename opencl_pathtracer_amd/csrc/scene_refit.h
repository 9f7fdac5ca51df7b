// scene_refit.h - updating a loaded scene in place: the host side without a device call (scene_refit_host.cpp: ptmi_bvh_refit, the
// screen of new triangles, the schedule of the device refit) and the launches of scene_refit.hip.  See DESIGN.md 1b.
#pragma once

#include <string>
#include <vector>

#include "ptmi.h"
#include "ptmi_internal.h"

namespace ptmi_internal {

// What ptmi_update_triangles has to know about the scene a context holds, kept by ptmi_initialize_memory (a few bytes per
// material: a context that never updates pays nothing else).
struct UpdateFacts {
    uint32_t triangulation_size = 0;
    uint32_t n_big_leaves = 0;
    bool tris_precomputed = false;
    std::vector<uint8_t> material_is_simple_color;
    // ptmi_update_materials, ptmi_update_lights, ptmi_set_sky: the rest of what DScene::plain_shading was decided from (a
    // material's type, a light's type: kernel_choice.h: scene_plain_shading), and the extents a texture id and a sky face are
    // checked against.  The three calls keep these, and the line above, in step with what the devices hold.
    std::vector<int32_t> material_type, light_type;
    uint32_t textures_size = 0, textures_data_size = 0;
};

// The screen of ptmi_update_triangles, applied before the first device write: build_layout's checks on triangles (materials,
// texture coordinates: PTMI_ERR_BAD_SCENE) and what an update cannot express without a new upload (PTMI_ERR_UNSUPPORTED): a record
// that could yield NaN distances (the kernel instantiation was chosen at upload), unequal w where the records are DTriPre, an
// aabb that is marked empty, not finite or not ordered (the references' empty flags and boxes_ordered are upload-time facts).
int screen_update(const UpdateFacts& facts, const ptmi_triangle* triangulation, uint32_t triangulation_size, std::string& err);
// ... in its two halves, which the device form shares (scene_refit_common.h: ScreenCode, one classification for host and device):
// the verdict on the whole array as one word - (index << 4) | code of the first refused triangle, or kScreenAccepted - and the
// status and message of such a word, whoever computed it (the loop here, or the screen kernel below).
uint32_t screen_update_word(const UpdateFacts& facts, const ptmi_triangle* triangulation, uint32_t triangulation_size);
int screen_verdict(uint32_t word, std::string& err);

// The inner records of the one record array by depth (root = level 0): level k is nodes[first[k] .. first[k + 1]).  A level pass
// of the refit reads the records of the level below and writes its own, so the passes run from the last level to level 0.
struct RefitSchedule {
    std::vector<uint32_t> nodes;
    std::vector<uint32_t> first;  // levels() + 1 entries
    uint32_t levels() const { return first.empty() ? 0u : (uint32_t)first.size() - 1u; }
};

// Walks the records top-down from root_ref and checks everything the refit kernels will index (record and triangle indices,
// leaf ranges, big_leaves, a record reached twice) and that a reference is flagged empty exactly where nothing lies below it -
// what ptmi_bvh_refit's tree would say.  PTMI_ERR_UNSUPPORTED where the uploaded tree says otherwise, PTMI_ERR_INTERNAL for
// an index out of range (the records are the library's own).
int build_refit_schedule(const DNode* records, const uint32_t* tri_ids, uint32_t n_records, const DBigLeaf* big_leaves,
                         uint32_t n_big_leaves, uint32_t root_ref, uint32_t triangulation_size, RefitSchedule& out, std::string& err);

// ---- scene_refit.hip: every launch is asynchronous on `stream`; the caller's bounds are the schedule's ---------------------
// The screen on the device (ptmi_update_triangles_device): *verdict = min(*verdict, the word of every refused triangle of
// triangulation[0 .. triangulation_size)), so a word the caller has set to kScreenAccepted ends as screen_update_word's.
// material_is_simple_color: one byte per material, on the device.  Reads the triangles, writes the one word.
int launch_screen_update(const ptmi_triangle* triangulation, uint32_t triangulation_size, const uint8_t* material_is_simple_color,
                         uint32_t materiaux_size, bool tris_precomputed, uint32_t* verdict, void* stream, std::string* err);
// The screen of ptmi_update_materials: the same protocol over the DShade records a device holds, shade[0 .. triangulation_size):
// the word ends as that of the first triangle whose materials are out of range or, one of them textured under
// material_is_simple_color, whose texture coordinates are not finite or beyond 2^30.  Reads the records, writes the one word.
int launch_screen_shade(const DShade* shade, uint32_t triangulation_size, const uint8_t* material_is_simple_color, uint32_t materiaux_size,
                        uint32_t* verdict, void* stream, std::string* err);
// records[r] = the DTri (or DTriPre, strict reciprocal) record of triangulation[tri_ids[r]] where tri_ids[r] < triangulation_size
// (a node record's is 0xFFFFFFFF)
int launch_update_tri_records(DTri* records, const uint32_t* tri_ids, uint32_t n_records, const ptmi_triangle* triangulation,
                              uint32_t triangulation_size, bool tris_precomputed, void* stream, std::string* err);
// shade[i] = the DShade record of triangulation[i]
int launch_update_shade_records(DShade* shade, const ptmi_triangle* triangulation, uint32_t triangulation_size, void* stream, std::string* err);
// one level pass: both child boxes of records[level_nodes[k]], k < n
int launch_refit_level(DNode* records, const uint32_t* level_nodes, uint32_t n, const DBigLeaf* big_leaves, const uint32_t* tri_ids,
                       const ptmi_triangle* triangulation, void* stream, std::string* err);

}  // namespace ptmi_internal
