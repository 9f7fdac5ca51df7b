// scene_layout.h - validation and re-layout of a scene for the device: host code without a device call (scene_layout.cpp).
// Used by ptmi_initialize_memory (ptmi_scene_memory.cpp) and, on its own, by ptmi_validate_scene - which is also how the tests run it
// under AddressSanitizer on a box without a GPU.
#pragma once

#include <string>
#include <vector>

#include "ptmi.h"
#include "ptmi_internal.h"

namespace ptmi_internal {

// Everything the kernel will index is checked so that a malformed scene is an error code, not a GPU fault.
struct Relayout {
    std::vector<DTri> recs;          // the traversal's one array: DNode and DTri/DTriPre records interleaved
    std::vector<uint32_t> tri_ids;   // per record: index into triangulation[] / shade[] (0xFFFFFFFF for a node)
    std::vector<DTri> tris;          // per input triangle, only a staging area for recs
    std::vector<DShade> shade;
    std::vector<DMat> mats;
    std::vector<uint8_t> material_is_simple_color;  // per material: what check_triangle_materials asks
    std::vector<int32_t> material_type, light_type;  // per material / light: with the line above, what plain_shading was decided from
    std::vector<DBigLeaf> big_leaves;
    bool tris_precomputed = false;
    bool plain_shading = false; // every material a plain-colour MAT_STANDART, every light a LIGHT_POINT
    bool boxes_ordered = true;  // all non-empty child boxes finite with pMin <= pMax
    uint32_t cullable_leaves = 0;  // leaves whose record bit says the kernel may count them untested (leaf_cull.h)
    std::string literal_kernel_reason;  // scene_needs_literal_kernel()
    uint32_t root_ref = 0;
    uint32_t max_depth = 0;
    // What a closest-hit query makes of a ray whose direction is not a number in ANY component (every comparison of the box
    // test and of the triangle test is false: every non-empty box is "hit", every triangle accepted): it walks the whole tree
    // in one fixed order and returns its LAST triangle.  The walk's box tests, triangle tests and last triangle (a record
    // index; 0xFFFFFFFF: the walk meets no triangle), so that the literal loops can skip it (ptmi_literal_path.hpp).
    uint32_t nan_walk_box_tests = 0, nan_walk_tri_tests = 0, nan_walk_last_tri = 0xFFFFFFFFu;
};

// The per-record parts of the validation, which an in-place update applies to new cameras and triangles (scene_refit_host.cpp):
// why the camera / triangle `i` can make a triangle test compute a NaN distance (empty: it cannot; scene_layout.cpp:
// scene_needs_literal_kernel), and whether the triangle's materials exist and its texture coordinates can index texels.
// The triangle's two are callers of the one classification the device shares (scene_refit_common.h: ScreenCode), and
// screen_refusal is its formatter: the status and the words for code `code` on triangle `i` (PTMI_OK and `err` untouched for
// kScreenOk).
int screen_refusal(uint32_t code, uint32_t i, std::string& err);
std::string camera_needs_literal_kernel(const ptmi_float4& position, const ptmi_float4& direction, const ptmi_float4& right, const ptmi_float4& up);
std::string triangle_needs_literal_kernel(const ptmi_triangle& t, uint32_t i);
int check_triangle_materials(const ptmi_triangle& t, uint32_t i, const uint8_t* material_is_simple_color, uint32_t materiaux_size, std::string& err);

// What build_layout asks of a material, of the lights and of the sky, one call each, for the in-place edits of a loaded scene
// (ptmi_update_materials, ptmi_update_lights, ptmi_set_sky), which ask the same with the same words: material `i`'s texture among
// `textures_size` textures (PTMI_ERR_BAD_SCENE); why the lights can make a triangle test compute a NaN distance (empty: they
// cannot); the six faces of the sky inside `textures_data_size` texels (PTMI_ERR_BAD_SCENE).
int check_material_texture(const ptmi_material& m, uint32_t i, uint32_t textures_size, std::string& err);
std::string lights_need_literal_kernel(const ptmi_light* lights, uint32_t lights_size);
int check_sky_textures(const ptmi_sky& sky, uint32_t textures_data_size, std::string& err);

// Returns PTMI_OK or an error code with its message in `err`.  cfg: lights_size and sampler are read.
int build_layout(const ptmi_config& cfg, const ptmi_scene* sc, Relayout& out, std::string& err);

}  // namespace ptmi_internal
