// material_screen_model.cpp - the host side of ptmi_update_materials / ptmi_update_lights as a program of its own, compiled by
// tests/test_scene_edit_model.py with -fsanitize=address,undefined together with csrc/scene_refit_host.cpp and
// csrc/scene_layout.cpp.  Two things:
//
//   material_screen_model screen <file>
//     The verdict of the screen kernel of ptmi_update_materials (csrc/scene_refit_common.h: screen_shade_materials, the function
//     csrc/scene_refit.hip runs lane by lane on DShade records) against build_layout's on the triangle the record was made from
//     (screen_materials).  The file holds blocks of
//         uint32 n_triangles, n_materials, 0, 0;  n_materials bytes (is_simple_color), padded to a multiple of 16;
//         n_triangles records of ptmi_triangle
//     and per block two lines are printed: the verdict word of the whole array in hex, the status and the message; then one
//     digit per triangle, its code.  Exit status 4 where the two functions disagree on a triangle.
//
//   material_screen_model plain
//     DScene::plain_shading: kernel_choice.h: scene_plain_shading on the types as given, against what build_layout reports for
//     a scene of those materials and lights, over every combination of 0..2 materials (STANDART or GLASS, plain or textured),
//     0..2 lights (POINT or another type) and the PTMI_GENERIC_SHADING switch.  One line per combination:
//         n_materials type0 simple0 type1 simple1 n_lights light0 light1 switch : layout function
//     Exit status 5 where build_layout fails, 6 where the two disagree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernel_choice.h"
#include "scene_layout.h"
#include "scene_refit.h"
#include "scene_refit_common.h"

using namespace ptmi_internal;

void ptmi_internal::set_global_error(const std::string&) {}

static int screen(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    uint32_t head[4];
    while (std::fread(head, 4, 4, f) == 4) {
        std::vector<uint8_t> simple((head[1] + 15u) / 16u * 16u);
        if (!simple.empty() && std::fread(simple.data(), 1, simple.size(), f) != simple.size()) return 3;
        simple.resize(head[1]);
        std::vector<ptmi_triangle> tris(head[0]);
        if (head[0] && std::fread(static_cast<void*>(tris.data()), sizeof(ptmi_triangle), head[0], f) != head[0]) return 3;
        // the records as a context holds them, and lane by lane, as the kernel takes them: the smallest word wins
        std::vector<DShade> shade(head[0]);
        std::string codes;
        uint32_t word = ptmi_refit::kScreenAccepted;
        for (uint32_t i = head[0]; i-- > 0;) {
            ptmi_refit::make_shade_record(tris[i], &shade[i]);
            const uint32_t code = ptmi_refit::screen_shade_record(shade[i], simple.data(), head[1]);
            if (code != ptmi_refit::screen_materials(tris[i], simple.data(), head[1])) return 4;
            if (code != ptmi_refit::kScreenOk && ptmi_refit::screen_word(i, code) < word) word = ptmi_refit::screen_word(i, code);
            codes.insert(codes.begin(), (char)('0' + code));
        }
        // build_layout's loop over the triangles, which stops at the first refusal, says the same with the same words
        std::string a, b;
        int rc = PTMI_OK;
        for (uint32_t i = 0; i < head[0] && rc == PTMI_OK; i++) rc = check_triangle_materials(tris[i], i, simple.data(), head[1], a);
        if (screen_verdict(word, b) != rc || a != b) return 4;
        std::printf("%08x %d %s\n%s\n", word, rc, b.c_str(), codes.c_str());
    }
    std::fclose(f);
    return 0;
}

static int plain()
{
    const int32_t material_types[2] = {PTMI_MAT_STANDART, PTMI_MAT_GLASS};
    const int32_t light_types[2][2] = {{PTMI_LIGHT_POINT, PTMI_LIGHT_SPOT}, {PTMI_LIGHT_POINT, PTMI_LIGHT_DIRECTIONNAL}};
    ptmi_node leaf{};
    leaf.is_leaf = 1;
    const ptmi_texture one_texel{1, 1, 0};
    const ptmi_uchar4 texel{1, 2, 3, 4};
    ptmi_sky sky{};
    for (ptmi_texture& face : sky.sky_textures) face = one_texel;
    for (uint32_t n_materials = 0; n_materials <= 2; n_materials++)
        for (uint32_t n_lights = 0; n_lights <= 2; n_lights++)
            for (uint32_t bits = 0; bits < (1u << (2 * n_materials + n_lights + 1)); bits++) {
                ptmi_material materials[2] = {};
                ptmi_light lights[2] = {};
                int32_t types[2] = {}, of_lights[2] = {};
                uint8_t simple[2] = {};
                uint32_t b = bits;
                for (uint32_t i = 0; i < n_materials; i++, b >>= 2) {
                    materials[i].type = types[i] = material_types[b & 1];
                    materials[i].is_simple_color = simple[i] = (b >> 1) & 1;
                    materials[i].texture_id = 0;
                }
                for (uint32_t i = 0; i < n_lights; i++, b >>= 1) lights[i].type = of_lights[i] = light_types[i][b & 1];
                const int generic = b & 1;
                if (generic) setenv("PTMI_GENERIC_SHADING", "1", 1);
                else unsetenv("PTMI_GENERIC_SHADING");
                ptmi_config cfg{};
                cfg.struct_size = sizeof cfg;
                cfg.image_width = cfg.image_height = 8;
                cfg.ray_max_depth = 1;
                cfg.lights_size = n_lights;
                ptmi_scene sc{};
                sc.struct_size = sizeof sc;
                sc.bvh = &leaf;
                sc.bvh_size = 1;
                sc.lights = lights;
                sc.lights_size = n_lights;
                sc.materiaux = materials;
                sc.materiaux_size = n_materials;
                sc.textures = &one_texel;
                sc.textures_size = 1;
                sc.textures_data = &texel;
                sc.textures_data_size = 1;
                sc.sky = &sky;
                sc.camera_direction = ptmi_float4{0, 1, 0, 0};
                Relayout lay;
                std::string err;
                if (build_layout(cfg, &sc, lay, err) != PTMI_OK) {
                    std::fprintf(stderr, "build_layout: %s\n", err.c_str());
                    return 5;
                }
                ptmi_switches::Switches upload;
                upload.generic_shading = generic;
                const bool by_function = ptmi_choice::scene_plain_shading(types, simple, n_materials, of_lights, n_lights, upload);
                std::printf("%u %d %u %d %u %u %d %d %d : %d %d\n", n_materials, types[0], simple[0], types[1], simple[1], n_lights, of_lights[0],
                            of_lights[1], generic, lay.plain_shading ? 1 : 0, by_function ? 1 : 0);
                if (lay.plain_shading != by_function) return 6;
            }
    unsetenv("PTMI_GENERIC_SHADING");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && std::strcmp(argv[1], "screen") == 0) return screen(argv[2]);
    if (argc == 2 && std::strcmp(argv[1], "plain") == 0) return plain();
    return 2;
}
