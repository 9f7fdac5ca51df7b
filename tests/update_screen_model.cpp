// update_screen_model.cpp - the screen of an in-place triangle update on the host, as a program of its own: the classification
// of csrc/scene_refit_common.h (screen_triangle: the function the screen kernel of csrc/scene_refit.hip runs lane by lane) and
// the host loop and formatter around it (csrc/scene_refit_host.cpp, csrc/scene_layout.cpp), compiled together with those two
// files by tests/test_update_screen_model.py with -fsanitize=address,undefined.
//
// Reads the file named on the command line: blocks of
//     uint32 n_triangles, n_materials, tris_precomputed, 0;  n_materials bytes (is_simple_color), padded to a multiple of 16;
//     n_triangles records of ptmi_triangle
// and prints one line per block: the verdict word of the whole array in hex, the status, the message.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scene_layout.h"
#include "scene_refit.h"
#include "scene_refit_common.h"

using namespace ptmi_internal;

void ptmi_internal::set_global_error(const std::string&) {}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[4];
    while (std::fread(head, 4, 4, f) == 4) {
        UpdateFacts facts;
        facts.triangulation_size = head[0];
        facts.tris_precomputed = head[2] != 0;
        std::vector<uint8_t> simple((head[1] + 15u) / 16u * 16u);
        if (!simple.empty() && std::fread(simple.data(), 1, simple.size(), f) != simple.size()) return 3;
        facts.material_is_simple_color.assign(simple.begin(), simple.begin() + head[1]);
        // (operator new: aligned for a 16-byte aligned record)
        std::vector<ptmi_triangle> tris(head[0]);
        if (head[0] && std::fread(static_cast<void*>(tris.data()), sizeof(ptmi_triangle), head[0], f) != head[0]) return 3;
        // lane by lane, as the kernel takes them: every triangle gets its verdict, the smallest word wins
        uint32_t word = ptmi_refit::kScreenAccepted;
        for (uint32_t i = head[0]; i-- > 0;) {
            const uint32_t code = ptmi_refit::screen_triangle(tris[i], facts.material_is_simple_color.data(), head[1], facts.tris_precomputed);
            if (code != ptmi_refit::kScreenOk && ptmi_refit::screen_word(i, code) < word) word = ptmi_refit::screen_word(i, code);
        }
        // the host loop, which stops at the first refusal, and its words
        if (screen_update_word(facts, tris.data(), head[0]) != word) return 4;
        std::string a, b;
        const int rc = screen_update(facts, tris.data(), head[0], a);
        if (screen_verdict(word, b) != rc || a != b) return 5;
        std::printf("%08x %d %s\n", word, rc, a.c_str());
    }
    std::fclose(f);
    return 0;
}
