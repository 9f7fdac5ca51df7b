// scene_refit_model.cpp - the device side of ptmi_update_triangles (csrc/scene_refit.hip), run serially on the host from the
// same __host__ __device__ header (csrc/scene_refit_common.h) and the same schedule (csrc/scene_refit_host.cpp), on the records
// build_layout makes (csrc/scene_layout.cpp) - compiled together with those two files by tests/test_scene_refit_model.py.
//
// A "lane" here is a loop trip.  What the model adds is the ORDER of the trips: the records, the triangles and the inner records
// of a level are taken in ascending order, in descending order or shuffled (order_seed 0, 1, other), since nothing on the device
// fixes the order inside a launch; the levels run from the deepest to the root, one after the other, as the launches do.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "scene_layout.h"
#include "scene_refit.h"
#include "scene_refit_common.h"

using namespace ptmi_internal;

static std::string g_error;
void ptmi_internal::set_global_error(const std::string& msg) { g_error = msg; }

namespace {

struct Layout {
    Relayout lay;
    uint32_t n_triangles = 0;
};

std::vector<uint32_t> trip_order(uint32_t n, uint32_t seed)
{
    std::vector<uint32_t> o(n);
    std::iota(o.begin(), o.end(), 0u);
    if (seed == 1) std::reverse(o.begin(), o.end());
    if (seed > 1) {
        uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
        for (uint32_t i = n; i > 1; i--) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(o[i - 1], o[(uint32_t)((s >> 33) % i)]);
        }
    }
    return o;
}

}  // namespace

extern "C" {

const char* model_error() { return g_error.c_str(); }

// build_layout's result for `scene` (what ptmi_initialize_memory uploads), or NULL with *status and model_error() set
// (a scene that the one-path-per-lane kernel renders, literal_kernel_reason, cannot be updated in place: refused here, where the
// layouts are made for model_update)
static void* layout_of(const ptmi_config* cfg, const ptmi_scene* scene, int* status, bool for_update)
{
    Layout* l = new Layout();
    *status = build_layout(*cfg, scene, l->lay, g_error);
    if (for_update && *status == PTMI_OK && !l->lay.literal_kernel_reason.empty()) { *status = PTMI_ERR_UNSUPPORTED; g_error = l->lay.literal_kernel_reason; }
    if (*status != PTMI_OK) { delete l; return nullptr; }
    l->n_triangles = scene->triangulation_size;
    return l;
}
void* model_layout(const ptmi_config* cfg, const ptmi_scene* scene, int* status) { return layout_of(cfg, scene, status, true); }
// ... and for any scene ptmi_initialize_memory accepts: what it uploads, to be read and never updated
void* model_layout_uploaded(const ptmi_config* cfg, const ptmi_scene* scene, int* status) { return layout_of(cfg, scene, status, false); }
void model_layout_free(void* h) { delete static_cast<Layout*>(h); }

// info: n_records, n_triangles, n_big_leaves, root_ref, tris_precomputed, max_depth
void model_layout_info(void* h, uint32_t info[6])
{
    const Layout& l = *static_cast<Layout*>(h);
    info[0] = (uint32_t)l.lay.recs.size(); info[1] = l.n_triangles; info[2] = (uint32_t)l.lay.big_leaves.size();
    info[3] = l.lay.root_ref; info[4] = l.lay.tris_precomputed; info[5] = l.lay.max_depth;
}
// recs: 64 bytes each; tri_ids: 4; shade: 112; big_leaves: 8
void model_layout_copy(void* h, void* recs, void* tri_ids, void* shade, void* big_leaves)
{
    const Layout& l = *static_cast<Layout*>(h);
    std::memcpy(recs, l.lay.recs.data(), l.lay.recs.size() * sizeof(DTri));
    std::memcpy(tri_ids, l.lay.tri_ids.data(), l.lay.tri_ids.size() * 4);
    std::memcpy(shade, l.lay.shade.data(), l.lay.shade.size() * sizeof(DShade));
    std::memcpy(big_leaves, l.lay.big_leaves.data(), l.lay.big_leaves.size() * sizeof(DBigLeaf));
}

// ptmi_update_triangles on the layout, in place: the screen, the schedule, then the three kernels' work.  *levels = the level
// passes (ptmi_update_info.levels).
int model_update(void* h, const ptmi_triangle* tris, uint32_t n, uint32_t order_seed, uint32_t* levels)
{
    Layout& l = *static_cast<Layout*>(h);
    Relayout& lay = l.lay;
    if (!tris || n != l.n_triangles) { g_error = "wrong count"; return PTMI_ERR_INVALID_ARGUMENT; }
    UpdateFacts facts;
    facts.triangulation_size = n;
    facts.n_big_leaves = (uint32_t)lay.big_leaves.size();
    facts.tris_precomputed = lay.tris_precomputed;
    facts.material_is_simple_color = lay.material_is_simple_color;
    if (int rc = screen_update(facts, tris, n, g_error)) return rc;
    DNode* const nodes = reinterpret_cast<DNode*>(lay.recs.data());
    const uint32_t n_records = (uint32_t)lay.recs.size();
    RefitSchedule schedule;
    if (int rc = build_refit_schedule(nodes, lay.tri_ids.data(), n_records, lay.big_leaves.data(), facts.n_big_leaves, lay.root_ref, n,
                                      schedule, g_error))
        return rc;
    // record kernel: one lane per record
    for (uint32_t r : trip_order(n_records, order_seed)) {
        const uint32_t id = lay.tri_ids[r];
        if (id == 0xFFFFFFFFu) continue;
        if (lay.tris_precomputed) ptmi_refit::make_tri_record_pre(tris[id], reinterpret_cast<DTriPre*>(&lay.recs[r]));
        else ptmi_refit::make_tri_record(tris[id], &lay.recs[r]);
    }
    // shade kernel: one lane per triangle
    for (uint32_t i : trip_order(n, order_seed)) ptmi_refit::make_shade_record(tris[i], &lay.shade[i]);
    // refit kernel: one launch per level, deepest first
    for (uint32_t level = schedule.levels(); level-- > 0;) {
        const uint32_t* list = schedule.nodes.data() + schedule.first[level];
        for (uint32_t k : trip_order(schedule.first[level + 1] - schedule.first[level], order_seed + (order_seed > 1 ? level : 0))) {
            DNode d = nodes[list[k]];  // (the lane's copy of the record: four 16-byte loads, four stores)
            ptmi_refit::refit_record(&d, nodes, lay.big_leaves.data(), lay.tri_ids.data(), tris);
            nodes[list[k]] = d;
        }
    }
    *levels = schedule.levels();
    return PTMI_OK;
}

}  // extern "C"
