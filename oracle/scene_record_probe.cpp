// scene_record_probe.cpp - TEST INFRASTRUCTURE: the record arrays a context holds on a device, copied to the host word for word
// (tests/test_scene_records_gpu.py).  Built into build/libscene_record_probe.so by `make probe` with the product's compiler,
// flags and PRIVATE headers (ptmi_context.h, ptmi_internal.h), so it sees a ptmi_ctx as libptmi.so lays it out; it is its own
// library, the product neither links nor loads it, and it is rebuilt whenever one of those headers changes.
//
// It launches no kernel and writes nothing on the device: ptmi_synchronize, hipSetDevice, four device-to-host copies of memory
// the context owns, at the sizes the context's own host copy of DScene and its update facts report.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptmi.h"
#include "ptmi_context.h"
#include "ptmi_internal.h"

using namespace ptmi_internal;

static_assert(sizeof(DTri) == 64 && sizeof(DNode) == 64 && sizeof(DShade) == 112 && sizeof(DBigLeaf) == 8, "record sizes the Python side allocates by");

namespace {

int checked(const ptmi_ctx* ctx, uint32_t device_index)
{
    if (!ctx) return PTMI_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return PTMI_ERR_STATE;
    if (device_index >= ctx->n_dev()) return PTMI_ERR_INVALID_ARGUMENT;
    return PTMI_OK;
}

}  // namespace

extern "C" {

// out: n_records, triangles, n_big_leaves, tris_precomputed, root_ref, listed devices - of the scene the context holds, as listed
// device `device_index` has it.  PTMI_ERR_STATE before ptmi_initialize_memory, PTMI_ERR_INVALID_ARGUMENT for a device index out
// of range (nothing is written then).
int probe_record_sizes(ptmi_ctx* ctx, uint32_t device_index, uint32_t out[6])
{
    if (int rc = checked(ctx, device_index)) return rc;
    if (!out) return PTMI_ERR_INVALID_ARGUMENT;
    const DScene& ds = ctx->dev[device_index].ds;
    out[0] = ds.n_records;
    out[1] = ctx->update.triangulation_size;
    out[2] = ctx->update.n_big_leaves;
    out[3] = ds.tris_precomputed;
    out[4] = ds.root_ref;
    out[5] = ctx->n_dev();
    return PTMI_OK;
}

// recs: 64 bytes x n_records; tri_ids: 4 x n_records; shade: 112 x triangles; big_leaves: 8 x n_big_leaves - buffers of the
// sizes probe_record_sizes reported.  Everything the context has in flight ends first (ptmi_synchronize).
int probe_read_records(ptmi_ctx* ctx, uint32_t device_index, void* recs, void* tri_ids, void* shade, void* big_leaves)
{
    if (int rc = checked(ctx, device_index)) return rc;
    if (!recs || !tri_ids || !shade || !big_leaves) return PTMI_ERR_INVALID_ARGUMENT;
    if (int rc = ptmi_synchronize(ctx)) return rc;
    const DeviceState& d = ctx->dev[device_index];
    const DScene& ds = d.ds;
    const size_t n_records = ds.n_records, n_triangles = ctx->update.triangulation_size, n_big = ctx->update.n_big_leaves;
    if (hipSetDevice(d.device) != hipSuccess) return PTMI_ERR_HIP;
    if (n_records && hipMemcpy(recs, ds.tris, n_records * sizeof(DTri), hipMemcpyDeviceToHost) != hipSuccess) return PTMI_ERR_HIP;
    if (n_records && hipMemcpy(tri_ids, ds.tri_ids, n_records * 4, hipMemcpyDeviceToHost) != hipSuccess) return PTMI_ERR_HIP;
    if (n_triangles && hipMemcpy(shade, ds.shade, n_triangles * sizeof(DShade), hipMemcpyDeviceToHost) != hipSuccess) return PTMI_ERR_HIP;
    if (n_big && hipMemcpy(big_leaves, ds.big_leaves, n_big * sizeof(DBigLeaf), hipMemcpyDeviceToHost) != hipSuccess) return PTMI_ERR_HIP;
    return PTMI_OK;
}

}  // extern "C"
