// bvh_build_device.hip - ptmi_bvh_create_device: the tree of ptmi_bvh_create (bvh_build.cpp), byte for byte, built on
// the device.
//
// Schedule: top-down, one level at a time.  k_level takes every open node of a level, one workgroup per node, and makes
// the decision Builder::build makes there (bvh_build_common.h): the leaf tests, 3 x 64 bins, the scans, the SAH, the best
// split.  It then partitions the node's range as the host's Hoare loop does and writes the two children into the next
// level.  No node's decision depends on another's - except where the host uses the scans of an earlier node for an axis
// skipped at this one; such a node is flagged and the call hands the scene to the host builder (ptmi.h).  When no node is
// open any more, the subtree sizes (k_sizes, bottom-up) give the depth-first pre-order numbers (k_preorder, top-down), and
// k_emit writes the nodes in that order.
//
// Order: every fold of boxes runs in the host's index order.  The bins are folded by one thread per (axis, bin) over the
// node's range in ascending order; the children's centroid boxes are folded in kFoldChunks consecutive chunks and the
// partials merged in chunk order (pbox_merge).  No float atomics; nothing depends on the grid or on the order in which
// workgroups run.  (The child slots of a level are handed out by an atomic counter: that order only decides where a
// node's record lies in the workspace, never a number in the output.)
//
// Partition: the host's loop swaps the k-th right-going triangle among the first L positions (L = left count) with the
// k-th left-going triangle counted from the end of the range, and moves nothing else.  Ranks from prefix counts give the
// same pairs.  The device permutes 4-byte triangle indices; the host applies the permutation to the 336-byte records
// once, at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "bvh_build_common.h"
#include "ptmi.h"
#include "ptmi_internal.h"

using namespace ptmi_bvh;

namespace {

constexpr int kThreads = 256;

// A node of the build, in level order
struct DevNode {
    ptmi_float4 t_min, t_max, t_cen;  // trianglesAABB
    ptmi_float4 c_min, c_max, c_cen;  // centroidsAABB
    uint32_t start, count, cut_axis, depth;
    int32_t leaf;    // -1: inner node; else its stop code
    uint32_t child;  // level-order index of son1 (son2 follows it)
    uint32_t pad[2];
};
static_assert(sizeof(DevNode) == 128, "DevNode");

enum : uint32_t { kFlagStale = 1, kFlagError = 2 };
struct LevelCounters {
    uint32_t next_count;
    uint32_t flags;
    uint32_t max_depth;
    uint32_t pad;
};

__device__ inline ptmi_float4 ld4(const ptmi_float4* p)
{
    const float4 v = *reinterpret_cast<const float4*>(p);
    return { v.x, v.y, v.z, v.w };
}

// exclusive prefix count of `flag` over the workgroup (thread order) and the total; `wsum` is kThreads / 64 words of LDS
__device__ inline uint32_t wg_prefix(bool flag, uint32_t* wsum, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kThreads / 64; w++) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    __syncthreads();
    *total = all;
    return before + below;
}

// The children's centroid box: the fold of the centroids of positions [lo, hi] - ascending, or descending from hi - in
// kFoldChunks consecutive chunks merged in order.
__device__ __forceinline__ PBox fold_centroids(const ptmi_float4* tbox, const uint32_t* perm, uint32_t lo, uint32_t hi, bool descending, PBox* red)
{
    const uint32_t m = hi - lo + 1, len = (m + kFoldChunks - 1) / kFoldChunks;
    const uint32_t t = threadIdx.x;
    PBox acc = pbox_empty();
    for (uint32_t k = t * len; k < m && k < (t + 1) * len; k++) {
        const uint32_t p = descending ? hi - k : lo + k;
        pbox_add_point(acc, ld4(&tbox[3 * (size_t)perm[p] + 2]));
    }
    red[t] = acc;
    __syncthreads();
    for (uint32_t s = 1; s < (uint32_t)kThreads; s *= 2) {
        if ((t & (2 * s - 1)) == 0) red[t] = pbox_merge(red[t], red[t + s]);
        __syncthreads();
    }
    const PBox r = red[0];
    __syncthreads();
    return r;
}

__device__ void write_child(DevNode* out, const PBox& tri, const PBox& cen, uint32_t start, uint32_t count, uint32_t depth)
{
    out->t_min = tri.p_min; out->t_max = tri.p_max; out->t_cen = pbox_centroid(tri);
    out->c_min = cen.p_min; out->c_max = cen.p_max; out->c_cen = pbox_centroid(cen);
    out->start = start; out->count = count; out->cut_axis = 0; out->depth = depth;
    out->leaf = -1; out->child = 0; out->pad[0] = out->pad[1] = 0;
}

struct LevelShared {
    // per batch of kThreads positions
    ptmi_float4 b_min[kThreads], b_max[kThreads], b_cen[kThreads];
    uint8_t bin[3][kThreads];
    // per node
    PBox bins[3][kBins];
    int counts[3][kBins];
    double rpart[3][kBins - 1];
    float sah[3][kBins - 1];
    float k1[3], lo[3];
    int binned[3];
    uint32_t wsum[kThreads / 64];
    int state;  // -1: go on; else stop
    int error;
    int axis, index;
    uint32_t left_count;
    PBox child_tri[2];
};

// One workgroup per open node of the level [begin, begin + count); children go to [begin + count, ...).
__global__ __launch_bounds__(kThreads) void k_level(DevNode* nodes, uint32_t begin, uint32_t capacity, const ptmi_float4* tbox,
                                                    uint32_t* perm, uint32_t* scratch, LevelCounters* counters)
{
    __shared__ LevelShared S;
    __shared__ PBox red[kThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t self = begin + blockIdx.x;
    DevNode* N = &nodes[self];
    const uint32_t first = N->start, nb = N->count, last = first + nb - 1, depth = N->depth;

    if (t == 0) {
        S.state = -1;
        S.error = 0;
        if (depth > kMaxBuildDepth) {
            atomicOr(&counters->flags, kFlagError);
            S.state = 0;
        } else {
            const int leaf = early_leaf(nb, N->c_min, N->c_max);
            if (leaf >= 0) {
                N->leaf = leaf;
                atomicMax(&counters->max_depth, depth);
                S.state = 0;
            }
        }
        for (int a = 0; a < 3; a++) {
            S.binned[a] = axis_k1(N->c_min, N->c_max, a, &S.k1[a]) ? 1 : 0;
            S.lo[a] = axis_of(N->c_min, a);
        }
    }
    __syncthreads();
    if (S.state >= 0) return;

    // ---- 3 x 64 bins: one thread per (axis, bin) folds the node's range in ascending order
    const int my_axis = min((int)t / kBins, 2), my_bin = (int)t % kBins;
    const bool folder = t < 3 * kBins && S.binned[my_axis];
    PBox acc = pbox_empty();
    int acc_count = 0;
    for (uint32_t base = first; base <= last; base += kThreads) {
        const uint32_t p = base + t;
        if (p <= last) {
            const uint32_t id = perm[p];
            const ptmi_float4 c = ld4(&tbox[3 * (size_t)id + 2]);
            S.b_min[t] = ld4(&tbox[3 * (size_t)id]);
            S.b_max[t] = ld4(&tbox[3 * (size_t)id + 1]);
            S.b_cen[t] = c;
            for (int a = 0; a < 3; a++) {
                uint8_t b = 0;
                if (S.binned[a]) {
                    const float s = scaled_pos(S.k1[a], axis_of(c, a), S.lo[a]);
                    if (bin_ok(s)) b = (uint8_t)(int)s;
                    else S.error = 1;
                }
                S.bin[a][t] = b;
            }
        }
        __syncthreads();
        if (folder) {
            const uint32_t n_here = min((uint32_t)kThreads, last - base + 1);
            const uint8_t* bins = S.bin[my_axis];
            for (uint32_t j = 0; j < n_here; j++)
                if (bins[j] == my_bin) {
                    pbox_unite(acc, S.b_min[j], S.b_max[j], S.b_cen[j]);
                    acc_count++;
                }
        }
        __syncthreads();
    }
    if (t < 3 * kBins) {
        S.bins[my_axis][my_bin] = acc;
        S.counts[my_axis][my_bin] = acc_count;
    }
    __syncthreads();
    if (S.error) {
        if (t == 0) atomicOr(&counters->flags, kFlagError);
        return;
    }

    // ---- scans and SAH per axis, then the decision
    if (t < 3) {
        if (S.binned[t]) axis_sah(S.bins[t], S.counts[t], S.rpart[t], S.sah[t]);
        else
            for (int i = 0; i < kBins - 1; i++) S.sah[t][i] = (float)INT_MAX;
    }
    __syncthreads();
    if (t == 0) {
        int axis, index;
        float best;
        best_split(&S.sah[0][0], &axis, &index, &best);
        if (sah_leaf(best, nb, N->t_min, N->t_max)) {
            N->leaf = PTMI_NODE_BAD_SAH;
            atomicMax(&counters->max_depth, depth);
            S.state = 0;
        } else if (!S.binned[axis]) {
            atomicOr(&counters->flags, kFlagStale);
            S.state = 0;
        } else {
            int lc, rc;
            split_sides(S.bins[axis], S.counts[axis], index, &S.child_tri[0], &lc, &S.child_tri[1], &rc);
            if (lc <= 0 || rc <= 0 || (uint32_t)lc + (uint32_t)rc != nb) {
                atomicOr(&counters->flags, kFlagError);
                S.state = 0;
            } else {
                S.axis = axis;
                S.index = index;
                S.left_count = (uint32_t)lc;
            }
        }
    }
    __syncthreads();
    if (S.state >= 0) return;
    const int axis = S.axis, index = S.index;
    const uint32_t L = S.left_count, mid = first + L;
    const float k = S.k1[axis], lo = S.lo[axis];

    // ---- partition: positions of the left-going triangles in [mid, last], counted from the end ...
    uint32_t running = 0;
    for (uint32_t off = 0; off < last - mid + 1; off += kThreads) {
        const uint32_t k_off = off + t;
        bool is_left = false;
        uint32_t q = 0;
        if (k_off < last - mid + 1) {
            q = last - k_off;
            is_left = goes_left(scaled_pos(k, axis_of(ld4(&tbox[3 * (size_t)perm[q] + 2]), axis), lo), index);
        }
        uint32_t total;
        const uint32_t rank = running + wg_prefix(is_left, S.wsum, &total);
        if (is_left) scratch[first + rank] = q;
        running += total;
    }
    const uint32_t n_pairs = running;
    __threadfence_block();
    __syncthreads();
    // ... and the k-th right-going triangle in [first, mid) swaps with the k-th of them
    running = 0;
    for (uint32_t off = 0; off < L; off += kThreads) {
        const uint32_t p = first + off + t;
        bool is_right = false;
        uint32_t id = 0;
        if (off + t < L) {
            id = perm[p];
            is_right = !goes_left(scaled_pos(k, axis_of(ld4(&tbox[3 * (size_t)id + 2]), axis), lo), index);
        }
        uint32_t total;
        const uint32_t rank = running + wg_prefix(is_right, S.wsum, &total);
        if (is_right && rank < n_pairs) {  // (always: the left count is the number of left-going triangles)
            const uint32_t q = scratch[first + rank];
            perm[p] = perm[q];
            perm[q] = id;
        }
        running += total;
    }
    __threadfence_block();
    __syncthreads();

    // ---- the children's centroid boxes: left range ascending, right range from the end down
    const PBox left_cen = fold_centroids(tbox, perm, first, mid - 1, false, red);
    const PBox right_cen = fold_centroids(tbox, perm, mid, last, true, red);
    if (t == 0) {
        const uint32_t slot = atomicAdd(&counters->next_count, 2u);
        const uint32_t c1 = begin + gridDim.x + slot;
        if (c1 + 1 >= capacity) {
            atomicOr(&counters->flags, kFlagError);
            return;
        }
        N->cut_axis = (uint32_t)axis;
        N->leaf = -1;
        N->child = c1;
        write_child(&nodes[c1], S.child_tri[0], left_cen, first, L, depth + 1);
        write_child(&nodes[c1 + 1], S.child_tri[1], right_cen, mid, nb - L, depth + 1);
    }
}

__global__ void k_iota(uint32_t* perm, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = i;
}

// subtree sizes, one level at a time from the deepest
__global__ void k_sizes(const DevNode* nodes, uint32_t begin, uint32_t count, uint32_t* size)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const DevNode& d = nodes[begin + i];
    size[begin + i] = d.leaf >= 0 ? 1u : 1u + size[d.child] + size[d.child + 1];
}

// depth-first pre-order numbers, one level at a time from the root: son1 = parent + 1, son2 = son1 + size(son1)
__global__ void k_preorder(const DevNode* nodes, uint32_t begin, uint32_t count, const uint32_t* size, uint32_t* pre)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const DevNode& d = nodes[begin + i];
    if (d.leaf >= 0) return;
    const uint32_t p = pre[begin + i];
    pre[d.child] = p + 1;
    pre[d.child + 1] = p + 1 + size[d.child];
}

// every node in pre-order, every field as BVH_CreateNode / make_leaf write it, padding zero
__global__ void k_emit(const DevNode* nodes, uint32_t total, const uint32_t* pre, ptmi_node* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const DevNode& d = nodes[i];
    union {
        ptmi_node n;
        uint4 q[sizeof(ptmi_node) / 16];
    } u;
#pragma unroll
    for (int k = 0; k < (int)(sizeof(ptmi_node) / 16); k++) u.q[k] = make_uint4(0, 0, 0, 0);
    u.n.triangles_aabb.p_min = d.t_min; u.n.triangles_aabb.p_max = d.t_max; u.n.triangles_aabb.centroid = d.t_cen;
    u.n.centroids_aabb.p_min = d.c_min; u.n.centroids_aabb.p_max = d.c_max; u.n.centroids_aabb.centroid = d.c_cen;
    u.n.triangle_start_index = d.start;
    u.n.nb_triangles = d.count;
    if (d.leaf >= 0) {
        u.n.is_leaf = 1;
        u.n.comments = d.leaf;
    } else {
        u.n.cut_axis = d.cut_axis;
        u.n.son1_id = pre[d.child];
        u.n.son2_id = pre[d.child + 1];
    }
    uint4* dst = reinterpret_cast<uint4*>(&out[pre[i]]);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(ptmi_node) / 16); k++) dst[k] = u.q[k];
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Device memory and stream of one call, released on every path out; the calling thread's device restored.
struct Workspace {
    int prev_device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<void*> blocks;
    uint64_t bytes = 0;
    hipError_t alloc(void** p, size_t n)
    {
        const hipError_t e = hipMalloc(p, n);
        if (e == hipSuccess) { blocks.push_back(*p); bytes += n; }
        return e;
    }
    ~Workspace()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : blocks) (void)hipFree(p);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
    }
};

enum class DeviceResult { Ok, Stale, Error, HipError };

struct DeviceBuild {
    std::string hip_error;
    uint32_t size = 0, max_depth = 0, levels = 0;
    double device_ms = 0, upload_ms = 0, download_ms = 0;
    uint64_t bytes = 0;
};

#define PTMI_BVH_HIP(call)                                                                          \
    do {                                                                                            \
        const hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                                     \
            out.hip_error = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return DeviceResult::HipError;                                                          \
        }                                                                                           \
    } while (0)

// The device build proper.  Writes `bvh` and `perm_out` only when it returns Ok.
DeviceResult build_on_device(int device, const std::vector<ptmi_float4>& boxes, uint32_t n, const DevNode& root,
                             ptmi_node* bvh, std::vector<uint32_t>& perm_out, DeviceBuild& out)
{
    Workspace ws;
    PTMI_BVH_HIP(hipGetDevice(&ws.prev_device));
    PTMI_BVH_HIP(hipSetDevice(device));
    PTMI_BVH_HIP(hipStreamCreateWithFlags(&ws.stream, hipStreamNonBlocking));
    PTMI_BVH_HIP(hipEventCreate(&ws.ev0));
    PTMI_BVH_HIP(hipEventCreate(&ws.ev1));
    const uint32_t capacity = 2u * n - 1u;
    ptmi_float4* d_box = nullptr;
    uint32_t *d_perm = nullptr, *d_scratch = nullptr, *d_size = nullptr, *d_pre = nullptr;
    DevNode* d_nodes = nullptr;
    ptmi_node* d_out = nullptr;
    LevelCounters* d_counters = nullptr;
    PTMI_BVH_HIP(ws.alloc((void**)&d_box, sizeof(ptmi_float4) * 3 * (size_t)n));
    PTMI_BVH_HIP(ws.alloc((void**)&d_perm, sizeof(uint32_t) * (size_t)n));
    PTMI_BVH_HIP(ws.alloc((void**)&d_scratch, sizeof(uint32_t) * (size_t)n));
    PTMI_BVH_HIP(ws.alloc((void**)&d_nodes, sizeof(DevNode) * (size_t)capacity));
    PTMI_BVH_HIP(ws.alloc((void**)&d_size, sizeof(uint32_t) * (size_t)capacity));
    PTMI_BVH_HIP(ws.alloc((void**)&d_pre, sizeof(uint32_t) * (size_t)capacity));
    PTMI_BVH_HIP(ws.alloc((void**)&d_out, sizeof(ptmi_node) * (size_t)capacity));
    PTMI_BVH_HIP(ws.alloc((void**)&d_counters, sizeof(LevelCounters)));
    out.bytes = ws.bytes;

    auto t0 = std::chrono::steady_clock::now();
    PTMI_BVH_HIP(hipMemcpyAsync(d_box, boxes.data(), sizeof(ptmi_float4) * boxes.size(), hipMemcpyHostToDevice, ws.stream));
    PTMI_BVH_HIP(hipMemcpyAsync(d_nodes, &root, sizeof(DevNode), hipMemcpyHostToDevice, ws.stream));
    PTMI_BVH_HIP(hipStreamSynchronize(ws.stream));
    out.upload_ms = ms_since(t0);

    PTMI_BVH_HIP(hipEventRecord(ws.ev0, ws.stream));
    PTMI_BVH_HIP(hipMemsetAsync(d_counters, 0, sizeof(LevelCounters), ws.stream));
    k_iota<<<(n + 255) / 256, 256, 0, ws.stream>>>(d_perm, n);
    PTMI_BVH_HIP(hipGetLastError());
    std::vector<uint32_t> level_begin{ 0 };
    uint32_t begin = 0, count = 1;
    LevelCounters h_counters{};
    while (count > 0) {
        PTMI_BVH_HIP(hipMemsetAsync(d_counters, 0, offsetof(LevelCounters, max_depth), ws.stream));
        k_level<<<count, kThreads, 0, ws.stream>>>(d_nodes, begin, capacity, d_box, d_perm, d_scratch, d_counters);
        PTMI_BVH_HIP(hipGetLastError());
        PTMI_BVH_HIP(hipMemcpyAsync(&h_counters, d_counters, sizeof h_counters, hipMemcpyDeviceToHost, ws.stream));
        PTMI_BVH_HIP(hipStreamSynchronize(ws.stream));
        out.levels++;
        if (h_counters.flags & kFlagStale) return DeviceResult::Stale;
        if (h_counters.flags & kFlagError) return DeviceResult::Error;
        begin += count;
        count = h_counters.next_count;
        level_begin.push_back(begin);
    }
    const uint32_t total = begin;
    for (size_t l = level_begin.size() - 1; l-- > 0;) {
        const uint32_t b = level_begin[l], c = level_begin[l + 1] - b;
        k_sizes<<<(c + 255) / 256, 256, 0, ws.stream>>>(d_nodes, b, c, d_size);
    }
    PTMI_BVH_HIP(hipMemsetAsync(d_pre, 0, sizeof(uint32_t), ws.stream));
    for (size_t l = 0; l + 1 < level_begin.size(); l++) {
        const uint32_t b = level_begin[l], c = level_begin[l + 1] - b;
        k_preorder<<<(c + 255) / 256, 256, 0, ws.stream>>>(d_nodes, b, c, d_size, d_pre);
    }
    k_emit<<<(total + 255) / 256, 256, 0, ws.stream>>>(d_nodes, total, d_pre, d_out);
    PTMI_BVH_HIP(hipGetLastError());
    PTMI_BVH_HIP(hipEventRecord(ws.ev1, ws.stream));
    PTMI_BVH_HIP(hipEventSynchronize(ws.ev1));
    float ms = 0;
    PTMI_BVH_HIP(hipEventElapsedTime(&ms, ws.ev0, ws.ev1));
    out.device_ms = ms;

    // only now: the caller's node array and the permutation
    t0 = std::chrono::steady_clock::now();
    perm_out.resize(n);
    PTMI_BVH_HIP(hipMemcpyAsync(perm_out.data(), d_perm, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ws.stream));
    PTMI_BVH_HIP(hipMemcpyAsync(bvh, d_out, sizeof(ptmi_node) * (size_t)total, hipMemcpyDeviceToHost, ws.stream));
    PTMI_BVH_HIP(hipStreamSynchronize(ws.stream));
    out.download_ms = ms_since(t0);
    out.size = total;
    out.max_depth = h_counters.max_depth;
    return DeviceResult::Ok;
}

// triangulation[i] = original[perm[i]], on a few host threads
void apply_permutation(ptmi_triangle* tris, uint32_t n, const std::vector<uint32_t>& perm)
{
    std::vector<ptmi_triangle> orig(tris, tris + n);
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const uint32_t workers = n < 65536 ? 1u : hw;
    auto run = [&](uint32_t w) {
        const uint32_t a = (uint32_t)((uint64_t)n * w / workers), b = (uint32_t)((uint64_t)n * (w + 1) / workers);
        for (uint32_t i = a; i < b; i++) std::memcpy(&tris[i], &orig[perm[i]], sizeof(ptmi_triangle));
    };
    std::vector<std::thread> pool;
    for (uint32_t w = 1; w < workers; w++) pool.emplace_back(run, w);
    run(0);
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" int ptmi_bvh_create_device(int32_t device, ptmi_triangle* triangulation, uint32_t n, ptmi_node* bvh,
                                      uint32_t* bvh_size, uint32_t* bvh_max_depth, ptmi_bvh_build_info* info)
{
    const auto t_call = std::chrono::steady_clock::now();
    ptmi_bvh_build_info local;
    std::memset(&local, 0, sizeof local);
    local.struct_size = sizeof(ptmi_bvh_build_info);
    auto finish = [&](int rc) {
        local.total_ms = ms_since(t_call);
        if (info) *info = local;
        return rc;
    };
    auto on_host = [&](uint32_t why) {
        local.fallback = why;
        return finish(ptmi_bvh_create(triangulation, n, bvh, bvh_size, bvh_max_depth));
    };
    if (!triangulation || !bvh || n == 0) {
        ptmi_internal::set_global_error("ptmi_bvh_create_device: null array or empty triangulation");
        return finish(PTMI_ERR_INVALID_ARGUMENT);
    }
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0 || device < 0 || device >= n_devices) {
        ptmi_internal::set_global_error("ptmi_bvh_create_device: no HIP device " + std::to_string(device) + " (" +
                                        std::to_string(n_devices) + " present)");
        return finish(PTMI_ERR_NO_DEVICE);
    }

    // The boxes the device folds, and the root.  Records the host builder refuses go to it for its message; records the
    // device does not fold go to it for the tree; whichever comes first in index order.
    std::vector<ptmi_float4> boxes(3 * (size_t)n);
    const RootFold fold = fold_records(triangulation, n, [&](uint32_t i, const ptmi_bounding_box& a) {
        boxes[3 * (size_t)i] = a.p_min;
        boxes[3 * (size_t)i + 1] = a.p_max;
        boxes[3 * (size_t)i + 2] = a.centroid;
    });
    if (fold.unfolded) return on_host(PTMI_BVH_FALLBACK_RECORDS);
    if (fold.refused) return on_host(PTMI_BVH_FALLBACK_HOST_ERROR);
    DevNode root;
    std::memset(&root, 0, sizeof root);
    root.t_min = fold.tri.p_min; root.t_max = fold.tri.p_max; root.t_cen = pbox_centroid(fold.tri);
    root.c_min = fold.cen.p_min; root.c_max = fold.cen.p_max; root.c_cen = pbox_centroid(fold.cen);
    root.start = 0; root.count = n; root.leaf = -1;

    DeviceBuild b;
    std::vector<uint32_t> perm;
    const DeviceResult r = build_on_device(device, boxes, n, root, bvh, perm, b);
    local.levels = b.levels;
    local.device_ms = b.device_ms;
    local.upload_ms = b.upload_ms;
    local.download_ms = b.download_ms;
    local.workspace_bytes = b.bytes;
    if (r == DeviceResult::HipError) {
        ptmi_internal::set_global_error("ptmi_bvh_create_device: " + b.hip_error);
        return finish(PTMI_ERR_HIP);
    }
    if (r == DeviceResult::Stale) return on_host(PTMI_BVH_FALLBACK_STALE_AXIS);
    if (r == DeviceResult::Error) return on_host(PTMI_BVH_FALLBACK_HOST_ERROR);

    const auto t_perm = std::chrono::steady_clock::now();
    apply_permutation(triangulation, n, perm);
    local.permute_ms = ms_since(t_perm);
    local.built_on_device = 1;
    if (bvh_size) *bvh_size = b.size;
    if (bvh_max_depth) *bvh_max_depth = b.max_depth;
    return finish(PTMI_OK);
}
