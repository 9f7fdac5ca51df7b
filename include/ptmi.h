/*
 * ptmi.h - C ABI of the MI355X path-tracing integrator (libptmi.so).
 *
 * Drop-in boundary: the three functions the reference's orchestration calls on
 * its device backend, Controleur/PathTracer_OpenCL.h:17-19
 *     OpenCL_SetupContext(GlobalVars&, Sampler)           (PathTracer_OpenCL.cpp:316-402)
 *     OpenCL_InitializeMemory(GlobalVars&)                (PathTracer_OpenCL.cpp:149-198)
 *     OpenCL_RunKernel(GlobalVars&, cb, nImages, t1,t2,t3)(PathTracer_OpenCL.cpp:56-140)
 * called once each, in that order, from PathTracer_Main (PathTracer.cpp:74,76,82),
 * plus the host BVH build that produces one of their inputs
 *     BVH_Create(GlobalVars&)                             (PathTracer_BVH.cpp:12-37).
 * Each entry point below names the reference code it replaces.  The C++ shim
 * with the reference's own signatures on top of this ABI is
 * opencl_pathtracer_amd/csrc/PathTracer_HIP.cpp.
 *
 * Conventions: plain pointers and sizes, caller-owned host memory,
 * context-owned device memory, no exceptions; every call returns PTMI_OK (0)
 * or a negative ptmi_status and leaves a message for ptmi_last_error().
 * There is NO CPU fallback: without a HIP device every compute entry point
 * fails with PTMI_ERR_NO_DEVICE.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>
#include "ptmi_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_ABI_VERSION 4 /* 3: PTMI_FLAG_DEFAULT_ARITHMETIC, ptmi_scheduler_stats::leaf_item_violations; 4: ::textured_hits */
#define PTMI_MAX_DEVICES 16       /* devices that can share one render */
#define PTMI_MAX_SNAPSHOT_SLOTS 65 /* ptmi_snapshot ring: slots 0..63 are the caller's, the last one the library's own */

typedef enum ptmi_status {
    PTMI_OK = 0,
    PTMI_ERR_INVALID_ARGUMENT = -1, /* null pointer, zero image, bad sampler ... */
    PTMI_ERR_NO_DEVICE = -2,        /* no HIP device / bad ordinal (reference: "Wrong context.", OpenCL.cpp:359-360) */
    PTMI_ERR_HIP = -3,              /* a HIP runtime call failed (reference: OpenCL_ErrorHandling, OpenCL.cpp:407-486) */
    PTMI_ERR_LIMIT = -4,            /* bvh depth >= 30 or lights >= 30 (reference guard, PathTracer.cpp:54-65) */
    PTMI_ERR_BAD_SCENE = -5,        /* scene arrays inconsistent (index out of range, cyclic bvh ...) */
    PTMI_ERR_STATE = -6,            /* call order violated (e.g. render before initialize_memory) */
    PTMI_ERR_UNSUPPORTED = -7,      /* feature compiled out / not available in this build */
    PTMI_ERR_INTERNAL = -8          /* a bug: the library refused to launch work that broke one of its own invariants */
} ptmi_status;

typedef struct ptmi_ctx ptmi_ctx;

/* What OpenCL_BuildOptions bakes into the kernel with -D (OpenCL.cpp:292-314),
 * plus the device choice made in OpenCL_SetupContext (OpenCL.cpp:356-366). */
typedef struct ptmi_config {
    uint32_t struct_size;    /* = sizeof(ptmi_config), ABI guard */
    int32_t device;          /* HIP device ordinal (reference: devices[0]) */
    uint32_t image_width;    /* -D IMAGE_WIDTH  (globalVars.imageWidth)  */
    uint32_t image_height;   /* -D IMAGE_HEIGHT (globalVars.imageHeight) */
    uint32_t ray_max_depth;  /* -D MAX_REFLECTION_NUMBER (globalVars.rayMaxDepth) */
    uint32_t lights_size;    /* -D LIGHTS_SIZE (globalVars.lightsSize) */
    uint32_t sampler;        /* PTMI_SAMPLER_* : -D SAMPLE_JITTERED / _RANDOM / _UNIFORM */
    uint32_t super_sampling; /* -D SUPER_SAMPLING (globalVars.superSampling): adaptive sampling, FullKernel.cl:1152-1172,1219-1222.
                                With the RANDOM sampler the reference races on the count / variance of the pixel a sample lands on;
                                here those updates are atomic (results statistically equal, not bit-equal, to a serial evaluation) */
    uint32_t flags;          /* PTMI_FLAG_* */
    /* Multi-GPU render (the reference drives devices[0] only, OpenCL.cpp:363-366): n_devices > 1 replicates the scene on
     * devices[0..n_devices) and spreads the iteration ids of every ptmi_render call over them (device k takes the ids
     * congruent to k modulo n_devices: the same id set as a single-device render, so the same samples); devices[0] is
     * the one the partial accumulators are summed on, by peer copies over xGMI + one add kernel IN DEVICE ORDER (the float
     * sums of an image are a function of the device list alone); the per-image loop (ptmi_read_snapshot), where one device's
     * share changes per image, re-sends only that share.  Environment PTMI_REDUCE=rccl: the sum is an ncclReduce instead
     * (librccl, loaded at run time, NCCL 2 API checked by ncclGetVersion) - opt-in: its order of additions for more than two
     * devices is the collective algorithm's, so the last bits of an image depend on it, and any failure (library absent,
     * device list refused, a run-time error) falls back to the peer path for the rest of the context's life.
     * n_devices 0 or 1 = single device `device`.  A device may be listed more than once (used by the tests on a one-GPU box;
     * RCCL refuses that, the peer path runs). */
    uint32_t n_devices;
    int32_t devices[PTMI_MAX_DEVICES];
} ptmi_config;

#define PTMI_FLAG_NO_HISTOGRAMS 1u /* skip the three per-path histogram atomics (FullKernel.cl:1319-1331); totals are still kept */
#define PTMI_FLAG_SCHEDULER_STATS 4u /* collect ptmi_scheduler_stats (a few scalar ops per loop trip; off by default) */
#define PTMI_FLAG_MEGAKERNEL 2u    /* one path per lane (kernels.hip) instead of the persistent wavefront kernel; same results */
#define PTMI_FLAG_RUSSIAN_ROULETTE 8u /* NON-PARITY mode: the termination block the reference ships commented out (FullKernel.cl:1306-1314,
                                         RUSSIAN_ROULETTE false in header.cl:12), as it is written there: from the 7th bounce on a path
                                         whose largest transfer component / (bounce - 5) is below 1 draws a random number, ends unless it
                                         exceeds that coefficient, and has its transfer divided by it.  Images differ from the reference's. */

#define PTMI_FLAG_SOURCE_SEED 32u /* NON-PARITY mode: InitializeRandomSeed as its SOURCE reads under wrapping arithmetic (header.cl:255-264:
                                    `seed *= 2011; seed *= seed; if(seed == 0) seed = 1;`).  The compiled reference tests the un-squared index
                                    instead (the square overflows a signed int: undefined, and LLVM folds the test), so a path whose index is a
                                    non-zero multiple of 2^16 keeps seed 0 and draws 0 for every random number - one path in 65536, the same
                                    pixels every 2^16 / gcd(2^16, W*H) iterations.  Parity modes reproduce that; this flag gives those paths
                                    seed 1, as the source intends.  Images differ from the reference's at those pixels only. */
#define PTMI_FLAG_DEFAULT_ARITHMETIC 16u /* The arithmetic of the build the reference's own build line produces (OpenCL_BuildOptions,
                                         OpenCL.cpp:292-314, passes no floating-point option): a*b+c written in one expression is one
                                         fused multiply-add, a/b goes through v_rcp_f32 of the divisor's mantissa (2.5 ulp), sqrt is
                                         v_sqrt_f32 - bit for bit what that build computes on this GPU.  Without the flag: the STRICT
                                         arithmetic (every operation of the source correctly rounded, the build the same source gives
                                         with -ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt), also bit for bit.  Same cost. */

/* What OpenCL_InitializeMemory copies with CL_MEM_COPY_HOST_PTR and passes as
 * kernel arguments 1..17 (OpenCL.cpp:165-197).  Arrays are raw dumps of the
 * ptmi_scene.h structs; a zero-length array may be NULL. */
typedef struct ptmi_scene {
    uint32_t struct_size; /* = sizeof(ptmi_scene) */
    const ptmi_node* bvh;                 uint32_t bvh_size;
    const ptmi_triangle* triangulation;   uint32_t triangulation_size;
    const ptmi_light* lights;             uint32_t lights_size;
    const ptmi_material* materiaux;       uint32_t materiaux_size;
    const ptmi_texture* textures;         uint32_t textures_size;
    const ptmi_uchar4* textures_data;     uint32_t textures_data_size;
    const ptmi_sky* sky;
    ptmi_float4 camera_position;  /* kernel arg 1 */
    ptmi_float4 camera_direction; /* kernel arg 2 */
    ptmi_float4 camera_right;     /* kernel arg 3 */
    ptmi_float4 camera_up;        /* kernel arg 4 */
} ptmi_scene;

/* Totals the roofline model is priced from: exact sums of the
 * reference's per-path counters over everything rendered since the last
 * ptmi_initialize_memory / ptmi_clear. */
typedef struct ptmi_counters {
    uint64_t paths;          /* Kernel_Main invocations that reached the epilogue */
    uint64_t segments;       /* BVH_IntersectRay calls ("samples": paths x bounces) */
    uint64_t surface_hits;   /* sum of r.reflectionId = segments that hit geometry */
    uint64_t shadow_rays;    /* BVH_IntersectShadowRay calls */
    uint64_t box_tests;      /* sum of numIntersectedBBx incl. shadow rays */
    uint64_t triangle_tests; /* sum of numIntersectedTri incl. shadow rays */
} ptmi_counters;

/* Wave-scheduler statistics of the persistent wavefront kernel since the last clear: how many loop trips a
 * wave spent on each step kind and how many of its 64 lanes were active in them (lanes / (64 * trips) =
 * SIMD utilisation of that kind).  Collected only with PTMI_FLAG_SCHEDULER_STATS; all zero otherwise and for the
 * one-path-per-lane kernel. */
typedef struct ptmi_scheduler_stats {
    uint64_t trips_node, lanes_node;         /* node trips: lanes that took an inner-node step */
    uint64_t trips_triangle, lanes_triangle; /* leaf passes: triangles tested, one per lane (+ the triangles of leaves beyond a
                                              * query's limit, which are counted without a pass: csrc/leaf_cull.h) */
    uint64_t trips_path, lanes_path;         /* path logic (shade / shadow set-up / scatter / regenerate) */
    uint64_t cycles_path, cycles_loop;       /* shader-clock cycles, summed over waves: inside path-logic passes / in the main loop */
    uint64_t leaf_item_violations;           /* leaf passes: work items whose owner lane or triangle record index was out of range when a
                                                lane read them (an item read before its writer: must be 0; checked only while collecting) */
    uint64_t paths_retraced;                 /* paths a launch gave up because one of their rays was not a number, traced again by the
                                                reference's literal loops (ptmi_literal_kernel_reason, below); counted ALWAYS, flag or not */
    uint64_t textured_hits;                  /* surface hits whose material has a file texture (one texel fetch each at least: the
                                                4 * N_texel term of the algorithmic-bytes model); counted only while collecting */
    uint64_t workgroup_lanes, resident_workgroups; /* the grid of the most recent wavefront-kernel launch on devices[0] (this context's
                                                or another's): lanes per workgroup, and how many workgroups the device holds at once
                                                - the persistent grid; 0 before the first launch; filled ALWAYS */
} ptmi_scheduler_stats;

/* The reference's device-side consistency checks: with -D LOG_INFO (OpenCL.cpp:310, globalVars.printLogInfos) its kernel
 * prints a line whenever one of the ASSERT / WARNING conditions of PathTracer_FullKernel_header.cl:21-48 fails.  Here the
 * failures of the checks on the live path are COUNTED, in the same debug instantiation of the kernel that collects the
 * scheduler statistics (PTMI_FLAG_SCHEDULER_STATS); all zero otherwise.  A clean render has zeros everywhere except
 * statistics_out_of_range, which counts what the reference's histograms silently drop. */
typedef struct ptmi_invariant_checks {
    uint64_t sample_out_of_range;      /* FullKernel.cl:1217 "SAMPLER - invalid pixel" */
    uint64_t normal_not_facing_ray;    /* :1275 "Kernel_Main incorrect normals": dot(dir, Ns) < 0 && dot(dir, Ng) < 0 */
    uint64_t negative_direct_radiance; /* :951 "Scene_ComputeDirectIllumination incorrect radiance L" */
    uint64_t scattered_below_surface;  /* header.cl:243 "Vector_PutInSameHemisphereAs": dot(out, N) > 0 */
    uint64_t statistics_out_of_range;  /* :1325,1330 "global__rayIntersectionBBx / Tri to large": >= 5000 tests on one path */
    /* NOT a check of the reference: bounces whose result the reference's SOURCE leaves undefined.  Its water material refracts
     * when random() >= the Fresnel fraction (FullKernel.cl:836-843); on total internal reflection the fraction is 1 and
     * Material_FresnelWaterReflectionFraction has returned (:237) BEFORE writing refractionDirection and refractionMultCoeff
     * (:249-251) - and random() returns exactly 1.0 for the 64 seeds nearest 2^31 (header.cl:246-253), so about one interior
     * water hit in 10^8 refracts along an uninitialised direction with an uninitialised factor (the compiled kernel reads
     * whatever its registers hold: stale values of other variables).  The integrator takes a zero direction and the factor
     * n2^2/n1^2 there.  Such a path is the one thing that may differ from the reference kernel's image; counted so that a
     * comparison can tell (tools/north_star_full_size.py). */
    uint64_t refraction_undefined_in_reference;
} ptmi_invariant_checks;

/* ---- lifecycle ---------------------------------------------------------- */

/* Replaces OpenCL_SetupContext (OpenCL.cpp:316-402): picks the device, creates
 * the stream and selects the kernel specialisation.  *ctx is NULL on failure. */
int ptmi_setup_context(ptmi_ctx** ctx, const ptmi_config* config);

/* Replaces OpenCL_InitializeMemory (OpenCL.cpp:149-198): validates the scene,
 * re-lays it out for the device, uploads it and allocates + ZEROES the
 * accumulators (the reference leaves them uninitialised, OpenCL.cpp:159-164).
 * May be called again on the same context with a new scene. */
int ptmi_initialize_memory(ptmi_ctx* ctx, const ptmi_scene* scene);

/* Replaces the clSetKernelArg(0, imageId) + clEnqueueNDRangeKernel(W x H) pair
 * of OpenCL_RunKernel's loop (OpenCL.cpp:85-89), generalised to a range:
 * renders iterations [first_iteration, first_iteration + n_iterations) for
 * every pixel and adds them into the accumulators in iteration order (the
 * float sums equal a launch-per-iteration loop's bit for bit).  Internally
 * at most 32 iterations per kernel launch (1 with super_sampling, whose stop
 * criterion reads the accumulators of the previous iteration).  Asynchronous
 * on the context's stream.
 * A caller that renders one short call (fewer than 4 iterations) after the other, in order, and waits for each - the
 * reference's loop - is RENDERED AHEAD OF: once the pattern has been seen the library keeps launches for the next calls in
 * flight (two per device, each for up to four calls), and a call that finds its iterations rendered adopts them.  Nothing a caller can
 * read differs from rendering on demand (image, sample counts, histograms, counters after every call); a call that leaves
 * the pattern drops what ran ahead.  Costs per device: up to 8 iterations of device time nobody asked for when such a caller
 * stops, and staging memory for 16 iterations (20 bytes per pixel each).  Environment: PTMI_RENDER_AHEAD=0 switches it off,
 * PTMI_RENDER_AHEAD_CALLS=1 keeps it to one call per launch. */
int ptmi_render(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations);

/* clFinish (OpenCL.cpp:89). */
int ptmi_synchronize(ptmi_ctx* ctx);

/* Replaces the two blocking clEnqueueReadBuffer of every image (OpenCL.cpp:97-98):
 * image_color = float[4*W*H] sum of radiance, image_ray_nb = float[W*H] sample
 * count.  Either pointer may be NULL.  Waits for everything queued so far.  The bytes cross the bus into pinned
 * memory: straight into the destination if the caller has page-locked it (ptmi_pin_host_buffer), through a
 * pinned staging buffer of the context and a host copy otherwise. */
int ptmi_read_image(ptmi_ctx* ctx, float* image_color, float* image_ray_nb);

/* Page-lock a host buffer the caller will hand to ptmi_read_image / ptmi_read_snapshot again and again (the viewer's
 * imageColor / imageRayNb, which the reference reads into after every image, OpenCL.cpp:97-98): readbacks then DMA
 * into it without an intermediate copy.  The buffer must stay allocated until ptmi_unpin_host_buffer or ptmi_release. */
int ptmi_pin_host_buffer(ptmi_ctx* ctx, void* buffer, size_t bytes);
int ptmi_unpin_host_buffer(ptmi_ctx* ctx, void* buffer);

/* The same readback split in two so that the launches of the NEXT images run while image k crosses the bus
 * (the reference blocks on every image: launch, clFinish, read, callback - OpenCL.cpp:85-103):
 *   ptmi_snapshot(slot)       queued behind the launches issued so far: a device-side copy of the accumulators
 *                             (every device of a multi-GPU render) into ring slot `slot` < PTMI_MAX_SNAPSHOT_SLOTS;
 *   ptmi_read_snapshot(slot)  waits for that copy only (not for launches queued after it), sums the devices'
 *                             partial images on devices[0] (any image size, an odd number of pixels too), copies
 *                             the result to the host buffers; with both
 *                             pointers NULL it only waits until the snapshot has been taken (clFinish of that image).
 * Loop of a viewer: render(k+1); read_snapshot(k); show; snapshot(k+1) ...  (csrc/PathTracer_HIP.cpp).
 *   ptmi_render_snapshots(first, n, first_slot)   ptmi_render(first, n) that ALSO leaves a snapshot after every one of
 *                             its n iterations - iteration first + k in slot (first_slot + k) % (PTMI_MAX_SNAPSHOT_SLOTS - 1)
 *                             - although the iterations share kernel launches: a viewer still gets every image of the
 *                             reference's launch-per-image loop, at the throughput of n iterations per launch.
 *                             n < PTMI_MAX_SNAPSHOT_SLOTS; JITTERED / UNIFORM sampler, wavefront kernel, no super_sampling. */
int ptmi_snapshot(ptmi_ctx* ctx, uint32_t slot);
int ptmi_render_snapshots(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations, uint32_t first_slot);
int ptmi_read_snapshot(ptmi_ctx* ctx, uint32_t slot, float* image_color, float* image_ray_nb);

/* ---- A rectangle of the image ----------------------------------------------------------------------------------------------
 * The render region of a look-development session (re-render the one object whose material changed, put more samples into a
 * noisy corner) and the unit by which callers share a frame between contexts or machines: tiles. */
typedef struct ptmi_region { uint32_t x, y, width, height; } ptmi_region;   /* pixels [x, x+width) x [y, y+height); row 0 first, as ptmi_read_image */

/* ptmi_render for the work-items of a rectangle: traces exactly the paths ptmi_render(first_iteration, n_iterations) traces
 * for the work-items (gx, gy) inside `region` and no other.  A path's seed index is still gx + gy * W + it * W * H over the
 * FULL image; its sample, its camera ray and, under super_sampling, its stop criterion are those of ptmi_render, in the
 * context's arithmetic.  It is ptmi_render with fewer work-items, not a second renderer: every mode ptmi_render serves is
 * served - super_sampling, PTMI_FLAG_MEGAKERNEL, PTMI_FLAG_RUSSIAN_ROULETTE, PTMI_FLAG_SOURCE_SEED, scenes with a
 * ptmi_literal_kernel_reason and scenes whose records can yield NaN distances, ptmi_bind_accumulators, ptmi_set_stream.
 *   JITTERED / UNIFORM   every pixel of the region gains, in iteration order, bit for bit what ptmi_render would add to it; no
 *                        word of any pixel outside the region is read or written.
 *   RANDOM               the region selects WORK-ITEMS; their samples land where they land, possibly outside the region,
 *                        atomically as in ptmi_render.
 *   statistics           the histograms, ptmi_counters and the scheduler and invariant statistics gain what those paths
 *                        contribute and nothing else.
 *   several devices      the iteration ids spread over the listed devices exactly as for ptmi_render, each device over the
 *                        same region.
 * Asynchronous on the context's stream like ptmi_render, and bracketed for ptmi_kernel_time like it; at most the context's
 * iterations per kernel launch (1 with super_sampling), as for ptmi_render.  A region caller is NEVER RENDERED AHEAD OF: the
 * call adopts no launch that ran ahead, launches in flight ahead are dropped as for any call that leaves the pattern, and none
 * is left in flight behind it; nothing a caller can read differs.  A region equal to the whole image goes the same way as any
 * other region - it does not delegate to ptmi_render; the two are equal in everything a caller can read.
 * Returns PTMI_ERR_STATE before ptmi_initialize_memory; PTMI_ERR_INVALID_ARGUMENT for a NULL region, a region that does not lie
 * inside the image (x + width and y + height are checked in 64 bits) or an iteration range that overflows 32 bits.  A width or
 * height of 0, or n_iterations == 0, is PTMI_OK and launches nothing.  After any error the context renders as before.
 * Not offered for a region: ptmi_render_snapshots, the guides, ptmi_denoise, reprojection; a list of rectangles is a loop. */
int ptmi_render_region(ptmi_ctx* ctx, const ptmi_region* region, uint32_t first_iteration, uint32_t n_iterations);

/* The region of what ptmi_read_image would return at this moment: image_color = float4[width * height], image_ray_nb =
 * float[width * height], densely packed, rows first.  Either pointer may be NULL.  Waits as ptmi_read_image does; the shares of
 * several devices are summed first, as ptmi_read_image does.  One strided device-to-host copy per plane - straight into the
 * destination where the caller has page-locked it (ptmi_pin_host_buffer) -, so 20 bytes per pixel of the REGION cross the bus.
 * Statuses as for ptmi_render_region (an empty region copies nothing). */
int ptmi_read_region(ptmi_ctx* ctx, const ptmi_region* region, float* image_color, float* image_ray_nb);

/* The inverse of ptmi_read_image: load the accumulators (e.g. to resume a render saved earlier, or to accumulate on top of
 * another device's partial result).  Either pointer may be NULL (left as is).  Synchronises first. */
int ptmi_write_image(ptmi_ctx* ctx, const float* image_color, const float* image_ray_nb);

/* What the reference's viewer does with those two buffers after every image - ConvertRGBAToBMPBuffer,
 * Alone/PathTracer_bitmap.cpp:237-286, called from Alone/PathTracer_Dialog.cpp:161-185 - done on the device:
 * 24-bit B,G,R scanlines, image row 0 first, each `row_stride` bytes long ((3*W + 3) & ~3, the BMP padding, zero
 * filled), pixel = (int) min(sum * 255.f / n, 255.f); 3 bytes per pixel cross the bus instead of 20.
 * `bgr` holds H * row_stride bytes.  Synchronises first. */
int ptmi_read_display(ptmi_ctx* ctx, uint8_t* bgr, uint32_t row_stride);

/* Replaces the three statistic reads after the loop (OpenCL.cpp:110-112):
 * ray_depths[ray_max_depth+1], ray_intersected_bbx[5000], ray_intersected_tri[5000].
 * Any pointer may be NULL. */
int ptmi_read_statistics(ptmi_ctx* ctx, uint32_t* ray_depths, uint32_t* ray_intersected_bbx,
                         uint32_t* ray_intersected_tri);

/* Zero accumulators, histograms and counters (new render of the same scene). */
int ptmi_clear(ptmi_ctx* ctx);

/* Replaces the release block at the end of OpenCL_RunKernel (OpenCL.cpp:120-139). */
void ptmi_release(ptmi_ctx* ctx);

/* ---- updating the loaded scene in place ---------------------------------- */

/* A scene that moves need not be uploaded again: these two calls rewrite, on the device, the part of the scene a context holds
 * that has changed, and leave everything else where it is.  Both need an initialised context (PTMI_ERR_STATE otherwise), both
 * synchronise first (launches rendered ahead are dropped and the launch streams waited for before any memory a launch reads is
 * rewritten), both update every device of a multi-device context, and both check everything on the host before the first
 * device write: after any error the context renders the scene it held before the call.
 * NEITHER TOUCHES what has been rendered: accumulators, histograms, counters, snapshots, bound accumulators and the caller's
 * stream stay as they are.  A caller who wants a fresh image of the new scene calls ptmi_clear; a caller who does not
 * accumulates over the motion - motion blur.  ptmi_set_camera_reprojected (below) is the third way: it takes the image along.
 *
 * ptmi_set_camera: a new camera (kernel arguments 1..4 of the reference), everything else stays.  A camera that is not finite or
 * beyond 2^21 would change the kernel instantiation chosen at upload (ptmi_literal_kernel_reason): PTMI_ERR_UNSUPPORTED, call
 * ptmi_initialize_memory instead. */
int ptmi_set_camera(ptmi_ctx* ctx, const ptmi_float4* position, const ptmi_float4* direction, const ptmi_float4* right,
                    const ptmi_float4* up);

/* ptmi_update_triangles: new records for the triangles the context holds - triangulation[i] replaces triangle i of the array
 * ptmi_initialize_memory was given (the builder's order); triangulation_size must be the uploaded count
 * (PTMI_ERR_INVALID_ARGUMENT otherwise).  The tree keeps its topology (children, leaf ranges, cut axes, empty flags); every box
 * is refit on the device, bottom-up, from the new triangles' `aabb` - the boxes ptmi_bvh_refit gives, so the context then holds
 * what ptmi_initialize_memory would upload for (the new triangles, ptmi_bvh_refit's tree).  The triangles pass the checks
 * ptmi_initialize_memory applies (materials in range, texture coordinates: PTMI_ERR_BAD_SCENE).  PTMI_ERR_UNSUPPORTED, scene
 * untouched, where an update cannot express the new scene and ptmi_initialize_memory must be called: the scene has, or the new
 * triangles would give it, a ptmi_literal_kernel_reason; a triangle with unequal w on its vertices where every uploaded one had
 * equal w; an `aabb` that is marked empty, not finite, or has pMin > pMax; an uploaded tree whose empty flags do not follow
 * from its triangles.  The first update of a scene allocates a scratch copy of the triangles and the refit's schedule on the
 * device (kept until ptmi_initialize_memory / ptmi_release); a context that never updates pays nothing.
 * A refit keeps the tree's topology, so its quality decays as the triangles move far from where they were built: watch
 * ptmi_counters.box_tests per path and build a new tree when it has grown.  `info` may be NULL. */
typedef struct ptmi_update_info {
    uint32_t struct_size; /* set by the library: sizeof(ptmi_update_info) */
    uint32_t levels;      /* level passes of the refit (the depth of the inner nodes) */
    double upload_ms;     /* host -> device copies of the new triangles, all devices (device form: the copies to the other devices) */
    double device_ms;     /* device work behind them (HIP events), all devices */
    double total_ms;      /* the whole call */
    double validate_ms;   /* the checks of the new triangles, on the host or (device form) by the screen kernel with its readback (and, in the first update, the schedule) */
} ptmi_update_info;

int ptmi_update_triangles(ptmi_ctx* ctx, const ptmi_triangle* triangulation, uint32_t triangulation_size, ptmi_update_info* info);

/* ptmi_update_triangles_device: the same update from triangles that are on the device already - d_triangulation is the address,
 * on devices[0], of triangulation_size records of ptmi_triangle, 16-byte aligned (a torch tensor's data_ptr(): a mesh skinned,
 * simulated or deformed on the GPU).  No record crosses the bus.  The checks ptmi_update_triangles makes on the host run as one
 * kernel on the context's main stream (ptmi_set_stream's, where one was given), one verdict per triangle, and one 32-bit word
 * comes back: the call's only device-to-host traffic.  Statuses and messages are those of ptmi_update_triangles for the same
 * records, the index of the refused triangle included, and as there nothing is written after a refusal.
 * PTMI_ERR_INVALID_ARGUMENT before any device work: d_triangulation NULL or not 16-byte aligned, a count other than the
 * uploaded one.  The kernels read the caller's buffer in place on devices[0] (a context of one device that uses only this
 * form never allocates the scratch copy); every other listed device gets a device-to-device copy into its own scratch.
 * SYNCHRONOUS like the host form: when it returns the work is done on every device and the buffer is no longer read.  The
 * library reads the buffer on the main stream - the caller orders its own writes before the call - and never writes it.
 * info: validate_ms is the host checks plus the screen kernel and its readback, upload_ms the device-to-device copies to the
 * other devices (0 on one device), device_ms and levels as above.  Both forms may be mixed freely on one context. */
int ptmi_update_triangles_device(ptmi_ctx* ctx, const void* d_triangulation, uint32_t triangulation_size, ptmi_update_info* info);

/* ptmi_update_vertices: the same update from what a caller has - a vertex buffer (and, for a smooth mesh, a normal buffer) and
 * a topology bound once.  The library derives the 336-byte records itself, one lane per triangle on devices[0], and hands them
 * to the update above: screen, records, shading records, refit.
 *
 * THE RECORD.  Assembled record i is a pure function of the bound topology and the vertex buffers: the importer's
 * Triangle_Create (Maya/PathTracer_MayaImporter.cpp:943-1047).  Every operation is one IEEE binary32 operation in the written
 * order - no contraction, correctly rounded / and sqrt, denormals kept - and the same in both arithmetic modes of a context.
 * dot3(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *  1. Corners, IN THE FACE'S OWN WINDING: p_k = (positions[indices[3i+k]].xyz, 1), m_k = (normals[indices[3i+k]].xyz, 0), or
 *     with no normal buffer m_k = (N.xyz, 0), N of step 3.  Points carry w = 1 and directions w = 0 (MayaImporter.h:29-37).
 *  2. Box (BoundingBox_Create, Structs.h:197-205, all four components): pMin = min(min(p0,p1),p2), pMax = max(max(p0,p1),p2)
 *     with min(a,b) = b < a ? b : a and max(a,b) = a < b ? b : a (std::min / std::max: a tie keeps the first);
 *     centroid = (pMin + pMax) / 2, isEmpty = 0, the other bytes of the 64 are 0.
 *  3. Normal: e1 = p1 - p0, e2 = p2 - p0, c = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x),
 *     l = sqrt(dot3(c,c)), n = (c.x/l, c.y/l, c.z/l, 1).
 *  4. Order: the Vector_LexLessThan cascade of MayaImporter.cpp:961-1020 with its six outcomes as written there puts the
 *     corners into s1 < s2 < s3; m, uvp and uvn follow it.  (Ties matter only for triangles the screen refuses.)
 *  5. Shading normals (:1030-1036): l_k = sqrt(dot3(m_k, m_k)); n_k = n (w = 1) where l_k < 0.5f, else m_k / l_k in all four
 *     components.
 *  6. t1..bt3 are +0: the integrator never reads them (and the scenes of this library leave them so).  mat_pos, mat_neg and
 *     id come from the topology.  Every padding byte is 0: all 336 bytes are defined.
 *
 * ptmi_bind_mesh copies the host arrays of `topology` to devices[0] (72 bytes per triangle, 24 where uvp and uvn are both NULL);
 * triangle i of the topology is triangle i of the array ptmi_initialize_memory was given.  It needs an initialised context
 * (PTMI_ERR_STATE).  PTMI_ERR_INVALID_ARGUMENT: a wrong struct_size, reserved != 0, n_triangles other than the uploaded count,
 * and with triangles n_vertices == 0, indices or mat_pos NULL, an index >= n_vertices (the message names triangle, corner and
 * index).  Material indices are NOT checked here: the update's screen does.  A second bind replaces the first, a NULL topology
 * unbinds; ptmi_initialize_memory and ptmi_release free it.  It touches nothing rendered and nothing of the scene.
 *
 * ptmi_update_vertices_device: positions (and normals, or NULL for a flat mesh) are addresses on devices[0], 16-byte aligned:
 * three floats at base + v * stride, whatever else the stride holds is never read (a torch (V,3) tensor has stride 12).
 * Checked in this order before any device work: PTMI_ERR_INVALID_ARGUMENT for a NULL or wrongly sized struct; PTMI_ERR_STATE
 * with no scene or no bound mesh; PTMI_ERR_INVALID_ARGUMENT for n_vertices other than the bound one, a stride below 12 or not
 * a multiple of 4, NULL positions, a pointer that is not 16-byte aligned; PTMI_ERR_UNSUPPORTED where the scene has a
 * ptmi_literal_kernel_reason, in ptmi_update_triangles' words.  Then one kernel on the main stream of devices[0]
 * (ptmi_set_stream's, where one was given) writes the records into the context's scratch copy of the triangles (336 bytes per
 * triangle, allocated by the first update, freed with the scene), and ptmi_update_triangles_device's work runs on them under
 * this entry point's name: statuses and messages are those of ptmi_update_triangles for the assembled records, the refused
 * triangle's index included; nothing of the scene is written after a refusal; every other listed device gets the
 * device-to-device copy.  SYNCHRONOUS; the buffers are read on the main stream and never written.
 *
 * ptmi_update_vertices: the same from host buffers (no alignment asked), copied to a staging buffer on devices[0] that grows
 * on demand.  Of each buffer the bytes from its address to the last vertex's third float are read, (n_vertices - 1) * stride + 12,
 * and none beyond: positions and normals may interleave in one allocation that ends with the last normal.  The 336-byte records never exist on the host, and the screen runs on the device.
 *
 * info: upload_ms includes the vertex copy, device_ms the assemble kernel (HIP events), total_ms is the whole call.  The call
 * waits once for the assemble kernel and the screen behind it, so validate_ms contains the wait for both.
 *
 * ptmi_assemble_triangles: steps 1-6 on the host - the same code - into out[0 .. n_triangles).  No context, no device; the
 * refusals of ptmi_bind_mesh's arguments and of the buffers as PTMI_ERR_INVALID_ARGUMENT, messages in ptmi_last_error(NULL).
 * For callers that keep GlobalVars.triangulation in step, as ptmi_bvh_refit is for the tree. */
typedef struct ptmi_mesh_topology {   /* host arrays, copied by the call */
    uint32_t struct_size;             /* = sizeof(ptmi_mesh_topology) */
    uint32_t n_triangles;             /* = the uploaded count */
    uint32_t n_vertices;              /* >= 1 */
    uint32_t reserved;                /* 0 */
    const uint32_t* indices;          /* [3*n_triangles], each < n_vertices; triangle i = triangle i of the uploaded array */
    const ptmi_float2* uvp;           /* [3*n_triangles] per corner in face order; NULL = zeros */
    const ptmi_float2* uvn;           /* NULL = uvp */
    const uint32_t* mat_pos;          /* [n_triangles] */
    const uint32_t* mat_neg;          /* NULL = mat_pos */
    const uint32_t* ids;              /* NULL = i */
} ptmi_mesh_topology;
typedef struct ptmi_vertex_buffers {
    uint32_t struct_size;             /* = sizeof(ptmi_vertex_buffers) */
    uint32_t n_vertices;              /* = the bound one */
    uint32_t position_stride;         /* bytes, >= 12, a multiple of 4 */
    uint32_t normal_stride;           /* the same; not read where normals is NULL */
    const void* positions;            /* float x,y,z at positions + v*position_stride; anything else in the stride is never read */
    const void* normals;              /* NULL: flat */
} ptmi_vertex_buffers;
int ptmi_bind_mesh(ptmi_ctx* ctx, const ptmi_mesh_topology* topology);
int ptmi_update_vertices(ptmi_ctx* ctx, const ptmi_vertex_buffers* host, ptmi_update_info* info);
int ptmi_update_vertices_device(ptmi_ctx* ctx, const ptmi_vertex_buffers* device, ptmi_update_info* info);
int ptmi_assemble_triangles(const ptmi_mesh_topology* topology, const ptmi_vertex_buffers* host, ptmi_triangle* out);

/* Materials, lights and sky of the loaded scene, edited in place: what a look-development session changes between renders.
 * The three calls below follow the contract of ptmi_set_camera and ptmi_update_triangles above, word for word: an initialised
 * context (PTMI_ERR_STATE otherwise), every check before the first device write (after any error the context renders the scene
 * it held), launches rendered ahead dropped and the streams waited for, every listed device updated, nothing that has been
 * rendered touched.  Afterwards the context holds what ptmi_initialize_memory would upload for the edited scene: a render after
 * ptmi_clear is bit-equal to a fresh context's.  The numbers of materials, lights and textures and the texels stay the
 * uploaded ones.
 *
 * ptmi_update_materials: materiaux[k] replaces material first + k, k < n.  first + n beyond the uploaded count, or NULL with
 * n > 0: PTMI_ERR_INVALID_ARGUMENT; n == 0 does nothing.  The checks are ptmi_initialize_memory's, in its order and with its
 * words (status and message are ptmi_validate_scene's for the edited scene): a textured material whose texture_id is outside
 * the uploaded textures, then - only where a material of the range is textured now and was a plain colour before - the
 * texture coordinates of the triangles that use a textured material, which must be finite and at most 2^30: PTMI_ERR_BAD_SCENE.
 * That second check reads the shading records the context holds on devices[0], one kernel on the main stream and one word
 * back; no triangle crosses the bus.  The kernel instantiation follows the edit: a scene whose materials are all plain-colour
 * PTMI_MAT_STANDART and whose lights are all PTMI_LIGHT_POINT renders with the plain one, any other with the general one
 * (plain_before, plain_after).  `info` may be NULL. */
typedef struct ptmi_material_update_info {
    uint32_t struct_size;        /* set by the library: sizeof(ptmi_material_update_info) */
    uint32_t screened_triangles; /* triangles the device screen looked at: 0 where it did not run */
    uint32_t plain_before, plain_after; /* 1: every material a plain-colour MAT_STANDART, every light a point light - around the call */
    double validate_ms; /* the checks, the screen kernel and its readback included */
    double total_ms;    /* the whole call */
} ptmi_material_update_info;

int ptmi_update_materials(ptmi_ctx* ctx, uint32_t first, const ptmi_material* materiaux, uint32_t n, ptmi_material_update_info* info);

/* ptmi_update_lights: the whole light array anew.  lights_size must be config.lights_size (LIGHTS_SIZE is baked at setup):
 * PTMI_ERR_INVALID_ARGUMENT otherwise.  PTMI_ERR_UNSUPPORTED, scene untouched, where a light's position or direction is not
 * finite or beyond 2^21 (it would give the scene a ptmi_literal_kernel_reason, as a camera would: ptmi_set_camera) and where
 * the scene has such a reason already (it may be a light's).  A spot or directional light leaves the plain instantiation; a
 * scene whose lights are all point lights again goes back to it. */
int ptmi_update_lights(ptmi_ctx* ctx, const ptmi_light* lights, uint32_t lights_size);

/* ptmi_set_sky: the sky record anew - rotation, ground scale, exposure factors and the six face descriptors, each of which
 * must lie inside the uploaded textures_data (PTMI_ERR_BAD_SCENE otherwise, as at upload). */
int ptmi_set_sky(ptmi_ctx* ctx, const ptmi_sky* sky);

/* ---- single rays against the loaded scene --------------------------------- */

/* Rays of the caller's own, traced against the geometry the context holds NOW (after any ptmi_update_triangles): viewport
 * picking, line-of-sight and occlusion probes, collision rays, and a probe of traversal cost that renders no image.  One query
 * is the reference's BVH_IntersectRay (PTMI_QUERY_CLOSEST) or BVH_IntersectShadowRay (PTMI_QUERY_ANY) (FullKernel.cl:620-783)
 * on a ray made by Ray3D_Create, bit for bit in the context's arithmetic: the same visit order, the same 1e-5 thresholds, the
 * same quirks (the box test compares a linear distance with the squared limit, cl:135; a NaN distance is accepted and from then
 * on the last triangle that passes wins - a scene with a ptmi_literal_kernel_reason is served too).  Ray contents are not
 * validated: a ray that is not finite gets what the reference's loops would give it, and no ray can make the kernel leave the
 * tree that was validated at upload.  Where a field of a hit is a NaN, its sign and payload mean nothing: IEEE 754 leaves them
 * open, and so does the reference.
 * A QUERY TOUCHES NOTHING THAT HAS BEEN RENDERED: accumulators, histograms, ptmi_counters, scheduler statistics and snapshots
 * stay as they are, and launches rendered ahead are neither dropped nor waited for.  Both calls run on devices[0] of a
 * multi-device context (every device holds the same scene).  PTMI_ERR_STATE before ptmi_initialize_memory;
 * PTMI_ERR_INVALID_ARGUMENT for an unknown kind, a NULL pointer with n_rays > 0 or a device pointer that is not 16-byte
 * aligned; n_rays == 0 is PTMI_OK and launches nothing. */
typedef struct ptmi_ray {            /* 48 bytes */
    ptmi_float4 origin;              /* all four components enter the arithmetic, as in the reference (dot() is 4-wide); w = 0 is the usual choice */
    ptmi_float4 direction;           /* normalised by the library exactly as Ray3D_Create / Ray3D_SetDirection does (header.cl:276-284) */
    float max_squared_distance;      /* initial distance limit (the reference's squaredDistance); INFINITY = unlimited */
    uint32_t reserved[3];            /* 0 */
} ptmi_ray;

typedef struct ptmi_ray_hit {        /* 48 bytes */
    ptmi_float4 point;               /* intersectionPoint */
    float squared_distance, s, t;    /* as Triangle_Intersects leaves them */
    uint32_t triangle_id;            /* index into the triangulation[] given to ptmi_initialize_memory (the convention of ptmi_update_triangles); 0xFFFFFFFF = miss */
    uint32_t front;                  /* 1: dot(N, dir) < 0, the side materialWithPositiveNormalIndex shades */
    uint32_t box_tests, triangle_tests; /* numIntersectedBBx / numIntersectedTri of this one query */
    uint32_t reserved;
} ptmi_ray_hit;                      /* a miss: triangle_id 0xFFFFFFFF, front 0, point / squared_distance / s / t +0; both counts are still filled */

enum { PTMI_QUERY_CLOSEST = 0,  /* BVH_IntersectRay */
       PTMI_QUERY_ANY = 1 };    /* BVH_IntersectShadowRay: stops at the first accepted triangle, which is the one reported */

/* Host arrays: the rays go up into a scratch buffer of the context (allocated by the first query, grown on demand, freed by
 * ptmi_release: a context that never queries pays nothing), the kernel runs, the hits come down, and the call returns with
 * them in place - straight into `hits` where the caller has page-locked it (ptmi_pin_host_buffer). */
int ptmi_query_rays(ptmi_ctx* ctx, uint32_t kind, const ptmi_ray* rays, uint32_t n_rays, ptmi_ray_hit* hits);
/* Device pointers (e.g. torch tensors), 16-byte aligned: asynchronous on the context's stream (ptmi_set_stream's, where one
 * was given).  ptmi_update_triangles, ptmi_set_camera and ptmi_initialize_memory wait for a pending query before they
 * rewrite the scene; the caller orders its own reads of d_hits behind the stream (or calls ptmi_synchronize). */
int ptmi_query_rays_device(ptmi_ctx* ctx, uint32_t kind, const void* d_rays, uint32_t n_rays, void* d_hits);

/* ---- full paths along the caller's rays ------------------------------------ */

/* What light arrives along rays of the caller's own: other camera models (thin lens, orthographic, fisheye, panorama, stereo,
 * per-ray motion blur), light probes and irradiance bakes, a radiance readout at a picked point.  Ray i is traced for the
 * iterations it = first_iteration, ..., first_iteration + n_iterations - 1, in that order, and each one is Kernel_Main's path
 * (FullKernel.cl:1180-1331) with its camera ray replaced by the caller's:
 *   index   = first_index + i + it * index_stride, modulo 2^32: the gx + gy * W + it * W * H of InitializeRandomSeed;
 *   seed    = InitializeRandomSeed of that index, with the compiled reference's zero rule (PTMI_FLAG_SOURCE_SEED is honoured);
 *   sampler = the context's sampler is then drawn as Kernel_Main draws it and the values are discarded: two random() for
 *             JITTERED and RANDOM, none for UNIFORM.  There is no SUPER_SAMPLING stop-criterion draw: SUPER_SAMPLING is ignored;
 *   ray     = Ray3D_Create of (origin, direction), exactly as in ptmi_query_rays; max_squared_distance and reserved are NOT
 *             read (Kernel_Main's segments start unlimited);
 *   loop    = Kernel_Main's bounce loop from there: ray_max_depth, every light at every hit, the materials, the sky,
 *             PTMI_FLAG_RUSSIAN_ROULETTE, in the context's arithmetic, against the geometry the context holds NOW.
 * sums[i].radiance starts at +0 and adds each path's radiance in iteration order, all four components; the five counts add what
 * ptmi_counters would have gained from those paths.  So with the built-in camera's rays, first_index = 0 and index_stride = W*H,
 * ray gy * W + gx gets bit for bit the radiance ptmi_render adds to that pixel (JITTERED and UNIFORM).  With RANDOM the result
 * is still the ray's own: nothing "lands" anywhere.  Where a word is a NaN its sign and payload mean nothing, as for
 * ptmi_ray_hit.  A scene with a ptmi_literal_kernel_reason is served, as by the ray queries.
 * ONE LANE OWNS ONE RAY FOR ALL ITS ITERATIONS: a caller with few rays and many iterations gets more parallelism by repeating
 * the ray with different first_index.  n_iterations is at most PTMI_MAX_PATH_ITERATIONS, which bounds the time of one launch
 * on a shared device: a caller who wants more chains calls (first_iteration moving on) and adds the sums itself.
 * A CALL TOUCHES NOTHING THAT HAS BEEN RENDERED, with the same list as the ray queries: accumulators, histograms, ptmi_counters,
 * scheduler statistics, snapshots and launches rendered ahead stay as they are.  Both calls run on devices[0] of a multi-device
 * context, on its main stream (ptmi_set_stream's, where one was given); the calls that rewrite scene records wait for that
 * stream first.
 * PTMI_ERR_STATE before ptmi_initialize_memory; PTMI_ERR_INVALID_ARGUMENT for NULL params, a wrong struct_size, a non-zero
 * reserved word, n_iterations > PTMI_MAX_PATH_ITERATIONS, NULL rays or sums with work to do, or a device pointer that is not
 * 16-byte aligned; n_rays == 0 or n_iterations == 0 is PTMI_OK, launches nothing and writes nothing.  After any error the
 * context renders as before. */
#define PTMI_MAX_PATH_ITERATIONS 4096u
typedef struct ptmi_path_params {   /* 32 bytes */
    uint32_t struct_size;           /* = sizeof(ptmi_path_params) */
    uint32_t first_iteration, n_iterations;   /* n_iterations <= PTMI_MAX_PATH_ITERATIONS */
    uint32_t first_index, index_stride;
    uint32_t reserved[3];           /* 0 */
} ptmi_path_params;

typedef struct ptmi_path_sum {      /* 48 bytes: three 16-byte quads, like ptmi_ray_hit */
    ptmi_float4 radiance;           /* sum over the iterations */
    uint32_t segments, surface_hits, shadow_rays, reserved;   /* the ptmi_counters terms of these paths alone */
    uint64_t box_tests, triangle_tests;
} ptmi_path_sum;

/* Host arrays: as for ptmi_query_rays - a scratch buffer of the context's own (allocated by the first call, grown on demand,
 * freed by ptmi_release: a context that never asks pays nothing), and the sums come down straight into `sums` where the caller
 * has page-locked it (ptmi_pin_host_buffer). */
int ptmi_trace_paths(ptmi_ctx* ctx, const ptmi_path_params* params, const ptmi_ray* rays, uint32_t n_rays, ptmi_path_sum* sums);
/* Device pointers, 16-byte aligned: asynchronous on the context's stream, ordered like ptmi_query_rays_device. */
int ptmi_trace_paths_device(ptmi_ctx* ctx, const ptmi_path_params* params, const void* d_rays, uint32_t n_rays, void* d_sums);

/* ---- first-hit guide buffers ----------------------------------------------- */

/* What the camera sees, per pixel, without rendering it: albedo, shading normal and position planes (denoiser inputs), a hit
 * count (the hit mask) and an id plane (picking, selection outlines).  Pixel p = gy * W + gx is visited for the iterations
 * it = first_iteration, ..., first_iteration + n_iterations - 1, in that order, and for each one the PRIMARY ray is traced that
 * ptmi_render traces for (gx, gy, it): the same seed (InitializeRandomSeed; PTMI_FLAG_SOURCE_SEED is honoured), the same sample
 * (sampler(), FullKernel.cl:1119-1150), the same camera expression (cl:1213) and Ray3D_Create, the same BVH_IntersectRay with
 * an unlimited distance - bit for bit in the context's arithmetic, against the geometry and the camera the context holds NOW
 * (after any ptmi_set_camera / ptmi_update_triangles).  Every sum starts at +0 and adds in iteration order, so the planes are a
 * function of the call's arguments alone.
 *   a hit:   albedo[p]    += the colour the integrator shades with: the material's, or the texel of Triangle_GetColorValueAt
 *            normal[p]    += Ns, the smooth normal after cl:1254-1274 (turned towards the ray, normalised)
 *            position[p]  += intersectionPoint
 *            hit_count[p] += 1
 *   a miss:  albedo[p]    += Sky_GetColorValue(direction), the colour the path would collect; nothing else is added.
 *   ids[4p .. 4p+3] describe iteration first_iteration ONLY: triangle_id (the caller's index, as in ptmi_ray_hit; 0xFFFFFFFF = a
 *            miss), the material index that was shaded (the positive-normal one where front, else the negative-normal one; 0 on
 *            a miss), front (as in ptmi_ray_hit; 0 on a miss), 0.
 * All four components of albedo, normal and position are summed, as the reference's float4 arithmetic carries them.  Where a
 * word is a NaN its sign and payload mean nothing, as for ptmi_ray_hit.  SUPER_SAMPLING is ignored: every iteration is traced
 * (the stop criterion's draw comes after the sample and cannot move the ray).  A scene with a ptmi_literal_kernel_reason is
 * served, as by the ray queries.
 * A GUIDE CALL TOUCHES NOTHING THAT HAS BEEN RENDERED, with the same list as the ray queries: accumulators, histograms,
 * ptmi_counters, scheduler statistics, snapshots and launches rendered ahead stay as they are.  Both calls run on devices[0] of
 * a multi-device context, on its main stream (ptmi_set_stream's, where one was given); the calls that rewrite scene records
 * wait for that stream first.
 * PTMI_ERR_STATE before ptmi_initialize_memory; PTMI_ERR_INVALID_ARGUMENT for a NULL struct, a wrong struct_size or a device
 * plane that is not 16-byte aligned; PTMI_ERR_UNSUPPORTED on a context set up with the RANDOM sampler (its samples land on
 * other pixels than the work-item's); n_iterations == 0, or every plane NULL, is PTMI_OK and launches nothing.  After any error
 * the context renders as before. */
typedef struct ptmi_guides {
    uint32_t struct_size;   /* = sizeof(ptmi_guides) */
    uint32_t reserved;      /* 0 */
    float*    albedo;       /* float4[W*H] */
    float*    normal;       /* float4[W*H] */
    float*    position;     /* float4[W*H] */
    float*    hit_count;    /* float [W*H] */
    uint32_t* ids;          /* uint32[4*W*H] */
} ptmi_guides;              /* any plane may be NULL: not written */

/* Host planes: the kernel fills a scratch buffer of the context (allocated by the first guide call for the planes it asks for,
 * grown when a later call asks for more, freed by ptmi_release: a context that never asks pays nothing), the planes come down -
 * straight into the ones the caller has page-locked (ptmi_pin_host_buffer) - and the call returns with them filled. */
int ptmi_render_guides(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations, const ptmi_guides* host_planes);
/* Device pointers (e.g. torch tensors), each 16-byte aligned: asynchronous on the context's stream, ordered like
 * ptmi_query_rays_device. */
int ptmi_render_guides_device(ptmi_ctx* ctx, uint32_t first_iteration, uint32_t n_iterations, const ptmi_guides* device_planes);

/* ---- denoising the image on the device ------------------------------------- */

/* The stage between the accumulators and the display: an edge-avoiding a-trous wavelet filter of the MEAN image, guided by the
 * first-hit planes above.  A 5 x 5 B3-spline footprint at steps 1, 2, 4, 8, 16 (pass k uses step 1 << k); a tap counts less
 * the further it is from the centre pixel in colour, shading normal and position, and is never taken across the hit mask.  With
 * PTMI_DENOISE_DEMODULATE_ALBEDO the image is divided by the albedo before the filter and multiplied back after it, so that
 * texture detail is not blurred.  sigma_position is in SCENE UNITS (a distance between first hits), sigma_normal a distance
 * between unit normals, sigma_color one between (demodulated) colours; it halves with every pass.
 *
 * THE ARITHMETIC, the same in both arithmetic modes of a context.  Every operation is one IEEE binary32 operation in the
 * written order: no contraction, correctly rounded division, denormals kept, no transcendental.
 * dot3(v) = (v.x*v.x + v.y*v.y) + v.z*v.z;  color / ray_nb = the image planes;  albedo, normal, position, hit_count = guide
 * planes summed over guide_iterations iterations;  B = {0.375f, 0.25f, 0.0625f}.
 *   prepass, pixel p:  n = ray_nb[p];  m = n > 0 ? color[p].xyz / n : 0;  G = (float)guide_iterations;  a = albedo[p].xyz / G;
 *       h = hit_count[p];  hit = h > 0;  nrm = hit ? normal[p].xyz / h : 0;  pos = hit ? position[p].xyz / h : 0;
 *       d_c = a_c > 1e-3f ? a_c : 1e-3f per channel with the flag (a NaN albedo gives 1e-3), d = 1 without;  e0 = m / d.
 *   pass k = 0 .. passes-1, s = 1 << k, from e(k):  inv_c = (float)(1 << 2k) / (sigma_color * sigma_color),
 *       inv_n = 1.f / (sigma_normal * sigma_normal), inv_p = 1.f / (sigma_position * sigma_position), computed on the host in
 *       float.  sw = 0, se = 0;  for dy = -2..2 (outer), dx = -2..2 (inner), q = (x + s*dx, y + s*dy):
 *         skipped when q is outside the image or hit_q != hit_p;  b = B[|dy|] * B[|dx|];
 *         xc = dot3(e_q - e_p) * inv_c;  xn = dot3(nrm_q - nrm_p) * inv_n;  xp = dot3(pos_q - pos_p) * inv_p;
 *         w = b / (((1.f + xc) * (1.f + xn)) * (1.f + xp));  skipped when !(w > 0) (a NaN anywhere, an overflow to b / inf);
 *         sw = sw + w;  se_c = se_c + w * e_q,c.
 *       e(k+1) = sw > 0 ? se / sw : e_p: a pixel whose own value is not a number keeps it and never reaches a neighbour.
 *   output:  out[p] = (e.x * d.x, e.y * d.y, e.z * d.z, n), e the last pass's; with passes = 0 that is e0 * d.
 * Where a word of the result is a NaN its sign and payload mean nothing, as everywhere here.
 *
 * A DENOISE CALL TOUCHES NOTHING THAT HAS BEEN RENDERED: accumulators, histograms, ptmi_counters, scheduler statistics, the
 * caller's snapshot slots and launches rendered ahead stay as they are - the promise of the ray queries and the guide calls.
 * Scratch on devices[0], allocated by the first call and freed by ptmi_release (a context that never denoises pays nothing):
 * 56 bytes per pixel of feature planes for either form, and for ptmi_denoise 68 more (its guide planes, 52, and the result, 16).
 * PTMI_ERR_STATE before ptmi_initialize_memory; PTMI_ERR_INVALID_ARGUMENT for a NULL struct, a wrong struct_size, passes > 5,
 * an unknown flag, a non-zero reserved word, guide_iterations of 0 or >= 2^24 (the planes' counts are exact floats below
 * that), a sigma that is not finite and > 0, a missing plane or a device pointer that is not 16-byte aligned.  After any error
 * the context renders as before. */
#define PTMI_DENOISE_DEMODULATE_ALBEDO 1u
#define PTMI_DENOISE_UNTILED 2u /* steps 1 and 2 read every tap from memory instead of a tile staged in LDS: the same words, for A/B */
typedef struct ptmi_denoise_params {
    uint32_t struct_size;           /* = sizeof(ptmi_denoise_params) */
    uint32_t passes;                /* 0..5: pass k uses step 1 << k */
    uint32_t flags;                 /* PTMI_DENOISE_* */
    uint32_t guide_first_iteration; /* ptmi_denoise only: the guides are rendered for [guide_first_iteration, + guide_iterations) */
    uint32_t guide_iterations;      /* >= 1, < 2^24: how many iterations the guide planes sum */
    float sigma_color, sigma_normal, sigma_position; /* each finite and > 0 */
    uint32_t reserved[2];           /* 0 */
} ptmi_denoise_params;

/* Host form: filters the image ptmi_read_image would return at this moment (on a multi-device context the devices' shares are
 * summed first, as for ptmi_read_display), with guides rendered for the iterations the struct names, exactly as
 * ptmi_render_guides would; image_out is float4[W*H] = (filtered mean r, g, b, the sample count), filled when the call returns -
 * directly where the caller has page-locked it (ptmi_pin_host_buffer).  PTMI_ERR_UNSUPPORTED with the RANDOM sampler, as for
 * ptmi_render_guides. */
int ptmi_denoise(ptmi_ctx* ctx, const ptmi_denoise_params* params, float* image_out);
/* Device form: every pointer is a device address, 16-byte aligned; asynchronous on the context's stream (ptmi_set_stream's,
 * where one was given), ordered like ptmi_render_guides_device: the calls that rewrite scene records wait for it.
 * device_guides carries albedo, normal, position and hit_count (ids is ignored), filled by ptmi_render_guides_device over
 * guide_iterations iterations: the caller may reuse them for as long as camera and geometry stand still.  d_image_color and
 * d_image_ray_nb are both given - any float4 sum plane and float count plane: a snapshot, another context's image, a tensor - or
 * both NULL: the context's own accumulators (PTMI_ERR_UNSUPPORTED on a multi-device context, as for
 * ptmi_device_accumulators).  d_image_out (float4[W*H]) MUST NOT ALIAS AN INPUT; the library cannot check that. */
int ptmi_denoise_device(ptmi_ctx* ctx, const ptmi_denoise_params* params, const ptmi_guides* device_guides,
                        const void* d_image_color, const void* d_image_ray_nb, void* d_image_out);

/* ---- carrying the image across a camera move ------------------------------ */

/* Temporal reprojection: the accumulated image of the PREVIOUS camera, resampled to where the same surfaces lie under the camera
 * of NOW, so that a viewer that orbits neither smears the old views into the new one (accumulating on) nor starts from one noisy
 * sample per pixel (ptmi_clear).  The position plane of the guides holds the world-space point a pixel sees; projecting it into
 * the previous camera finds the previous pixels that saw that point, and the previous position and normal planes say whether
 * they really saw the same surface.  A pure function of planes and one camera: the camera of NOW is not an argument, the
 * current position plane already holds world-space points.
 *
 * THE ARITHMETIC, the same in both arithmetic modes of a context.  Every operation is one IEEE binary32 operation in the
 * written order: no contraction, correctly rounded division, denormals kept, no transcendental.
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;  min(a, b) = a < b ? a : b;  prev.* = the previous planes (position, normal,
 * hit_count of previous_guides; color, ray_nb), cur.* = current_guides.
 *   on the host, in DOUBLE, each result rounded to float once:  cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 *       a.x*b.y - a.y*b.x);  with the previous camera's dir, right, up (xyz): c = cross(right, up), det = dot3(dir, c),
 *       r0 = c / det, r1 = cross(up, dir) / det, r2 = cross(dir, right) / det - the rows that solve
 *       v = t * (dir + sx*right + sy*up) for any camera, orthogonal or not (the camera expression is cl:1213).
 *   on the host, in float:  tp = position_tolerance * position_tolerance, tn = normal_tolerance * normal_tolerance,
 *       Wf = (float)W, Hf = (float)H.
 *   pixel p = (x, y) of the new frame:
 *     1. h = cur.hit_count[p]; no history unless h > 0.
 *     2. P = cur.position[p].xyz / h, N = cur.normal[p].xyz / h, v = P - previous_camera[0].xyz.
 *     3. t = dot3(r0, v), a = dot3(r1, v), b = dot3(r2, v); no history unless t > 0.
 *     4. u = (a / t + 0.5f) * Wf - 0.5f, w_ = (b / t + 0.5f) * Hf - 0.5f (the centre of previous pixel gx is u = gx); no history
 *        unless u > -1 && u < Wf && w_ > -1 && w_ < Hf (a NaN fails).
 *     5. x0 = floorf(u), fx = u - x0, y0 = floorf(w_), fy = w_ - y0, lim = tp * dot3(v, v).
 *     6. the taps (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1), in this order, with weights w = (1-fx)*(1-fy), fx*(1-fy),
 *        (1-fx)*fy, fx*fy.  A tap q is taken only when it lies inside the image, w > 0, hq = prev.hit_count[q] > 0,
 *        nq = prev.ray_nb[q] > 0, dot3(Pq - P, Pq - P) <= lim with Pq = prev.position[q].xyz / hq,
 *        dot3(Nq - N, Nq - N) <= tn with Nq = prev.normal[q].xyz / hq, and all four channels of mq = prev.color[q] / nq are
 *        finite (mq_c - mq_c == 0).
 *     7. a taken tap adds sw = sw + w, sm_c = sm_c + w * mq_c (all four channels), sn = sn + w * nq.
 *     8. history exists when sw > 0 and n = floorf(min(sn / sw, max_history)) >= 1:
 *        out_color[p]_c = (sm_c / sw) * n, out_ray_nb[p] = n; otherwise four +0 and a count of +0.
 * WHAT FOLLOWS.  All four channels of the radiance are treated alike, as everywhere here.  Counts stay integral floats.  A MISS
 * pixel (the sky) carries no history: it has no world point, and it converges in a few samples.  A pixel without history comes
 * out exactly as ptmi_clear leaves it.  A bad previous pixel (a NaN or infinite channel, a count that is zero, negative or NaN)
 * never reaches the output, so with finite counts no word of the output is a NaN.  position_tolerance is RELATIVE, a fraction of
 * the point's distance from the previous camera (neighbouring pixels lie further apart the further away they are);
 * normal_tolerance is a distance between mean shading normals, as the denoiser's sigma_normal.  (A position_tolerance of 0.64,
 * the Python binding's measured default, lets every tap of an ordinary scene pass: the position test is then off.)  Geometry that
 * ptmi_update_triangles has moved is tested at its new position: it mostly fails the position test and restarts (per-object
 * motion vectors are not kept).
 *
 * PTMI_ERR_STATE before ptmi_initialize_memory; PTMI_ERR_INVALID_ARGUMENT for a NULL or wrongly sized struct (the params or
 * either ptmi_guides), a non-zero flags or reserved, a tolerance that is not finite and > 0, max_history that is NaN or < 1,
 * guide_iterations of 0 or >= 2^24 (host form), a missing plane, a pointer that is not 16-byte aligned, a previous camera whose
 * position, direction, right or up (xyz) is not finite or whose det is 0 or not finite.  After any error the context renders,
 * and holds, what it did before. */
typedef struct ptmi_reproject_params {   /* 32 bytes */
    uint32_t struct_size;            /* = sizeof(ptmi_reproject_params) */
    uint32_t flags;                  /* 0: none defined yet */
    uint32_t guide_first_iteration;  /* ptmi_set_camera_reprojected only */
    uint32_t guide_iterations;       /* ptmi_set_camera_reprojected only: >= 1, < 2^24 */
    float position_tolerance;        /* finite, > 0: RELATIVE - a fraction of the point's distance from the previous camera */
    float normal_tolerance;          /* finite, > 0: a distance between mean shading normals, as the denoiser's sigma_normal */
    float max_history;               /* >= 1, +INFINITY allowed, not NaN: cap of the sample count a pixel carries over */
    uint32_t reserved;               /* 0 */
} ptmi_reproject_params;

/* Device form: every pointer is a device address, 16-byte aligned; asynchronous on the context's main stream (ptmi_set_stream's,
 * where one was given), ordered like ptmi_denoise_device: the calls that rewrite scene records wait for it.  It TOUCHES NOTHING
 * THAT HAS BEEN RENDERED (the list of the guide and denoise calls) and needs no scratch at all.  previous_camera = position,
 * direction, right, up the previous planes were made with; previous_guides and current_guides carry normal, position and
 * hit_count (albedo and ids are ignored), summed over any number of iterations; d_previous_color / d_previous_ray_nb are the
 * float4[W*H] sums and float[W*H] counts of the previous image; d_out_color (float4[W*H]) and d_out_ray_nb (float[W*H]) MUST NOT
 * ALIAS AN INPUT; the library cannot check that. */
int ptmi_reproject_device(ptmi_ctx* ctx, const ptmi_reproject_params* params, const ptmi_float4 previous_camera[4],
                          const ptmi_guides* previous_guides, const void* d_previous_color, const void* d_previous_ray_nb,
                          const ptmi_guides* current_guides, void* d_out_color, void* d_out_ray_nb);

/* Host form: ptmi_set_camera that takes the image along.  In this order, what a caller could do with the calls above:
 *   1. guides (position, normal, hit count) for [guide_first_iteration, + guide_iterations) under the camera the context holds;
 *   2. the image ptmi_read_image would return (on a multi-device context the shares are summed, as for ptmi_denoise);
 *   3. everything ptmi_set_camera does (synchronise, drop launches rendered ahead, every device);
 *   4. the same guides under the new camera;
 *   5. the reprojection above, with the camera of step 1 as the previous one;
 *   6. the result stored as ptmi_write_image would: devices[0] gets it, every other device restarts from zero - copied on the
 *      device, nothing crosses the bus.
 * Afterwards the context is in the state "ptmi_set_camera + ptmi_write_image(reprojected)": histograms, ptmi_counters,
 * scheduler statistics and the caller's snapshot slots are unchanged, bound accumulators (ptmi_bind_accumulators) are written in
 * place.  Scratch on devices[0], allocated by the first call and freed by ptmi_release: 92 bytes per pixel - two sets of the
 * three guide planes at 36 bytes each, and the result at 20 (plus at most 45 bytes: every plane starts 16-byte aligned).  Every
 * check and every allocation happens before the first write to the camera or the accumulators.
 * PTMI_ERR_UNSUPPORTED for everything ptmi_set_camera refuses; on a context with the RANDOM sampler (no guides, as
 * ptmi_denoise); and on a context with super_sampling, whose variance accumulator and per-pixel stop decisions cannot be
 * carried over. */
int ptmi_set_camera_reprojected(ptmi_ctx* ctx, const ptmi_float4* position, const ptmi_float4* direction, const ptmi_float4* right,
                                const ptmi_float4* up, const ptmi_reproject_params* params);

/* ---- displaying an image ------------------------------------------------- */

/* The last stage of a viewer's pipeline: any image plane -> 8-bit pixels, on the device, so that 3 (or 4) bytes per pixel cross
 * the bus and no float plane does.  Exposure, a tone operator, a display transfer function, quantisation by rounding to the
 * nearest encoded value; and a luminance histogram of the same image, from which a viewer chooses the exposure without reading
 * the image back.  ptmi_read_display (above) stays what it is: the reference viewer's linear clamp, the parity path.
 *
 * THE IMAGE.  The host forms take the image ptmi_read_image would return at this moment (on a multi-device context the shares
 * are summed first, as for ptmi_read_display and ptmi_denoise).  The device forms take
 *   d_color and d_count    any float4[W*H] sum plane and float[W*H] count plane: a snapshot, ptmi_reproject_device's result;
 *   d_color alone          a float4[W*H] MEAN plane whose fourth word is ignored: exactly what ptmi_denoise_device writes;
 *   neither                the context's own accumulators (PTMI_ERR_UNSUPPORTED on a multi-device context, as for
 *                          ptmi_denoise_device);
 *   d_count alone          PTMI_ERR_INVALID_ARGUMENT.
 *
 * THE ARITHMETIC, the same in both arithmetic modes of a context.  Every operation is one IEEE binary32 operation in the
 * written order: no contraction, correctly rounded division, denormals kept, no transcendental on the device.
 * min(a, b) = a < b ? a : b.  Pixel p, channel c of r, g, b:
 *   1. mean.      sum form: n = count[p]; m_c = n > 0 ? sum_c / n : 0 (a count that is zero, negative or NaN shows BLACK, not
 *                 255);  mean form: m_c = plane_c.
 *   2. exposure.  x = m_c * exposure;  if (!(x > 0)) x = 0  (NaN and negative values go to 0).
 *   3. tone.      CLAMP: t = x.   REINHARD: w2 = white * white on the host in float; t = (x * (1.f + x / w2)) / (1.f + x).
 *                 FILMIC (Narkowicz's fit of the ACES curve): t = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f).
 *                 Then, for all three, t = min(t, 1.f): the NaN of inf / inf at a huge x becomes 1, white.
 *   4. transfer and quantisation.  byte = the largest k in 0..255 with T[k] <= t, T = ptmi_display_table(transfer):
 *                 T[0] = 0, T[k] = (float) EOTF((k - 0.5) / 255.0) with the EOTF evaluated in double - round to nearest AFTER
 *                 encoding.  LINEAR: v.  SRGB: v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4).  GAMMA22: pow(v, 2.2).
 *                 The three tables are constants of the source (csrc/display_tables.inc), strictly increasing.
 *   5. output.    BGR24: B, G, R per pixel in scanlines of row_stride bytes, EVERY padding byte written 0 (ptmi_read_display's
 *                 layout);  RGBA32: R, G, B, 255.  Image row 0 first.
 * THE LUMINANCE HISTOGRAM works on the mean m of step 1, before exposure:  Y = (0.2126f * m.x + 0.7152f * m.y) + 0.0722f * m.z.
 *   words 0..255   the pixels with Y > 0 and Y finite, in quarter-octave bins read off the float's own bits:
 *                  bin = clamp((bits(Y) >> 21) - 380, 0, 255); bin b starts at (1 + (b & 3) / 4) * 2^((b >> 2) - 32), bin 128 at 1.0;
 *   word 256       the pixels with !(Y > 0): black, negative, NaN, never sampled;
 *   word 257       the pixels with Y == +inf;    words 258, 259: 0.
 * The 260 words sum to W*H.  Counts are integers added with atomics: the result does not depend on an order.
 *
 * ORDER AND STATE.  The device forms are asynchronous on the context's main stream (ptmi_set_stream's, where one was given),
 * ordered like ptmi_denoise_device; the host forms wait for their own stream before they return.  All four calls TOUCH NOTHING
 * THAT HAS BEEN RENDERED (the list of the guide and denoise calls).  Scratch on devices[0]: none for the device forms; for the
 * host forms the display buffer ptmi_read_display uses, grown on demand, and 1040 bytes for the histogram.
 * PTMI_ERR_STATE before ptmi_initialize_memory; PTMI_ERR_INVALID_ARGUMENT for a NULL struct, a wrong struct_size, a non-zero
 * flags or reserved word, an unknown tone, transfer or format, a row_stride outside its range, an exposure that is not finite
 * and > 0, under REINHARD a white that is NaN or <= 0, a NULL output, a device pointer that is not 16-byte aligned.  After any
 * error the context renders as before. */
enum { PTMI_TONE_CLAMP = 0, PTMI_TONE_REINHARD = 1, PTMI_TONE_FILMIC = 2 };
enum { PTMI_TRANSFER_LINEAR = 0, PTMI_TRANSFER_SRGB = 1, PTMI_TRANSFER_GAMMA22 = 2 };
enum { PTMI_PIXELS_BGR24 = 0,   /* B,G,R scanlines of row_stride bytes, padding zero-filled: ptmi_read_display's layout */
       PTMI_PIXELS_RGBA32 = 1 };/* R,G,B,255 - 4 bytes per pixel, row_stride = 4*W exactly */

typedef struct ptmi_display_params {   /* 48 bytes */
    uint32_t struct_size;   /* = sizeof(ptmi_display_params) */
    uint32_t flags;         /* 0: none defined */
    uint32_t tone, transfer, format;
    uint32_t row_stride;    /* BGR24: 3*W .. 3*W+3;  RGBA32: 4*W */
    float exposure;         /* finite, > 0 */
    float white;            /* REINHARD only: > 0, +INFINITY allowed (= plain x/(1+x)), not NaN; ignored otherwise */
    uint32_t reserved[4];   /* 0 */
} ptmi_display_params;

#define PTMI_LUMINANCE_WORDS 260u

/* The 256 thresholds of a transfer function (step 4).  Host only: no device, no context.  PTMI_ERR_INVALID_ARGUMENT for an
 * unknown transfer or a NULL table, with the message in ptmi_last_error(NULL). */
int ptmi_display_table(uint32_t transfer, float table[256]);
/* Host form: `pixels` holds H * row_stride bytes, filled when the call returns - directly where the caller has page-locked it
 * (ptmi_pin_host_buffer). */
int ptmi_read_display_tonemapped(ptmi_ctx* ctx, const ptmi_display_params* params, uint8_t* pixels);
/* Device form: d_pixels holds H * row_stride bytes, 16-byte aligned like the planes, and MUST NOT ALIAS AN INPUT. */
int ptmi_display_device(ptmi_ctx* ctx, const ptmi_display_params* params, const void* d_color, const void* d_count, void* d_pixels);
int ptmi_luminance_histogram(ptmi_ctx* ctx, uint32_t histogram[PTMI_LUMINANCE_WORDS]);
/* Device form: d_histogram holds PTMI_LUMINANCE_WORDS words, 16-byte aligned; the call zeroes it on the stream before it counts. */
int ptmi_luminance_histogram_device(ptmi_ctx* ctx, const void* d_color, const void* d_count, void* d_histogram);

/* ---- measurement / plumbing -------------------------------------------- */

int ptmi_get_counters(ptmi_ctx* ctx, ptmi_counters* out);
int ptmi_get_scheduler_stats(ptmi_ctx* ctx, ptmi_scheduler_stats* out);
int ptmi_get_invariant_checks(ptmi_ctx* ctx, ptmi_invariant_checks* out);
/* NaN distances.  The reference's triangle test (FullKernel.cl:519-589) rejects with comparisons only, so a triangle on which
 * it computes NaNs is ACCEPTED, with a NaN distance, and from then on the LAST triangle that passes wins, not the nearest.
 * The integrator reproduces that bit for bit.  Where the RAY is not a number (a refraction at |cos| = 1 + 1 ulp, cl:235) the
 * wavefront kernel gives the path up and re-traces it with the reference's literal loops (every sampler; RANDOM: a give-up list).
 * Where the scene's RECORDS are the source - zero-area triangles, whose normal the importer computes as 0/0; non-finite or
 * astronomically large coordinates - this call returns why (else NULL), and the scene is rendered by an instantiation of the
 * wavefront kernel that looks at every accepted triangle of a closest-hit query: only the paths that REACH such a record are
 * given up and traced again by the literal loops (ptmi_scheduler_stats.paths_retraced), every other path runs as in a clean
 * scene.  With the RANDOM sampler (nothing is staged there, so nothing can be traced again) such a scene is rendered by the
 * one-path-per-lane kernel as a whole (as with PTMI_FLAG_MEGAKERNEL: same results, slower; PTMI_ERR_UNSUPPORTED with
 * super_sampling).  The string lives until the next ptmi_initialize_memory / ptmi_release. */
const char* ptmi_literal_kernel_reason(const ptmi_ctx* ctx);

/* How a multi-device context sums its devices' partial images (for records and scaling logs): *rccl_state = 1 when the last sum
 * went through ncclReduce (PTMI_REDUCE=rccl), 0 when the collective has not been tried, -1 when it is unavailable or was refused
 * (peer copies + the add kernel in device order: the default); *n_communicators = the communicators ncclCommInitAll returned for
 * this context (= the device count when the collective is in use, else 0); *nccl_version = ncclGetVersion's code (0: library not
 * loaded).  Any pointer may be NULL. */
int ptmi_reduce_path(const ptmi_ctx* ctx, int* rccl_state, int* n_communicators, int* nccl_version);

/* Device time of the integrator kernel launches issued by ptmi_render since the
 * last call, measured with HIP events on the context's stream.  Synchronises. */
int ptmi_kernel_time(ptmi_ctx* ctx, double* total_ms, uint32_t* n_launches);

/* Run on a caller-owned hipStream_t (passed as void*; NULL = context's own).  Single-device contexts only, like the
 * three accumulator entry points below (PTMI_ERR_UNSUPPORTED with n_devices > 1: each device has partial sums). */
int ptmi_set_stream(ptmi_ctx* ctx, void* hip_stream);

/* Device pointers of the accumulators (float[4*W*H], float[W*H]) so a caller
 * that owns a collective library can reduce them in place (multi-GPU spp shards). */
int ptmi_device_accumulators(ptmi_ctx* ctx, void** d_image_color, void** d_image_ray_nb);

/* SUPER_SAMPLING only: the per-pixel variance accumulator global__imageV (float4[W*H]; the sum of squared
 * deviations the stop criterion reads, FullKernel.cl:1152-1172,1346-1349).  On a multi-device context every device
 * samples adaptively on its own accumulators (its stop decisions are its own) and ptmi_read_variance returns the moments
 * of all devices merged pairwise (Chan's update; the same arithmetic as opencl_pathtracer_amd/distributed.py:
 * merge_moments, which does it across processes).  PTMI_ERR_STATE without super_sampling. */
int ptmi_read_variance(ptmi_ctx* ctx, float* image_v);
int ptmi_write_variance(ptmi_ctx* ctx, const float* image_v); /* with ptmi_write_image: resume a SUPER_SAMPLING render */
int ptmi_device_variance(ptmi_ctx* ctx, void** d_image_v);

/* Adopt caller-allocated device buffers as accumulators (e.g. torch tensors);
 * they are NOT zeroed and NOT freed by the context.  Pass NULLs to go back. */
int ptmi_bind_accumulators(ptmi_ctx* ctx, void* d_image_color, void* d_image_ray_nb);

/* Message of the last failure on this context (ctx may be NULL for failures of
 * ptmi_setup_context / ptmi_bvh_create).  Never NULL. */
const char* ptmi_last_error(const ptmi_ctx* ctx);

int ptmi_abi_version(void);
int ptmi_device_count(void);

/* Which iteration ids of [first_iteration, first_iteration + n_iterations) device `k` of `n_devices` renders: the ids
 * congruent to k modulo n_devices = *first_k, *first_k + n_devices, ... (*n_k of them).  Pure arithmetic, no device. */
void ptmi_device_share(uint32_t first_iteration, uint32_t n_iterations, uint32_t k, uint32_t n_devices, uint32_t* first_k,
                       uint32_t* n_k);

/* ---- host-side producer of the bvh input -------------------------------- */

/* Replaces BVH_Create (PathTracer_BVH.cpp:12-37 -> BVH_BuildStructure :109-356):
 * binned-SAH build, bit-compatible with the reference (same node order, same
 * in-place reordering of `triangulation`).  `bvh` must hold 2*n-1 nodes.
 * Host only; needs no device. */
/* Host-only (no device, no context): would ptmi_initialize_memory accept `scene` on a context set up with `config`?  The same
 * checks - every index the kernel will follow, texture extents, texture coordinates, the tree's structure and depth - and the
 * same error codes, with the message in ptmi_last_error(NULL).  For importers and asset pipelines on machines without a GPU. */
int ptmi_validate_scene(const ptmi_config* config, const ptmi_scene* scene);

int ptmi_bvh_create(ptmi_triangle* triangulation, uint32_t triangulation_size, ptmi_node* bvh,
                    uint32_t* bvh_size, uint32_t* bvh_max_depth);

/* ptmi_bvh_create on device `device`: the same tree and the same reordering of `triangulation`, byte for byte, with the
 * same in/out contract and the same status codes and messages.  The caller's host arrays go in and come out; the call
 * uses a stream and workspace of its own, leaves the calling thread's current device as it found it and does not touch
 * any context.  PTMI_ERR_NO_DEVICE (arrays untouched) when `device` is not a HIP device: no CPU fallback, the caller
 * chooses; PTMI_ERR_HIP when a runtime call fails (arrays untouched).
 *
 * The device builds the tree level by level.  The host builder keeps per-axis state from node to node: at a node where an
 * axis is skipped (centroid extent < 1e-3) the axis keeps the bin scans of the node built before it in depth-first
 * order, and if the SAH then chooses that axis (possible only when every other candidate cost is >= INT_MAX - large
 * flat walls) the split is made from that stale state.  A level-synchronous build cannot reproduce it, so the call then
 * discards the device work and runs ptmi_bvh_create on the caller's unmodified arrays (PTMI_BVH_FALLBACK_STALE_AXIS).
 * Likewise for every condition the host builder turns into an error (a bin out of range, a split with an empty side,
 * a tree deeper than 8 * PTMI_BVH_MAX_DEPTH): the host builder runs and its status and message are returned
 * (PTMI_BVH_FALLBACK_HOST_ERROR), and for records whose boxes the device does not fold (a NaN w, a box marked empty:
 * PTMI_BVH_FALLBACK_RECORDS).  Nothing is written to the caller's arrays before the device build has succeeded.
 * `info` may be NULL. */
enum {
    PTMI_BVH_FALLBACK_NONE = 0,
    PTMI_BVH_FALLBACK_STALE_AXIS = 1,
    PTMI_BVH_FALLBACK_HOST_ERROR = 2,
    PTMI_BVH_FALLBACK_RECORDS = 3
};
typedef struct ptmi_bvh_build_info {
    uint32_t struct_size;     /* set by the library: sizeof(ptmi_bvh_build_info) */
    uint32_t built_on_device; /* 1: the device built the tree; 0: the host builder did (see fallback) */
    uint32_t fallback;        /* PTMI_BVH_FALLBACK_* */
    uint32_t levels;          /* level passes the device ran */
    double device_ms;         /* device work between the upload and the download (HIP events) */
    double total_ms;          /* the whole call, copies and the reordering of the triangles included */
    double upload_ms, download_ms, permute_ms; /* host -> device; device -> host; reordering the caller's triangles */
    uint64_t workspace_bytes; /* device memory the call allocated */
} ptmi_bvh_build_info;

int ptmi_bvh_create_device(int32_t device, ptmi_triangle* triangulation, uint32_t triangulation_size, ptmi_node* bvh,
                           uint32_t* bvh_size, uint32_t* bvh_max_depth, ptmi_bvh_build_info* info);

/* Host only, no device: the refit of ptmi_update_triangles on a tree in the reference's layout (for callers that keep
 * GlobalVars.bvh in step with the device, and the yardstick of the device refit).  A leaf's trianglesAABB is the union of the
 * `aabb` of its triangles in ascending index order (boxes marked empty are skipped), its centroidsAABB takes their centroids; an
 * inner node's boxes are its sons' merged, son1 first; a corner whose new value compares equal to the one the tree holds keeps the
 * bits it holds (a -0 / +0 tie stays as the builder decided it).  With unchanged triangles ptmi_bvh_create's tree comes out byte
 * for byte.
 * son1Id / son2Id, cutAxis and the leaf ranges are not written.  The tree is walked from bvh[0] with ptmi_initialize_memory's
 * structural checks (a child index out of range, a node reached twice, a leaf range out of bounds): PTMI_ERR_BAD_SCENE, tree
 * untouched. */
int ptmi_bvh_refit(const ptmi_triangle* triangulation, uint32_t triangulation_size, ptmi_node* bvh, uint32_t bvh_size);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
