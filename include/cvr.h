/*
 * cvr.h - C ABI of the MI355X volumetric path tracer (libcvr.so).
 *
 * This is the drop-in boundary for the reference's kernel-launcher layer
 * (Fe0437/CudaVolumeRenderer, implementation/src/RenderKernelLauncher.h:20-174)
 * and for the CudaVolPath driver above it (CudaVolPath.{h,cpp}).  Plain C
 * types only: pointers, sizes, status codes.  Every call returns 0 (CVR_OK) or
 * a negative CVR_ERR_* and never exits the process (the reference's
 * CHECK_CUDA_ERROR calls exit(), Debug.h:19-37); the message is available from
 * cvr_last_error().
 *
 * Unlike the reference, launch parameters live in a per-context struct passed
 * by value to the kernels (the reference keeps them in module-global
 * __constant__ symbols, RenderKernelLauncher.cu:67-72), so one process can
 * hold one context per GPU.
 */
#ifndef CVR_H_
#define CVR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history: 3: cvr_render_frame takes the host buffer size; 4: cvr_stats.words;
 *              5: CVR_OPT_MEDIUM_FORMAT, cvr_half_round, cvr_medium_info;
 *              6: CVR_OPT_MOMENTS, cvr_copy_moments, cvr_block_error, cvr_adaptive_*
 *              6 + CVR_HAS_DENOISE (no new number, an addition within 6): cvr_denoise_desc, cvr_denoise*
 *              6 + CVR_HAS_DEVICE_MEDIUM (likewise): cvr_device_medium_desc, cvr_set_medium_device,
 *                  cvr_medium_layout
 *              6 + CVR_HAS_TRANSFER (likewise): cvr_transfer_desc, cvr_scalar_medium_desc,
 *                  cvr_classify_host, cvr_raw_transfer_table, cvr_set_medium_scalar,
 *                  cvr_set_medium_scene_transfer
 *              6 + CVR_HAS_GRADIENT_TRANSFER (likewise): cvr_gradient_transfer_desc,
 *                  cvr_gradient_medium_desc, cvr_classify_gradient_host, cvr_set_medium_gradient,
 *                  cvr_set_medium_scene_gradient
 *              6 + CVR_HAS_ENVMAP (likewise): cvr_environment_desc, cvr_set_environment,
 *                  cvr_clear_environment, cvr_environment_info, cvr_environment_eval*, cvr_trace_env,
 *                  cvr_read_image, cvr_free_image
 *              6 + CVR_HAS_MEDIUM_READBACK (likewise): cvr_debug_copy_medium, cvr_debug_build_geometry
 *              6 + CVR_HAS_FEATURES (likewise): cvr_features_desc, cvr_features_host, cvr_features_buffers,
 *                  cvr_features, cvr_denoise_guided_desc, cvr_denoise_guided_host, cvr_denoise_guided_buffers,
 *                  cvr_denoise_guided
 *              6 + CVR_HAS_FIELD_HISTOGRAM (likewise): cvr_field_desc, cvr_field_stats, cvr_histogram_desc,
 *                  cvr_field_stats_host, cvr_field_histogram_host, cvr_field_stats, cvr_field_histogram,
 *                  cvr_field_histogram_buffers, cvr_debug_field_geometry
 *              6 + CVR_HAS_CLIP (likewise): cvr_clip_desc, cvr_set_clip, cvr_clear_clip, cvr_get_clip,
 *                  cvr_clip_host, cvr_medium_clip_info
 *              6 + CVR_HAS_LABELS (likewise): cvr_label_transfer_desc, cvr_labeled_medium_desc,
 *                  cvr_classify_labels_host, cvr_set_medium_labeled, cvr_medium_label_info,
 *                  cvr_set_medium_scene_labels
 *              6 + CVR_HAS_PREVIEW (likewise): cvr_preview_desc, cvr_preview_host, cvr_preview_buffers,
 *                  cvr_preview
 *              6 + CVR_HAS_SHADOWS (likewise): cvr_light_volume_desc, cvr_light_volume_info,
 *                  cvr_light_volume_host, cvr_build_light_volume, cvr_light_volume_default_res,
 *                  cvr_copy_light_volume, cvr_clear_light_volume, cvr_preview_shadowed_host, cvr_preview_shadowed_buffers,
 *                  cvr_preview_shadowed
 *              6 + CVR_HAS_FIELD_PROJECT (likewise): cvr_project_desc, cvr_field_project_host,
 *                  cvr_field_project_buffers, cvr_field_project
 *              6 + CVR_HAS_WPOOL_DEBUG (likewise): cvr_debug_wpool_rows, cvr_debug_last_wpool
 * CVR_ABI_VERSION is the ABI this header declares: 6, the library's (cvr_abi_version()).  ABI 6 only
 * adds to ABI 5, so a host that must also load an ABI 5 library can hold itself to that surface:
 * with CVR_ABI_TARGET defined as 5 before the include, the ABI 6 functions and structs are not
 * declared (a use of one then fails to compile) and CVR_ABI_VERSION is 5. */
#if defined(CVR_ABI_TARGET) && CVR_ABI_TARGET == 5
#define CVR_ABI_VERSION 5
#elif defined(CVR_ABI_TARGET) && CVR_ABI_TARGET != 6
#error "CVR_ABI_TARGET must be 5 or 6"
#else
#define CVR_ABI_VERSION 6
#endif

enum {
  CVR_OK = 0,
  CVR_ERR_INVALID = -1,     /* bad argument */
  CVR_ERR_HIP = -2,         /* HIP runtime failure */
  CVR_ERR_STATE = -3,       /* call out of lifecycle order */
  CVR_ERR_IO = -4,          /* file / parse error */
  CVR_ERR_UNSUPPORTED = -5, /* kernel or feature not available */
  CVR_ERR_NOMEM = -6
};

/* Config::Kernel order and names (Config.h:87-95, :210-213). */
typedef enum {
  CVR_KERNEL_NAIVE_SK = 0,
  CVR_KERNEL_NAIVE_MK = 1,
  CVR_KERNEL_REGENERATION_SK = 2,
  CVR_KERNEL_STREAMING_MK = 3,
  CVR_KERNEL_STREAMING_SK = 4,
  CVR_KERNEL_SORTING_SK = 5,
  CVR_KERNEL_UNKNOWN = 6
} cvr_kernel;

/* Scene type names of the --scene-type flag (ConfigParser.cpp:16-18). */
typedef enum {
  CVR_SCENE_AUTO = 0,
  CVR_SCENE_MITSUBA_XML = 1,
  CVR_SCENE_VDB = 2,
  CVR_SCENE_RAW = 3,
  CVR_SCENE_MHD = 4,
  CVR_SCENE_VDB_SPARSE = 5 /* extension: read a VDB straight into 8^3 leaves (cvr_scene_sparse_medium);
                              Vdb/Auto do so by themselves above 2^30 voxels */
} cvr_scene_type;

/* Options for cvr_set_option. */
typedef enum {
  CVR_OPT_MAX_SEGMENTS = 1,   /* safety cap on segments per path (default 1<<20, 0 = none) */
  CVR_OPT_CHUNK = 2,          /* paths per wave dequeue (persistent schedulers); 0 (default): 256, the
                                 wave pool 64..256 by the paths each of its waves gets */
  CVR_OPT_EVENT_THRESHOLD = 3,/* lanes per wave that must wait before events run */
  CVR_OPT_GRID = 4,           /* persistent grid size in blocks (0 = occupancy); for the wave-pool scheduler in
                                 waves, rounded down to whole workgroups (four waves on sparse media) */
  CVR_OPT_SCATTER_EPS = 5,    /* -1 kernel default, 0 off, 1 on */
  CVR_OPT_SCHEDULER = 6,      /* how paths map onto threads: 0 single persistent kernel, 1 wavefront
                                 pair (streamingMK's multi-kernel structure), 2 workgroup path pool
                                 in LDS (streamingSK's block streaming), 3 wave-private path pool in
                                 LDS (the default for every kernel id; round 4 and before: naiveSK 4,
                                 streamingSK 2, streamingMK 1, naiveMK its own per-item kernel), 4 one
                                 path per work-item (naiveSK's structure; naiveMK: k_naive_mk).
                                 naiveMK runs the wave pool with 3 and k_naive_mk with any other
                                 value (its per-bounce kernels with CVR_OPT_MK_COMPACTION 1).  Scheduling only: results depend on the
                                 kernel id, not on the scheduler. */
  CVR_OPT_POOL = 7,           /* wavefront ray-slot pool size (default 2^21) */
  CVR_OPT_TIMING = 8,         /* 1: time every wavefront kernel (track_ms / events_ms) */
  CVR_OPT_CELLS = 9           /* 1 (default): corner-replicated density cells (8x density bytes
                                 in HBM, 2 x 16 B loads per Woodcock step); applies at set_medium */,
  CVR_OPT_WAVES = 10,         /* register/LDS budget in waves per SIMD: persistent kernel 4 (default), 5, 6,
                                 8; wave-pool kernel 3, 4, 5, 6 (default: 5; 6 is dense only
                                 and spills) */
  CVR_OPT_ORDER = 11,         /* 2 (default): 8x8-pixel blocks, samples innermost, each XCD band's blocks in
                                 2-D Morton order; 1: the same blocks row-major; 0: path-id order */
  CVR_OPT_QUEUES = 12,        /* work bands / queues, one per XCD (default 8) */
  CVR_OPT_BOUNDS = 13,        /* brick bounds: log2 brick size 1..5, 0 = off (default 2 dense,
                                 3 sparse; sparse caps at 3); next cvr_set_medium.  Results are
                                 identical either way. */
  CVR_OPT_TAIL = 14,          /* pool scheduler: lanes below which a wave ends a track phase (16) */
  CVR_OPT_BATCH = 15,         /* wave-pool scheduler: idle lanes that trigger a refill (8) */
  CVR_OPT_RNG_BINDING = 16,   /* regenerationSK: 0 (default) RNG bound to the path id (Q2 fixed:
                                 deterministic, scheduler-independent); 1 the reference's binding,
                                 Rng(seed + tid) per persistent thread, roulette draw after an
                                 escape, isect kept across a thread's paths
                                 (RegenerationVolPTsk_kernel.cuh:146-232).  streamingSK / sortingSK:
                                 1 runs the reference's block scheduler, 256-thread blocks with
                                 Rng(seed + gtid) per thread, one segment per iteration and a
                                 stable Morton-sort compaction that moves paths between threads
                                 (StreamingVolPTsk_kernel.cuh:328-349, SortingVolPTsk_kernel.cuh
                                 :306-330, its deferred albedo included).  streamingMK: 1 runs the
                                 reference's regenerate / extend kernel pair per iteration of a host
                                 loop, a new path's Rng(seed + path_id) becoming its thread's state
                                 and the states staying with the threads when compaction moves the
                                 paths (StreamingVolPTmk_kernel.cuh:26-253).  Thread-bound results
                                 depend on which thread takes which path: deterministic only for a
                                 one-wave (regenerationSK) or one-block (streaming/sorting/
                                 streamingMK) launch, CVR_OPT_GRID 1.  Reproduced quirk Q23
                                 (streamingSK / sortingSK): the sort key of an inactive thread is
                                 morton3D(1,1,1) = 2^30 - 1 (MortonSort.h:39-43), which an active
                                 path whose origin lies within 1/1024 of box_max on all three axes
                                 also gets; the stable tie-break on the thread index can then place
                                 that path past n_active, where the next regeneration overwrites it
                                 (dropped without a splat, not counted as truncated), as in the
                                 reference's cub sort.  streamingMK with 1 blocks the host until the
                                 render ends (one stream sync per iteration, as the reference's host
                                 loop). */
  CVR_OPT_MORTON = 17,         /* workgroup pool scheduler (CVR_OPT_SCHEDULER 2): 1 sorts each track phase's paths by the
                                 Morton code of their origin in the box (MortonSort.h:28-49,
                                 StreamingVolPTsk_kernel.cuh:188-216); default 0 (measured slower
                                 here).  Scheduling only: results are unchanged. */
  CVR_OPT_WORLD_TO_AABB = 18,  /* quirk Q4: 0 (default) the reference's worldToAABB, p - min/extent
                                 (operator precedence, Utilities.cuh:129-132); 1 the intended
                                 (p - min)/extent, computed as (p - box_min) * ((res - 1)/extent) (the
                                 grid scale folded in: shift = box_min, gx = (res - 1)/extent).  The two
                                 agree for the unit box of VDB/Raw/MHD scenes. */
  CVR_OPT_SUBQUEUES = 20,      /* wave-pool scheduler: work queues per XCD band (1..8, default 8), each
                                 over a contiguous part of the band, so that small dequeue chunks do not
                                 contend on one head.  Scheduling only. */
  CVR_OPT_INFLIGHT = 23,       /* wave-pool scheduler: renders the caller keeps in flight on this device
                                 (default 1).  Sets the grid of small launches (CVR_OPT_GRID 0): below 64
                                 paths per wave of the occupancy grid half of it (a quarter with renders
                                 in flight), below 1024 paths per wave half of it with renders in flight,
                                 else all of it.  Scheduling only. */
  CVR_OPT_UNIFORM_ALBEDO = 25, /* dense media: 1 (default) a grid whose voxels all hold the same rgb is
                                 read as that constant (the 8 taps interpolated with the same
                                 operations, no loads: the same result); 0 always load.  Takes
                                 effect at the next cvr_set_medium. */
  CVR_OPT_FRAME_FLUSH = 24,    /* cvr_render_frame, one part, wave-pool scheduler, pinned or registered
                                 host image: 1 (default) the launch itself stores each 8x8 block's
                                 normalised pixels into the host image once all its paths have
                                 ended (cvr_frame_flush_info); 0 normalise + copy after the launch.
                                 Same image either way (C2: 5.14 vs 5.29 ms per call).  2 (tests):
                                 the flushers give up at once, so the call takes its fallback copy. */
  CVR_OPT_SAMPLE_ORDER = 27,   /* wave-pool scheduler, pixel-block work order: 0 within an 8x8 block the
                                 units run sample by sample, the 64 pixels innermost; 1 pixel by pixel
                                 with the samples innermost, and each event batch sums its escapes per
                                 pixel before the framebuffer atomics (C3: 2.23 -> 0.99 GB written per
                                 launch; a launch with cvr_render_frame's in-launch output keeps
                                 order 0 and per-lane atomics).  -1 (default) = 0: order 1 costs C2 / C3 2.7% / 3.6%
                                 and C5 2.2% (with the empty-region mask).
                                 Scheduling and summation order only. */
  CVR_OPT_WAVE_PAIR = 26,      /* retired experiment; 0 accepted, 1 refused */
  CVR_OPT_EMPTY_MASK = 28,     /* wave-pool scheduler, sparse media: 1 (default) each workgroup (four
                                 wave-private pools) stages the medium's empty-region mask (one bit per
                                 super-brick of whole leaves, 256 bytes) in LDS once for its waves, which
                                 load the brick word of a Woodcock point only when its super-brick holds
                                 density; 0 loads every point's word.  The words it skips are known
                                 (0): results are unchanged. */
  CVR_OPT_COUNT_WORDS = 29,    /* wave-pool scheduler, sparse media, 5 waves per SIMD: 1 runs the counting
                                 instance, which also counts the brick words its Woodcock points load
                                 into cvr_stats.words (the benchmark's exact algorithmic bytes; one
                                 more VGPR in the track loop, so not the benchmarked kernel); 0
                                 (default) counts nothing.  Results are unchanged. */
  CVR_OPT_MEDIUM_FORMAT = 30,  /* storage precision of the voxel values in HBM, taken at the next cvr_set_medium /
                                 cvr_set_medium_sparse (as CVR_OPT_CELLS): 0 (default, CVR_FORMAT_F32) fp32;
                                 1 (CVR_FORMAT_F16) IEEE binary16: half the bytes of the density, the density
                                 cells and the albedo (cvr_medium_info).  Other values: CVR_ERR_INVALID.
                                 Format 1 contract:
                                 - every density voxel and the r, g, b of every albedo voxel (and the sparse
                                   albedo_background) is rounded to binary16, round to nearest even, before
                                   anything is built from it; fp16 subnormals are kept, not flushed;
                                 - the majorant used is max_density_eff = max(max_density,
                                   f32(f16(max_density))) (max_density itself if that rounds to inf): rounding
                                   is monotonic, so a valid majorant stays valid;
                                 - a half converts to fp32 exactly and all arithmetic after the load is fp32,
                                   so the render is bit-identical per path to a format-0 render of the rounded
                                   medium (cvr_half_round) with max_density_eff: the same image id, flags, T
                                   bits, segment count and counters; pixels equal up to fp32 summation order;
                                 - a finite value that rounds to +-inf (|v| >= 65520) fails the set-medium call
                                   with CVR_ERR_INVALID, the message names the first one, and the context is
                                   left without a medium; NaN, inf and negative values pass through rounded,
                                   as format 0 passes them;
                                 - the fp32 arrays are staged on the device, converted there and the staging
                                   freed before the call returns: the resident medium is halved, the peak
                                   during the upload is not (fp32 staging + the half grid).
                                 Runs on the wave-pool scheduler at 5 waves per SIMD (every kernel id,
                                 cvr_render_frame's in-launch output, cvr_trace_launch, CVR_OPT_CELLS 0 too) and
                                 in cvr_trace_paths; with another CVR_OPT_SCHEDULER or CVR_OPT_WAVES value,
                                 CVR_OPT_RNG_BINDING 1, CVR_OPT_COUNT_WORDS 1 or CVR_OPT_MK_COMPACTION 1 a
                                 launch on a format-1 medium returns CVR_ERR_UNSUPPORTED. */
  CVR_OPT_MOMENTS = 31,        /* wave-pool scheduler: 0 (default) off; 1 every launch also accumulates per-pixel
                                 second moments.  The context's own framebuffer allocation then holds a
                                 second float4 per pixel directly behind the tile (tile_w * tile_h float4
                                 after cvr_output_ptr): (sum fl(T.r T.r), sum fl(T.g T.g), sum fl(T.b T.b),
                                 the escapes splatted into the pixel: an fp32 count, exact below 2^24),
                                 read with cvr_copy_moments and cleared with the tile by cvr_clear_output.
                                 Turning it on may reallocate the framebuffer (both halves then start
                                 cleared).  Other values: CVR_ERR_INVALID.  The framebuffer half, the
                                 counters and every path are those of the same launch with the option off
                                 (pixels up to fp32 summation order).  Runs on the wave-pool scheduler at 5
                                 waves per SIMD with its generic dense instance (cells, bounds, uniform
                                 albedo and the half format read at run time) or the fp32 sparse one.  A
                                 caller's output buffer (cvr_set_output) with moments on is
                                 CVR_ERR_UNSUPPORTED, and so is a launch with another CVR_OPT_SCHEDULER or
                                 CVR_OPT_WAVES value, CVR_OPT_RNG_BINDING 1, CVR_OPT_COUNT_WORDS 1,
                                 CVR_OPT_MK_COMPACTION 1, kernel id naiveMK, a sparse half medium,
                                 cvr_trace_launch, cvr_render_frame, cvr_render_image, cvr_render_tiles or
                                 cvr_render_share_to_host. */
  /* 21: unused (a drain-time path migration between waves, measured slower: DESIGN.md §6) */
  CVR_OPT_DRAIN = 22,          /* wave-pool scheduler, once the queues are empty: an event batch runs as
                                 soon as the waiting segments x d >= the tracking ones (d = 0: only when
                                 no lane tracks, or 64 events wait).  -1 (default) = 1.  Scheduling only. */
  CVR_OPT_MK_COMPACTION = 19   /* quirk Q11, naiveMK only: 0 (default) every live path is extended
                                 until it ends; 1 the reference's compaction count end - begin - 1
                                 (RenderKernelLauncher.cu:266-271): after every bounce the live path
                                 with the highest pixel id is dropped, and a bounce that leaves no live
                                 path (the count underflows to 2^32 - 1 in the reference) fails the
                                 launch with CVR_ERR_STATE.  Runs the reference's per-bounce kernel
                                 sequence (one launch and host sync per bounce). */
} cvr_option;
enum { CVR_FORMAT_F32 = 0, CVR_FORMAT_F16 = 1 }; /* CVR_OPT_MEDIUM_FORMAT */

/* HeterogeneousMedium + GGX boundary (Medium.h:110-190, Bsdf.h:17-30). */
typedef struct cvr_medium_desc {
  uint32_t res[3];        /* grid resolution x, y, z */
  const float* density;   /* host, res[0]*res[1]*res[2] fp32, x fastest */
  const float* albedo;    /* host, same grid, 4 floats per voxel (r,g,b,1) */
  float box_min[3];       /* AABB (density_AABB) */
  float box_max[3];
  float scale;            /* density scale (VDB 100, Raw 40) */
  float max_density;      /* majorant / scale */
  float g;                /* HG asymmetry; the reference never uploads it (Q7): 0.  A negative g scatters
                             as |g|: ImportanceSampleHG divides by 2|g| (HG.h:51, Q24) */
  float roughness[2];     /* GGX alpha (0.1, 0.1) */
  float eta;              /* int_ior / ext_ior (1.05f / 1.01f) */
} cvr_medium_desc;

/* Sparse medium (extension): the grid of cvr_medium_desc
 * stored as 8^3-voxel leaves (the OpenVDB leaf size).  Voxel (x,y,z) is
 * leaf_density[slot*512 + ((z&7)*8 + (y&7))*8 + (x&7)] with
 * slot = leaf_table[((z>>3)*leaf_dims[1] + (y>>3))*leaf_dims[0] + (x>>3)];
 * a slot of CVR_NO_LEAF means density 0 and albedo albedo_background for
 * all 512 voxels.  Rendering is identical to cvr_set_medium on the densified
 * grid: only the storage differs.  Replaces the reference's dense textures
 * (CudaVolPath.cpp:117-186) where they do not fit (a 2048x1024x2048 cloud is
 * 17 GB of fp32 density + 69 GB of float4 albedo dense). */
#define CVR_NO_LEAF 0xFFFFFFFFu
typedef struct cvr_sparse_medium_desc {
  uint32_t res[3];             /* index-space grid resolution (as cvr_medium_desc.res) */
  uint32_t leaf_dims[3];       /* ceil(res / 8) */
  const uint32_t* leaf_table;  /* host, leaf_dims product entries, x fastest: slot or CVR_NO_LEAF */
  uint32_t n_leaves;           /* slots in the pools */
  const float* leaf_density;   /* host, n_leaves * 512 fp32 */
  const float* leaf_albedo;    /* host, n_leaves * 512 * 4 fp32 (r,g,b,1), or NULL: albedo_background everywhere */
  float albedo_background[4];  /* albedo outside the leaves */
  float box_min[3];
  float box_max[3];
  float scale;
  float max_density;
  float g;
  float roughness[2];
  float eta;
} cvr_sparse_medium_desc;

typedef struct cvr_stats {
  uint64_t paths;      /* paths started */
  uint64_t segments;   /* loop iterations (RAYS_STATISTICS count) */
  uint64_t steps;      /* Woodcock steps drawn */
  uint64_t density;    /* density evaluations (8 fp32 taps each) */
  uint64_t albedo;     /* albedo evaluations (8 float4 taps each) */
  uint64_t escaped;    /* paths that splatted into the framebuffer */
  uint64_t truncated;  /* paths cut by CVR_OPT_MAX_SEGMENTS */
  double kernel_ms;    /* device time of the last launch (HIP events) */
  uint64_t iterations; /* wavefront: events/track kernel pairs of the last launch */
  double track_ms;     /* wavefront: summed device time of the tracking kernels (CVR_OPT_TIMING) */
  double events_ms;    /* wavefront: summed device time of the event kernels (CVR_OPT_TIMING) */
  uint64_t fetches;    /* density evaluations that read their density (a 32-byte cell, or the 8-tap
                          gather off the cell grid or with CVR_OPT_CELLS 0): exactly those whose brick
                          bound does not settle the test, !(bound_value(code) < test draw), where a point
                          with 0 <= c < res on every axis of its grid coordinate reads its brick's code
                          and any other point reads 255 (no bound); bounds off: equal to `density`.
                          Independent of scheduler, kernel instance and the empty-region mask. */
  uint64_t words;      /* sparse media: brick words loaded; counted only by launches with
                          CVR_OPT_COUNT_WORDS 1, else 0.  A word is loaded for each of the two tentative
                          points of a lookahead pair that lies on the cell grid in a super-brick whose
                          mask bit is set (mask off or bounds off: on the cell grid), dropped points
                          included.  So W_lo <= words <= W_lo + 2 S + fetches, W_lo the evaluated points
                          of that kind and S the segments that ran Woodcock tracking (each ends past
                          max_t at most once, dropping at most two points; each fetch drops at most one). */
} cvr_stats;

/* The medium a context renders: device bytes by part.  The function cvr_medium_info fills it, so
 * the type has no typedef: write `struct cvr_medium_info`. */
struct cvr_medium_info {
  int32_t format;          /* CVR_FORMAT_F32 / CVR_FORMAT_F16 */
  float max_density_eff;   /* the majorant in use (format 0: max_density as given) */
  uint64_t density_bytes;  /* density grid, or the leaf density pool */
  uint64_t cells_bytes;    /* density cells, or the cell-leaf pool (0 with CVR_OPT_CELLS 0) */
  uint64_t albedo_bytes;   /* albedo grid, or the leaf albedo pool (0: background only) */
  uint64_t bounds_bytes;   /* brick bounds; sparse: brick words + leaf table + empty-region mask */
  uint64_t total_bytes;    /* the four above */
};

typedef struct cvr_path_record {
  uint32_t image_id;
  uint32_t flags; /* bit0 escaped, bit1 truncated */
  float T[3];
  uint32_t n_segments, n_steps, n_density, n_albedo;
} cvr_path_record;

typedef struct cvr_ctx cvr_ctx;
typedef struct cvr_scene cvr_scene;

/* ---- lifecycle (RenderKernelLauncher.h:20-52) ------------------------- */
int cvr_create(int device, int kernel, cvr_ctx** out);
int cvr_destroy(cvr_ctx* ctx);
const char* cvr_last_error(const cvr_ctx* ctx); /* ctx may be NULL */
int cvr_abi_version(void);

/* setScene + createTextureWithVolume (CudaVolPath.cpp:88-186): copies the
 * host volumes into HBM (the caller keeps ownership of the host arrays).
 * Limits (the kernels index with 24-bit multiplies and 32-bit sums), judged from res alone before
 * the arrays are looked at, the context keeping its previous medium:
 *  - an empty grid, or more than 2^32 - 1 voxels: CVR_ERR_INVALID;
 *  - res[0] * res[1] >= 2^24 or res[1] * res[2] >= 2^24: CVR_ERR_UNSUPPORTED (use the sparse upload);
 *  - 2^31 voxels or more in CVR_FORMAT_F32 with CVR_OPT_CELLS 1: CVR_ERR_UNSUPPORTED (use
 *    CVR_OPT_MEDIUM_FORMAT 1, CVR_OPT_CELLS 0 or the sparse upload). */
int cvr_set_medium(cvr_ctx* ctx, const cvr_medium_desc* medium);
/* Sparse upload: leaf pools go to HBM as they are; the density cells and
 * brick bounds are built on the device for the leaves whose cells can
 * interpolate a non-zero density (a brick-pool instead of dense cells).
 * Limits, with B the brick size in cells (8; CVR_OPT_BOUNDS 1 or 2: 2 or 4; CVR_OPT_BOUNDS 0: 4) and
 * bn = ceil(res / B) per axis:
 *  - an empty grid, leaf_dims != ceil(res / 8), more than 2^32 - 1 leaf table entries: CVR_ERR_INVALID;
 *  - bn[0] * bn[1] >= 2^24, bn[2] > 2^24 or 2^32 - 1 bricks or more: CVR_ERR_UNSUPPORTED, judged
 *    from res alone before anything is read (an axis may so have up to 2^27 cells; grid
 *    coordinates of 2^24 and above are whole numbers in fp32, in the reference too);
 *  - more than 2^24 cell leaves (the leaves that exist or have an existing forward neighbour,
 *    plus one): CVR_ERR_UNSUPPORTED, and an entry >= n_leaves: CVR_ERR_INVALID, both after the
 *    shape has passed, the arrays are non-NULL and the leaf table has been read.
 * In each of these cases the context keeps its previous medium. */
int cvr_set_medium_sparse(cvr_ctx* ctx, const cvr_sparse_medium_desc* medium);
/* Extension: `ctx` renders the medium of `src` (same device) without a copy:
 * its kernels read src's device buffers, which stay owned by src (destroy
 * `ctx` first, or give it a medium of its own, before `src` changes or frees
 * its medium).  For several contexts with renders in flight on one GPU. */
int cvr_share_medium(cvr_ctx* ctx, const cvr_ctx* src);
/* Format and device bytes of the context's medium, either format.  A context that
 * shares a medium (cvr_share_medium) reports the source's, and renders in that
 * format whatever its own CVR_OPT_MEDIUM_FORMAT says.  CVR_ERR_STATE: no medium. */
int cvr_medium_info(const cvr_ctx* ctx, struct cvr_medium_info* out);
/* Host only (no GPU): out[i] = f32(f16(in[i])), exactly the rounding of CVR_OPT_MEDIUM_FORMAT 1
 * (nearest even, subnormals kept, |v| >= 65520 -> +-inf, NaN stays NaN), so that a caller
 * can build the fp32 medium a format-1 render is bit-identical to.  in == out is allowed. */
int cvr_half_round(const float* in, float* out, size_t n);
/* copyInvViewMatrix (12 floats), copyRasterToView, copyPixelIndexRange */
int cvr_set_camera(cvr_ctx* ctx, const float inv_view[12], const float raster_to_view[2],
                   const float full_res[2]);
/* setResolution(tile_dim).  CVR_ERR_INVALID: a zero side, more than 2^24 pixels (the reference's
 * float pixel row, floor((float)id / w)), or tile_w * tile_h * iterations above 2^32 - 1 (the
 * reference's uint32 path ids; cvr_set_iterations checks the same product). */
int cvr_set_resolution(cvr_ctx* ctx, uint32_t tile_w, uint32_t tile_h);
/* The tile resolution the context renders now (set by cvr_set_resolution, or
 * by cvr_render_image / cvr_render_tiles to their tile size): the size of the
 * host image cvr_render_frame writes (tile_w * tile_h float4).  Extension. */
int cvr_get_resolution(const cvr_ctx* ctx, uint32_t* tile_w, uint32_t* tile_h);
/* copyOffset(tile origin) */
int cvr_set_offset(cvr_ctx* ctx, uint32_t x, uint32_t y);
/* setNIterations: n_paths = tile_w * tile_h * iterations */
int cvr_set_iterations(cvr_ctx* ctx, uint32_t iterations);
/* Extension for sharding: launch only path ids [first, first+count) of the
 * tile's n_paths (default: all; count UINT64_MAX: to the end).  The part of a range past
 * n_paths is clipped.  A range that ends past 2^32 - 1 (other than count UINT64_MAX) is a
 * mistake: the setter stores it and every launch returns CVR_ERR_INVALID; so does a launch
 * whose queue heads could pass 2^32 - 1 (a range in path-id order within a few chunks per
 * wave of 2^32).  More than 2^20 whole samples in one launch run in path-id order. */
int cvr_set_path_range(cvr_ctx* ctx, uint64_t first, uint64_t count);
/* Extension for multi-GPU strong scaling: restrict every launch to shard
 * `rank` of `world` of the tile's work.  Launches in the pixel-block work
 * order (whole samples of a tile whose sides are multiples of 8) take the
 * tile's 8x8 pixel blocks rank, rank + world, ... with all their samples, so
 * every shard sees the whole image and costs about the same; other launches
 * take a contiguous 1/world share of their path ids.  Either way the shards of
 * ranks 0..world-1 partition the launch's path ids, and the RNG stays bound
 * to the path id, so their summed images equal the unsharded render up to
 * fp32 summation order.  (0, 1) = no shard (default). */
int cvr_set_block_shard(cvr_ctx* ctx, uint32_t rank, uint32_t world);
/* Extension (scheduling only; results are bound to path ids): the order in
 * which the pixel-block work order hands out its blocks.  `perm` is a
 * permutation of [0, n) with n = the launch's block count (cvr_launch_blocks);
 * block b of the launch is taken as perm[b]'s turn.  Applies to launches with
 * that block count; NULL / n = 0 restores the natural order.  Used to start
 * costly blocks first (cvr_plan_block_order), so a launch does not end on
 * their long paths running on few lanes. */
int cvr_set_block_order(cvr_ctx* ctx, const uint32_t* perm, uint32_t n);
/* The pixel-block work order of the current launch configuration: its block
 * count (0 = not block ordered), its queues and their bands qbeg[0..n_queues]. */
int cvr_launch_blocks(const cvr_ctx* ctx, uint32_t* n_blocks, uint32_t* n_queues, uint32_t qbeg[9]);
/* RNG seed base (RegenerationVolPTsk_kernel.cuh:18 `seed`); path p uses
 * curand_init(seed + p). */
int cvr_set_seed(cvr_ctx* ctx, uint32_t seed);
int cvr_get_seed(const cvr_ctx* ctx, uint32_t* seed);
/* setOutputPtr: device float4 tile buffer; NULL selects a context-owned one. */
int cvr_set_output(cvr_ctx* ctx, void* device_tile_buffer);
void* cvr_output_ptr(cvr_ctx* ctx);
/* Run on a caller stream (hipStream_t), e.g. a framework's current stream;
 * NULL is the device's null stream.  cvr_own_stream() returns the
 * non-blocking stream the context creates for itself (the default).
 * Every call ordered "on the context's stream" is ordered on this stream, after
 * what the caller queued there before the call and before what it queues there
 * afterwards; the library touches no other stream for it.
 * Leaving a stream: the context's work queues, wave-pool scratch, filter images
 * and light volume are single-stream state, so a call that names a different
 * stream first waits (on the host) for the work pending on the stream it
 * leaves; naming the stream already in use waits for nothing.  The caller's
 * stream must stay valid until the context has left it (this call with another
 * stream has returned) or has been destroyed: cvr_destroy waits for it too.
 * CVR_ERR_STATE inside an adaptive session. */
int cvr_set_stream(cvr_ctx* ctx, void* hip_stream);
void* cvr_own_stream(cvr_ctx* ctx);
int cvr_set_option(cvr_ctx* ctx, int option, int64_t value);
/* init(): occupancy-based launch sizing (Occupancy.cuh:24-70). */
int cvr_init(cvr_ctx* ctx);
/* launchRender(): asynchronous on the context stream; accumulates into the
 * output buffer. */
int cvr_launch_render(cvr_ctx* ctx);
/* reset(): synchronise, rewind the work queue, advance the seed by n_paths
 * for regenerationSK (RenderKernelLauncher.cu:353-361). */
int cvr_reset(cvr_ctx* ctx);
int cvr_synchronize(cvr_ctx* ctx);
/* memset of the tile buffer (CudaVolPath.cpp:194-209). */
int cvr_clear_output(cvr_ctx* ctx);
/* Counters of the last launch (RAYS_STATISTICS analogue) + its device time. */
int cvr_get_stats(cvr_ctx* ctx, cvr_stats* stats);
/* D->H copy of the tile buffer, every component divided by `scale`. */
int cvr_copy_output(cvr_ctx* ctx, float* host_rgba, float scale);
#if CVR_ABI_VERSION >= 6
/* CVR_OPT_MOMENTS 1: D->H copy of the raw sums, unscaled: host_sum_rgba the tile buffer,
 * host_m2_rgba the moments (each tile_w * tile_h * 4 floats; either may be NULL).
 * Synchronous.  CVR_ERR_STATE with the option off. */
int cvr_copy_moments(cvr_ctx* ctx, float* host_sum_rgba, float* host_m2_rgba);
#endif
/* Extension, asynchronous on `stream` (a hipStream_t; NULL = the null
 * stream): host_dst[i] = device_src[i] / scale for n_floats floats, written by
 * a kernel straight into pinned (hipHostMalloc) or registered (hipHostRegister)
 * host memory: the transfer delegate's Scale + D->H copy
 * (ImageBufferTransfer.cu:61-78) in stream order, with no copy engine. */
int cvr_image_to_host(const float* device_src, float* host_dst, size_t n_floats, float scale, void* stream);
/* CudaVolPath::render for one tile (CudaVolPath.cpp:339-347, getImage
 * ImageBufferTransfer.cu:61-78): clear the framebuffer, render the context's
 * launch (resolution, iterations, camera, offset as set) and return once the
 * image, divided by the iteration count, is in `host_image` (width * height
 * float4; pinned memory makes the copy asynchronous).  parts 0 or 1: one
 * launch.  parts 2..3: the launch split into bands of 8-pixel block rows, the
 * largest first, each rendered with its own stream and work queues (helper
 * contexts that share this context's medium and framebuffer), so that a
 * band's normalise + copy runs while the later bands render; measured slower
 * on C2 (5.35 / 5.66 ms for 2 / 3 bands vs 5.37 for one launch: each band
 * adds ~0.15 ms of kernel span, more than its overlapped copy saves;
 * DESIGN.md §6).  Every path renders exactly as in one launch (the RNG is bound
 * to the path id).  Launches that cannot take bands (naive kernels, the
 * thread-bound RNG, sides that are not multiples of 8, partial path ranges,
 * block shards) render as one part.  Afterwards the seed has advanced as the
 * reference's reset() advances it (cvr_reset).  stats (may be NULL, which
 * saves a synchronous counter read per band): the summed counters;
 * kernel_ms = from the clear to the end of the last band.  With one part on
 * the wave-pool scheduler (5 waves per SIMD) and a pinned or registered host
 * image the copy happens inside the launch (CVR_OPT_FRAME_FLUSH, default on):
 * eight flusher waves store
 * each 8x8 block, normalised, as soon as all of its paths have ended, so the
 * image is complete when the kernel ends; if a flusher gives up (no block
 * finished for a second) the call copies the image the usual way instead.
 * host_floats: the floats host_image holds; fewer than tile_w * tile_h * 4
 * (cvr_get_resolution) is CVR_ERR_INVALID and nothing is rendered (ABI 3). */
int cvr_render_frame(cvr_ctx* ctx, float* host_image, size_t host_floats, uint32_t parts, cvr_stats* stats);
/* The last cvr_render_frame's in-launch output: blocks the flushers stored (0
 * if the call copied after the launch) and the number of calls so far that
 * fell back to the copy because a flusher gave up. */
int cvr_frame_flush_info(const cvr_ctx* ctx, uint32_t* blocks, uint32_t* fallbacks);
/* Extension (multi-GPU output): the pixels of block shard (rank, world) of a
 * width x height float4 image (cvr_set_block_shard: 8x8 blocks rank,
 * rank + world, ..., row-major; sides multiples of 8), divided by `scale`,
 * stored by a kernel on `stream` at their places in the full pinned or
 * registered host image `host_dst` (width * height * 4 floats).  The ranks'
 * block shards are pixel-disjoint, so every rank writing its own blocks into
 * one shared host image IS the reference's Scale + D->H copy
 * (ImageBufferTransfer.cu:61-78) of the whole render: no reduction. */
int cvr_blocks_to_host(const float* device_src, float* host_dst, uint32_t width, uint32_t height, uint32_t rank,
                       uint32_t world, float scale, void* stream);
/* Debug/parity: trace path ids [first, first+count) one per work-item and
 * return per-path records (no framebuffer splat). */
int cvr_trace_paths(cvr_ctx* ctx, uint32_t first, uint32_t count, cvr_path_record* host_out);
/* Debug: the production launch (cvr_launch_render on the wave-pool scheduler,
 * regenerationSK / sortingSK) writing every path's final record as it ends:
 * out[p - first] for the path ids p of the launch range [first, first + n_out)
 * (cvr_set_path_range; n_out must equal the range's length).  image_id, flags,
 * T and n_segments are filled (n_steps, n_density, n_albedo stay 0: the wave
 * pool counts those per lane); ids outside a block shard stay zero.
 * Synchronous.  The traced launch splats into a scratch buffer (the context's
 * output is untouched); cvr_get_stats afterwards reports its counters. */
int cvr_trace_launch(cvr_ctx* ctx, cvr_path_record* out, uint64_t n_out);
/* Diagnostic builds (-DCVR_STAMPS=1) only: per-phase cycle counters of the
 * persistent kernel {event cycles, track cycles, event phases, track
 * iterations}, summed over waves; zeros otherwise. */
int cvr_debug_counters(cvr_ctx* ctx, uint64_t out[16]);
/* Device properties used for sizing: CU count, persistent grid. */
int cvr_device_info(cvr_ctx* ctx, int* cu_count, int* persistent_grid);

/* ---- renderer (CudaVolPath::render, CudaVolPath.cpp:339-347) ---------- */
typedef struct cvr_render_desc {
  uint32_t resolution[2]; /* full image W, H */
  uint32_t n_tiles[2];    /* --number-of-tiles (TilingConfig, Config.h:61-78) */
  uint32_t iterations;    /* --iterations */
} cvr_render_desc;
/* Render all tiles: per tile set offset, launch, normalise by iterations
 * into the image, reset.  `device_image` (W*H float4, may be NULL) receives
 * the normalised image on the device, `host_image` (may be NULL) a copy.
 * Pixels outside tile_dim*n_tiles are not written (Q1).  stats->kernel_ms is
 * the sum of the tile launches' HIP-event times; one tile into host memory
 * only (no device_image) runs as cvr_render_frame, whose kernel_ms spans the
 * clear, the launch and its in-launch output. */
int cvr_render_image(cvr_ctx* ctx, const cvr_render_desc* desc, void* device_image, float* host_image,
                     cvr_stats* stats);
/* Tile-sharded variant (tile k -> GPU k): render only the
 * tiles k = first_tile, first_tile + tile_stride, ... of the same tile loop,
 * each with the seed it has in the full loop, so the per-rank images (zero
 * elsewhere when `device_image` starts zeroed) sum to cvr_render_image's.
 * The context's seed ends where the full loop leaves it.  Stats cover the
 * rendered tiles.  cvr_render_image == cvr_render_tiles(ctx, desc, 0, 1, ...). */
int cvr_render_tiles(cvr_ctx* ctx, const cvr_render_desc* desc, uint32_t first_tile, uint32_t tile_stride,
                     void* device_image, float* host_image, cvr_stats* stats);
/* Extension (multi-device renderer; the CLI's --devices): one
 * device's share of a render, stored normalised by a kernel straight into the
 * full pinned host image (cvr_host_alloc, or registered memory; width *
 * height * 4 floats, host_floats checked) at its places, nothing else written:
 *  - more than one tile (desc->n_tiles): tiles first_tile, first_tile +
 *    tile_stride, ... of the tile loop (tile k -> device k mod N,
 *    CudaVolPath.cpp:249-280), each with its sequential-loop seed;
 *  - one tile: the context's block shard (cvr_set_block_shard; sides multiples
 *    of 8; first_tile must be 0).
 * Disjoint shares from N contexts (one host thread each, any devices) leave
 * cvr_render_image's image in the one buffer, with no reduction.  Synchronous;
 * stats cover this share. */
int cvr_render_share_to_host(cvr_ctx* ctx, const cvr_render_desc* desc, uint32_t first_tile, uint32_t tile_stride,
                             float* host_image, size_t host_floats, cvr_stats* stats);
#if CVR_ABI_VERSION >= 6
/* ---- adaptive sampling (extension, ABI 6) ------------------------------- */
/* Host only (no GPU): the noise metric the adaptive render stops on, the written statement
 * of what the device computes (k_block_error).  For n_pixels pixels that have each received
 * n_samples samples, with sums S1 (sum_rgba, the framebuffer) and S2 (m2_rgba, the moments;
 * 4 floats per pixel each, the w components unused), per channel c, in fp64:
 *   m_c = S1_c / N, v_c = max(0, S2_c / N - m_c^2) / (N - 1),
 *   e_pixel = sqrt(v_r + v_g + v_b) / (m_r + m_g + m_b + floor),
 * the relative standard error of the pixel's mean, and *out = the mean of e_pixel over the
 * pixels (an 8x8 block: e_block).  A pixel with a NaN (or infinite) sum has e_pixel = +inf,
 * one whose denominator is 0 (black, floor 0) has 0.  n_samples < 2: CVR_ERR_INVALID. */
int cvr_block_error(const float* sum_rgba, const float* m2_rgba, uint32_t n_pixels, uint32_t n_samples, float floor,
                    double* out);
typedef struct cvr_adaptive_desc {
  uint32_t min_iterations;   /* samples every block gets before the first check (>= 2) */
  uint32_t max_iterations;   /* cap per block */
  uint32_t pass_iterations;  /* samples added per pass; min and max are multiples of it */
  float target;              /* a block stops once e_block <= target; negative: never */
  float floor;               /* the metric's floor (the CLI default is 0.01) */
} cvr_adaptive_desc;
typedef struct cvr_adaptive_result {
  uint32_t passes, blocks, blocks_active;  /* active = still sampling after this pass */
  uint64_t paths;                          /* paths traced so far */
  double max_error, mean_error;            /* over all blocks, each at its last check */
  int32_t done;                            /* 1: nothing active, or max reached */
} cvr_adaptive_result;
/* A noise-targeted render of the context's tile: every 8x8-pixel block is sampled until its
 * e_block (cvr_block_error) is at most desc->target or it has max_iterations samples.
 * cvr_adaptive_begin opens the session: CVR_OPT_MOMENTS on, both buffers cleared, every
 * block active with 0 samples.  It needs tile sides that are multiples of 8, one tile (the
 * context's resolution, offset and camera as set), no block shard and no path range, the
 * pixel-block work order (CVR_OPT_ORDER 1 or 2) and what CVR_OPT_MOMENTS needs
 * (CVR_ERR_UNSUPPORTED otherwise); a bad descriptor is CVR_ERR_INVALID.  The context's
 * iteration count is max_iterations until cvr_adaptive_end.
 * cvr_adaptive_pass: the first pass renders samples [0, min_iterations) of every block,
 * each later one pass_iterations more samples of the active blocks only, as one launch whose
 * block list is the active blocks (a cvr_set_block_order table is ignored meanwhile).  The
 * path ids are those of one launch of max_iterations, so every path is that launch's path,
 * wherever its block stops.  Then the active blocks' errors are computed on the device and
 * read back (one small copy per pass), and the blocks with e_block <= target, or with
 * max_iterations samples, leave the list.  result (may be NULL) is the state after the
 * pass.  A pass after done is CVR_ERR_STATE.
 * cvr_adaptive_maps: every block's error at its last check and its sample count, tile
 * blocks row-major (tile_w / 8 per row); either pointer may be NULL.  The last session's
 * maps stay readable after its cvr_adaptive_end.
 * cvr_adaptive_image: the image, every pixel divided by its own block's sample count
 * (host_floats >= tile_w * tile_h * 4), stored by a kernel straight into pinned or
 * registered host memory, through a staging copy otherwise.  Synchronous.
 * cvr_adaptive_end: restores CVR_OPT_MOMENTS, the iteration count and the block list, and
 * advances the seed exactly as one cvr_reset after a launch of max_iterations would.
 * Between begin and end every other render call, cvr_set_option and the setters of the
 * launch (medium, camera, resolution, offset, iterations, path range, block shard, seed,
 * output, stream, cvr_clear_output, cvr_reset) return CVR_ERR_STATE; cvr_get_stats (the last
 * pass's launch), cvr_synchronize, cvr_copy_moments, cvr_copy_output and cvr_denoise stay available. */
int cvr_adaptive_begin(cvr_ctx* ctx, const cvr_adaptive_desc* desc);
int cvr_adaptive_pass(cvr_ctx* ctx, cvr_adaptive_result* result);
int cvr_adaptive_maps(cvr_ctx* ctx, double* block_error, uint32_t* block_samples);
int cvr_adaptive_image(cvr_ctx* ctx, float* host_rgba, size_t host_floats);
int cvr_adaptive_end(cvr_ctx* ctx);
/* begin, passes until done, image, end.  result and stats may be NULL; stats are the
 * passes' summed counters, kernel_ms the sum of their launches' device times. */
int cvr_render_adaptive(cvr_ctx* ctx, const cvr_adaptive_desc* desc, float* host_rgba, size_t host_floats,
                        cvr_adaptive_result* result, cvr_stats* stats);

/* ---- variance-guided denoiser (extension within ABI 6: CVR_HAS_DENOISE) -- */
/* An edge-avoiding a-trous wavelet filter on colour alone, its edge-stopping term scaled by the
 * local standard deviation of the pixel mean, which the second moments give.  Every operation is
 * fp32 +, -, x, /, sqrt in the order written here, no fused multiply-add, so the device kernels
 * and cvr_denoise_host return the same bits (one definition compiles for both, cvr_kernels.h).
 * Per pixel N is n_samples, or with block_samples the entry of the pixel's 8x8 block (row-major,
 * w / 8 per row).  A pixel is valid if N >= 2 and the r, g, b of both of its sums are finite.
 * Prepare, per valid pixel and channel c:  m_c = S1_c / N, d_c = S2_c / N - m_c m_c,
 *   v_c = max(d_c, 0) / (N - 1);  l = (k_r m_r + k_g m_g) + k_b m_b,
 *   v = ((k_r k_r) v_r + (k_g k_g) v_g) + (k_b k_b) v_b, k = (0.2126f, 0.7152f, 0.0722f).
 *   It stores (m_r, m_g, m_b, v); an invalid pixel stores (0, 0, 0, -1): v < 0 marks it.
 * Pass k = 0 .. passes - 1, step s = 2^k, between two buffers; a tap counts only if it lies in
 * the image and is valid.  For a valid centre p, over the 3x3 taps q = p + (i, j), rows first,
 * G = (1/4, 1/2, 1/4):  w = G_j G_i, gs += w v(q), gw += w;  den = sigma sqrt(gs / gw) + floor.
 * Then over the 5x5 taps q = p + s (i, j), rows first, h = (1/16, 1/4, 3/8, 1/4, 1/16), l(.)
 * recomputed from the stored rgb:  a = |l(q) - l(p)| / den, u = 1 + a a, w = (h_j h_i) / (u u),
 *   cs_c += w c_c(q), vs += (w w) v(q), ws += w;  out = (cs_r / ws, cs_g / ws, cs_b / ws,
 *   vs / (ws ws)).  An invalid centre runs the 5x5 loop with w = h_j h_i (no edge term: it is
 * in-painted from its valid taps) and stays (0, 0, 0, -1) if ws == 0.
 * Output: out_rgba = (r, g, b, S1_w / N) (w: 0 where N < 2; rgb 0 where still invalid);
 * out_var = the filtered v, -1 where invalid.
 * passes 1..6, sigma >= 0 and finite, floor > 0 and finite, flags 0: else CVR_ERR_INVALID.
 * The defaults of the bindings and the CLI are 5, 4.0 and 0.01. */
#define CVR_HAS_DENOISE 1
typedef struct cvr_denoise_desc {
  uint32_t passes;
  float sigma;
  float floor;
  uint32_t flags;
} cvr_denoise_desc; /* 16 bytes */
/* Host only, no GPU: the written statement of the filter.  sum_rgba / m2_rgba: w * h * 4 floats
 * (the layout of cvr_copy_moments).  block_samples may be NULL (uniform n_samples >= 2); with a
 * map w and h are multiples of 8 and n_samples is ignored.  out_var (w * h floats) may be NULL.
 * More than 2^24 pixels: CVR_ERR_INVALID. */
int cvr_denoise_host(const float* sum_rgba, const float* m2_rgba, uint32_t w, uint32_t h, uint32_t n_samples,
                     const uint32_t* block_samples, const cvr_denoise_desc* desc, float* out_rgba, float* out_var);
/* The same on device buffers of any origin (e.g. torch tensors; the rgba ones 16-byte aligned),
 * asynchronous on the context's stream; the two scratch images are owned by the context (a
 * larger image than before synchronises the stream once to grow them).  d_out_rgba may be the
 * device address of pinned host memory.  The inputs are only read. */
int cvr_denoise_buffers(cvr_ctx* ctx, const float* d_sum_rgba, const float* d_m2_rgba, uint32_t w, uint32_t h,
                        uint32_t n_samples, const uint32_t* d_block_samples, const cvr_denoise_desc* desc,
                        float* d_out_rgba, float* d_out_var);
/* The context's own framebuffer and moments (CVR_OPT_MOMENTS 1, else CVR_ERR_STATE), filtered
 * into host_rgba (tile_w * tile_h * 4 floats; host_floats smaller: CVR_ERR_INVALID).  Synchronous.
 * Pinned or registered host memory is stored into by the kernel, other memory through a staging
 * copy (as cvr_adaptive_image).  Inside an adaptive session n_samples must be 0 and every block
 * has its own count (cvr_adaptive_maps); outside one n_samples >= 2 is the number of samples
 * accumulated since the last clear (else CVR_ERR_INVALID).  Reads the framebuffer and the
 * moments and never writes them.  Available between cvr_adaptive_begin and cvr_adaptive_end. */
int cvr_denoise(cvr_ctx* ctx, const cvr_denoise_desc* desc, uint32_t n_samples, float* host_rgba, size_t host_floats);

/* ---- media built from device memory (extension within ABI 6: CVR_HAS_DEVICE_MEDIUM) -- */
/* The dense grid of cvr_medium_desc, read from device memory (a torch tensor, a simulation's
 * output): no array of the medium crosses to the host, only scalars do (counts, flags, the
 * majorant, the first overflowing index, voxel 0's albedo and the 256 bytes of the mask).
 * The call leaves the context in the state the host call leaves it in on host copies of the same
 * arrays: the same cvr_medium_info and cvr_medium_layout, the same paths bit for bit.
 *  - without CVR_DEVMED_SPARSE the host call is cvr_set_medium;
 *  - with it, cvr_set_medium_sparse on the leaves of this rule (the one cvr_scene_sparse_medium
 *    applies): leaves in z, y, x order, x fastest, slots numbered in that order; a leaf exists
 *    iff one of its in-grid voxels has density != 0.0f (-0 makes none, NaN makes one) or 16
 *    albedo bytes that differ from voxel (0,0,0)'s, which are the background; out-of-grid voxels
 *    of a stored leaf hold density 0 and the background; the leaf albedo pool is dropped when no
 *    in-grid voxel differs from the background;
 *  - CVR_DEVMED_CONST_ALBEDO is the host call on a grid filled with const_albedo (dense: the
 *    context's albedo grid is filled on the device; sparse: the constant is the background, no
 *    leaf albedo, leaves exist by density alone);
 *  - CVR_DEVMED_MAX_DENSITY takes max(0, every non-NaN voxel) for max_density.
 * Refusals: the shape guards of the host call, in its order, with its codes and texts, from res
 * alone and before any pointer is looked at (the previous medium is kept); unknown flags, a NULL
 * pointer (d_albedo: NULL without CVR_DEVMED_CONST_ALBEDO, non-NULL with it) or one that
 * hipPointerGetAttributes does not report as device-accessible memory of the context's device:
 * CVR_ERR_INVALID (previous medium kept); CVR_FORMAT_F16 overflow: the host call's code and
 * message (density before albedo, the smallest index; the context is left without a medium);
 * more than 2^24 cell leaves: CVR_ERR_UNSUPPORTED; inside an adaptive session: CVR_ERR_STATE.
 * Synchronous; reads the arrays on the context's stream, so the caller has made them ready
 * before the call.  The context copies what it keeps: the arrays are only read and may be freed
 * afterwards.  In CVR_FORMAT_F16 the halves are converted straight from the caller's fp32 arrays:
 * there is no fp32 staging buffer (the host calls allocate one of the albedo's fp32 size), so the
 * upload's peak device memory is the stored medium plus, for CVR_DEVMED_SPARSE, the build tables
 * (up to three words per leaf and three per cell leaf).
 * Not supported: aliasing the caller's arrays (the context always copies), partial updates. */
#define CVR_HAS_DEVICE_MEDIUM 1
enum { CVR_DEVMED_SPARSE = 1,        /* store as 8^3 leaves (the rule above) */
       CVR_DEVMED_CONST_ALBEDO = 2,  /* d_albedo is NULL: every voxel has const_albedo */
       CVR_DEVMED_MAX_DENSITY = 4 }; /* ignore max_density: use max(0, every non-NaN voxel), found on the device */
typedef struct cvr_device_medium_desc {
  uint32_t res[3];
  uint32_t flags;
  const float* d_density; /* device, res product fp32, x fastest, contiguous */
  const float* d_albedo;  /* device, 4 floats per voxel (16-byte aligned), or NULL with CONST_ALBEDO */
  float const_albedo[4];
  float box_min[3], box_max[3];
  float scale, max_density, g, roughness[2], eta;
} cvr_device_medium_desc; /* 96 bytes */
int cvr_set_medium_device(cvr_ctx* ctx, const cvr_device_medium_desc* medium);
/* Measurement only: with CVR_OPT_TIMING 1, the device milliseconds (HIP events) the last
 * cvr_set_medium_device, cvr_set_medium_scalar or cvr_set_medium_gradient spent in {density scan,
 * albedo scan, leaf flags, scans and scatters, copy / conversion / gather, cells + bounds + brick
 * words}; zeros otherwise.  Timing adds a host synchronisation per group. */
int cvr_debug_device_medium_ms(const cvr_ctx* ctx, double out_ms[6]);

/* What was built, by either upload path (a shared medium: the source's).  mask: the empty-region
 * mask words, all 0 when there is none (dense media, bounds off).  CVR_ERR_STATE: no medium. */
struct cvr_medium_layout {
  uint32_t sparse, albedo_uniform, n_leaves, n_cell_leaves, brick_shift, mask_shift;
  float albedo_bg[3];
  uint32_t mask[64];
};
int cvr_medium_layout(const cvr_ctx* ctx, struct cvr_medium_layout* out);

/* ---- read-back of the stored medium (tests; extension within ABI 6: CVR_HAS_MEDIUM_READBACK) -- */
/* Debug: one stored array of the medium in use (a shared medium: the source's), copied to the
 * host as stored: fp32 or binary16 values by the medium's format, u32 words, u8 bounds.
 * *needed always receives the array's size in bytes; an array the medium does not have (a dense
 * array of a sparse medium, no albedo pool, bounds off, no mask) gives *needed = 0 and CVR_OK
 * and copies nothing.  bytes < *needed (or a NULL host_dst): CVR_ERR_INVALID, nothing is
 * copied, so a first call with bytes 0 asks for the size.  No medium: CVR_ERR_STATE.
 * Synchronous (the device is synchronised first). */
#define CVR_HAS_MEDIUM_READBACK 1
enum { CVR_MEDIUM_DENSITY = 0,      /* dense: one value per voxel, x fastest */
       CVR_MEDIUM_ALBEDO = 1,       /* dense: four values per voxel */
       CVR_MEDIUM_CELLS = 2,        /* dense: 8 corner values per voxel (CVR_OPT_CELLS) */
       CVR_MEDIUM_BOUNDS = 3,       /* dense: one u8 code per brick and the no-bound entry behind them */
       CVR_MEDIUM_LEAF_TABLE = 4,   /* sparse: per leaf (z, y, x; x fastest) its slot or CVR_NO_LEAF */
       CVR_MEDIUM_LEAF_DENSITY = 5, /* sparse: 512 values per slot */
       CVR_MEDIUM_LEAF_ALBEDO = 6,  /* sparse: 512 x 4 values per slot */
       CVR_MEDIUM_CELL_SLOTS = 7,   /* sparse: per leaf its cell-leaf slot, 0 the zero leaf.  Kept in the low
                                       24 bits of the leaf's brick words: taken from the leaf's first brick */
       CVR_MEDIUM_SPARSE_CELLS = 8, /* sparse: 512 cells of 8 corner values per cell-leaf slot */
       CVR_MEDIUM_BRICK_WORDS = 9,  /* sparse: code << 24 | cell-leaf slot per brick and the no-bound word */
       CVR_MEDIUM_MASK = 10,        /* sparse, bounded: the empty-region mask's 64 words */
       CVR_MEDIUM_ARRAY_COUNT = 11 };
int cvr_debug_copy_medium(const cvr_ctx* ctx, int which, void* host_dst, size_t bytes, size_t* needed);
/* Debug, host only (no device is needed): the launch geometry of the medium build kernels, the
 * constants the launches themselves use, so that a test can size a medium that makes a capped
 * grid loop and fails when a cap moves.  out[0] the value scans' and classified passes' grid cap
 * (workgroups of 256); [1] the streaming kernels' grid cap (albedo fill, cell-leaf flags, leaf
 * gather); [2] flags per workgroup of the leaf scan (its tile); [3] tile sums the scan's middle
 * launch takes per trip; [4] the gradient passes' grid cap in tasks and [5] the z planes of a
 * task (a task: 256 x of one y); [6] the x run of a leaf-flag task in voxels and [7] in leaves,
 * [8] that launch's grid cap; [9] the binary16 conversion's grid cap; [10] the dense cells',
 * [11] dense bounds', [12] sparse cells' and [13] sparse brick words' fixed grids; [14] 0;
 * [15] the number of entries filled, 14. */
int cvr_debug_build_geometry(uint32_t out[16]);

/* ---- transfer functions: scalar volumes classified on the device (extension within ABI 6:
 *      CVR_HAS_TRANSFER) -- */
/* A scalar field (u8, u16, i16 or f32) and a table of n entries (r, g, b, density) give every
 * voxel a density and an albedo.  Every operation is fp32 +, -, x, /, floorf, ceilf and
 * comparisons in the order written here, no fused multiply-add, so the build kernels and
 * cvr_classify_host return the same bits (one definition compiles for both, cvr_kernels.h).
 * Per voxel:
 *   s = the voxel converted to float (exact for the integer types);
 *   t = (s - lo) / (hi - lo);
 *   u = t > 0 ? t : 0, then u = u < 1 ? u : 1 (a NaN scalar so gives 0);
 *   x = u * (float)(n - 1);
 *   with CVR_TF_CEIL:  i = min((uint)ceilf(x), n - 1), e = entry i;
 *   otherwise:         i = min((uint)floorf(x), n - 2), f = x - (float)i,
 *                      e_c = a_c + f * (b_c - a_c) per component c of r, g, b, density, a = entry i,
 *                      b = entry i + 1 (one subtract, one multiply, one add, in that order);
 *   albedo = (e_r, e_g, e_b, 1.0f);
 *   density = u with CVR_TF_DENSITY_U, else e's density.
 * The reference's Raw scenes (RawSceneBuilder.h:95-140) are cvr_raw_transfer_table() with
 * CVR_TF_CEIL | CVR_TF_DENSITY_U, lo 0 and hi the largest byte.
 * A descriptor is refused (CVR_ERR_INVALID) for n outside 2..4096, unknown flags, a NULL table,
 * lo or hi not finite, or hi <= lo. */
#define CVR_HAS_TRANSFER 1
enum { CVR_SCALAR_F32 = 0, CVR_SCALAR_U8 = 1, CVR_SCALAR_U16 = 2, CVR_SCALAR_I16 = 3 };
enum { CVR_TF_CEIL = 1,        /* entry ceil(x) instead of linear interpolation (the Raw scenes' rule) */
       CVR_TF_DENSITY_U = 2 }; /* density = u, the normalised scalar, not the table's w */
typedef struct cvr_transfer_desc {
  uint32_t n;         /* table entries, 2..4096 */
  uint32_t flags;
  const float* table; /* HOST, n * 4 floats: (r, g, b, density) */
  float lo, hi;       /* finite, hi > lo */
} cvr_transfer_desc; /* 24 bytes */
/* Host only, no GPU: the statement above over n_voxels voxels of `scalar` (host memory of type
 * scalar_type).  density (n_voxels floats) and albedo (4 * n_voxels floats) may each be NULL. */
int cvr_classify_host(const void* scalar, uint32_t scalar_type, size_t n_voxels, const cvr_transfer_desc* transfer,
                      float* density, float* albedo);
/* Host only: the reference's 100-entry Raw table, green -> red over 20 entries, then red -> blue
 * over 80, each with density 1 (Raw scenes take their density from u); the one table the Raw
 * loader classifies with. */
int cvr_raw_transfer_table(float out[400]);
/* The medium from a scalar field in device memory and a table: density and albedo are computed
 * per voxel inside the build kernels and written straight into the context's storage, fp32 or
 * binary16; no dense array of the classified medium exists outside the context.
 * The context ends in the state cvr_set_medium_device leaves on device copies of the arrays
 * cvr_classify_host makes of the same scalar field and table, with the same flags, box and
 * parameters, and so, through that call's contract, in the state the host uploads leave: equal
 * cvr_medium_info and cvr_medium_layout, the same paths bit for bit, in both medium formats, dense
 * and sparse.  Everything that call derives from values is derived from the classified values:
 * the majorant (CVR_DEVMED_MAX_DENSITY), the binary16 overflow refusal with its code and message
 * (density before albedo, the smallest index; the context is left without a medium), uniform-albedo
 * detection, the leaf rule with voxel (0,0,0)'s classified albedo as background, and dropping the
 * leaf albedo pool.
 * flags: CVR_DEVMED_SPARSE and / or CVR_DEVMED_MAX_DENSITY.  d_scalar: res product elements, x
 * fastest, aligned to its element size only.
 * Refusals, in this order: the host call's shape guards, from res alone and before any pointer is
 * looked at; unknown flags (CVR_DEVMED_CONST_ALBEDO is one here) or scalar_type; n outside
 * 2..4096; a NULL table or d_scalar; lo / hi not finite or hi <= lo; a d_scalar that is not
 * device-accessible memory of the context's device or is misaligned for its type.  All are
 * CVR_ERR_INVALID with the previous medium kept.  Inside an adaptive session: CVR_ERR_STATE.
 * Synchronous on the context's stream; the scalar field is only read (dense: at most twice, one
 * scan and one store; sparse: once for the leaf flags, a pass that also finds the scans' results,
 * and once in the gather; a binary16 overflow reads the stored leaves' voxels once more to name
 * its index) and may be freed afterwards;
 * the context does not keep it: changing the table means calling again with the same field.
 * cvr_debug_device_medium_ms reports this call's groups too (the one scan under "density scan",
 * the store under "copy / conversion / gather"). */
typedef struct cvr_scalar_medium_desc {
  uint32_t res[3];
  uint32_t flags;
  const void* d_scalar; /* device, res product elements of scalar_type, x fastest, contiguous */
  uint32_t scalar_type; /* CVR_SCALAR_* */
  uint32_t reserved;    /* 0 */
  cvr_transfer_desc transfer;
  float box_min[3], box_max[3];
  float scale, max_density, g, roughness[2], eta;
} cvr_scalar_medium_desc; /* 104 bytes */
int cvr_set_medium_scalar(cvr_ctx* ctx, const cvr_scalar_medium_desc* medium);
/* cvr_set_medium_scalar on a Raw scene's bytes (cvr_scene_raw_bytes, one byte per voxel): they
 * are uploaded to a temporary device buffer, classified as CVR_SCALAR_U8 with lo 0 and hi the
 * largest byte (transfer's lo and hi are ignored), and the buffer is freed.  The box, scale and
 * BSDF parameters are the scene's; max_density is found on the device (flags: CVR_DEVMED_SPARSE
 * or 0).  A scene without raw bytes: CVR_ERR_INVALID. */
int cvr_set_medium_scene_transfer(cvr_ctx* ctx, const cvr_scene* scene, const cvr_transfer_desc* transfer,
                                  uint32_t flags);

/* ---- gradient-magnitude transfer functions: 2-D tables classified on the device (extension
 *      within ABI 6: CVR_HAS_GRADIENT_TRANSFER) -- */
/* A scalar field and a table of m rows of n entries (r, g, b, density) give every voxel a
 * density and an albedo from its value and the magnitude of its gradient, so that a homogeneous
 * region and a material boundary of the same value can be told apart.  Row j belongs to gradient
 * entry j; entry (j, i) is at j * n + i.  Every operation is fp32 +, -, x, /, sqrtf, floorf and
 * comparisons in the order written here, no fused multiply-add, / and sqrtf correctly rounded, so
 * the build kernels and cvr_classify_gradient_host return the same bits (one definition compiles
 * for both, cvr_kernels.h).  For voxel (x, y, z) of a field of res = (nx, ny, nz), S(.) the voxel
 * converted to float (exact for the integer types):
 *   xm = x > 0 ? x - 1 : x, xp = x + 1 < nx ? x + 1 : x;
 *   kx = (xp - xm == 2) ? hx2 : hx1, with hx1 = 1.0f / spacing[0] and hx2 = 0.5f / spacing[0]
 *        computed once on the host in fp32;
 *   gx = (S(xp, y, z) - S(xm, y, z)) * kx: a central difference in the interior, a one-sided one
 *        on a face; on an axis of one voxel xp == xm and a finite field gives 0;
 *   gy, gz likewise with spacing[1], spacing[2];
 *   q = (gx * gx + gy * gy) + gz * gz, mag = sqrtf(q);
 *   w = (mag - glo) / (ghi - glo), v = w > 0 ? w : 0, then v = v < 1 ? v : 1 (a NaN gives 0,
 *        +inf gives 1);
 *   u from s = S(x, y, z), lo, hi exactly as the 1-D statement above, xt = u * (float)(n - 1);
 *   i = min((uint)floorf(xt), n - 2), f = xt - (float)i;
 *   yt = v * (float)(m - 1), j = min((uint)floorf(yt), m - 2), h = yt - (float)j;
 *   P = entry (j, i), Q = (j, i + 1), R = (j + 1, i), W = (j + 1, i + 1); per component c of r, g,
 *   b, density: a_c = P_c + f * (Q_c - P_c), b_c = R_c + f * (W_c - R_c), e_c = a_c + h * (b_c - a_c)
 *   (each one subtract, one multiply, one add, in that order);
 *   albedo = (e_r, e_g, e_b, 1.0f), density = e's density.
 * There is no CEIL and no DENSITY_U mode in 2-D: flags must be 0.
 * Not supported: gradient-based shading, classification at render
 * time (the medium is classified once, when it is built), keeping the field. */
#define CVR_HAS_GRADIENT_TRANSFER 1
typedef struct cvr_gradient_transfer_desc {
  uint32_t n, m;      /* n >= 2, m >= 2, n * m <= 4096 (64 KB of LDS, the 1-D table's budget) */
  uint32_t flags;     /* 0 */
  uint32_t reserved;  /* 0 */
  const float* table; /* HOST, m * n * 4 floats */
  float lo, hi;       /* finite, hi > lo */
  float glo, ghi;     /* finite, 0 <= glo < ghi */
  float spacing[3];   /* finite, > 0; (1, 1, 1): the gradient per voxel */
} cvr_gradient_transfer_desc; /* 56 bytes */
/* Host only, no GPU: the statement above over a field of res = (nx, ny, nz) voxels in host memory
 * (x fastest).  density and gradient_magnitude (res product floats each) and albedo (4 floats per
 * voxel) may each be NULL.  The descriptor is checked as cvr_set_medium_gradient checks it. */
int cvr_classify_gradient_host(const void* scalar, uint32_t scalar_type, const uint32_t res[3],
                               const cvr_gradient_transfer_desc* transfer, float* density, float* albedo,
                               float* gradient_magnitude);
/* cvr_set_medium_scalar with the statement above: its contract, with cvr_classify_gradient_host in
 * the place of cvr_classify_host.  The context ends in the state cvr_set_medium_device leaves on
 * device copies of that call's density and albedo (equal cvr_medium_info and cvr_medium_layout,
 * the same paths bit for bit, dense and sparse, in both medium formats), and everything derived
 * from values is derived from the classified values: the majorant, the binary16 overflow refusal
 * with the host call's code and message, uniform-albedo detection, the leaf rule with voxel
 * (0,0,0)'s classified albedo as background, and dropping the leaf albedo pool.  No dense array of
 * the classified medium or of the gradient exists outside the context's storage.  A sparse build
 * reads in-grid neighbours from the field even where they lie in a leaf that does not exist: the
 * gradient is the field's.
 * flags: CVR_DEVMED_SPARSE and / or CVR_DEVMED_MAX_DENSITY.
 * Refusals, all CVR_ERR_INVALID with the previous medium kept, in this order:
 *   1. the host call's shape guards, from res alone and before any pointer is looked at;
 *   2. unknown flags (CVR_DEVMED_CONST_ALBEDO is one here) or scalar_type;
 *   3. n < 2, m < 2 or n * m > 4096;
 *   4. transfer flags or reserved not 0;
 *   5. a NULL table or a NULL d_scalar;
 *   6. lo / hi not finite, or hi <= lo;
 *   7. glo / ghi not finite, glo < 0 or ghi <= glo;
 *   8. a spacing that is not finite or not > 0;
 *   9. a d_scalar that is not device-accessible memory of the context's device or is misaligned
 *      for its type.
 * Inside an adaptive session: CVR_ERR_STATE.
 * Synchronous on the context's stream; the field is only read and may be freed afterwards, the
 * context does not keep it.  cvr_debug_device_medium_ms reports this call's groups as it reports
 * cvr_set_medium_scalar's. */
typedef struct cvr_gradient_medium_desc {
  uint32_t res[3];
  uint32_t flags;
  const void* d_scalar; /* device, res product elements of scalar_type, x fastest, contiguous */
  uint32_t scalar_type; /* CVR_SCALAR_* */
  uint32_t reserved;    /* 0 */
  cvr_gradient_transfer_desc transfer;
  float box_min[3], box_max[3];
  float scale, max_density, g, roughness[2], eta;
} cvr_gradient_medium_desc; /* 136 bytes */
int cvr_set_medium_gradient(cvr_ctx* ctx, const cvr_gradient_medium_desc* medium);
/* cvr_set_medium_gradient on a Raw scene's bytes, as cvr_set_medium_scene_transfer: CVR_SCALAR_U8
 * with lo 0 and hi the largest byte (transfer's lo and hi are ignored); glo, ghi and spacing are
 * the descriptor's.  flags: CVR_DEVMED_SPARSE or 0.  A scene without raw bytes: CVR_ERR_INVALID. */
int cvr_set_medium_scene_gradient(cvr_ctx* ctx, const cvr_scene* scene, const cvr_gradient_transfer_desc* transfer,
                                  uint32_t flags);

/* ---- label volumes: per-segment transfer tables classified on the device (extension within
 *      ABI 6: CVR_HAS_LABELS) -- */
/* A scalar field, a label volume of one byte per voxel on the same grid (a segmentation: the byte
 * names the organ, bone, vessel or tumour the voxel belongs to) and a table of m rows of n entries
 * (r, g, b, density) give every voxel a density and an albedo: row j is the 1-D transfer function
 * of label j, entry (j, i) is at j * n + i.  Per voxel, with L its label byte and s its scalar
 * converted to float (exact for the integer types):
 *   j = L < m ? L : 0: row 0 is the unlabelled / background row, and a label the table has no row
 *       for is treated as unlabelled;
 *   e = exactly the CVR_HAS_TRANSFER statement above applied to entries j * n .. j * n + n - 1, with
 *       the descriptor's n, lo, hi and flags (CVR_TF_CEIL and CVR_TF_DENSITY_U mean what they mean
 *       there), the same fp32 operations in the same order, no fused multiply-add;
 *   albedo = (e_r, e_g, e_b, 1.0f), and the density is as there.
 * Nothing interpolates across rows.  With m = 1 the statement is cvr_set_medium_scalar's, whatever
 * the labels hold.  One definition compiles for the build kernels and cvr_classify_labels_host
 * (cvr_kernels.h), so both return the same bits.  Hiding a segment is a row of density 0: in a
 * sparse build the leaves that hold only such voxels (and the background's colour) do not exist.
 * Not supported: labels combined with the 2-D gradient table, per-label lo / hi windows, label
 * types wider than a byte, smooth (sub-voxel) segment borders (a border voxel's cell interpolates
 * between the two segments' classified values, as any two neighbours do), labels in cvr_features,
 * cvr_field_stats or cvr_field_histogram, keeping either field, the host uploads. */
#define CVR_HAS_LABELS 1
typedef struct cvr_label_transfer_desc {
  uint32_t n, m;      /* n >= 2, 1 <= m <= 256, n * m <= 4096 (64 KB of LDS, the 1-D table's budget; the
                         build's 256 label counters, 1 KB, lie beside it) */
  uint32_t flags;     /* CVR_TF_* */
  uint32_t reserved;  /* 0 */
  const float* table; /* HOST, m * n * 4 floats, row by row */
  float lo, hi;       /* finite, hi > lo */
} cvr_label_transfer_desc; /* 32 bytes */
/* Host only, no GPU: the statement above over n_voxels voxels of `scalar` (host memory of type
 * scalar_type) and `labels` (n_voxels bytes).  density (n_voxels floats), albedo (4 * n_voxels
 * floats) and counts may each be NULL; counts is uint64_t[256], the number of voxels with each
 * label byte.  The descriptor is checked as cvr_set_medium_labeled checks it. */
int cvr_classify_labels_host(const void* scalar, uint32_t scalar_type, const uint8_t* labels, size_t n_voxels,
                             const cvr_label_transfer_desc* transfer, float* density, float* albedo,
                             uint64_t* counts);
/* cvr_set_medium_scalar with the statement above: its contract, with cvr_classify_labels_host in
 * the place of cvr_classify_host.  The context ends in the state cvr_set_medium_device leaves on
 * device copies of that call's density and albedo: equal cvr_medium_info and cvr_medium_layout,
 * every stored array equal byte for byte, the same paths bit for bit, dense and sparse, in both
 * medium formats.  Everything derived from values is derived from the classified values: the
 * majorant, the binary16 overflow refusal with the host call's code, message and index,
 * uniform-albedo detection, the leaf rule with voxel (0,0,0)'s classified albedo as background,
 * and dropping the leaf albedo pool.  No dense array of the classified medium exists outside the
 * context's storage.
 * flags: CVR_DEVMED_SPARSE and / or CVR_DEVMED_MAX_DENSITY.  d_scalar as cvr_set_medium_scalar's;
 * d_labels: device memory, res product bytes, x fastest, of any alignment.
 * Refusals, all CVR_ERR_INVALID with the previous medium kept, in this order:
 *   1. the host call's shape guards, from res alone and before any pointer is looked at;
 *   2. unknown flags (CVR_DEVMED_CONST_ALBEDO is one here) or scalar_type;
 *   3. n < 2, m < 1, m > 256 or n * m > 4096;
 *   4. unknown transfer flags or reserved not 0;
 *   5. a NULL table, d_scalar or d_labels;
 *   6. lo / hi not finite, or hi <= lo;
 *   7. a d_scalar that is not device-accessible memory of the context's device or is misaligned
 *      for its type;
 *   8. a d_labels that is not device-accessible memory of the context's device.
 * Inside an adaptive session: CVR_ERR_STATE.
 * Synchronous on the context's stream; both fields are only read (as often as cvr_set_medium_scalar
 * reads its field) and may be freed afterwards, the context keeps neither.
 * cvr_debug_device_medium_ms reports this call's groups as it reports cvr_set_medium_scalar's. */
typedef struct cvr_labeled_medium_desc {
  uint32_t res[3];
  uint32_t flags;
  const void* d_scalar; /* device, res product elements of scalar_type, x fastest, contiguous */
  uint32_t scalar_type; /* CVR_SCALAR_* */
  uint32_t reserved;    /* 0 */
  cvr_label_transfer_desc transfer;
  float box_min[3], box_max[3];
  float scale, max_density, g, roughness[2], eta;
  const void* d_labels; /* device, res product bytes, x fastest, contiguous, any alignment */
} cvr_labeled_medium_desc; /* 120 bytes */
int cvr_set_medium_labeled(cvr_ctx* ctx, const cvr_labeled_medium_desc* medium);
/* Of the current medium, own or shared: *m the rows of the table cvr_set_medium_labeled built it
 * with, 0 if another call built it, and counts[b] the number of voxels with label byte b that the
 * build kept, counted on the device in the build's own store or leaf-flag pass.  Voxels a clip
 * removes are not counted, so the counts sum to cvr_medium_clip_info's kept.  A medium another call
 * built: all counts 0.  Either pointer may be NULL.  CVR_ERR_STATE: no medium. */
int cvr_medium_label_info(const cvr_ctx* ctx, uint32_t* m, uint64_t counts[256]);
/* cvr_set_medium_labeled on a Raw scene's bytes, as cvr_set_medium_scene_transfer: CVR_SCALAR_U8
 * with lo 0 and hi the largest byte (transfer's lo and hi are ignored).  host_labels: n_labels
 * bytes in host memory, uploaded to a temporary device buffer and freed; n_labels must equal the
 * scene's voxel count (CVR_ERR_INVALID).  flags: CVR_DEVMED_SPARSE or 0. */
int cvr_set_medium_scene_labels(cvr_ctx* ctx, const cvr_scene* scene, const cvr_label_transfer_desc* transfer,
                                const uint8_t* host_labels, size_t n_labels, uint32_t flags);

/* ---- crop box and clip planes for media built from device memory (extension within ABI 6:
 *      CVR_HAS_CLIP) -- */
/* A clip region cuts the volume open where the voxel is classified: the four device builds
 * (cvr_set_medium_device, cvr_set_medium_scalar, cvr_set_medium_gradient, cvr_set_medium_labeled
 * and their _scene_ forms)
 * store a voxel outside the region as empty.  Every operation is an integer comparison or fp32 +,
 * x and a comparison in the order written here, no fused multiply-add, so the build kernels and
 * cvr_clip_host decide the same voxels (one definition compiles for both, cvr_clip.h).  For voxel
 * (x, y, z) of a grid of res voxels:
 *   crop:   lo[a] <= c_a < min(hi[a], res[a]) on each axis a, in integer voxel indices; hi above
 *           res is allowed and means "to the end";
 *   planes: for plane k < n_planes with planes[k] = (A, B, C, D), coefficients in voxel-index space,
 *           t = ((A * (float)x + B * (float)y) + C * (float)z) + D, each product rounded, summed
 *           in that order; the plane keeps the voxel iff t >= 0 (a tie is kept, a NaN t is not);
 *   kept:   iff the crop keeps the voxel and every plane keeps it.
 * A clipped voxel's density is +0.0f and its albedo is the 16 bytes of the unclipped source's voxel
 * (0, 0, 0); the same holds for voxel 0 itself.  That is the value the leaf rule compares against
 * and the sparse background, so a leaf whose in-grid voxels are all clipped does not exist, and a
 * dense grid clipped to one colour region is still detected as uniform.  Colour within one cell
 * of the cut interpolates toward that background, exactly as it already does at the border of a
 * leaf that does not exist.  A kept voxel is exactly what the unclipped call stores; for
 * cvr_set_medium_gradient its gradient neighbours are read from the field whether they are
 * clipped or not: the gradient is the uncut field's, and a cut surface is no material boundary.
 *
 * Contract: with a clip set, a device build leaves the context in the state that
 * cvr_set_medium_device with no clip leaves on device copies of cvr_clip_host's output (for the
 * classified routes: cvr_clip_host applied to cvr_classify_host's / cvr_classify_gradient_host's /
 * cvr_classify_labels_host's arrays): equal cvr_medium_info and cvr_medium_layout, every stored array equal byte for byte,
 * the same paths bit for bit, dense and sparse, in both formats.  Everything derived from values
 * is derived from the clipped values: the CVR_DEVMED_MAX_DENSITY majorant, the binary16 overflow
 * refusal with its code, message and index, uniform-albedo detection, the leaf rule, dropping the
 * leaf albedo pool.  A given max_density is used as given.  An all-clipped grid behaves as the
 * call behaves on an all-zero density.  A context that sets no clip runs what it ran before.
 *
 * The clip is context state, taken at the next device build as CVR_OPT_CELLS is taken; the medium
 * already built is not touched.  cvr_set_clip refuses with CVR_ERR_INVALID, in this order:
 *   1. a NULL descriptor;
 *   2. flags not 0;
 *   3. n_planes > CVR_CLIP_MAX_PLANES;
 *   4. lo[a] > hi[a] on some axis (lo == hi is an empty crop: everything is clipped);
 *   5. a coefficient of a plane k < n_planes that is not finite;
 *   6. a plane k < n_planes whose A, B and C are all zero.
 * Inside an adaptive session cvr_set_clip and cvr_clear_clip return CVR_ERR_STATE.
 * With a clip set the host uploads cvr_set_medium and cvr_set_medium_sparse return
 * CVR_ERR_UNSUPPORTED and keep the previous medium; cvr_share_medium shares whatever the source
 * built, with its clip information.
 * Not supported: cuts at ray level (sub-voxel smooth cut surfaces), per-voxel mask volumes
 * (a label volume with a row of density 0 hides a segment: CVR_HAS_LABELS), clipping of cvr_features, cvr_field_stats or cvr_field_histogram (they still see the
 * whole field), the host uploads, inverted or unioned regions. */
#define CVR_HAS_CLIP 1
#define CVR_CLIP_MAX_PLANES 8
typedef struct cvr_clip_desc {
  uint32_t lo[3], hi[3]; /* the crop box in voxel indices, lo <= c < hi; (0,0,0) and UINT32_MAX: no crop */
  uint32_t n_planes;     /* 0..CVR_CLIP_MAX_PLANES */
  uint32_t flags;        /* 0 */
  float planes[CVR_CLIP_MAX_PLANES][4]; /* A, B, C, D; the entries from n_planes on are ignored */
} cvr_clip_desc; /* 160 bytes */
int cvr_set_clip(cvr_ctx* ctx, const cvr_clip_desc* clip);
int cvr_clear_clip(cvr_ctx* ctx);
/* The context's clip (*set 1) or, with none set, the descriptor that keeps everything (*set 0).
 * Either pointer may be NULL. */
int cvr_get_clip(const cvr_ctx* ctx, cvr_clip_desc* clip, int* set);
/* Host only, no GPU: the statement above, in place, on host arrays of a grid of res voxels (x
 * fastest).  density (one float per voxel), albedo (4 floats per voxel) and keep (one byte per
 * voxel: 1 kept, 0 clipped) may each be NULL.  The descriptor is checked as cvr_set_clip checks
 * it; an empty grid or more than 2^32 - 1 voxels: CVR_ERR_INVALID. */
int cvr_clip_host(const uint32_t res[3], const cvr_clip_desc* clip, float* density, float* albedo, uint8_t* keep);
/* The clip the current medium (own or shared) was built under and the number of voxels it keeps,
 * counted on the device in the build's own store or leaf-flag pass.  A medium built without a
 * clip: the descriptor that keeps everything and the grid's voxel count.  Either pointer may be
 * NULL.  CVR_ERR_STATE: no medium. */
int cvr_medium_clip_info(const cvr_ctx* ctx, cvr_clip_desc* clip, uint64_t* kept);

/* ---- field statistics and value-gradient histograms (extension within ABI 6:
 *      CVR_HAS_FIELD_HISTOGRAM) -- */
/* What the two classifications above need to be aimed: the value range and the largest gradient
 * magnitude of a scalar field (lo, hi and ghi of their descriptors), and the histogram of its
 * voxels over the nodes of a 1-D or 2-D table, the joint histogram of value and gradient magnitude
 * a 2-D table is designed on.  The gradient is the one stated above and is never stored.
 * Every operation is fp32 +, -, x, /, sqrtf, floorf and comparisons in the order written, no
 * fused multiply-add, / and sqrtf correctly rounded; the results are integer counts and
 * order-independent extrema, so the device calls return exactly what the *_host statements return
 * (one definition compiles for both, cvr_kernels.h).  For voxel (x, y, z), S(.) the voxel converted
 * to float:
 *   mag = the gradient magnitude of CVR_HAS_GRADIENT_TRANSFER's statement, with its one-sided rule
 *         on a face and hx1 = 1.0f / spacing[0], hx2 = 0.5f / spacing[0] (and y, z) computed once on
 *         the host;
 *   u:  t = (s - lo) / (hi - lo), u = t > 0 ? t : 0, then u = u < 1 ? u : 1 (a NaN gives 0): the
 *       classifications' u, bit for bit;
 *   v:  likewise from mag, glo and ghi;
 *   the bin of a coordinate c on an axis of k nodes: x = c * (float)(k - 1),
 *       i0 = min((uint)floorf(x), k - 1), f = x - (float)i0 (exact),
 *       bin = min(i0 + (f >= 0.5f ? 1 : 0), k - 1): the nearest table node, ties upward, with no
 *       rounded x + 0.5.  Values outside [lo, hi] fall into the edge bins, as the classification
 *       clamps them; a NaN into bin 0.
 * Histogram: n value bins by m gradient bins, the shape of an m-row, n-entry table;
 *   counts[j * n + i] = the number of voxels with value bin i and gradient bin j, as uint32.
 *   2 <= n, 1 <= m, n * m <= 65536.  m == 1 is the 1-D histogram: no gradient is computed and glo,
 *   ghi and spacing are neither read nor judged.  The counts sum to the voxel count; a field of
 *   more than 2^32 - 1 voxels is refused.
 * Statistics:
 *   vmin, vmax over the voxels whose value is not NaN, ordered by the total order of the bits that
 *     puts -0 below +0 (so the returned bits are defined); with no such voxel +inf and -inf;
 *   gmax over the voxels whose magnitude is not NaN (+inf counts); with none, 0;
 *   nan_values, nan_gradients: the voxels whose value, whose magnitude is NaN (inf - inf is one).
 * Refusals, all CVR_ERR_INVALID, in this order:
 *   1. NULL arguments (the context, a descriptor, the statistics' output);
 *   2. a zero extent, or more than 2^32 - 1 voxels: from res alone, before any pointer is looked at;
 *   3. an unknown scalar_type, or a non-zero reserved or flags;
 *   4. n < 2, m < 1 or n * m > 65536;
 *   5. lo / hi not finite, or hi <= lo;
 *   6. for m > 1 only: glo / ghi not finite, glo < 0 or ghi <= glo;
 *   7. for m > 1 only, and always for the statistics: a spacing that is not finite or not > 0;
 *   8. a NULL scalar or counts pointer;
 *   9. a scalar (the device calls: or d_counts) that is misaligned for its type, or, the device
 *      calls, is not device-accessible memory of the context's device.
 * The device calls take the device and the stream from the context and otherwise only read it:
 * they work with or without a medium and inside an adaptive session, and leave cvr_medium_info,
 * the medium and the framebuffer untouched.  cvr_field_stats and cvr_field_histogram are
 * synchronous and the field may be freed when they return; cvr_field_histogram_buffers is ordered
 * on the context's stream and does not synchronise, and it overwrites all n * m words of d_counts,
 * so the caller need not clear them.
 * Not supported: weighted or float histograms, histograms of the stored medium or of a sparse
 * leaf pool, percentiles or automatic table design, second-derivative axes, keeping the field. */
#define CVR_HAS_FIELD_HISTOGRAM 1
typedef struct cvr_field_desc {
  uint32_t res[3];
  uint32_t scalar_type; /* CVR_SCALAR_* */
  const void* scalar;   /* device for the context calls, host for *_host; res product elements, x fastest */
  float spacing[3];     /* finite, > 0; read where a gradient is taken */
  uint32_t reserved;    /* 0 */
} cvr_field_desc; /* 40 bytes */
/* (a struct tag only: the name cvr_field_stats is the device call's, so the struct is written
 * `struct cvr_field_stats` in C and in C++) */
struct cvr_field_stats {
  float vmin, vmax, gmax;
  uint32_t reserved; /* 0 */
  uint64_t nan_values, nan_gradients;
}; /* 32 bytes */
typedef struct cvr_histogram_desc {
  uint32_t n, m;     /* value bins, gradient bins */
  uint32_t flags;    /* 0 */
  uint32_t reserved; /* 0 */
  float lo, hi;      /* finite, hi > lo */
  float glo, ghi;    /* m > 1: finite, 0 <= glo < ghi */
} cvr_histogram_desc; /* 32 bytes */
/* Host only, no GPU: the statements above over a field in host memory. */
int cvr_field_stats_host(const cvr_field_desc* field, struct cvr_field_stats* stats);
int cvr_field_histogram_host(const cvr_field_desc* field, const cvr_histogram_desc* histogram, uint32_t* counts);
/* The same of a field in device memory; host_counts: n * m words of host memory, d_counts: of
 * device memory. */
int cvr_field_stats(cvr_ctx* ctx, const cvr_field_desc* field, struct cvr_field_stats* stats);
int cvr_field_histogram(cvr_ctx* ctx, const cvr_field_desc* field, const cvr_histogram_desc* histogram,
                        uint32_t* host_counts);
int cvr_field_histogram_buffers(cvr_ctx* ctx, const cvr_field_desc* field, const cvr_histogram_desc* histogram,
                                uint32_t* d_counts);
/* Debug, host only: the launch geometry of the field kernels, as cvr_debug_build_geometry reports
 * the build's.  out[0] the stencil walk's grid cap in tasks and [1] the z planes of a task (a
 * task: 256 x of one y); [2] the 1-D histogram's grid cap (workgroups of 256 lanes, 16 bytes per
 * lane and trip for the integer types); [3] the most bins a workgroup keeps in LDS (more: global
 * atomics); [4] the largest n * m; [5], [6] 0; [7] the number of entries filled, 5. */
int cvr_debug_field_geometry(uint32_t out[8]);

/* ---- environment-map lighting (extension within ABI 6: CVR_HAS_ENVMAP) -- */
/* Without an environment every path that leaves the box adds its throughput T: a constant white
 * environment of radiance 1 (the reference's only light).  With one, an escaping path adds
 * C = T (.) L(d), L the radiance of a latitude-longitude map in its direction d at escape.
 * The lookup is fp32 only, every operation in the order written here, the fused ones explicit
 * (det_fmaf; cvr_detmath.h), so the kernels and cvr_environment_eval_host return the same bits
 * (one definition compiles for both, cvr_env.h).  For a direction d (unit or not), the row-major
 * world-to-environment rotation R[9] and W x H stored texels (row 0 is the top, +Y is up, -Z is
 * the centre column: Mitsuba's envmap convention):
 *   e_x = (R0 d.x + R1 d.y) + R2 d.z        (likewise e_y from R3..5, e_z from R6..8)
 *   u = det_fmaf(det_atan2f(e_x, -e_z), 0.15915494309189535f, 0.5f)
 *   v = det_acosf(det_fminf(det_fmaxf(e_y, -1), 1)) * 0.3183098861837907f
 *   u = det_fminf(det_fmaxf(u, 0), 1), v likewise                  (a NaN becomes 0)
 *   x = det_fmaf(u, (float)W, -0.5f), y = det_fmaf(v, (float)H, -0.5f)
 *   x0 = det_floor_i32(x), fx = x - (float)x0;  y0, fy likewise
 *   xa = x0 < 0 ? W-1 : x0,  xb = x0+1 >= W ? 0 : x0+1           (u wraps)
 *   ya = y0 < 0 ? 0 : y0,    yb = y0+1 >= H ? H-1 : y0+1         (v clamps)
 *   per channel, A, B = row ya at xa, xb and C, D = row yb at xa, xb:
 *     t = det_fmaf(fx, B - A, A), b = det_fmaf(fx, D - C, C), L = det_fmaf(fy, b - t, t)
 * So no index leaves the image, a constant map returns exactly its constant, the seam
 * d = (+-0, 0, 1) reads columns W-1 and 0, and the poles read rows 0 and H-1 alone.
 * Stored texels are (fl(scale r), fl(scale g), fl(scale b), 0): 16 bytes, one load per tap.
 *
 * cvr_set_environment: the context keeps its own copy (W * H * 16 device bytes); the caller's
 * array is only read and may be freed afterwards.  From CVR_ENV_DEVICE memory (a torch tensor) no
 * array crosses to the host: one kernel converts the 3- or 4-channel input and in the same pass
 * finds the largest stored component and the smallest index of an invalid one; a host array is
 * staged on the device and takes the same kernel.  Synchronous on the context's stream.
 * Refusals, in this order, the previous environment (or none) kept in each case:
 *   inside an adaptive session: CVR_ERR_STATE;
 *   width outside 2..16384, height outside 2..8192, channels other than 3 or 4, an unknown
 *   location, a NULL pixels pointer, a scale that is negative or not finite, a rotation entry
 *   that is not finite: CVR_ERR_INVALID;
 *   CVR_ENV_DEVICE pixels that are not device-accessible memory of the context's device, or
 *   4-channel ones that are not 16-byte aligned: CVR_ERR_INVALID;
 *   a stored component that is negative or not finite (after scaling): CVR_ERR_INVALID, the
 *   message names the smallest index (texel * channels + channel) of one.  (The framebuffer's
 *   sums are then never -0 and all contributions have one sign.)
 * cvr_clear_environment: back to radiance 1, with the launches and kernel instances of a
 * context that never had an environment.
 * With an environment a launch runs on the wave-pool scheduler at 5 waves per SIMD with its
 * generic dense instance or a sparse one (fp32 or half), without or with CVR_OPT_MOMENTS (the
 * moments are then sums of fl(C C), the count is unchanged): cvr_launch_render, cvr_render_frame
 * (always its normalise-and-copy path in one part: cvr_frame_flush_info reports 0 blocks),
 * cvr_render_image / _tiles / _share_to_host, block shards, path ranges, a caller's output buffer,
 * the adaptive session and cvr_denoise.  CVR_ERR_UNSUPPORTED, the message naming the obstacle:
 * kernel id naiveMK, another CVR_OPT_SCHEDULER or CVR_OPT_WAVES value, CVR_OPT_RNG_BINDING 1,
 * CVR_OPT_COUNT_WORDS 1, CVR_OPT_MK_COMPACTION 1, cvr_trace_launch, and second moments on a sparse
 * half medium.
 * Not supported: next-event estimation or importance sampling of the map (a small bright sun is
 * noisy), the XML scenes' envmap emitter, sharing one environment between contexts (each keeps a
 * copy; cvr_render_frame's helper contexts are not used with one), naiveMK. */
#define CVR_HAS_ENVMAP 1
enum { CVR_ENV_HOST = 0, CVR_ENV_DEVICE = 1 }; /* cvr_environment_desc.location */
typedef struct cvr_environment_desc {
  uint32_t width, height; /* 2..16384, 2..8192 */
  uint32_t channels;      /* floats per texel: 3, or 4 (the fourth is ignored) */
  uint32_t location;      /* CVR_ENV_HOST / CVR_ENV_DEVICE: where pixels lives */
  const float* pixels;    /* width * height * channels floats, row 0 the top, contiguous */
  float scale;            /* finite, >= 0: every component is multiplied by it when stored */
  float rotation[9];      /* row-major world-to-environment; all zero: the identity */
} cvr_environment_desc;   /* 64 bytes */
struct cvr_environment_info {
  uint32_t width, height; /* 0, 0: no environment */
  uint64_t bytes;         /* device bytes of the stored texels */
  float max_component;    /* the largest stored component */
  uint32_t reserved;
};
int cvr_set_environment(cvr_ctx* ctx, const cvr_environment_desc* desc);
int cvr_clear_environment(cvr_ctx* ctx);
int cvr_environment_info(const cvr_ctx* ctx, struct cvr_environment_info* out);
/* Host only, no GPU: the statement above for n directions (dirs: 3 n floats) of a
 * CVR_ENV_HOST descriptor, into out_rgb (3 n floats).  The descriptor is checked as
 * cvr_set_environment checks it, its texel values excepted. */
int cvr_environment_eval_host(const cvr_environment_desc* desc, const float* dirs, size_t n, float* out_rgb);
/* The same with the stored texel (x, y) taken from a callback instead of an array (rgba[0..2]
 * are used as they are: no scale), for maps too large to hold on the host.  rotation: 9 floats
 * or NULL (the identity). */
typedef void (*cvr_texel_fn)(void* user, uint32_t x, uint32_t y, float rgba[4]);
int cvr_environment_eval_host_fn(uint32_t width, uint32_t height, const float* rotation, cvr_texel_fn texel,
                                 void* user, const float* dirs, size_t n, float* out_rgb);
/* The device's lookup of the context's environment for n arbitrary directions (host arrays),
 * by a small kernel: the parity hook that is independent of the walk.  Synchronous.
 * CVR_ERR_STATE: no environment. */
int cvr_environment_eval(cvr_ctx* ctx, const float* host_dirs, size_t n, float* host_out_rgb);
/* cvr_trace_paths' one-path-per-work-item walk with the environment applied: T is the
 * throughput before the environment (cvr_path_record's T), d the direction at escape and
 * C = T (.) L(d) the contribution; d and C are zero for a path that does not escape.  Kernel id
 * naiveMK: CVR_ERR_UNSUPPORTED; no environment: CVR_ERR_STATE. */
typedef struct cvr_env_record {
  uint32_t image_id;
  uint32_t flags; /* bit0 escaped, bit1 truncated */
  uint32_t n_segments;
  float T[3], d[3], C[3];
} cvr_env_record; /* 48 bytes */
int cvr_trace_env(cvr_ctx* ctx, uint32_t first, uint32_t count, cvr_env_record* host_out);
/* Host only: read a Radiance .hdr (32-bit_rle_rgbe, "-Y h +X w" only; flat scanlines as
 * cvr_write_hdr writes them, or new-style run-length encoded ones) or a colour .pfm ("PF",
 * either byte order, rows bottom-up in the file) into a malloc'ed array of width * height * 3
 * floats, row 0 the top; the format is taken from the file's first bytes.  Release it with
 * cvr_free_image.  A file that cannot be opened, is truncated or malformed, has a zero
 * dimension or (.hdr) a run that passes its scanline: CVR_ERR_IO. */
int cvr_read_image(const char* path, uint32_t* width, uint32_t* height, float** rgb);
void cvr_free_image(float* rgb);

/* ---- primary-ray feature buffers (extension within ABI 6: CVR_HAS_FEATURES) -- */
/* Noise-free guide buffers of the medium the context holds, and the classic emission-absorption
 * preview of a transfer function: per pixel, one ray march along the straight camera ray through
 * the pixel's centre gives the opacity, the mean first-collision albedo and the mean collision
 * depth.  No RNG, no walk.  Every operation is fp32 +, -, x, /, sqrt in the order written here
 * (correctly rounded, no fused multiply-add but the fma named below), so the device kernel and
 * cvr_features_host return the same bits (one definition compiles for both, cvr_features.h).
 * Per pixel (ix, iy) of the tile (resolution, offset, camera, CVR_OPT_WORLD_TO_AABB as set):
 * Ray: camera_ray's operations with both pixel jitters 0.5f: px = (float)ix + (float)off_x,
 *   rx = r2v_x (((px + 0.5f) 2) / full_res_x - 1), ry likewise, v = (rx, ry, 1) / sqrt((rx rx +
 *   ry ry) + 1), o = column 3 of inv_view, d_a = (v_x M_a0 + v_y M_a1) + v_z M_a2.
 * Chord: the walk's slab test.  Per axis i = 1 / d, tbot = i (box_min - o), ttop = i (box_max - o),
 *   lo = minNum(ttop, tbot), hi = maxNum(ttop, tbot), where minNum / maxNum return the other
 *   operand when the first is NaN and the first when the second is; a +-0 direction component
 *   gives i = +-inf, and an origin on that axis' plane then a NaN that the other plane's +-inf
 *   replaces.  enter = maxNum(maxNum(lo_x, lo_y), maxNum(lo_x, lo_z)), t1 = minNum(minNum(hi_x,
 *   hi_y), minNum(hi_x, hi_z)), t0 = enter > 0 ? enter : 0 (0 for an eye inside the box).  There
 *   is a chord iff t1 > enter and t1 > t0 (a NaN compares false); a pixel without one outputs
 *   (0, 0, 0, 0) and depth 0.  Every ray the walk's box test calls a miss has no chord.
 * Steps: delta = step min(min(e_x / res_x, e_y / res_y), e_z / res_z), e = box_max - box_min,
 *   n = min(max_steps, ceil((t1 - t0) / delta)), t_i = t0 + ((float)i + 0.5f) delta for i < n; a
 *   t_i >= t1 is dropped.
 * Per step, from T = 1 and A = Z = W = 0:
 *   p = o + t_i d (a multiply, then an add);
 *   rho = the walk's interpolated density at p: c = p - shift, grid coordinate fma(c, g, +0) with
 *     shift = box_min / e, g = res - 1 (quirk Q4; CVR_OPT_WORLD_TO_AABB 1: shift = box_min,
 *     g = (res - 1) / e), corner floor, weights coordinate - corner, the reference's 8 clamped
 *     taps (quirk Q5) and its trilinear, lerp(a, b, f) = fma(b, f, a (1 - f)), x then y then z;
 *   s = (scale rho) delta; if not s > 0 the step contributes nothing; otherwise
 *   a = s / (1 + s) (a rational step opacity: cvr_detmath.h has no exp), w = T a,
 *   c = the walk's albedo at p: coordinate ((p - box_min) / e) (res - 1), the same taps and trilinear;
 *   A_c += w c_c, Z += w t_i, W += w, T = T - w; the march ends after a step that leaves T < t_stop.
 * Output: feat_rgba = (A_r / W, A_g / W, A_b / W, W), feat_depth = (Z / W) / sqrt((e_x e_x +
 *   e_y e_y) + e_z e_z); all 0 where W = 0.
 * The bit-equality contract covers media with finite, non-negative density and finite albedo;
 * other media are read inside their arrays and return something.  Under the contract a step with
 * rho = 0 changes no accumulator, so the device skips, exactly, the samples of a sparse medium
 * that lie in an empty super-brick or in the zero cell leaf; it skips nothing else (a dense
 * medium's brick-bound code 0 does not prove a zero brick).  The output does not depend on the
 * storage: dense or sparse, CVR_OPT_CELLS, CVR_OPT_BOUNDS, CVR_OPT_UNIFORM_ALBEDO,
 * CVR_OPT_EMPTY_MASK; a CVR_FORMAT_F16 medium gives the bits of the cvr_half_round-ed arrays.
 * step in [1/8, 8], t_stop in [0, 1) (0: the march never stops early), max_steps 1..65536,
 * flags 0: else CVR_ERR_INVALID.  The defaults of the bindings and the CLI are 1, 1/256, 4096.
 * Not supported: a ray refracted at the GGX boundary (the ray is the straight camera ray; the
 * buffers are guides, not radiance), shading or lighting (CVR_HAS_PREVIEW below is the lit pass), temporal accumulation. */
#define CVR_HAS_FEATURES 1
typedef struct cvr_features_desc {
  float step;
  float t_stop;
  uint32_t max_steps;
  uint32_t flags;
} cvr_features_desc; /* 16 bytes */
/* Host only, no GPU: the written statement on a dense medium's host arrays (a sparse medium is
 * stated through its densified arrays, a half medium through its cvr_half_round-ed ones; g,
 * roughness, eta and max_density are not read).  out_rgba: tile_w * tile_h * 4 floats;
 * out_depth: tile_w * tile_h floats, may be NULL.  A NULL pointer, an empty grid, a zero side,
 * more than 2^24 pixels, world_to_aabb other than 0 / 1: CVR_ERR_INVALID. */
int cvr_features_host(const cvr_medium_desc* medium, const float inv_view[12], const float raster_to_view[2],
                      const float full_res[2], uint32_t tile_w, uint32_t tile_h, uint32_t off_x, uint32_t off_y,
                      int world_to_aabb, const cvr_features_desc* desc, float* out_rgba, float* out_depth);
/* The pass on the context's medium (own or shared, any storage), camera, resolution and offset,
 * into device memory or the device address of pinned host memory (d_out_rgba 16-byte aligned;
 * d_out_depth may be NULL), asynchronous on the context's stream.  Reads the context and writes
 * nothing of it: not the framebuffer, the moments, the seed or the stats.  Available between
 * cvr_adaptive_begin and cvr_adaptive_end.  No medium, camera or resolution: CVR_ERR_STATE. */
int cvr_features_buffers(cvr_ctx* ctx, const cvr_features_desc* desc, float* d_out_rgba, float* d_out_depth);
/* The same into host memory (host_rgba: tile_w * tile_h * 4 floats, host_floats smaller:
 * CVR_ERR_INVALID; host_depth: tile_w * tile_h floats or NULL).  Synchronous.  Pinned or
 * registered memory is stored into by the kernel, other memory through a staging copy. */
int cvr_features(cvr_ctx* ctx, const cvr_features_desc* desc, float* host_rgba, float* host_depth,
                 size_t host_floats);
/* The feature-guided filter: the filter written at CVR_HAS_DENOISE with three more edge-stopping
 * terms from the feature planes F = feat_rgba and z = feat_depth.  In the 5x5 loop, for a valid
 * centre p and tap q, the tap's weight becomes  w = (h_j h_i) / (u u) / (g g)  with u as there and
 *   g = 1 + ((f_a f_a + f_z f_z) + f_o f_o),
 *   f_a = ((|F_r(q) - F_r(p)| + |F_g(q) - F_g(p)|) + |F_b(q) - F_b(p)|) / sigma_albedo,
 *   f_z = |z(q) - z(p)| / sigma_depth,  f_o = |F_w(q) - F_w(p)| / sigma_alpha;
 * a sigma <= 0 switches its term off (f = 0).  The planes are noise-free: they are read at p and
 * q and never filtered, and play no part in validity, in the 3x3 variance estimate or in the
 * in-painting of an invalid centre.  With all three sigmas <= 0, g = 1 and w / 1 = w: the bits
 * of cvr_denoise.  Same operations on host and device: the same bits.
 * base as cvr_denoise_desc; a sigma that is NaN or +inf, flags != 0: CVR_ERR_INVALID.  The
 * defaults of the bindings and the CLI: base 5, 4.0, 0.01; sigmas 0.4, 0.1, 0.4 (profiles/features/README.md).
 * Not supported: albedo demodulation (the colour is filtered as it is), temporal accumulation. */
typedef struct cvr_denoise_guided_desc {
  cvr_denoise_desc base;
  float sigma_albedo, sigma_depth, sigma_alpha;
  uint32_t flags;
} cvr_denoise_guided_desc; /* 32 bytes */
/* cvr_denoise_host's arguments plus the two planes (feat_rgba w * h * 4 floats, feat_depth w * h). */
int cvr_denoise_guided_host(const float* sum_rgba, const float* m2_rgba, uint32_t w, uint32_t h, uint32_t n_samples,
                            const uint32_t* block_samples, const cvr_denoise_guided_desc* desc,
                            const float* feat_rgba, const float* feat_depth, float* out_rgba, float* out_var);
/* cvr_denoise_buffers' arguments plus two device planes of any origin (d_feat_rgba 16-byte aligned). */
int cvr_denoise_guided_buffers(cvr_ctx* ctx, const float* d_sum_rgba, const float* d_m2_rgba, uint32_t w, uint32_t h,
                               uint32_t n_samples, const uint32_t* d_block_samples,
                               const cvr_denoise_guided_desc* desc, const float* d_feat_rgba, const float* d_feat_depth,
                               float* d_out_rgba, float* d_out_var);
/* cvr_denoise with the guide: runs the feature pass (`features`) into planes the context owns
 * (they grow as the denoiser's scratch images do), then filters the context's sums.  State,
 * n_samples and the adaptive session as cvr_denoise. */
int cvr_denoise_guided(cvr_ctx* ctx, const cvr_denoise_guided_desc* desc, const cvr_features_desc* features,
                       uint32_t n_samples, float* host_rgba, size_t host_floats);

/* ---- shaded preview (extension within ABI 6: CVR_HAS_PREVIEW) ----------- */
/* The picture a volume viewer shows while tables, crops and clip planes are edited: a
 * gradient-shaded emission-absorption rendering of the medium the context holds.  Per pixel, one
 * deterministic ray march along the straight camera ray through the pixel's centre composites
 * colour front to back, lights each contributing sample with Blinn-Phong shading on the gradient
 * of the stored density and lays the result over a background colour.  No RNG, no walk, nothing
 * of the context is written.  All arithmetic is fp32 +, -, x, /, sqrt in the order written here
 * (correctly rounded, no fused multiply-add but the ones the density and albedo lookups of
 * CVR_HAS_FEATURES name), so the device kernel and cvr_preview_host return the same bits (one
 * definition compiles for both, cvr_preview.h).
 * The ray, the chord, the steps and the per-step values p, rho, s, a, w and c (the albedo at p) are
 * exactly those of CVR_HAS_FEATURES, with `march` as its descriptor.  From T = 1 and C = W = 0; a
 * step with not s > 0 contributes nothing and computes no gradient.  For each contributing step:
 *   With CVR_PREVIEW_UNSHADED: e = c.
 *   Otherwise, the gradient: h_a = e_a / res_a (the three cell sizes delta is made from; e =
 *     box_max - box_min), G_a = (rho(p + h_a u_a) - rho(p - h_a u_a)) / h_a, where u_a is the unit
 *     vector of axis a and rho(.) the interpolated density of CVR_HAS_FEATURES at a point that
 *     differs from p in component a only (one add or one subtract): six more lookups, with the
 *     clamped taps and all.  m = sqrt((G_x G_x + G_y G_y) + G_z G_z).
 *   If not m > 0 (zero or NaN): e = c.
 *   Otherwise, shading: n_a = G_a / m (the outward normal is -n).
 *     L = -d with CVR_PREVIEW_HEADLIGHT; without it the descriptor's light direction, normalised
 *     once per call: light_a / sqrt((l_x l_x + l_y l_y) + l_z l_z).  V = -d.
 *     nl = -((n_x L_x + n_y L_y) + n_z L_z), replaced by 0 unless nl > 0.
 *     sp = 0.  If specular > 0: H = L + V, hh = sqrt((H_x H_x + H_y H_y) + H_z H_z); if hh > 0:
 *       nh = -((n_x H_x + n_y H_y) + n_z H_z) / hh, replaced by 0 unless nh > 0, then squared
 *       shininess_log2 times (nh = nh nh: the exponent 2^shininess_log2 without a pow, which
 *       cvr_detmath.h does not have); sp = the result.
 *     f = ambient + diffuse nl,  lit_c = f c_c + specular sp,
 *     q = m / (m + knee_abs) with knee_abs = knee (max_density / min(min(h_x, h_y), h_z)) computed
 *       once per call; max_density is the majorant in use: cvr_medium_info.max_density_eff on the
 *       device, medium->max_density in cvr_preview_host.  The blend keeps homogeneous regions,
 *       where the normal is noise, unlit.
 *     e_c = (1 - q) c_c + q lit_c.
 *   C_c += w e_c, W += w, T = T - w; the march ends after a step that leaves T < t_stop.
 * Output: (C_r + T bg_r, C_g + T bg_g, C_b + T bg_b, W); a pixel without a chord gives
 *   (bg_r, bg_g, bg_b, 0).
 * The bit-equality contract is that of CVR_HAS_FEATURES: media with finite, non-negative density
 * and finite albedo; independent of the storage (dense or sparse, CVR_OPT_CELLS, CVR_OPT_BOUNDS,
 * CVR_OPT_UNIFORM_ALBEDO, CVR_OPT_EMPTY_MASK); a CVR_FORMAT_F16 medium gives the bits of the
 * cvr_half_round-ed arrays with max_density_eff as max_density.  The six gradient lookups are
 * skipped, exactly, where the feature pass's are (an empty super-brick, the zero cell leaf).
 * Refused with CVR_ERR_INVALID, in this order: a NULL descriptor; `march` as cvr_features refuses
 * it; flags other than the two below; ambient, diffuse or specular negative or not finite;
 * shininess_log2 > 10; knee negative or not finite; a background component negative or not
 * finite; without either flag, a light that is not finite or has zero length (the fp32 length as
 * computed above: components so small or large that it is 0 or inf are refused as well).
 * The defaults of the bindings and the CLI: CVR_PREVIEW_HEADLIGHT, ambient 0.3, diffuse 0.7,
 * specular 0.2, shininess_log2 4, knee 0.05, a black background, march 1, 1/256, 4096.
 * Not supported: ambient occlusion (directional shadows: CVR_HAS_SHADOWS below), the environment
 * map as a light, more than one light, the refraction at the GGX boundary (the ray is the straight camera ray), gradients of
 * the original scalar field (the pass sees the stored density only; CVR_HAS_FIELD_PROJECT below lights an
 * isosurface of the field itself), tone mapping, the preview
 * as a denoiser guide, more than one tile or device in the CLI, temporal accumulation. */
#define CVR_HAS_PREVIEW 1
#define CVR_PREVIEW_UNSHADED 1u  /* e = c: plain emission-absorption compositing, no gradient */
#define CVR_PREVIEW_HEADLIGHT 2u /* the light shines along the ray: L = -d */
typedef struct cvr_preview_desc {
  cvr_features_desc march;
  float light[3]; /* the direction towards the light, any length; not read with a flag set */
  float ambient, diffuse, specular;
  uint32_t shininess_log2; /* the specular exponent is 2^shininess_log2, 0..10 */
  float knee;
  float background[3];
  uint32_t flags;
} cvr_preview_desc; /* 64 bytes */
/* Host only, no GPU: the written statement on a dense medium's host arrays; the arguments of
 * cvr_features_host with this descriptor and no depth plane.  out_rgba: tile_w * tile_h * 4
 * floats.  Refuses what cvr_features_host refuses. */
int cvr_preview_host(const cvr_medium_desc* medium, const float inv_view[12], const float raster_to_view[2],
                     const float full_res[2], uint32_t tile_w, uint32_t tile_h, uint32_t off_x, uint32_t off_y,
                     int world_to_aabb, const cvr_preview_desc* desc, float* out_rgba);
/* The pass on the context's medium (own or shared, any storage), camera, resolution and offset,
 * into device memory or the device address of pinned host memory (16-byte aligned), asynchronous
 * on the context's stream.  State as cvr_features_buffers: the context is only read; available
 * between cvr_adaptive_begin and cvr_adaptive_end; no medium, camera or resolution: CVR_ERR_STATE. */
int cvr_preview_buffers(cvr_ctx* ctx, const cvr_preview_desc* desc, float* d_out_rgba);
/* The same into host memory (tile_w * tile_h * 4 floats; host_floats smaller: CVR_ERR_INVALID).
 * Synchronous.  Pinned or registered memory is stored into by the kernel, other memory through a
 * staging copy. */
int cvr_preview(cvr_ctx* ctx, const cvr_preview_desc* desc, float* host_rgba, size_t host_floats);

/* ---- shadowed preview (extension within ABI 6: CVR_HAS_SHADOWS) --------- */
/* Directional shadows for the preview: a light volume holds, per node of a grid over the medium's
 * box, the transmittance from the node to the box's surface towards the light; the shadowed
 * preview scales the light of every contributing sample by the volume's trilinear value there.
 * The volume is computed once per (medium, light): an edit of the camera, the shading weights or
 * the shadow strength costs nothing extra, an edit of the table, the crop or the clip one rebuild.
 * All arithmetic is fp32 +, -, x, /, sqrt in the order written here (correctly rounded, no fused
 * multiply-add but the ones the density and albedo lookups and the trilinear of CVR_HAS_FEATURES
 * name), so the kernels and the two host statements return the same bits (one definition compiles
 * for both, cvr_shadow.h).
 * Light volume.  res_a nodes per axis, each 1..1024, their product at most 2^27; fp32, x fastest.
 *   L_a = light_a / sqrt((l_x l_x + l_y l_y) + l_z l_z): the direction towards the light,
 *     normalised as CVR_HAS_PREVIEW normalises its light.
 *   Node (i, j, k) sits at its cell's centre: p0_a = box_min_a + ((float)i_a + 0.5f) (e_a /
 *     (float)res_a), e = box_max - box_min.
 *   The march is that of CVR_HAS_FEATURES with `march` as its descriptor (delta from march.step
 *   and the medium's cell sizes), along the ray p0 + t L: the chord is its slab test with o = p0,
 *   d = L (t0 is 0 for a node inside); no chord: S = 1.  n = min(max_steps, ceil(t1 / delta)) (a
 *   quotient that is NaN or inf marches max_steps).  From T = 1, for i < n: t = ((float)i + 0.5f)
 *   delta, the march ends unless t < t1; p = p0 + t L (a multiply, then an add, per component);
 *   rho = the interpolated density at p; s = (scale rho) delta; a step with not s > 0 is skipped;
 *   otherwise T = T - T (s / (1 + s)), and the march ends after a step that leaves T < t_stop.
 *   S = T.  The step opacity is the preview's own, so light and eye see the same medium.
 * Lookup at a world point p: u_a = ((p_a - box_min_a) / e_a) (float)res_a - 0.5f, i_a =
 *   floor(u_a) (as an int, saturating), f_a = u_a - (float)i_a, taps i_a and i_a + 1, each clamped
 *   into [0, res_a - 1] as signed integers; the eight taps interpolate by the trilinear of
 *   CVR_HAS_FEATURES (x, then y, then z).
 * Shadowed preview: the pass of CVR_HAS_PREVIEW with, per contributing sample, S = lookup(p) and
 *   V = 1 - shadow (1 - S), and e replaced:
 *   With CVR_PREVIEW_UNSHADED, or if not m > 0: e_c = V c_c.
 *   Otherwise: L is the light volume's; the descriptor's `light` is neither read nor judged.
 *     f = ambient + (diffuse nl) V,  lit_c = f c_c + (specular sp) V,
 *     e_c = (1 - q) (V c_c) + q lit_c.
 *   w, W, T and the early stop are untouched.  Hence, exactly: shadow = 0 gives cvr_preview's bits
 *   for the same descriptor with `light` set to the light volume descriptor's; the alpha plane is
 *   cvr_preview's for every shadow; every rgb value is at most the one shadow = 0 gives (fp32
 *   multiply and add are monotone and 0 <= V <= 1).
 * The contract on the medium and the independence of the storage are those of CVR_HAS_FEATURES;
 * the build skips, exactly, what the feature pass skips on a sparse medium.
 * cvr_build_light_volume refuses with CVR_ERR_INVALID, in this order: a NULL descriptor; flags
 * other than 0; a res axis of 0 or above 1024, or a product above 2^27; a light that is not
 * finite or whose fp32 length as computed above is 0 or inf; `march` as cvr_features refuses it.
 * No medium: CVR_ERR_STATE.
 * The shadowed preview refuses, in this order: what cvr_preview refuses but for the light;
 * CVR_PREVIEW_HEADLIGHT (shadows need the directional light); a shadow that is not finite or
 * outside [0, 1] (CVR_ERR_INVALID); no light volume, then a stale one (CVR_ERR_STATE).  Every call
 * that replaces or drops the context's medium drops the light volume: cvr_set_medium* (the
 * cvr_set_medium_scene_* calls included), cvr_share_medium, and their failures that leave the
 * context without a medium.  A volume built under another CVR_OPT_WORLD_TO_AABB than the one in
 * force at preview time is stale.
 * The defaults of the bindings and the CLI: res_a = min(256, ceil(medium res_a / 2)), shadow 0.7,
 * march 1, 1/256, 4096.
 * Not supported: ambient occlusion, shadows under the headlight, more than one light, a binary16
 * light volume, partial rebuilds, the environment map as a light, shadows in cvr_features or the
 * path tracer. */
#define CVR_HAS_SHADOWS 1
typedef struct cvr_light_volume_desc {
  uint32_t res[3];
  uint32_t flags; /* 0 */
  float light[3]; /* the direction towards the light, any length */
  float reserved;
  cvr_features_desc march;
} cvr_light_volume_desc; /* 48 bytes */
struct cvr_light_volume_info {
  uint32_t res[3];
  uint32_t valid; /* 1: the context holds a volume of its medium (res, light, bytes are its); else all 0 */
  float light[3]; /* normalised */
  float reserved;
  uint64_t bytes;
}; /* 40 bytes */
/* Host only, no GPU: the written statement on a dense medium's host arrays (as cvr_features_host
 * reads them).  out: res_x * res_y * res_z floats.  A NULL pointer, an empty grid, world_to_aabb
 * other than 0 / 1, and what cvr_build_light_volume refuses: CVR_ERR_INVALID. */
int cvr_light_volume_host(const cvr_medium_desc* medium, int world_to_aabb, const cvr_light_volume_desc* desc,
                          float* out);
/* The light volume of the context's medium (own or shared, any storage), asynchronous on the
 * context's stream, into memory the context owns (also when the medium is shared); it replaces
 * the context's previous volume.  Honours CVR_OPT_EMPTY_MASK as cvr_features does.  Touches
 * neither the medium nor the framebuffer: available between cvr_adaptive_begin and
 * cvr_adaptive_end. */
int cvr_build_light_volume(cvr_ctx* ctx, const cvr_light_volume_desc* desc);
/* The default grid for the context's medium: res_a = min(256, ceil(medium res_a / 2)).  No medium: CVR_ERR_STATE. */
int cvr_light_volume_default_res(const cvr_ctx* ctx, uint32_t res[3]);
int cvr_light_volume_info(const cvr_ctx* ctx, struct cvr_light_volume_info* out);
/* Synchronous.  No valid volume: CVR_ERR_STATE; fewer floats than nodes: CVR_ERR_INVALID. */
int cvr_copy_light_volume(cvr_ctx* ctx, float* host, size_t host_floats);
/* Drops the volume and frees its memory (waits for the context's stream). */
int cvr_clear_light_volume(cvr_ctx* ctx);
/* cvr_preview_host's arguments, the descriptor the volume was made with (cvr_light_volume_host),
 * its array, and the shadow strength. */
int cvr_preview_shadowed_host(const cvr_medium_desc* medium, const float inv_view[12], const float raster_to_view[2],
                              const float full_res[2], uint32_t tile_w, uint32_t tile_h, uint32_t off_x,
                              uint32_t off_y, int world_to_aabb, const cvr_preview_desc* desc,
                              const cvr_light_volume_desc* volume_desc, const float* volume, float shadow,
                              float* out_rgba);
/* cvr_preview_buffers and cvr_preview with the context's light volume: the same destinations and
 * state rules. */
int cvr_preview_shadowed_buffers(cvr_ctx* ctx, const cvr_preview_desc* desc, float shadow, float* d_out_rgba);
int cvr_preview_shadowed(cvr_ctx* ctx, const cvr_preview_desc* desc, float shadow, float* host_rgba,
                         size_t host_floats);

/* ---- field projections (extension within ABI 6: CVR_HAS_FIELD_PROJECT) --- */
/* The two views a volume viewer shows before any transfer table exists, and what a user reads a
 * threshold from (the iso, lo or hi of the classifications): intensity projections of the raw
 * scalar field (maximum: MIP, minimum: MinIP, mean: the X-ray view) and its first-hit isosurface
 * lit by the field's own gradient.  The field is a typed scalar field in device memory
 * (cvr_field_desc); no medium is needed or touched.  Per pixel, one deterministic march along the
 * straight camera ray through the pixel's centre.  Every operation is fp32 +, -, x, /, sqrt in the
 * order written here (correctly rounded, no fused multiply-add but the fma of the trilinear's
 * lerps), so the device kernels and cvr_field_project_host return the same bits (one definition
 * compiles for both, cvr_project.h).
 * Ray, chord and steps are exactly those of CVR_HAS_FEATURES with the descriptor's box as the box
 * and the field's res as res: the ray through the pixel centre, the slab test with its minNum /
 * maxNum rules, delta = step min(min(e_x / res_x, e_y / res_y), e_z / res_z), e = box_max -
 * box_min, n = min(max_steps, ceil((t1 - t0) / delta)), t_i = t0 + ((float)i + 0.5f) delta, a
 * t_i >= t1 is dropped; there is no t_stop.  p_i = o + t_i d (a multiply, then an add).
 * Field value S(p) at a world point p: c_a = ((p_a - box_min_a) / e_a) (float)(res_a - 1): voxel i
 *   sits at node i / (res - 1) of the box, the albedo coordinate of CVR_HAS_FEATURES, geometrically
 *   right for every box (no quirk Q4).  Lower corner floor(c) (saturating, a NaN to INT_MIN),
 *   weights c - corner, the 8 taps clamped as the feature pass clamps its (quirk Q5: an index below
 *   0 wraps and clamps to res - 1), each tap converted to float (exact for the integer types), and
 *   the feature pass's trilinear, lerp(a, b, f) = fma(b, f, a (1 - f)), x then y then z.
 *   The view aligns with cvr_preview of a medium built from the same field in the same box
 *   whenever CVR_OPT_WORLD_TO_AABB is 1 or the box is the unit box at the origin.
 * CVR_PROJECT_MAX: from cnt = 0; for each sample v = S(p_i), a NaN v is skipped; if cnt == 0 or
 *   v > V: V = v, tz = t_i (the first maximum wins); cnt++.  value = V.
 * CVR_PROJECT_MIN: the same with v < V.
 * CVR_PROJECT_MEAN: from Sum = 0: Sum += v, cnt++, a NaN skipped.  value = Sum / (float)cnt, tz = 0.
 * These three: t = (value - lo) / (hi - lo), u = t > 0 ? t : 0, then u = u < 1 ? u : 1 (the
 *   classifications' u); rgba = (u colour_r, u colour_g, u colour_b, 1); depth = tz / diag, diag =
 *   sqrt((e_x e_x + e_y e_y) + e_z e_z).  With cnt == 0 (no chord, or only NaN samples):
 *   rgba = (bg_r, bg_g, bg_b, 0), value 0, depth 0.
 * CVR_PROJECT_ISO: inside(v) is v >= iso (a NaN is not inside).  The hit is the first sample i
 *   with inside(S(p_i)); with none the output is the background, alpha 0, value 0, depth 0.
 *   i = 0: t_hit = t_0 (the cut face, where the box slices the solid).  Otherwise ta = t_(i-1),
 *   tb = t_i, and `refine` times: tm = ta + 0.5f (tb - ta); if inside(S(o + tm d)) tb = tm, else
 *   ta = tm; t_hit = tb.  p = o + t_hit d, value = S(p) (recomputed at p), depth = t_hit / diag.
 *   The gradient is the construction of CVR_HAS_PREVIEW on S: h_a = e_a / res_a,
 *   G_a = (S(p + h_a u_a) - S(p - h_a u_a)) / h_a (six more lookups, clamped taps and all),
 *   m = sqrt((G_x G_x + G_y G_y) + G_z G_z).  If not m > 0: rgb = colour.  Otherwise n = G / m and
 *   L, V, nl, H, hh, nh, the shininess_log2 squarings and sp exactly as CVR_HAS_PREVIEW writes
 *   them (CVR_PROJECT_HEADLIGHT: L = -d; else the light normalised once per call);
 *   f = ambient + diffuse nl, rgb_c = f colour_c + specular sp: no knee.  rgba = (rgb, 1).
 * Refusals, all CVR_ERR_INVALID, in this order:
 *   1. NULL arguments (the context, a descriptor, a camera array of the host call);
 *   2. a zero extent, or more than 2^32 - 1 voxels: from res alone;
 *   3. an unknown scalar_type or mode, unknown flags, or a non-zero reserved (either descriptor's);
 *   4. a box that is not finite or has box_max_a <= box_min_a;
 *   5. step outside [1/8, 8] or max_steps outside 1..65536;
 *   6. the three projections: lo / hi not finite, or hi <= lo;
 *   7. CVR_PROJECT_ISO: iso not finite, refine > 8, or ambient, diffuse, specular, shininess_log2
 *      and (without the headlight) the light as cvr_preview refuses them;
 *   8. a colour or background component that is negative or not finite;
 *   9. a NULL scalar or rgba pointer;
 *  10. a scalar misaligned for its type, an rgba plane not 16-byte aligned (a value or depth plane:
 *      4-byte), or, the device calls, memory that is not device-accessible on the context's device.
 * The tile is judged between 8 and 9 (a zero side or more than 2^24 pixels: CVR_ERR_INVALID; the
 * device calls: host_floats too small likewise).  The device calls return CVR_ERR_STATE without a
 * camera or a resolution, after rule 1.  The field's spacing is not read: the box gives the
 * geometry.  Fields of modes the rule does not name (lo, hi for ISO; iso, refine, the light and
 * the weights for the projections) are neither read nor judged.
 * Like the field calls above, the device calls only borrow the context's device, stream, camera,
 * resolution and offset: they work without a medium and inside an adaptive session and write
 * nothing of the context.  The defaults of the bindings and the CLI: step 1, max_steps 4096,
 * refine 4, the headlight, 0.3 / 0.7 / 0.2, exponent 2^4, a white colour, a black background.
 * Not supported: the context's crop and clip planes, transfer-function colouring of the
 * projection, depth-cued or local MIP, more than one isosurface or translucent surfaces,
 * empty-space skipping (a brick's maximum does not bound a trilinear sample: DESIGN.md), sparse
 * fields, keeping the field, more than one tile or device in the CLI. */
#define CVR_HAS_FIELD_PROJECT 1
enum { CVR_PROJECT_MAX = 0, CVR_PROJECT_MIN = 1, CVR_PROJECT_MEAN = 2, CVR_PROJECT_ISO = 3 };
#define CVR_PROJECT_HEADLIGHT 1u /* ISO: the light shines along the ray, L = -d */
typedef struct cvr_project_desc {
  uint32_t mode;  /* CVR_PROJECT_* */
  uint32_t flags; /* CVR_PROJECT_HEADLIGHT */
  float box_min[3], box_max[3];
  float step;         /* in cells of the finest axis, 1/8..8 */
  uint32_t max_steps; /* 1..65536 */
  float lo, hi;       /* the projections' display window */
  float iso;
  uint32_t refine; /* bisections of the hit's bracket, 0..8 */
  float light[3];  /* the direction towards the light, any length; not read with the headlight */
  float ambient, diffuse, specular;
  uint32_t shininess_log2; /* the specular exponent is 2^shininess_log2, 0..10 */
  float colour[3], background[3];
  uint32_t reserved; /* 0 */
} cvr_project_desc; /* 112 bytes */
/* Host only, no GPU: the written statement on a field in host memory, the camera and tile as
 * cvr_features_host takes them.  out_rgba: tile_w * tile_h * 4 floats; out_value, out_depth:
 * tile_w * tile_h floats each, may be NULL. */
int cvr_field_project_host(const cvr_field_desc* field, const cvr_project_desc* desc, const float inv_view[12],
                           const float raster_to_view[2], const float full_res[2], uint32_t tile_w, uint32_t tile_h,
                           uint32_t off_x, uint32_t off_y, float* out_rgba, float* out_value, float* out_depth);
/* The pass on a field in device memory (or pinned host memory) for the context's camera,
 * resolution and offset, into device memory or the device address of pinned host memory
 * (d_out_value, d_out_depth may be NULL), asynchronous on the context's stream: the field must
 * stay until the stream has run it. */
int cvr_field_project_buffers(cvr_ctx* ctx, const cvr_field_desc* field, const cvr_project_desc* desc,
                              float* d_out_rgba, float* d_out_value, float* d_out_depth);
/* The same into host memory (host_rgba: tile_w * tile_h * 4 floats, host_floats smaller:
 * CVR_ERR_INVALID; host_value, host_depth: tile_w * tile_h floats or NULL).  Synchronous: the
 * field may be freed when it returns.  Pinned or registered memory is stored into by the kernel,
 * other memory (host_rgba not 16-byte aligned included) through a staging copy. */
int cvr_field_project(cvr_ctx* ctx, const cvr_field_desc* field, const cvr_project_desc* desc, float* host_rgba,
                      float* host_value, float* host_depth, size_t host_floats);

/* ---- which wave-pool kernel instance ran (tests; extension within ABI 6: CVR_HAS_WPOOL_DEBUG) -- */
/* The wave pool (CVR_OPT_SCHEDULER 3) is one kernel compiled once per combination of scatter
 * offset, register budget, medium layout and feature.  An instance is five ints:
 *   [0] 1: a scatter's origin is moved back by eps (every kernel id but regenerationSK);
 *   [1] waves per SIMD (CVR_OPT_WAVES: 3, 4, 5 or 6);
 *   [2] the medium: layout 0 any dense medium, 1 sparse, 2 dense with cells and bounds, 3 the same
 *       with a uniform albedo; or-ed with 4 naiveMK's walk, 8 CVR_OPT_COUNT_WORDS, 16 the half
 *       format, 32 CVR_OPT_MOMENTS, 64 an environment map;
 *   [3] 1: cvr_trace_launch's records;  [4] 1: cvr_render_frame's in-launch output. */
#define CVR_HAS_WPOOL_DEBUG 1
/* Debug, host only (no device is needed): the instances the library ships.  *count receives their
 * number; the first min(capacity, *count) are written to rows, five ints each (rows may be NULL
 * when capacity is 0, so a first call asks for the count). */
int cvr_debug_wpool_rows(int32_t* rows, uint32_t capacity, uint32_t* count);
/* Debug: the instance the context's last wave-pool launch ran (cvr_launch_render, cvr_trace_launch,
 * cvr_render_frame and every other call that renders on this context) and that launch's grid in
 * waves.  Written once the launch is enqueued; a launch that fails, an empty launch and a launch
 * of another scheduler leave it as it was.  No wave-pool launch yet: CVR_ERR_STATE. */
int cvr_debug_last_wpool(const cvr_ctx* ctx, int32_t instance[5], uint32_t* grid_waves);
#endif /* CVR_ABI_VERSION >= 6 */

/* Pinned, device-mapped host memory for cvr_render_share_to_host /
 * cvr_render_frame's in-launch output (hipHostMalloc, mapped + portable: every
 * device can store into it), and its release. */
int cvr_host_alloc(size_t bytes, void** out);
int cvr_host_free(void* p);

/* ---- camera / tiling helpers ------------------------------------------ */
/* Default Camera (Camera.h:25-71, MITSUBA_COMPARABLE) after
 * setResolution(w,h), flattened as CudaVolPath::initCamera (CudaVolPath.cpp:67-85). */
int cvr_default_camera(uint32_t width, uint32_t height, float inv_view[12], float raster_to_view[2]);
/* TilingConfig (Config.h:61-78) + initTileArray (CudaVolPath.cpp:13-29). */
int cvr_tiling(uint32_t width, uint32_t height, uint32_t ntx, uint32_t nty, uint32_t tile_dim[2]);
int cvr_tile_origin(uint32_t tile_id, uint32_t ntx, const uint32_t tile_dim[2], uint32_t origin[2]);

/* ---- scenes (SceneBuilder family, Scene.h:56-81) ----------------------- */
/* Load a scene file: Raw (RawSceneBuilder.h), Vdb (VDBSceneBuilder.h), Mhd
 * (convert-mhd semantics), MitsubaXml.  AUTO picks by extension
 * (ConfigParser.cpp:79-97). */
int cvr_scene_load(const char* path, int scene_type, cvr_scene** out);
/* Extension: cvr_scene_load with options.  CVR_LOAD_DEFAULT_ALBEDO (quirk
 * Q17's flag): a VDB file without an "albedo" grid, which the reference
 * refuses (VDBAdapter.cpp:32-37), loads with albedo (r,g,b) everywhere, as
 * the dense grid or, sparse, as leaves without albedo over that background
 * (a wdas_cloud-style density-only file); files with an albedo grid are read
 * as before.  opts may be NULL (= cvr_scene_load). */
enum { CVR_LOAD_DEFAULT_ALBEDO = 1 };
typedef struct cvr_load_options {
  uint32_t flags;
  float default_albedo[3];
} cvr_load_options;
int cvr_scene_load_ex(const char* path, int scene_type, const cvr_load_options* opts, cvr_scene** out);
/* Synthetic proxies for the missing data blobs:
 * "bucky" (32^3 raw), "manix" (256x230x256 VDB-like), "hetvol" (128x128x50),
 * "cloud" (C5: sparse fBm cumulus in a 2048x1024x2048 index box, albedo
 * (1,1,1), stored sparse only).  dims may be NULL (default size). */
int cvr_scene_synthetic(const char* name, uint32_t seed, const uint32_t* dims, cvr_scene** out);
/* Medium description; pointers stay owned by the scene. */
int cvr_scene_medium(const cvr_scene* scene, cvr_medium_desc* out);
/* Sparse view of a scene: sparse scenes (the "cloud" proxy) are stored as
 * leaves; a dense scene is converted once (leaves holding any non-zero
 * density or an albedo other than the voxel (0,0,0)'s, which becomes the
 * background) and the leaves are kept in the scene.  Pointers stay valid
 * while the scene lives.  Dense scenes: cvr_scene_medium; a sparse scene has
 * no dense view (CVR_ERR_UNSUPPORTED). */
int cvr_scene_sparse_medium(cvr_scene* scene, cvr_sparse_medium_desc* out);
/* 1 if the scene is stored sparse only. */
int cvr_scene_is_sparse(const cvr_scene* scene);
/* The scene's camera at a render resolution: the fixed eye and orientation
 * of Camera.h:25-45 with the scene's horizontal fov (0.7 degrees for VDB,
 * Raw and MHD scenes; the XML sensor's fov, default 45, for Mitsuba scenes,
 * XmlSceneBuilder.h:120-150). */
int cvr_scene_camera(const cvr_scene* scene, uint32_t width, uint32_t height, float inv_view[12],
                     float raster_to_view[2]);
int cvr_scene_raw_bytes(const cvr_scene* scene, const uint8_t** bytes, size_t* n);
void cvr_scene_destroy(cvr_scene* scene);
/* Radiance RGBE .hdr of an RGBA float image (Image::saveHDR, Image.cpp:58-62). */
int cvr_write_hdr(const char* path, const float* rgba, uint32_t width, uint32_t height);
/* Kernel name <-> id (Config.h:210-213); unknown -> CVR_KERNEL_UNKNOWN. */
int cvr_kernel_from_name(const char* name);
const char* cvr_kernel_name(int kernel);

#ifdef __cplusplus
}
#endif
#endif /* CVR_H_ */
