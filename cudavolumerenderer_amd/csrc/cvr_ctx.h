// cvr_ctx.h - the context behind the C ABI's cvr_ctx handle and what its call sites need with it
// (internal: the cvr_*.cpp sources of the library; what the launch path shares is in cvr_host.h).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "cvr.h"
#include "cvr_env.h"
#include "cvr_kernels.h"

namespace cvr {
// The launcher settings a helper context of cvr_render_frame takes from its parent in one assignment
// (cvr_frame.cpp copy_settings): a setting declared here travels to the helpers, so the bands of one
// frame render under the same settings.  Resources (streams, buffers, caches, the grids computed at
// init) and what a helper must not take are members of cvr_ctx itself.
struct Settings {
  // the parent's medium (re-shared every frame: the parent may have loaded another)
  cvr::MediumParams m{};
  size_t n_cell_leaves = 0;  // cell-leaf pool slots (incl. the zero slot)
  bool have_medium = false;

  // launcher state (the reference's __constant__ symbols)
  float inv_view[12] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 100};
  float r2v[2] = {0, 0};
  float full_res[2] = {0, 0};
  bool have_camera = false;
  uint32_t tile_w = 0, tile_h = 0;
  uint32_t off[2] = {0, 0};
  uint32_t iterations = 1;
  uint64_t n_paths = 0;
  uint64_t range_first = 0, range_count = UINT64_MAX;
  uint32_t shard_rank = 0, shard_world = 1;  // cvr_set_block_shard
  uint32_t seed = 0;

  uint32_t n_queues = 8;            // work-order bands (one per XCD)
  uint32_t subqueues = 8;           // wave pool: queues per band (CVR_OPT_SUBQUEUES)
  int drain = -1;                   // wave pool: drain-mode event trigger (CVR_OPT_DRAIN; -1 = 1)
  int order = 2;                    // 1: pixel-block/sample-inner order when the launch allows it; 2: blocks
                                    // in 2-D Morton order within each band

  // options
  uint32_t max_segments = 1u << 20;
  uint32_t chunk = 0;  // paths per wave dequeue; 0: auto (wave pool: 64..256 by the launch's size, others 256)
  uint32_t ev_thresh = 56;
  uint32_t grid_override = 0;
  uint32_t inflight = 1;  // CVR_OPT_INFLIGHT: renders the caller keeps in flight (wave-pool grid rule)
  int scatter_eps = -1;
  int rng_binding = 0;  // CVR_OPT_RNG_BINDING
  int world_to_aabb = 0;  // CVR_OPT_WORLD_TO_AABB (Q4)
  int mk_compaction = 0;  // CVR_OPT_MK_COMPACTION (Q11)

  uint32_t pool_tail = 16;
  // wave-pool register/LDS budget in waves per SIMD (CVR_OPT_WAVES: 3, 4, 5);
  // 0 = the default, 5 (dense and sparse, split slots)
  int wpool_waves = 0;
  int morton = 0;  // CVR_OPT_MORTON
  int sample_order = -1;  // CVR_OPT_SAMPLE_ORDER (-1: the default, 0)
  int empty_mask = 1;     // CVR_OPT_EMPTY_MASK
  int count_words = 0;    // CVR_OPT_COUNT_WORDS
  uint32_t swap_batch = 8;
  int scheduler = -1;  // 0 persistent, 1 wavefront pair, 2 workgroup pool, 3 wave-private pool, -1 per kernel id
  int waves = 4;      // persistent kernel register budget (waves per SIMD)
  uint32_t pool_max = 1u << 21;  // CVR_OPT_POOL: the wavefront pool's slots at most
};
}  // namespace cvr

struct cvr_ctx : cvr::Settings {
  int device = 0;
  int kernel = CVR_KERNEL_REGENERATION_SK;
  std::string err;

  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  bool timed = false;

  // medium in HBM
  float* d_density = nullptr;
  float4* d_albedo = nullptr;
  float4* d_cells = nullptr;  // corner-replicated density (MediumParams::cells)
  // Not in Settings on purpose: use_cells, uniform_albedo, bound_shift and medium_format take effect
  // at the next medium upload, and a helper shares its parent's medium as built.
  bool use_cells = true;
  bool uniform_albedo = true;  // CVR_OPT_UNIFORM_ALBEDO
  uint8_t* d_bounds = nullptr;  // brick bounds (MediumParams::bounds)
  uint32_t bound_shift = 2;     // log2 brick size, 0 = off
  bool bound_shift_set = false; // CVR_OPT_BOUNDS given (else sparse media use 8^3 bricks)
  size_t n_voxels = 0;
  uint32_t grids_format = 0;  // format d_density / d_albedo were allocated for
  // sparse medium (cvr_set_medium_sparse)
  uint32_t* d_leaves = nullptr;
  float* d_leaf_density = nullptr;
  float4* d_leaf_albedo = nullptr;
  uint32_t* d_sbounds = nullptr;
  uint32_t* d_emask = nullptr;       // empty-region mask (MediumParams::emask)
  uint32_t* d_block_perm = nullptr;  // cvr_set_block_order
  uint32_t block_perm_n = 0;
  int medium_format = 0;     // CVR_OPT_MEDIUM_FORMAT (the next set-medium's; the medium's own is m.format)
  struct cvr_medium_info minfo{};  // cvr_medium_info of the medium in use (own or shared)
  // cvr_set_clip: taken at the next device build (not in Settings, as use_cells above); and what
  // the medium in use (own or shared) was built under, cvr_medium_clip_info's
  bool clip_set = false;
  cvr_clip_desc clip{};
  bool medium_clipped = false;
  cvr_clip_desc medium_clip{};
  uint64_t medium_kept = 0;
  // cvr_medium_label_info's: the rows of the table the medium in use (own or shared) was built
  // with by cvr_set_medium_labeled (0: by another call) and the kept voxels per label byte
  uint32_t medium_label_rows = 0;
  uint64_t medium_label_counts[256] = {};

  // Not in Settings on purpose: external_out here, and frame_flush, moments and wf_timing below.  A
  // helper always renders into its parent's buffer, without moments, in-launch output or timing.
  float4* d_out_owned = nullptr;
  size_t out_owned_px = 0;
  float4* d_out = nullptr;  // active output (owned or external)
  bool external_out = false;

  unsigned char* d_work = nullptr;  // queue heads + stats counters (kWork* layout)
  float4* d_pool_T = nullptr;       // wave-pool scheduler: event-only slot part (LaunchParams::pool_T)
  unsigned char* d_smk = nullptr;   // thread-bound streamingMK: slot buffers, flags, RNG states, counters
  size_t smk_n = 0;                 // threads d_smk is carved for
  size_t pool_T_n = 0;
  // cached Morton permutation of the launch's blocks (order 2), for the block layout in zkey
  uint32_t* d_zperm = nullptr;
  std::vector<uint32_t> h_zperm;
  uint64_t zkey[5] = {0, 0, 0, 0, 0};

  int cu_count = 0;
  int persistent_grid = 0;
  int pool_grid = 0;
  int wpool_grid = 0, wpool_grid_sparse = 0;
  int track_grid = 0;
  bool inited = false;

  // wavefront pool (cvr_wavefront.hip)
  unsigned char* d_pool = nullptr;
  size_t pool_bytes = 0;
  uint32_t pool_cap = 0;  // slots the allocation holds
  cvr::WfPool pool{};
  unsigned int* h_alive = nullptr;  // pinned ring of per-iteration flags
  std::vector<hipEvent_t> it_events;
  uint64_t last_iterations = 0;
  double last_track_ms = 0, last_events_ms = 0;
  bool wf_timing = false;
  // cvr_set_medium_device with CVR_OPT_TIMING: device ms of its last call's density scan, albedo
  // scan, leaf flags, scans and scatters, gather, and cells / bounds / brick words
  double devmed_ms[6] = {0, 0, 0, 0, 0, 0};

  cvr_stats last{};

  // cvr_render_frame: the helper contexts that render the frame's other bands (each with its own
  // stream and work queues, sharing this context's medium and framebuffer), the copy stream, and
  // the normalised device image the bands are copied from
  std::vector<cvr_ctx*> frame_kids;
  hipStream_t frame_copy = nullptr;
  hipEvent_t frame_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // [0] cleared, [1 + k] band k rendered
  float4* d_frame = nullptr;
  size_t frame_px = 0;
  // cvr_render_frame's in-launch output (CVR_OPT_FRAME_FLUSH, wave pool): [FrameFlush
  // header | per-block ended-path counts], the flushers' status words (pinned), the
  // header as last written
  int frame_flush = 1;
  unsigned char* d_flush = nullptr;
  size_t flush_blocks = 0;
  unsigned int* h_flush_status = nullptr;
  cvr::FrameFlush flush_hdr{};
  bool flush_hdr_valid = false;  // d_flush holds flush_hdr
  uint32_t flush_last_blocks = 0, flush_fallbacks = 0;
  // cvr_debug_last_wpool: the instance and the grid (in waves) of the last wave-pool launch that was enqueued
  bool last_wpool_valid = false;
  cvr::WpoolInstance last_wpool{};
  uint32_t last_wpool_grid = 0;

  // CVR_OPT_MOMENTS: the owned framebuffer holds a second float4 per pixel behind the tile
  int moments = 0;
  // The active block list (cvr_adaptive_*): while active_on, a launch renders exactly the tile
  // blocks of `active` (ascending ids), n_blocks = its length; d_active holds them in the
  // launch's order (each XCD band in 2-D Morton order), h_active the same on the host.
  bool active_on = false;
  std::vector<uint32_t> active, h_active;
  uint32_t* d_active = nullptr;  // tile_px / 64 entries
  // the adaptive session
  struct Adaptive {
    bool on = false;        // between cvr_adaptive_begin and cvr_adaptive_end
    cvr_adaptive_desc d{};
    uint32_t n_blocks = 0, passes = 0;
    int done = 0;
    uint64_t paths = 0;
    std::vector<uint32_t> samples;  // per tile block
    std::vector<double> err;        // per tile block, at its last check
    std::vector<double> h_err;      // the last pass's errors, in h_active order
    double* d_err = nullptr;        // tile_px / 64 doubles
    uint32_t* d_counts = nullptr;   // tile_px / 64 sample counts (cvr_adaptive_image)
    int saved_moments = 0;
    uint32_t saved_iterations = 1;
    cvr_stats acc{};
  } ad;
  // cvr_denoise*: the two scratch images the passes alternate between (dn_px pixels each)
  float4* d_dn = nullptr;
  size_t dn_px = 0;
  // cvr_denoise_guided: the feature planes of its own pass, feat_px float4 then feat_px floats
  float4* d_feat = nullptr;
  size_t feat_px = 0;
  // cvr_set_environment: the context's own stored texels, the header as the kernels read it
  // (device memory, 64 bytes: LaunchParams::rec of the kMedEnv instances) and its host copy
  bool have_env = false;
  cvr::EnvParams env{};
  cvr::EnvParams* d_env_hdr = nullptr;
  float env_max = 0.0f;  // the largest stored component
  // cvr_build_light_volume: the context's own light volume (its own also when the medium is
  // shared) and its record: the grid, the light as given and normalised, and the
  // CVR_OPT_WORLD_TO_AABB it was built under.  The allocation is kept when the volume is dropped.
  float* d_lightvol = nullptr;
  size_t lightvol_floats = 0;  // floats the allocation holds
  struct LightVol {
    bool valid = false;
    uint32_t res[3] = {0, 0, 0};
    float light[3] = {0, 0, 0}, L[3] = {0, 0, 0};
    int world_to_aabb = 0;
  } lightvol;
};

namespace cvr {
// The thread's last-error text, and *dst when given, become the formatted message; returns code.
int set_err(std::string* dst, int code, const char* fmt, ...);
int ensure_device(cvr_ctx* c);
// The context's own medium buffers, freed and reset: the sparse medium's five, the dense medium's four grids.
void free_sparse(cvr_ctx* c);
void drop_dense(cvr_ctx* c);
// p is memory the context's device can read, by what the runtime knows of it
bool device_readable(const cvr_ctx* c, const void* p);
// The context's environment map and its device header, freed and reset (cvr_environment.cpp)
void free_environment(cvr_ctx* c);
// The feature pass (cvr_features_api.cpp) for the context's medium, camera and tile: what the
// entry points check (state, descriptor, tile), and the launch on the context's stream
int features_check(cvr_ctx* c, const cvr_features_desc* d);
int features_launch(cvr_ctx* c, const cvr_features_desc* d, float4* rgba, float* depth);
// Its parts, for the passes that march as it does (cvr_preview_api.cpp): the descriptor's and the
// tile's checks (err may be null), the camera and tile of a FeatureParams, and the whole
// FeatureParams of a context that features_check has passed
struct FeatureParams;
int features_desc_check(std::string* err, const cvr_features_desc* d);
int features_tile_check(std::string* err, uint32_t w, uint32_t h);
void features_set_view(FeatureParams& P, const float inv_view[12], const float r2v[2], const float full_res[2],
                       uint32_t tile_w, uint32_t tile_h, uint32_t off_x, uint32_t off_y);
FeatureParams features_ctx_params(const cvr_ctx* c, const cvr_features_desc* d);
// The preview pass's (cvr_preview_api.cpp), for the pass that shadows it (cvr_shadow_api.cpp): the
// descriptor's own fields in cvr.h's order (err may be null; check_light 0: the light is not
// read, so not judged), and a PreviewParams' shading constants for a light (Q.F is filled)
struct PreviewParams;
int preview_shading_check(std::string* err, const cvr_preview_desc* d, bool check_light);
void preview_set_shading(PreviewParams& Q, const cvr_preview_desc* d, const float light[3], float max_density);
// The light volume is no longer the medium's: every call that replaces or drops the context's
// medium calls this (the allocation stays for the next build; cvr_clear_light_volume frees it)
inline void drop_light_volume(cvr_ctx* c) { c->lightvol.valid = false; }
// f32 -> binary16 -> f32, round to nearest even, subnormals kept (CVR_OPT_MEDIUM_FORMAT 1)
float half_round1(float f);
// first finite value of v[0..n) (of every `stride`-th group's first `take` values) that rounds to +-inf
bool half_overflows(const float* v, size_t n, size_t stride, size_t take, size_t* at);
// the format-1 majorant: max(max_density, f32(f16(max_density))), max_density itself if that overflows
float half_majorant(float max_density);
}  // namespace cvr

// Calls that are out of order inside an adaptive session.
#define CVR_NOT_IN_SESSION(c, what)                                                                       \
  do {                                                                                                    \
    if ((c)->ad.on)                                                                                       \
      return cvr::set_err(&(c)->err, CVR_ERR_STATE, "%s inside an adaptive session (cvr_adaptive_end first)", what); \
  } while (0)

#define HIP_TRY(ctx, expr)                                                                         \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return cvr::set_err((ctx) ? &(ctx)->err : nullptr, CVR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
