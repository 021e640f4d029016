// cvr_api.cpp - C ABI implementation: contexts (kernel launchers) and their setters, stats, copies
// and traces, camera/tiling helpers (the launch: cvr_launch.cpp; the tile loop and the frame:
// cvr_frame.cpp; adaptive sessions: cvr_adaptive.cpp; the denoiser: cvr_denoise_api.cpp; the
// medium: cvr_medium.cpp).
//
// Reference map:
//   RenderKernelLauncher / VolPTKernelLauncher  RenderKernelLauncher.h:20-174,
//                                                RenderKernelLauncher.cu:86-361
//   Camera + initCamera                          Camera.h:25-71, CudaVolPath.cpp:67-85
//   TilingConfig + initTileArray                 Config.h:61-78, CudaVolPath.cpp:13-29
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cvr_host.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace cvr {
int set_err(std::string* dst, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  if (dst) *dst = buf;
  return code;
}

int ensure_device(cvr_ctx* c) {
  HIP_TRY(c, hipSetDevice(c->device));
  return CVR_OK;
}

void set_last_error(const std::string& msg) { g_last_error = msg; }

// Camera(res, fov_x) then setResolution(w, h) -> setFovFromX (Camera.h:25-71),
// and CudaVolPath::initCamera's rows of the model view (CudaVolPath.cpp:67-85).
void camera_for_fov(float fov_x, uint32_t w, uint32_t h, float inv_view[12], float r2v[2]) {
  const float fov_y = ((float)h / (float)w) * fov_x;
  r2v[0] = tanf(fov_x * CVR_PI_F / 360.f);
  r2v[1] = tanf(fov_y * CVR_PI_F / 360.f);
  // glm column-major model view: col0 right (1,0,0,0) [MITSUBA_COMPARABLE],
  // col1 up (0,-1,0,0), col2 view (0,0,-1,0), col3 position (0,0,100,1);
  // initCamera takes rows of its transpose's first three rows.
  const float mv[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 100.0f, 1};
  const int idx[12] = {0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14};
  for (int i = 0; i < 12; ++i) inv_view[i] = mv[idx[i]];
}
}  // namespace cvr

using cvr::check_ready;
using cvr::do_init;
using cvr::ensure_device;
using cvr::ensure_output;
using cvr::set_err;
using cvr::kWorkDebug;
using cvr::kWorkStats;
// d_work layout: cvr_kernels.h (stats, debug counters, queue heads)
constexpr size_t kWorkBytes = cvr::kWorkBytesBase;

static bool kernel_supported(int k) { return k >= 0 && k < CVR_KERNEL_UNKNOWN; }

namespace cvr {
int ensure_output(cvr_ctx* c) {
  if (c->external_out) return CVR_OK;
  const size_t px = (size_t)c->tile_w * c->tile_h;
  if (px == 0) return set_err(&c->err, CVR_ERR_STATE, "resolution not set");
  // CVR_OPT_MOMENTS: a second float4 per pixel behind the tile (out_owned_px: float4 allocated)
  const size_t need = c->moments ? 2 * px : px;
  if (c->out_owned_px < need) {
    // the old framebuffer may still be written by a launch in flight
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_out_owned) (void)hipFree(c->d_out_owned);
    c->d_out_owned = nullptr;
    c->out_owned_px = 0;
    HIP_TRY(c, hipMalloc(&c->d_out_owned, need * sizeof(float4)));
    HIP_TRY(c, hipMemsetAsync(c->d_out_owned, 0, need * sizeof(float4), c->stream));
    c->out_owned_px = need;
  }
  c->d_out = c->d_out_owned;
  return CVR_OK;
}

int check_ready(cvr_ctx* c) {
  if (!c->have_medium) return set_err(&c->err, CVR_ERR_STATE, "medium not set (cvr_set_medium)");
  if (!c->have_camera) return set_err(&c->err, CVR_ERR_STATE, "camera not set (cvr_set_camera)");
  if (c->tile_w == 0 || c->tile_h == 0) return set_err(&c->err, CVR_ERR_STATE, "resolution not set");
  return CVR_OK;
}

// Per-tile seed advance (RenderKernelLauncher.cu): RegenerationVolPTsk and
// StreamingVolPTmk add n_paths per reset (:359, :480), StreamingVolPTsk and
// SortingVolPTsk add 1 (:573, :664), NaiveVolPTsk and NaiveVolPTmk keep it.
// Returns the seed after `resets` resets starting from `seed` (u32 wrap).
uint32_t seed_after_resets(const cvr_ctx* c, uint32_t seed, uint32_t resets) {
  if (c->kernel == CVR_KERNEL_REGENERATION_SK || c->kernel == CVR_KERNEL_STREAMING_MK)
    return seed + (uint32_t)c->n_paths * resets;
  if (c->kernel == CVR_KERNEL_STREAMING_SK || c->kernel == CVR_KERNEL_SORTING_SK) return seed + resets;
  return seed;
}

int check_host_floats(cvr_ctx* c, size_t host_floats, uint32_t w, uint32_t h, const char* what) {
  const size_t need = (size_t)w * h * 4u;
  if (host_floats < need)
    return set_err(&c->err, CVR_ERR_INVALID, "host image holds %zu floats, the %ux%u %s needs %zu", host_floats, w, h,
                   what, need);
  return CVR_OK;
}

void add_stats(cvr_stats& acc, const cvr_stats& s, unsigned fields) {
  acc.paths += s.paths;
  acc.segments += s.segments;
  acc.steps += s.steps;
  acc.density += s.density;
  acc.albedo += s.albedo;
  acc.escaped += s.escaped;
  acc.truncated += s.truncated;
  acc.fetches += s.fetches;
  if (fields & kStatWords) acc.words += s.words;
  if (fields & kStatKernelMs) acc.kernel_ms += s.kernel_ms;
}
}  // namespace cvr

extern "C" {

int cvr_abi_version(void) { return CVR_ABI_VERSION; }

const char* cvr_last_error(const cvr_ctx* ctx) {
  if (ctx && !ctx->err.empty()) return ctx->err.c_str();
  return g_last_error.c_str();
}

int cvr_create(int device, int kernel, cvr_ctx** out) {
  if (!out) return set_err(nullptr, CVR_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (kernel < 0 || kernel >= CVR_KERNEL_UNKNOWN)
    return set_err(nullptr, CVR_ERR_INVALID, "unknown kernel id %d", kernel);
  if (!kernel_supported(kernel))
    return set_err(nullptr, CVR_ERR_UNSUPPORTED, "kernel %s is not implemented yet", cvr_kernel_name(kernel));
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return set_err(nullptr, CVR_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= ndev) return set_err(nullptr, CVR_ERR_INVALID, "device %d out of range", device);
  cvr_ctx* c = new cvr_ctx();
  c->device = device;
  c->kernel = kernel;
  auto fail = [&](const char* what, hipError_t err) {
    int r = set_err(nullptr, CVR_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
    cvr_destroy(c);
    return r;
  };
  if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess)
    return fail("hipStreamCreate", e);
  c->stream = c->own_stream;
  if ((e = hipEventCreate(&c->ev_start)) != hipSuccess) return fail("hipEventCreate", e);
  if ((e = hipEventCreate(&c->ev_stop)) != hipSuccess) return fail("hipEventCreate", e);
  if ((e = hipMalloc(&c->d_work, kWorkBytes)) != hipSuccess) return fail("hipMalloc(work)", e);
  // stats words: [64,128) single-kernel launches / wavefront events, [128,192) wavefront track
  if ((e = hipMemset(c->d_work, 0, kWorkBytes)) != hipSuccess) return fail("hipMemset(work)", e);
  *out = c;
  return CVR_OK;
}

int cvr_destroy(cvr_ctx* c) {
  if (!c) return CVR_OK;
  (void)hipSetDevice(c->device);
  // the frame helpers first: their launches read this context's medium and framebuffer
  for (cvr_ctx* k : c->frame_kids) cvr_destroy(k);
  c->frame_kids.clear();
  if (c->frame_copy) (void)hipStreamSynchronize(c->frame_copy);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  cvr::drop_dense(c);
  cvr::free_sparse(c);
  cvr::free_environment(c);
  if (c->d_out_owned) (void)hipFree(c->d_out_owned);
  if (c->d_work) (void)hipFree(c->d_work);
  if (c->d_pool_T) (void)hipFree(c->d_pool_T);
  if (c->d_smk) (void)hipFree(c->d_smk);
  if (c->d_block_perm) (void)hipFree(c->d_block_perm);
  if (c->d_zperm) (void)hipFree(c->d_zperm);
  if (c->d_active) (void)hipFree(c->d_active);
  if (c->ad.d_err) (void)hipFree(c->ad.d_err);
  if (c->ad.d_counts) (void)hipFree(c->ad.d_counts);
  if (c->d_dn) (void)hipFree(c->d_dn);
  if (c->d_feat) (void)hipFree(c->d_feat);
  if (c->d_lightvol) (void)hipFree(c->d_lightvol);
  if (c->ev_start) (void)hipEventDestroy(c->ev_start);
  if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  if (c->d_pool) (void)hipFree(c->d_pool);
  if (c->h_alive) (void)hipHostFree(c->h_alive);
  for (auto& e : c->it_events) (void)hipEventDestroy(e);
  for (auto& e : c->frame_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->frame_copy) (void)hipStreamDestroy(c->frame_copy);
  if (c->d_frame) (void)hipFree(c->d_frame);
  if (c->d_flush) (void)hipFree(c->d_flush);
  if (c->h_flush_status) (void)hipHostFree(c->h_flush_status);
  delete c;
  return CVR_OK;
}

int cvr_set_camera(cvr_ctx* c, const float inv_view[12], const float r2v[2], const float full_res[2]) {
  if (!c || !inv_view || !r2v || !full_res) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_camera");
  memcpy(c->inv_view, inv_view, sizeof(c->inv_view));
  c->r2v[0] = r2v[0];
  c->r2v[1] = r2v[1];
  c->full_res[0] = full_res[0];
  c->full_res[1] = full_res[1];
  c->have_camera = true;
  return CVR_OK;
}

int cvr_set_resolution(cvr_ctx* c, uint32_t w, uint32_t h) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_resolution");
  if (w == 0 || h == 0) return set_err(&c->err, CVR_ERR_INVALID, "zero tile resolution");
  if ((uint64_t)w * h > (1ull << 24))
    return set_err(&c->err, CVR_ERR_INVALID, "tile of %ux%u exceeds 2^24 pixels (float pixel indexing)", w, h);
  if ((uint64_t)w * h * c->iterations > 0xFFFFFFFFull)
    return set_err(&c->err, CVR_ERR_INVALID, "n_paths = %llu exceeds the reference's uint32 path ids",
                   (unsigned long long)((uint64_t)w * h * c->iterations));
  c->tile_w = w;
  c->tile_h = h;
  c->n_paths = (uint64_t)w * h * c->iterations;
  return ensure_output(c);
}

int cvr_get_resolution(const cvr_ctx* c, uint32_t* w, uint32_t* h) {
  if (!c || !w || !h) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  *w = c->tile_w;
  *h = c->tile_h;
  return CVR_OK;
}

int cvr_set_offset(cvr_ctx* c, uint32_t x, uint32_t y) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_offset");
  c->off[0] = x;
  c->off[1] = y;
  return CVR_OK;
}

int cvr_set_iterations(cvr_ctx* c, uint32_t it) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_iterations");
  const uint64_t np = (uint64_t)c->tile_w * c->tile_h * it;
  if (np > 0xFFFFFFFFull)
    return set_err(&c->err, CVR_ERR_INVALID, "n_paths = %llu exceeds the reference's uint32 path ids",
                   (unsigned long long)np);
  c->iterations = it;
  c->n_paths = np;
  return CVR_OK;
}

int cvr_set_path_range(cvr_ctx* c, uint64_t first, uint64_t count) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_path_range");
  c->range_first = first;
  c->range_count = count;
  return CVR_OK;
}

int cvr_set_block_shard(cvr_ctx* c, uint32_t rank, uint32_t world) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_block_shard");
  if (world == 0 || rank >= world) return set_err(&c->err, CVR_ERR_INVALID, "bad shard %u of %u", rank, world);
  c->shard_rank = rank;
  c->shard_world = world;
  return CVR_OK;
}

int cvr_set_block_order(cvr_ctx* c, const uint32_t* perm, uint32_t n) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (c->d_block_perm) (void)hipFree(c->d_block_perm);
  c->d_block_perm = nullptr;
  c->block_perm_n = 0;
  if (!perm || n == 0) return CVR_OK;  // natural order
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (perm[i] >= n || seen[perm[i]])
      return set_err(&c->err, CVR_ERR_INVALID, "block order is not a permutation of [0, %u)", n);
    seen[perm[i]] = 1;
  }
  int r = ensure_device(c);
  if (r) return r;
  HIP_TRY(c, hipMalloc(&c->d_block_perm, (size_t)n * sizeof(uint32_t)));
  HIP_TRY(c, hipMemcpy(c->d_block_perm, perm, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->block_perm_n = n;
  return CVR_OK;
}


int cvr_set_seed(cvr_ctx* c, uint32_t seed) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_seed");
  c->seed = seed;
  return CVR_OK;
}

int cvr_get_seed(const cvr_ctx* c, uint32_t* seed) {
  if (!c || !seed) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  *seed = c->seed;
  return CVR_OK;
}

int cvr_set_output(cvr_ctx* c, void* p) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_output");
  if (p) {
    if (c->moments)
      return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                     "a caller's output buffer does not run with second moments (CVR_OPT_MOMENTS 1): the moments lie "
                     "behind the tile in the context's own allocation");
    c->d_out = static_cast<float4*>(p);
    c->external_out = true;
    return CVR_OK;
  }
  c->external_out = false;
  if (c->tile_w && c->tile_h) return ensure_output(c);
  c->d_out = nullptr;
  return CVR_OK;
}

void* cvr_output_ptr(cvr_ctx* c) { return c ? c->d_out : nullptr; }

int cvr_set_stream(cvr_ctx* c, void* s) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_stream");
  const hipStream_t next = static_cast<hipStream_t>(s);  // NULL = the device's null stream
  if (next != c->stream) {
    // the work queues, the wave-pool scratch, the filter's images and the light volume are
    // single-stream state: what is pending on the stream being left ends before the next call
    // starts on the new one
    int r = ensure_device(c);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->stream = next;
  return CVR_OK;
}

void* cvr_own_stream(cvr_ctx* c) { return c ? (void*)c->own_stream : nullptr; }

int cvr_set_option(cvr_ctx* c, int opt, int64_t v) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_option");
  switch (opt) {
    case CVR_OPT_MAX_SEGMENTS:
      if (v < 0) return set_err(&c->err, CVR_ERR_INVALID, "max_segments < 0");
      c->max_segments = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_CHUNK:
      if (v < 1 || v > (1 << 20)) return set_err(&c->err, CVR_ERR_INVALID, "chunk out of range");
      c->chunk = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_EVENT_THRESHOLD:
      if (v < 1 || v > 64) return set_err(&c->err, CVR_ERR_INVALID, "event threshold must be 1..64");
      c->ev_thresh = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_GRID:
      if (v < 0) return set_err(&c->err, CVR_ERR_INVALID, "grid < 0");
      c->grid_override = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_SCHEDULER:
      if (v < 0 || v > cvr::kSchedPerItem) return set_err(&c->err, CVR_ERR_INVALID, "scheduler must be 0..4");
      c->scheduler = (int)v;
      return CVR_OK;
    case CVR_OPT_POOL:
      if (v < 256 || v > (1 << 26)) return set_err(&c->err, CVR_ERR_INVALID, "pool size out of range");
      c->pool_max = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_TIMING:
      c->wf_timing = v != 0;
      return CVR_OK;
    case CVR_OPT_ORDER:
      if (v < 0 || v > 2) return set_err(&c->err, CVR_ERR_INVALID, "order must be 0, 1 or 2");
      c->order = (int)v;
      return CVR_OK;
    case CVR_OPT_QUEUES:
      if (v < 1 || v > 8) return set_err(&c->err, CVR_ERR_INVALID, "queues must be 1..8");
      c->n_queues = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_SUBQUEUES:
      if (v < 1 || v > 8) return set_err(&c->err, CVR_ERR_INVALID, "subqueues must be 1..8");
      c->subqueues = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_INFLIGHT:
      if (v < 1 || v > 64) return set_err(&c->err, CVR_ERR_INVALID, "inflight must be 1..64");
      c->inflight = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_FRAME_FLUSH:
      if (v < 0 || v > 2) return set_err(&c->err, CVR_ERR_INVALID, "frame flush must be 0, 1 or 2");
      c->frame_flush = (int)v;
      return CVR_OK;
    case CVR_OPT_DRAIN:
      if (v < -1 || v > 64) return set_err(&c->err, CVR_ERR_INVALID, "drain must be -1..64");
      c->drain = (int)v;
      return CVR_OK;
    case CVR_OPT_WAVES:
      if (v != 3 && v != 4 && v != 5 && v != 6 && v != 8)
        return set_err(&c->err, CVR_ERR_INVALID, "waves must be 3, 4, 5, 6 or 8");
      c->waves = (int)v;
      c->wpool_waves = (v == 5 || v == 3 || v == 6) ? (int)v : 4;
      c->inited = false;
      return CVR_OK;
    case CVR_OPT_MORTON:
      if (v < 0 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "morton must be 0 or 1");
      c->morton = (int)v;
      return CVR_OK;
    case CVR_OPT_BATCH:
      if (v < 1 || v > 64) return set_err(&c->err, CVR_ERR_INVALID, "batch must be 1..64");
      c->swap_batch = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_TAIL:
      if (v < 0 || v > 64) return set_err(&c->err, CVR_ERR_INVALID, "tail must be 0..64");
      c->pool_tail = (uint32_t)v;
      return CVR_OK;
    case CVR_OPT_BOUNDS:
      // takes effect at the next cvr_set_medium
      if (v < 0 || v > 5) return set_err(&c->err, CVR_ERR_INVALID, "bounds must be 0 (off) or log2 brick size 1..5");
      c->bound_shift = (uint32_t)v;
      c->bound_shift_set = true;
      return CVR_OK;
    case CVR_OPT_CELLS:
      // takes effect at the next cvr_set_medium
      c->use_cells = v != 0;
      return CVR_OK;
    case CVR_OPT_MEDIUM_FORMAT:
      // takes effect at the next medium upload (cvr_medium.cpp)
      if (v != CVR_FORMAT_F32 && v != CVR_FORMAT_F16)
        return set_err(&c->err, CVR_ERR_INVALID, "medium format must be 0 (fp32) or 1 (half)");
      c->medium_format = (int)v;
      return CVR_OK;
    case CVR_OPT_MOMENTS:
      if (v != 0 && v != 1) return set_err(&c->err, CVR_ERR_INVALID, "moments must be 0 or 1");
      if (v == 1 && c->external_out)
        return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                       "second moments (CVR_OPT_MOMENTS 1) do not run with a caller's output buffer (cvr_set_output)");
      if (v == 1 && !c->moments) {
        c->moments = 1;
        if (c->tile_w && c->tile_h) {
          // the moments half behind the tile (a grown allocation starts cleared, a reused one is cleared here)
          const size_t px = (size_t)c->tile_w * c->tile_h;
          const bool grown = c->out_owned_px < 2 * px;
          int r = ensure_output(c);
          if (r) {
            c->moments = 0;
            return r;
          }
          if (!grown) HIP_TRY(c, hipMemsetAsync(c->d_out + px, 0, px * sizeof(float4), c->stream));
        }
      }
      if (v == 0) c->moments = 0;
      return CVR_OK;
    case CVR_OPT_SAMPLE_ORDER:
      if (v < -1 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "sample order must be -1, 0 or 1");
      c->sample_order = (int)v;
      return CVR_OK;
    case CVR_OPT_EMPTY_MASK:
      if (v < 0 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "empty mask must be 0 or 1");
      c->empty_mask = (int)v;
      return CVR_OK;
    case CVR_OPT_COUNT_WORDS:
      if (v < 0 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "count words must be 0 or 1");
      c->count_words = (int)v;
      return CVR_OK;
    case CVR_OPT_WAVE_PAIR:
      if (v < 0 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "wave pair must be 0 or 1");
      if (v == 1)
        return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                       "wave pair (workgroup-shared event lists) was an experiment and has been removed");
      return CVR_OK;
    case CVR_OPT_UNIFORM_ALBEDO:
      // takes effect at the next cvr_set_medium
      c->uniform_albedo = v != 0;
      return CVR_OK;
    case CVR_OPT_RNG_BINDING:
      if (v < 0 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "rng binding must be 0 (path) or 1 (thread)");
      c->rng_binding = (int)v;
      return CVR_OK;
    case CVR_OPT_WORLD_TO_AABB:
      if (v < 0 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "world_to_aabb must be 0 (reference) or 1 (fixed)");
      c->world_to_aabb = (int)v;
      return CVR_OK;
    case CVR_OPT_MK_COMPACTION:
      if (v < 0 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "mk_compaction must be 0 (fixed) or 1 (reference)");
      c->mk_compaction = (int)v;
      return CVR_OK;
    case CVR_OPT_SCATTER_EPS:
      if (v < -1 || v > 1) return set_err(&c->err, CVR_ERR_INVALID, "scatter_eps must be -1, 0 or 1");
      c->scatter_eps = (int)v;
      c->inited = false;
      return CVR_OK;
    default:
      return set_err(&c->err, CVR_ERR_INVALID, "unknown option %d", opt);
  }
}

int cvr_init(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  return do_init(c);
}

int cvr_device_info(cvr_ctx* c, int* cu_count, int* grid) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  int r = do_init(c);
  if (r) return r;
  if (cu_count) *cu_count = c->cu_count;
  if (grid) *grid = c->persistent_grid;
  return CVR_OK;
}

int cvr_synchronize(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CVR_OK;
}

int cvr_reset(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_reset");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // Queue heads are re-zeroed per launch; only the seed carries over.
  c->seed = cvr::seed_after_resets(c, c->seed, 1);
  return CVR_OK;
}

int cvr_clear_output(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_clear_output");
  if (!c->d_out) return set_err(&c->err, CVR_ERR_STATE, "no output buffer");
  // (CVR_OPT_MOMENTS: both halves, the moments lie directly behind the tile)
  const size_t halves = (c->moments && c->d_out == c->d_out_owned) ? 2 : 1;
  HIP_TRY(c, hipMemsetAsync(c->d_out, 0, halves * c->tile_w * c->tile_h * sizeof(float4), c->stream));
  return CVR_OK;
}

int cvr_copy_moments(cvr_ctx* c, float* host_sum, float* host_m2) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!c->moments) return set_err(&c->err, CVR_ERR_STATE, "second moments are off (CVR_OPT_MOMENTS)");
  const size_t px = (size_t)c->tile_w * c->tile_h;
  if (!c->d_out || c->d_out != c->d_out_owned || c->out_owned_px < 2 * px || px == 0)
    return set_err(&c->err, CVR_ERR_STATE, "the framebuffer holds no moments (cvr_set_resolution)");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (host_sum) HIP_TRY(c, hipMemcpy(host_sum, c->d_out, px * sizeof(float4), hipMemcpyDeviceToHost));
  if (host_m2) HIP_TRY(c, hipMemcpy(host_m2, c->d_out + px, px * sizeof(float4), hipMemcpyDeviceToHost));
  return CVR_OK;
}

int cvr_block_error(const float* sum_rgba, const float* m2_rgba, uint32_t n_pixels, uint32_t n_samples, float floor,
                    double* out) {
  if (!sum_rgba || !m2_rgba || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (n_samples < 2) return set_err(nullptr, CVR_ERR_INVALID, "the error metric needs at least 2 samples");
  if (n_pixels == 0) return set_err(nullptr, CVR_ERR_INVALID, "no pixels");
  double acc = 0.0;
  for (size_t i = 0; i < n_pixels; ++i) acc += cvr::pixel_error(sum_rgba + 4 * i, m2_rgba + 4 * i, n_samples, floor);
  *out = acc / (double)n_pixels;
  return CVR_OK;
}

int cvr_blocks_to_host(const float* device_src, float* host_dst, uint32_t width, uint32_t height, uint32_t rank,
                       uint32_t world, float scale, void* stream) {
  if (!device_src || !host_dst) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (width % 8 || height % 8 || world == 0 || rank >= world)
    return set_err(nullptr, CVR_ERR_INVALID, "block shards need sides that are multiples of 8 and rank < world");
  if ((((uintptr_t)device_src) | ((uintptr_t)host_dst)) & 15u)
    return set_err(nullptr, CVR_ERR_INVALID, "image buffers must be 16-byte aligned");
  if (width == 0 || height == 0) return CVR_OK;
  void* dptr = nullptr;
  hipError_t e = hipHostGetDevicePointer(&dptr, host_dst, 0);
  if (e != hipSuccess || !dptr)
    return set_err(nullptr, CVR_ERR_INVALID, "host buffer is not pinned or registered: %s", hipGetErrorString(e));
  e = cvr::launch_blocks_to_host(device_src, static_cast<float*>(dptr), width, height, rank, world, scale,
                                 static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return set_err(nullptr, CVR_ERR_HIP, "blocks_to_host: %s", hipGetErrorString(e));
  return CVR_OK;
}

int cvr_image_to_host(const float* device_src, float* host_dst, size_t n_floats, float scale, void* stream) {
  if (!device_src || !host_dst) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (n_floats == 0) return CVR_OK;
  void* dptr = nullptr;  // the host buffer's device address (pinned / registered memory)
  hipError_t e = hipHostGetDevicePointer(&dptr, host_dst, 0);
  if (e != hipSuccess || !dptr)
    return set_err(nullptr, CVR_ERR_INVALID, "host buffer is not pinned or registered: %s", hipGetErrorString(e));
  e = cvr::launch_image_to_host(device_src, static_cast<float*>(dptr), n_floats, scale, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return set_err(nullptr, CVR_ERR_HIP, "image to host: %s", hipGetErrorString(e));
  return CVR_OK;
}

int cvr_get_stats(cvr_ctx* c, cvr_stats* st) {
  if (!c || !st) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  unsigned long long w[32] = {0};  // 16 stats (two rows of 8) and the diagnostic row
  static_assert(cvr::kStatWordsSlot < 32 && kWorkDebug == kWorkStats + 16 * sizeof(unsigned long long), "work area layout");
  HIP_TRY(c, hipMemcpy(w, c->d_work + kWorkStats, sizeof(w), hipMemcpyDeviceToHost));
  unsigned long long v[8];
  for (int k = 0; k < 8; ++k) v[k] = w[k] + w[8 + k];  // wavefront: events + track rows
  cvr_stats s{};
  s.paths = v[cvr::STAT_PATHS];
  s.segments = v[cvr::STAT_SEGMENTS];
  s.steps = v[cvr::STAT_STEPS];
  s.density = v[cvr::STAT_DENSITY];
  s.albedo = v[cvr::STAT_ALBEDO];
  s.escaped = v[cvr::STAT_ESCAPED];
  s.truncated = v[cvr::STAT_TRUNCATED];
  s.fetches = v[cvr::STAT_FETCH];
  s.words = w[cvr::kStatWordsSlot];  // counting launches only (CVR_OPT_COUNT_WORDS)
  s.kernel_ms = 0.0;
  if (c->timed) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
    s.kernel_ms = ms;
  }
  s.iterations = c->last_iterations;
  s.track_ms = c->last_track_ms;
  s.events_ms = c->last_events_ms;
  *st = s;
  c->last = s;
  return CVR_OK;
}

int cvr_debug_counters(cvr_ctx* c, uint64_t out[16]) {
  if (!c || !out) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, c->d_work + kWorkDebug, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return CVR_OK;
}

// Debug (tests; like cvr_debug_tailstamps not part of cvr.h): q[i] = u[i] / d by make_fastdiv(d)'s
// constants.  on_device 0: the formula of cvr_walk.h fastdiv restated on the host (no GPU is
// touched); 1: cvr::fastdiv itself in a trivial kernel on the current device.
int cvr_debug_fastdiv(uint32_t d, const uint32_t* u, uint32_t* q, size_t n, int on_device) {
  if (d == 0 || (n && (!u || !q))) return set_err(nullptr, CVR_ERR_INVALID, "cvr_debug_fastdiv: d = 0 or NULL array");
  const cvr::FastDiv f = cvr::make_fastdiv(d);
  if (!on_device) {
    for (size_t i = 0; i < n; ++i) {
      const uint32_t t = (uint32_t)(((uint64_t)u[i] * f.m) >> 32);
      q[i] = (t + ((u[i] - t) >> (f.sh & 0xFFu))) >> (f.sh >> 8);
    }
    return CVR_OK;
  }
  if (n == 0) return CVR_OK;
  uint32_t *d_u = nullptr, *d_q = nullptr;
  hipError_t e = hipMalloc(&d_u, n * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&d_q, n * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(d_u, u, n * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = cvr::launch_debug_fastdiv(f, d_u, d_q, n, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(q, d_q, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (d_u) (void)hipFree(d_u);
  if (d_q) (void)hipFree(d_q);
  if (e != hipSuccess) return set_err(nullptr, CVR_ERR_HIP, "cvr_debug_fastdiv: %s", hipGetErrorString(e));
  return CVR_OK;
}


int cvr_copy_output(cvr_ctx* c, float* host, float scale) {
  if (!c || !host) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->d_out) return set_err(&c->err, CVR_ERR_STATE, "no output buffer");
  const size_t n = (size_t)c->tile_w * c->tile_h * 4;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(host, c->d_out, n * sizeof(float), hipMemcpyDeviceToHost));
  if (scale != 1.0f)
    for (size_t i = 0; i < n; ++i) host[i] = host[i] / scale;
  return CVR_OK;
}

int cvr_trace_launch(cvr_ctx* c, cvr_path_record* out, uint64_t n_out) {
  if (!c || !out) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_trace_launch");
  if (c->moments)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED, "second moments (CVR_OPT_MOMENTS 1) do not run with cvr_trace_launch");
  if (c->have_env)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "an environment map (cvr_set_environment) does not run with cvr_trace_launch");
  int r = check_ready(c);
  if (r) return r;
  if ((r = do_init(c))) return r;
  // (no walk of naiveMK's has a record instance; a budget without one is launch_wpool's to refuse, CVR_ERR_HIP)
  if (cvr::scheduler_for(c) != 3 || c->rng_binding || c->kernel == CVR_KERNEL_NAIVE_MK)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED, "cvr_trace_launch traces the wave-pool scheduler only");
  cvr::LaunchArgs args;
  const cvr::LaunchPlan plan = cvr::plan_launch(c, args);  // (its range, shard and grid are the traced launch's)
  const uint64_t first = plan.first, count = plan.count;
  if (n_out != count)
    return set_err(&c->err, CVR_ERR_INVALID, "record buffer holds %llu records, the launch range %llu",
                   (unsigned long long)n_out, (unsigned long long)count);
  cvr::WpoolRequest q = plan.request;
  q.record = true;
  cvr::WpoolInstance k;  // (none: no ids, and the launch below fails)
  const bool have = cvr::wpool_select(q, &k);
  const size_t pid_bytes = have ? (size_t)plan.grid * cvr::wpool_slots(k) * sizeof(uint32_t) : 0;
  const size_t rec_bytes = (size_t)count * sizeof(cvr_path_record);
  // the traced launch splats into a scratch framebuffer, not the context's
  const size_t out_bytes = (size_t)c->tile_w * c->tile_h * sizeof(float4);
  const size_t out_at = (pid_bytes + rec_bytes + 16 + 255) & ~(size_t)255;
  char* d = nullptr;
  HIP_TRY(c, hipMalloc(&d, out_at + out_bytes));
  hipError_t e = hipMemsetAsync(d, 0, out_at + out_bytes, c->stream);
  if (e == hipSuccess) {
    args.out = reinterpret_cast<float4*>(d + out_at);
    args.rec = d + pid_bytes;
    r = cvr::launch(c, args);
    if (!r) {
      // the kernel writes path p's record at p - L.path_first: a contiguous
      // shard (no block order) moved path_first to the shard's first id
      const cvr::LaunchParams& Ls = plan.L;
      const uint64_t shift = Ls.path_first - first;
      e = hipStreamSynchronize(c->stream);
      if (e == hipSuccess && shift) {
        memset(out, 0, rec_bytes);
        e = hipMemcpy(out + shift, d + pid_bytes, (size_t)Ls.path_count * sizeof(cvr_path_record),
                      hipMemcpyDeviceToHost);
      } else if (e == hipSuccess) {
        e = hipMemcpy(out, d + pid_bytes, rec_bytes, hipMemcpyDeviceToHost);
      }
    }
  }
  (void)hipFree(d);
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "trace launch: %s", hipGetErrorString(e));
  return CVR_OK;
}

static void wpool_instance_ints(const cvr::WpoolInstance& k, int32_t out[5]) {
  out[0] = k.eps;
  out[1] = k.waves;
  out[2] = k.med;
  out[3] = k.record;
  out[4] = k.flush;
}

int cvr_debug_wpool_rows(int32_t* rows, uint32_t capacity, uint32_t* count) {
  if (!count || (capacity && !rows)) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  std::vector<cvr::WpoolInstance> ids(capacity);
  *count = cvr::wpool_rows(ids.data(), capacity);
  for (uint32_t i = 0; i < capacity && i < *count; ++i) wpool_instance_ints(ids[i], rows + 5 * (size_t)i);
  return CVR_OK;
}

int cvr_debug_last_wpool(const cvr_ctx* c, int32_t instance[5], uint32_t* grid_waves) {
  if (!c || !instance || !grid_waves) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->last_wpool_valid) return set_err(nullptr, CVR_ERR_STATE, "no wave-pool launch yet");
  wpool_instance_ints(c->last_wpool, instance);
  *grid_waves = c->last_wpool_grid;
  return CVR_OK;
}

int cvr_trace_paths(cvr_ctx* c, uint32_t first, uint32_t count, cvr_path_record* out) {
  if (!c || !out) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_trace_paths");
  int r = check_ready(c);
  if (r) return r;
  if (count == 0) return CVR_OK;
  const cvr::LaunchParams L = cvr::trace_params(c, first, count);
  cvr::PathRecord* d_rec = nullptr;
  HIP_TRY(c, hipMalloc(&d_rec, (size_t)count * sizeof(cvr::PathRecord)));
  hipError_t e = cvr::launch_trace(cvr::launch_medium(c), L, cvr::scatter_eps_for(c), d_rec, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess)
    e = hipMemcpy(out, d_rec, (size_t)count * sizeof(cvr::PathRecord), hipMemcpyDeviceToHost);
  (void)hipFree(d_rec);
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "trace: %s", hipGetErrorString(e));
  return CVR_OK;
}

int cvr_trace_env(cvr_ctx* c, uint32_t first, uint32_t count, cvr_env_record* out) {
  static_assert(sizeof(cvr_env_record) == sizeof(cvr::EnvRecord) && sizeof(cvr_env_record) == 48, "record layouts");
  if (!c || !out) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_trace_env");
  int r = check_ready(c);
  if (r) return r;
  if (!c->have_env) return set_err(&c->err, CVR_ERR_STATE, "no environment (cvr_set_environment)");
  if (c->kernel == CVR_KERNEL_NAIVE_MK)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED, "an environment map (cvr_set_environment) does not run with kernel id naiveMK");
  if (count == 0) return CVR_OK;
  const cvr::LaunchParams L = cvr::trace_params(c, first, count);
  cvr::EnvRecord* d_rec = nullptr;
  HIP_TRY(c, hipMalloc(&d_rec, (size_t)count * sizeof(cvr::EnvRecord)));
  hipError_t e = cvr::launch_trace_env(cvr::launch_medium(c), L, cvr::scatter_eps_for(c), c->d_env_hdr, d_rec, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_rec, (size_t)count * sizeof(cvr::EnvRecord), hipMemcpyDeviceToHost);
  (void)hipFree(d_rec);
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "trace: %s", hipGetErrorString(e));
  return CVR_OK;
}

int cvr_host_alloc(size_t bytes, void** out) {
  if (!out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable);
  if (e != hipSuccess) return set_err(nullptr, CVR_ERR_HIP, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
  return CVR_OK;
}

int cvr_host_free(void* p) {
  if (p && hipHostFree(p) != hipSuccess) return set_err(nullptr, CVR_ERR_HIP, "hipHostFree failed");
  return CVR_OK;
}

// ------------------------------------------------------------- helpers ----
int cvr_default_camera(uint32_t w, uint32_t h, float inv_view[12], float r2v[2]) {
  if (!inv_view || !r2v || w == 0 || h == 0) return set_err(nullptr, CVR_ERR_INVALID, "bad camera arguments");
  cvr::camera_for_fov(0.7f, w, h, inv_view, r2v);  // Camera(400, 400, 0.7), Camera.h:25
  return CVR_OK;
}

int cvr_tiling(uint32_t w, uint32_t h, uint32_t ntx, uint32_t nty, uint32_t tile_dim[2]) {
  if (!tile_dim || ntx == 0 || nty == 0) return set_err(nullptr, CVR_ERR_INVALID, "bad tiling arguments");
  // tile_dim = (int)ceil(resolution / n_tiles) with integer division inside
  // ceil: the remainder is never rendered (Q1).
  tile_dim[0] = w / ntx;
  tile_dim[1] = h / nty;
  if (tile_dim[0] == 0 || tile_dim[1] == 0) return set_err(nullptr, CVR_ERR_INVALID, "more tiles than pixels");
  return CVR_OK;
}

int cvr_tile_origin(uint32_t id, uint32_t ntx, const uint32_t tile_dim[2], uint32_t org[2]) {
  if (!tile_dim || !org || ntx == 0) return set_err(nullptr, CVR_ERR_INVALID, "bad tile arguments");
  org[0] = tile_dim[0] * (id % ntx);
  org[1] = tile_dim[1] * (uint32_t)(int)((float)id / (float)ntx);
  return CVR_OK;
}

int cvr_kernel_from_name(const char* name) {
  static const char* names[] = {"naiveSK", "naiveMK", "regenerationSK", "streamingMK", "streamingSK", "sortingSK"};
  if (!name) return CVR_KERNEL_UNKNOWN;
  for (int i = 0; i < 6; ++i)
    if (strcmp(name, names[i]) == 0) return i;
  return CVR_KERNEL_UNKNOWN;
}

const char* cvr_kernel_name(int k) {
  static const char* names[] = {"naiveSK", "naiveMK", "regenerationSK", "streamingMK", "streamingSK", "sortingSK"};
  if (k < 0 || k > 5) return "unknown";
  return names[k];
}

}  // extern "C"
