// cvr_adaptive.cpp - the adaptive session of the C ABI (cvr_adaptive_*, cvr_render_adaptive): passes
// of the launch over the active block list, and the per-block errors between them (k_block_error
// and the count-normalised image: cvr_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cvr_host.h"

using cvr::check_ready;
using cvr::do_init;
using cvr::ensure_device;
using cvr::ensure_output;
using cvr::seed_after_resets;
using cvr::set_err;

extern "C" {

// ---------------------------------------------------- adaptive sampling ----
// A noise-targeted render (cvr.h): passes over the still-active 8x8 blocks, each pass one
// launch whose block list is the active blocks (ensure_active_order) and whose path range
// is the next whole samples of the max_iterations launch, then k_block_error on the
// moments and one small read-back, from which the host drops the converged blocks.
static void adaptive_result(const cvr_ctx* c, cvr_adaptive_result* out) {
  if (!out) return;
  const cvr_ctx::Adaptive& a = c->ad;
  cvr_adaptive_result r{};
  r.passes = a.passes;
  r.blocks = a.n_blocks;
  r.blocks_active = (uint32_t)c->active.size();
  r.paths = a.paths;
  double mx = 0.0, sum = 0.0;
  for (double e : a.err) {
    mx = std::max(mx, e);
    sum += e;
  }
  r.max_error = mx;
  r.mean_error = a.n_blocks ? sum / a.n_blocks : 0.0;
  r.done = a.done;
  *out = r;
}

int cvr_adaptive_begin(cvr_ctx* c, const cvr_adaptive_desc* d) {
  if (!c || !d) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  if (c->ad.on) return set_err(&c->err, CVR_ERR_STATE, "an adaptive session is already open (cvr_adaptive_end)");
  int r = check_ready(c);
  if (r) return r;
  if (d->pass_iterations == 0 || d->min_iterations < 2 || d->max_iterations < d->min_iterations ||
      d->min_iterations % d->pass_iterations || d->max_iterations % d->pass_iterations)
    return set_err(&c->err, CVR_ERR_INVALID,
                   "adaptive descriptor: min %u (>= 2) and max %u (>= min) must be multiples of pass %u (>= 1)",
                   d->min_iterations, d->max_iterations, d->pass_iterations);
  if (!(d->floor >= 0.0f) || !std::isfinite(d->floor) || d->target != d->target)
    return set_err(&c->err, CVR_ERR_INVALID, "adaptive descriptor: floor must be finite and >= 0, target not NaN");
  const uint64_t P = (uint64_t)c->tile_w * c->tile_h;
  if (P * d->max_iterations > 0xFFFFFFFFull)
    return set_err(&c->err, CVR_ERR_INVALID, "n_paths = %llu exceeds the reference's uint32 path ids",
                   (unsigned long long)(P * d->max_iterations));
  const cvr::LaunchPlan whole = cvr::plan_launch(c, cvr::LaunchArgs{});
  const uint64_t rf = whole.first, rc = whole.count;
  const char* why = (c->tile_w % 8 || c->tile_h % 8)       ? "tile sides that are not multiples of 8"
                    : c->shard_world != 1                   ? "a block shard (cvr_set_block_shard)"
                    : (rf != 0 || rc != c->n_paths)         ? "a path range (cvr_set_path_range)"
                    : c->order == 0                         ? "CVR_OPT_ORDER 0 (no pixel-block work order)"
                                                            : cvr::wpool_refusal(c, cvr::kForMoments);
  if (why) return set_err(&c->err, CVR_ERR_UNSUPPORTED, "an adaptive render does not run with %s", why);
  if ((r = ensure_device(c)) || (r = do_init(c)) || (r = ensure_output(c))) return r;
  cvr_ctx::Adaptive& a = c->ad;
  const uint32_t nb = (uint32_t)(P / 64);
  if (a.n_blocks != nb || !c->d_active) {  // the per-block device tables
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_active) (void)hipFree(c->d_active);
    if (a.d_err) (void)hipFree(a.d_err);
    if (a.d_counts) (void)hipFree(a.d_counts);
    c->d_active = nullptr;
    a.d_err = nullptr;
    a.d_counts = nullptr;
    a.n_blocks = 0;
    HIP_TRY(c, hipMalloc(&c->d_active, (size_t)nb * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc(&a.d_err, (size_t)nb * sizeof(double)));
    HIP_TRY(c, hipMalloc(&a.d_counts, (size_t)nb * sizeof(uint32_t)));
    a.n_blocks = nb;
  }
  a.saved_moments = c->moments;
  if (!c->moments && (r = cvr_set_option(c, CVR_OPT_MOMENTS, 1))) return r;
  HIP_TRY(c, hipMemsetAsync(c->d_out, 0, 2 * (size_t)P * sizeof(float4), c->stream));
  a.saved_iterations = c->iterations;
  c->iterations = d->max_iterations;
  c->n_paths = P * d->max_iterations;
  a.d = *d;
  a.passes = 0;
  a.done = 0;
  a.paths = 0;
  a.samples.assign(nb, 0u);
  a.err.assign(nb, HUGE_VAL);
  a.acc = cvr_stats{};
  c->active.resize(nb);
  for (uint32_t b = 0; b < nb; ++b) c->active[b] = b;
  c->active_on = true;
  a.on = true;
  return CVR_OK;
}

int cvr_adaptive_pass(cvr_ctx* c, cvr_adaptive_result* result) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  cvr_ctx::Adaptive& a = c->ad;
  if (!a.on) return set_err(&c->err, CVR_ERR_STATE, "no adaptive session (cvr_adaptive_begin)");
  if (a.done) return set_err(&c->err, CVR_ERR_STATE, "the adaptive render is done: no block is active");
  const uint64_t P = (uint64_t)c->tile_w * c->tile_h;
  // the active blocks advance in step: all of them hold the same sample count
  const uint32_t s0 = a.passes == 0 ? 0u : a.samples[c->active[0]];
  const uint32_t add = a.passes == 0 ? a.d.min_iterations : a.d.pass_iterations, N = s0 + add;
  const uint32_t n = (uint32_t)c->active.size();
  cvr::LaunchArgs args;
  args.range.first = s0 * P;  // whole samples [s0, s0 + add) of the max_iterations launch: its path ids
  args.range.count = add * P;
  int r = cvr::launch(c, args);
  if (r) return r;
  // the active blocks' errors, in the launch's block order (d_active / h_active)
  HIP_TRY(c, cvr::launch_block_error(c->d_out, (uint32_t)P, c->tile_w, c->d_active, n, N, a.d.floor, a.d_err, c->stream));
  a.h_err.resize(n);
  HIP_TRY(c, hipMemcpyAsync(a.h_err.data(), a.d_err, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  cvr_stats s{};
  if ((r = cvr_get_stats(c, &s))) return r;  // synchronises: the errors are on the host
  cvr::add_stats(a.acc, s, cvr::kStatKernelMs);
  std::vector<uint32_t> next;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t b = c->h_active[i];
    const double e = a.h_err[i];
    a.samples[b] = N;
    a.err[b] = e;
    if (!(e <= (double)a.d.target) && N < a.d.max_iterations) next.push_back(b);
  }
  std::sort(next.begin(), next.end());
  c->active.swap(next);
  a.passes += 1;
  a.paths += (uint64_t)n * 64u * add;
  a.done = c->active.empty() ? 1 : 0;
  adaptive_result(c, result);
  return CVR_OK;
}

int cvr_adaptive_maps(cvr_ctx* c, double* block_error, uint32_t* block_samples) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  // (the maps of the last session stay readable after its cvr_adaptive_end, at that tile size)
  if (c->ad.err.empty() || c->ad.err.size() != (size_t)(c->tile_w / 8u) * (c->tile_h / 8u))
    return set_err(&c->err, CVR_ERR_STATE, "no adaptive session (cvr_adaptive_begin)");
  if (block_error) memcpy(block_error, c->ad.err.data(), c->ad.err.size() * sizeof(double));
  if (block_samples) memcpy(block_samples, c->ad.samples.data(), c->ad.samples.size() * sizeof(uint32_t));
  return CVR_OK;
}

int cvr_adaptive_image(cvr_ctx* c, float* host, size_t host_floats) {
  if (!c || !host) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  cvr_ctx::Adaptive& a = c->ad;
  if (!a.on) return set_err(&c->err, CVR_ERR_STATE, "no adaptive session (cvr_adaptive_begin)");
  const size_t px = (size_t)c->tile_w * c->tile_h;
  int r = cvr::check_host_floats(c, host_floats, c->tile_w, c->tile_h, "tile");
  if (r) return r;
  HIP_TRY(c, hipMemcpyAsync(a.d_counts, a.samples.data(), (size_t)a.n_blocks * sizeof(uint32_t), hipMemcpyHostToDevice,
                            c->stream));
  void* dhost = nullptr;  // pinned or registered memory: the kernel stores the image itself
  if (((uintptr_t)host & 15u) || hipHostGetDevicePointer(&dhost, host, 0) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: not an error, the staging copy below
    dhost = nullptr;
  }
  if (dhost) {
    HIP_TRY(c, cvr::launch_tile_to_image_counts(c->d_out, c->tile_w, c->tile_h, a.d_counts, static_cast<float4*>(dhost),
                                                c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CVR_OK;
  }
  float4* stage = nullptr;
  HIP_TRY(c, hipMalloc(&stage, px * sizeof(float4)));
  hipError_t e = cvr::launch_tile_to_image_counts(c->d_out, c->tile_w, c->tile_h, a.d_counts, stage, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(host, stage, px * sizeof(float4), hipMemcpyDeviceToHost);
  (void)hipFree(stage);
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "adaptive image: %s", hipGetErrorString(e));
  return CVR_OK;
}

int cvr_adaptive_end(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  cvr_ctx::Adaptive& a = c->ad;
  if (!a.on) return set_err(&c->err, CVR_ERR_STATE, "no adaptive session (cvr_adaptive_begin)");
  const hipError_t e = hipStreamSynchronize(c->stream);
  // reset() after a launch of max_iterations (n_paths is that launch's): wherever the blocks stopped
  c->seed = seed_after_resets(c, c->seed, 1);
  c->iterations = a.saved_iterations;
  c->n_paths = (uint64_t)c->tile_w * c->tile_h * c->iterations;
  c->moments = a.saved_moments;
  c->active_on = false;
  c->active.clear();
  a.on = false;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
  return CVR_OK;
}

int cvr_render_adaptive(cvr_ctx* c, const cvr_adaptive_desc* d, float* host, size_t host_floats,
                        cvr_adaptive_result* result, cvr_stats* stats) {
  if (!c || !d || !host) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = cvr::check_host_floats(c, host_floats, c->tile_w, c->tile_h, "tile");
  if (r || (r = cvr_adaptive_begin(c, d))) return r;
  cvr_adaptive_result res{};
  while (!r && !c->ad.done) r = cvr_adaptive_pass(c, &res);
  if (!r) r = cvr_adaptive_image(c, host, host_floats);
  const cvr_stats acc = c->ad.acc;
  const std::string msg = c->err;
  const int r2 = cvr_adaptive_end(c);
  if (r) return set_err(&c->err, r, "%s", msg.c_str());
  if (r2) return r2;
  if (result) *result = res;
  if (stats) *stats = acc;
  return CVR_OK;
}
}  // extern "C"
