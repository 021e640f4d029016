// cvr_denoise_api.cpp - the denoiser of the C ABI (cvr_denoise*): its checks, the host statement
// and the launches of the filter passes (cvr_denoise.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "cvr_host.h"

using cvr::ensure_device;
using cvr::set_err;

extern "C" {

// ------------------------------------------------------------ denoiser ----
// The variance-guided a-trous filter of cvr.h.  The host statement and the kernels
// (cvr_denoise.hip) run the same per-pixel functions of cvr_kernels.h.
static int denoise_check(std::string* err, const cvr_denoise_desc* d, uint32_t w, uint32_t h, uint32_t n_samples,
                         bool have_map) {
  if (d->passes < 1u || d->passes > 6u) return set_err(err, CVR_ERR_INVALID, "denoise: passes %u not in 1..6", d->passes);
  if (!(d->sigma >= 0.0f) || !std::isfinite(d->sigma) || !(d->floor > 0.0f) || !std::isfinite(d->floor))
    return set_err(err, CVR_ERR_INVALID, "denoise: sigma must be finite and >= 0, floor finite and > 0");
  if (d->flags != 0u) return set_err(err, CVR_ERR_INVALID, "denoise: flags must be 0");
  if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 24))
    return set_err(err, CVR_ERR_INVALID, "denoise: a %ux%u image (1 to 2^24 pixels)", w, h);
  if (have_map && (w % 8u || h % 8u))
    return set_err(err, CVR_ERR_INVALID, "denoise: a block-sample map needs sides that are multiples of 8, not %ux%u", w,
                   h);
  if (!have_map && n_samples < 2u) return set_err(err, CVR_ERR_INVALID, "denoise: the variance needs at least 2 samples");
  return CVR_OK;
}

// The guided descriptor's own fields (the base goes through denoise_check)
static int guided_check(std::string* err, const cvr_denoise_guided_desc* g) {
  const float s[3] = {g->sigma_albedo, g->sigma_depth, g->sigma_alpha};
  for (float v : s)
    if (!(v == v) || v == INFINITY)
      return set_err(err, CVR_ERR_INVALID, "denoise: a guide sigma is a number below +inf (<= 0: the term is off)");
  if (g->flags != 0u) return set_err(err, CVR_ERR_INVALID, "denoise: guided flags must be 0");
  return CVR_OK;
}
static cvr::DenoiseGuide make_guide(const cvr_denoise_guided_desc* g, const float* feat_rgba, const float* feat_depth) {
  return cvr::DenoiseGuide{feat_rgba, feat_depth, g->sigma_albedo, g->sigma_depth, g->sigma_alpha};
}

// The host statement, unguided (guide null) or guided; checked arguments
static void denoise_host_run(const float* sum_rgba, const float* m2_rgba, uint32_t w, uint32_t h, uint32_t n_samples,
                             const uint32_t* block_samples, const cvr_denoise_desc* desc, const cvr::DenoiseGuide* guide,
                             float* out_rgba, float* out_var);

int cvr_denoise_host(const float* sum_rgba, const float* m2_rgba, uint32_t w, uint32_t h, uint32_t n_samples,
                     const uint32_t* block_samples, const cvr_denoise_desc* desc, float* out_rgba, float* out_var) {
  if (!sum_rgba || !m2_rgba || !desc || !out_rgba) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = denoise_check(nullptr, desc, w, h, n_samples, block_samples != nullptr);
  if (r) return r;
  denoise_host_run(sum_rgba, m2_rgba, w, h, n_samples, block_samples, desc, nullptr, out_rgba, out_var);
  return CVR_OK;
}

int cvr_denoise_guided_host(const float* sum_rgba, const float* m2_rgba, uint32_t w, uint32_t h, uint32_t n_samples,
                            const uint32_t* block_samples, const cvr_denoise_guided_desc* desc, const float* feat_rgba,
                            const float* feat_depth, float* out_rgba, float* out_var) {
  if (!sum_rgba || !m2_rgba || !desc || !feat_rgba || !feat_depth || !out_rgba)
    return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = denoise_check(nullptr, &desc->base, w, h, n_samples, block_samples != nullptr);
  if (r) return r;
  if ((r = guided_check(nullptr, desc))) return r;
  const cvr::DenoiseGuide guide = make_guide(desc, feat_rgba, feat_depth);
  denoise_host_run(sum_rgba, m2_rgba, w, h, n_samples, block_samples, &desc->base, &guide, out_rgba, out_var);
  return CVR_OK;
}

static void denoise_host_run(const float* sum_rgba, const float* m2_rgba, uint32_t w, uint32_t h, uint32_t n_samples,
                             const uint32_t* block_samples, const cvr_denoise_desc* desc, const cvr::DenoiseGuide* guide,
                             float* out_rgba, float* out_var) {
  const size_t px = (size_t)w * h;
  // (floats, not float4: the caller's arrays need no 16-byte alignment)
  auto at = [](const float* a, size_t i) { return make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]); };
  std::vector<float4> a(px), b(px);
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      a[i] = cvr::denoise_prepare(at(sum_rgba, i), at(m2_rgba, i), cvr::denoise_count(block_samples, n_samples, w, x, y));
    }
  for (uint32_t k = 0; k < desc->passes; ++k) {
    for (uint32_t y = 0; y < h; ++y)
      for (uint32_t x = 0; x < w; ++x)
        b[(size_t)y * w + x] = guide ? cvr::denoise_pass(a.data(), w, h, x, y, 1u << k, desc->sigma, desc->floor, *guide)
                                     : cvr::denoise_pass(a.data(), w, h, x, y, 1u << k, desc->sigma, desc->floor);
    a.swap(b);
  }
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      const float4 f = a[i];
      const float4 o = cvr::denoise_final(f, at(sum_rgba, i), cvr::denoise_count(block_samples, n_samples, w, x, y));
      out_rgba[4 * i] = o.x;
      out_rgba[4 * i + 1] = o.y;
      out_rgba[4 * i + 2] = o.z;
      out_rgba[4 * i + 3] = o.w;
      if (out_var) out_var[i] = f.w < 0.0f ? -1.0f : f.w;
    }
}

// prepare + passes on the context's stream, the last pass storing into out (checked arguments)
static int denoise_launch(cvr_ctx* c, const float4* sum, const float4* m2, uint32_t w, uint32_t h, uint32_t n_samples,
                          const uint32_t* d_counts, const cvr_denoise_desc* d, float4* out, float* out_var,
                          const cvr::DenoiseGuide* guide = nullptr) {
  const size_t px = (size_t)w * h;
  if (c->dn_px < px) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // an earlier filter may still read the old images
    if (c->d_dn) (void)hipFree(c->d_dn);
    c->d_dn = nullptr;
    c->dn_px = 0;
    HIP_TRY(c, hipMalloc(&c->d_dn, 2 * px * sizeof(float4)));
    c->dn_px = px;
  }
  float4* img[2] = {c->d_dn, c->d_dn + c->dn_px};
  HIP_TRY(c, cvr::launch_denoise_prepare(sum, m2, w, h, n_samples, d_counts, img[0], c->stream));
  for (uint32_t k = 0; k + 1 < d->passes; ++k)
    HIP_TRY(c, cvr::launch_denoise_pass(img[k & 1u], img[(k & 1u) ^ 1u], w, h, 1u << k, d->sigma, d->floor, c->stream,
                                        guide));
  const uint32_t last = d->passes - 1u;
  HIP_TRY(c, cvr::launch_denoise_last(img[last & 1u], w, h, 1u << last, d->sigma, d->floor, sum, n_samples, d_counts, out,
                                      out_var, c->stream, guide));
  return CVR_OK;
}

int cvr_denoise_buffers(cvr_ctx* c, const float* d_sum_rgba, const float* d_m2_rgba, uint32_t w, uint32_t h,
                        uint32_t n_samples, const uint32_t* d_block_samples, const cvr_denoise_desc* desc,
                        float* d_out_rgba, float* d_out_var) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!d_sum_rgba || !d_m2_rgba || !desc || !d_out_rgba) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = denoise_check(&c->err, desc, w, h, n_samples, d_block_samples != nullptr);
  if (r) return r;
  if ((((uintptr_t)d_sum_rgba) | ((uintptr_t)d_m2_rgba) | ((uintptr_t)d_out_rgba)) & 15u)
    return set_err(&c->err, CVR_ERR_INVALID, "denoise: the rgba buffers must be 16-byte aligned");
  if ((uintptr_t)d_out_var & 3u) return set_err(&c->err, CVR_ERR_INVALID, "denoise: out_var must be 4-byte aligned");
  if ((r = ensure_device(c))) return r;
  return denoise_launch(c, reinterpret_cast<const float4*>(d_sum_rgba), reinterpret_cast<const float4*>(d_m2_rgba), w, h,
                        n_samples, d_block_samples, desc, reinterpret_cast<float4*>(d_out_rgba), d_out_var);
}

int cvr_denoise_guided_buffers(cvr_ctx* c, const float* d_sum_rgba, const float* d_m2_rgba, uint32_t w, uint32_t h,
                               uint32_t n_samples, const uint32_t* d_block_samples, const cvr_denoise_guided_desc* desc,
                               const float* d_feat_rgba, const float* d_feat_depth, float* d_out_rgba,
                               float* d_out_var) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!d_sum_rgba || !d_m2_rgba || !desc || !d_feat_rgba || !d_feat_depth || !d_out_rgba)
    return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = denoise_check(&c->err, &desc->base, w, h, n_samples, d_block_samples != nullptr);
  if (r) return r;
  if ((r = guided_check(&c->err, desc))) return r;
  if ((((uintptr_t)d_sum_rgba) | ((uintptr_t)d_m2_rgba) | ((uintptr_t)d_out_rgba) | ((uintptr_t)d_feat_rgba)) & 15u)
    return set_err(&c->err, CVR_ERR_INVALID, "denoise: the rgba buffers must be 16-byte aligned");
  if (((uintptr_t)d_out_var | (uintptr_t)d_feat_depth) & 3u)
    return set_err(&c->err, CVR_ERR_INVALID, "denoise: out_var and feat_depth must be 4-byte aligned");
  if ((r = ensure_device(c))) return r;
  const cvr::DenoiseGuide guide = make_guide(desc, d_feat_rgba, d_feat_depth);
  return denoise_launch(c, reinterpret_cast<const float4*>(d_sum_rgba), reinterpret_cast<const float4*>(d_m2_rgba), w, h,
                        n_samples, d_block_samples, &desc->base, reinterpret_cast<float4*>(d_out_rgba), d_out_var, &guide);
}

// cvr_denoise and cvr_denoise_guided (gdesc, fdesc non-null: the feature pass into the context's
// planes first, then the guided passes)
static int denoise_ctx(cvr_ctx* c, const cvr_denoise_desc* desc, const cvr_denoise_guided_desc* gdesc,
                       const cvr_features_desc* fdesc, uint32_t n_samples, float* host, size_t host_floats);

int cvr_denoise(cvr_ctx* c, const cvr_denoise_desc* desc, uint32_t n_samples, float* host, size_t host_floats) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !host) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  return denoise_ctx(c, desc, nullptr, nullptr, n_samples, host, host_floats);
}

int cvr_denoise_guided(cvr_ctx* c, const cvr_denoise_guided_desc* desc, const cvr_features_desc* features,
                       uint32_t n_samples, float* host, size_t host_floats) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !features || !host) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  return denoise_ctx(c, &desc->base, desc, features, n_samples, host, host_floats);
}

static int denoise_ctx(cvr_ctx* c, const cvr_denoise_desc* desc, const cvr_denoise_guided_desc* gdesc,
                       const cvr_features_desc* fdesc, uint32_t n_samples, float* host, size_t host_floats) {
  if (!c->moments) return set_err(&c->err, CVR_ERR_STATE, "second moments are off (CVR_OPT_MOMENTS)");
  const size_t px = (size_t)c->tile_w * c->tile_h;
  if (!c->d_out || c->d_out != c->d_out_owned || c->out_owned_px < 2 * px || px == 0)
    return set_err(&c->err, CVR_ERR_STATE, "the framebuffer holds no moments (cvr_set_resolution)");
  cvr_ctx::Adaptive& a = c->ad;
  if (a.on && n_samples != 0)
    return set_err(&c->err, CVR_ERR_INVALID,
                   "denoise: inside an adaptive session n_samples must be 0 (every block has its own count)");
  int r = denoise_check(&c->err, desc, c->tile_w, c->tile_h, n_samples, a.on);
  if (r) return r;
  if ((r = cvr::check_host_floats(c, host_floats, c->tile_w, c->tile_h, "tile"))) return r;
  cvr::DenoiseGuide guide_v{};
  const cvr::DenoiseGuide* guide = nullptr;
  if (gdesc) {
    if ((r = guided_check(&c->err, gdesc))) return r;
    if ((r = cvr::features_check(c, fdesc))) return r;
  }
  if ((r = ensure_device(c))) return r;
  if (gdesc) {
    if (c->feat_px < px) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // an earlier filter may still read the old planes
      if (c->d_feat) (void)hipFree(c->d_feat);
      c->d_feat = nullptr;
      c->feat_px = 0;
      HIP_TRY(c, hipMalloc(&c->d_feat, px * (sizeof(float4) + sizeof(float))));
      c->feat_px = px;
    }
    float* depth = reinterpret_cast<float*>(c->d_feat + c->feat_px);
    if ((r = cvr::features_launch(c, fdesc, c->d_feat, depth))) return r;
    guide_v = make_guide(gdesc, reinterpret_cast<const float*>(c->d_feat), depth);
    guide = &guide_v;
  }
  const uint32_t* d_counts = nullptr;
  if (a.on) {
    HIP_TRY(c, hipMemcpyAsync(a.d_counts, a.samples.data(), (size_t)a.n_blocks * sizeof(uint32_t), hipMemcpyHostToDevice,
                              c->stream));
    d_counts = a.d_counts;
  }
  void* dhost = nullptr;  // pinned or registered memory: the last pass stores the image itself
  if (((uintptr_t)host & 15u) || hipHostGetDevicePointer(&dhost, host, 0) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: not an error, the staging copy below
    dhost = nullptr;
  }
  if (dhost) {
    if ((r = denoise_launch(c, c->d_out, c->d_out + px, c->tile_w, c->tile_h, n_samples, d_counts, desc,
                            static_cast<float4*>(dhost), nullptr, guide)))
      return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CVR_OK;
  }
  float4* stage = nullptr;
  HIP_TRY(c, hipMalloc(&stage, px * sizeof(float4)));
  r = denoise_launch(c, c->d_out, c->d_out + px, c->tile_w, c->tile_h, n_samples, d_counts, desc, stage, nullptr, guide);
  hipError_t e = hipStreamSynchronize(c->stream);
  if (!r && e == hipSuccess) e = hipMemcpy(host, stage, px * sizeof(float4), hipMemcpyDeviceToHost);
  (void)hipFree(stage);
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "denoise: %s", hipGetErrorString(e));
  return CVR_OK;
}
}  // extern "C"
