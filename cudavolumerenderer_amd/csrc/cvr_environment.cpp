// cvr_environment.cpp - C ABI of the environment map (cvr.h, CVR_HAS_ENVMAP): the context's stored
// map and its header, the host statement of the lookup and the device's lookup for arbitrary
// directions.  The lookup itself: cvr_env.h; the kernels: cvr_env.hip; the walk's use of it:
// cvr_wpool.hip (kMedEnv) and k_trace_env (cvr_kernels.hip, cvr_trace_env in cvr_api.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "cvr_ctx.h"

using cvr::set_err;

namespace {

// What a descriptor says besides its texel values, checked in cvr.h's order; R: the rotation in use.
int check_desc(std::string* err, const cvr_environment_desc* d, float R[9]) {
  if (!d) return set_err(err, CVR_ERR_INVALID, "NULL environment descriptor");
  if (d->width < 2u || d->width > 16384u || d->height < 2u || d->height > 8192u)
    return set_err(err, CVR_ERR_INVALID, "environment of %ux%u texels: the width is 2..16384, the height 2..8192",
                   d->width, d->height);
  if (d->channels != 3u && d->channels != 4u)
    return set_err(err, CVR_ERR_INVALID, "environment with %u channels: 3 or 4", d->channels);
  if (d->location != CVR_ENV_HOST && d->location != CVR_ENV_DEVICE)
    return set_err(err, CVR_ERR_INVALID, "unknown environment location %u", d->location);
  if (!d->pixels) return set_err(err, CVR_ERR_INVALID, "environment pixels are NULL");
  if (!(d->scale >= 0.0f) || !std::isfinite(d->scale))
    return set_err(err, CVR_ERR_INVALID, "environment scale %g: finite and >= 0", (double)d->scale);
  bool zero = true;
  for (int i = 0; i < 9; ++i) {
    if (!std::isfinite(d->rotation[i])) return set_err(err, CVR_ERR_INVALID, "environment rotation[%d] is not finite", i);
    zero = zero && d->rotation[i] == 0.0f;
  }
  for (int i = 0; i < 9; ++i) R[i] = zero ? (i % 4 == 0 ? 1.0f : 0.0f) : d->rotation[i];
  return CVR_OK;
}

// Texels behind a callback (cvr_environment_eval_host_fn)
struct EnvCallback {
  cvr_texel_fn fn;
  void* user;
  float4 operator()(uint32_t x, uint32_t y) const {
    float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    fn(user, x, y, t);
    return make_float4(t[0], t[1], t[2], 0.0f);
  }
};
// Texels of a caller's host array, stored as cvr_set_environment stores them
struct EnvHostArray {
  const float* px;
  uint32_t w, channels;
  float scale;
  float4 operator()(uint32_t x, uint32_t y) const {
    const float* t = px + ((size_t)y * w + x) * channels;
    return make_float4(scale * t[0], scale * t[1], scale * t[2], 0.0f);
  }
};

void drop_env(cvr_ctx* c) {
  if (c->env.texels) (void)hipFree(const_cast<float4*>(c->env.texels));
  c->env = cvr::EnvParams{};
  c->have_env = false;
  c->env_max = 0.0f;
}

}  // namespace

namespace cvr {
void free_environment(cvr_ctx* c) {
  drop_env(c);
  if (c->d_env_hdr) (void)hipFree(c->d_env_hdr);
  c->d_env_hdr = nullptr;
}
}  // namespace cvr

extern "C" {

int cvr_set_environment(cvr_ctx* c, const cvr_environment_desc* d) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_set_environment");
  cvr::EnvParams E{};
  int r = check_desc(&c->err, d, E.R);
  if (r) return r;
  if ((r = cvr::ensure_device(c))) return r;
  if (d->location == CVR_ENV_DEVICE) {
    if (!cvr::device_readable(c, d->pixels))
      return set_err(&c->err, CVR_ERR_INVALID, "environment pixels are not device-accessible memory of device %d",
                     c->device);
    if (d->channels == 4u && (reinterpret_cast<uintptr_t>(d->pixels) & 15u))
      return set_err(&c->err, CVR_ERR_INVALID, "4-channel environment pixels are not 16-byte aligned");
  }
  E.w = d->width;
  E.h = d->height;
  const size_t n = (size_t)d->width * d->height;
  // the new map is built beside the old one, which a refusal keeps
  float4* texels = nullptr;
  float* staged = nullptr;
  cvr::EnvScan* d_scan = nullptr;
  cvr::EnvScan scan{~0ull, 0u, 0u};
  hipError_t e = hipMalloc(&texels, n * sizeof(float4));
  if (e == hipSuccess) e = hipMalloc(&d_scan, sizeof(scan));
  if (e == hipSuccess) e = hipMemcpyAsync(d_scan, &scan, sizeof(scan), hipMemcpyHostToDevice, c->stream);
  const float* src = d->pixels;
  if (e == hipSuccess && d->location == CVR_ENV_HOST) {
    e = hipMalloc(&staged, n * d->channels * sizeof(float));
    if (e == hipSuccess)
      e = hipMemcpyAsync(staged, d->pixels, n * d->channels * sizeof(float), hipMemcpyHostToDevice, c->stream);
    src = staged;
  }
  if (e == hipSuccess) e = cvr::launch_env_convert(src, d->channels, n, d->scale, texels, d_scan, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&scan, d_scan, sizeof(scan), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (staged) (void)hipFree(staged);
  if (d_scan) (void)hipFree(d_scan);
  if (e == hipSuccess && !c->d_env_hdr) e = hipMalloc(&c->d_env_hdr, sizeof(cvr::EnvParams));
  if (e != hipSuccess) {
    if (texels) (void)hipFree(texels);
    return set_err(&c->err, e == hipErrorOutOfMemory ? CVR_ERR_NOMEM : CVR_ERR_HIP, "cvr_set_environment: %s",
                   hipGetErrorString(e));
  }
  if (scan.first_bad != ~0ull) {
    (void)hipFree(texels);
    return set_err(&c->err, CVR_ERR_INVALID,
                   "environment component %llu (texel %llu, channel %llu) is negative or not finite after scaling",
                   scan.first_bad, scan.first_bad / d->channels, scan.first_bad % d->channels);
  }
  E.texels = texels;
  // launches in flight read the old header and texels: the stream is idle here (synchronised above)
  e = hipMemcpy(c->d_env_hdr, &E, sizeof(E), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(texels);
    return set_err(&c->err, CVR_ERR_HIP, "cvr_set_environment: %s", hipGetErrorString(e));
  }
  drop_env(c);
  c->env = E;
  c->have_env = true;
  memcpy(&c->env_max, &scan.max_bits, sizeof(float));
  return CVR_OK;
}

int cvr_clear_environment(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_clear_environment");
  if (!c->have_env) return CVR_OK;
  int r = cvr::ensure_device(c);
  if (r) return r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // a launch in flight may read the texels
  drop_env(c);
  return CVR_OK;
}

int cvr_environment_info(const cvr_ctx* c, struct cvr_environment_info* out) {
  if (!c || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  memset(out, 0, sizeof(*out));
  if (!c->have_env) return CVR_OK;
  out->width = c->env.w;
  out->height = c->env.h;
  out->bytes = (uint64_t)c->env.w * c->env.h * sizeof(float4);
  out->max_component = c->env_max;
  return CVR_OK;
}

int cvr_environment_eval_host(const cvr_environment_desc* d, const float* dirs, size_t n, float* out) {
  float R[9];
  int r = check_desc(nullptr, d, R);
  if (r) return r;
  if (d->location != CVR_ENV_HOST) return set_err(nullptr, CVR_ERR_INVALID, "cvr_environment_eval_host reads host pixels");
  if (n && (!dirs || !out)) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  const EnvHostArray tap{d->pixels, d->width, d->channels, d->scale};
  for (size_t i = 0; i < n; ++i)
    cvr::env_lookup_at(tap, R, d->width, d->height, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], out + 3 * i);
  return CVR_OK;
}

int cvr_environment_eval_host_fn(uint32_t width, uint32_t height, const float* rotation, cvr_texel_fn texel, void* user,
                                 const float* dirs, size_t n, float* out) {
  if (width < 2u || width > 16384u || height < 2u || height > 8192u || !texel || (n && (!dirs || !out)))
    return set_err(nullptr, CVR_ERR_INVALID, "cvr_environment_eval_host_fn: bad dimensions or a NULL argument");
  const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const float* R = rotation ? rotation : I;
  const EnvCallback tap{texel, user};
  for (size_t i = 0; i < n; ++i)
    cvr::env_lookup_at(tap, R, width, height, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], out + 3 * i);
  return CVR_OK;
}

int cvr_environment_eval(cvr_ctx* c, const float* dirs, size_t n, float* out) {
  if (!c || (n && (!dirs || !out))) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->have_env) return set_err(&c->err, CVR_ERR_STATE, "no environment (cvr_set_environment)");
  if (n == 0) return CVR_OK;
  int r = cvr::ensure_device(c);
  if (r) return r;
  float *d_dirs = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_dirs, 3 * n * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&d_out, 3 * n * sizeof(float));
  if (e == hipSuccess) e = hipMemcpyAsync(d_dirs, dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = cvr::launch_env_eval(c->d_env_hdr, d_dirs, n, d_out, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (d_dirs) (void)hipFree(d_dirs);
  if (d_out) (void)hipFree(d_out);
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "cvr_environment_eval: %s", hipGetErrorString(e));
  return CVR_OK;
}

}  // extern "C"
