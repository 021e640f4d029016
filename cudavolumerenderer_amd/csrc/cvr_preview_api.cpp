// cvr_preview_api.cpp - C ABI of the shaded preview pass (cvr.h, CVR_HAS_PREVIEW): the host
// statement on a dense medium's host arrays and the device pass on the medium a context holds.
// The pass itself: cvr_preview.h; the kernel: cvr_preview.hip; the march's descriptor, tile and
// view: the feature pass's (cvr_features_api.cpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "cvr_ctx.h"
#include "cvr_preview.h"

using cvr::set_err;

namespace {
bool weight_ok(float v) { return std::isfinite(v) && !(v < 0.0f); }
}  // namespace

// The descriptor's own fields, in cvr.h's order (the NULL test and `march` come before)
int cvr::preview_shading_check(std::string* err, const cvr_preview_desc* d, bool check_light) {
  if (d->flags & ~(CVR_PREVIEW_UNSHADED | CVR_PREVIEW_HEADLIGHT))
    return set_err(err, CVR_ERR_INVALID, "preview: unknown flags 0x%x", d->flags);
  if (!weight_ok(d->ambient) || !weight_ok(d->diffuse) || !weight_ok(d->specular))
    return set_err(err, CVR_ERR_INVALID, "preview: ambient %g, diffuse %g, specular %g must be finite and >= 0",
                   (double)d->ambient, (double)d->diffuse, (double)d->specular);
  if (d->shininess_log2 > 10u)
    return set_err(err, CVR_ERR_INVALID, "preview: shininess_log2 %u not in 0..10", d->shininess_log2);
  if (!weight_ok(d->knee)) return set_err(err, CVR_ERR_INVALID, "preview: knee %g must be finite and >= 0", (double)d->knee);
  for (int a = 0; a < 3; ++a)
    if (!weight_ok(d->background[a]))
      return set_err(err, CVR_ERR_INVALID, "preview: background %g must be finite and >= 0", (double)d->background[a]);
  if (check_light && !(d->flags & (CVR_PREVIEW_UNSHADED | CVR_PREVIEW_HEADLIGHT))) {
    // the length as preview_constants computes it: components that underflow or overflow it are refused too
    const float* l = d->light;
    const float len = det_sqrtf((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
    if (!std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2]) || !(len > 0.0f) || !std::isfinite(len))
      return set_err(err, CVR_ERR_INVALID, "preview: the light direction must be finite and of a length above zero");
  }
  return CVR_OK;
}

// Q.F is filled; light: the direction in use (the descriptor's for cvr_preview); max_density: the majorant in use
void cvr::preview_set_shading(cvr::PreviewParams& Q, const cvr_preview_desc* d, const float light[3], float max_density) {
  const int headlight = (d->flags & (CVR_PREVIEW_UNSHADED | CVR_PREVIEW_HEADLIGHT)) != 0;  // (unshaded: no light is read)
  cvr::preview_constants(Q, light, headlight, d->ambient, d->diffuse, d->specular, d->shininess_log2, d->knee,
                         d->background, max_density);
}

namespace {

// State, descriptor and tile of a context call
int preview_check(cvr_ctx* c, const cvr_preview_desc* d) {
  int r = cvr::features_check(c, d ? &d->march : nullptr);
  if (r) return r;
  return cvr::preview_shading_check(&c->err, d, true);
}

int preview_launch(cvr_ctx* c, const cvr_preview_desc* d, float4* rgba) {
  cvr::MediumParams m = c->m;
  if (!c->empty_mask) m.emask = nullptr;  // CVR_OPT_EMPTY_MASK 0, as features_launch honours it
  cvr::PreviewParams Q{};
  Q.F = cvr::features_ctx_params(c, &d->march);
  cvr::preview_set_shading(Q, d, d->light, c->minfo.max_density_eff);
  HIP_TRY(c, cvr::launch_preview(m, Q, !(d->flags & CVR_PREVIEW_UNSHADED), rgba, c->stream));
  return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_preview_host(const cvr_medium_desc* medium, const float inv_view[12], const float raster_to_view[2],
                     const float full_res[2], uint32_t tile_w, uint32_t tile_h, uint32_t off_x, uint32_t off_y,
                     int world_to_aabb, const cvr_preview_desc* desc, float* out_rgba) {
  if (!desc) return set_err(nullptr, CVR_ERR_INVALID, "NULL preview descriptor");
  if (!medium || !inv_view || !raster_to_view || !full_res || !out_rgba)
    return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!medium->density || !medium->albedo) return set_err(nullptr, CVR_ERR_INVALID, "NULL medium array");
  if (medium->res[0] == 0 || medium->res[1] == 0 || medium->res[2] == 0)
    return set_err(nullptr, CVR_ERR_INVALID, "empty grid");
  if (world_to_aabb != 0 && world_to_aabb != 1)
    return set_err(nullptr, CVR_ERR_INVALID, "preview: world_to_aabb must be 0 or 1");
  int r = cvr::features_desc_check(nullptr, &desc->march);
  if (r) return r;
  if ((r = cvr::preview_shading_check(nullptr, desc, true))) return r;
  if ((r = cvr::features_tile_check(nullptr, tile_w, tile_h))) return r;
  cvr::PreviewParams Q{};
  cvr::feature_geometry(Q.F, medium->res, medium->box_min, medium->box_max, medium->scale, world_to_aabb,
                        desc->march.step, desc->march.t_stop, desc->march.max_steps);
  cvr::features_set_view(Q.F, inv_view, raster_to_view, full_res, tile_w, tile_h, off_x, off_y);
  cvr::preview_set_shading(Q, desc, desc->light, medium->max_density);
  const cvr::FeatureHostTexels tex{medium->density, medium->albedo, medium->res[0], medium->res[1]};
  const bool shaded = !(desc->flags & CVR_PREVIEW_UNSHADED);
  for (uint32_t y = 0; y < tile_h; ++y)
    for (uint32_t x = 0; x < tile_w; ++x) {
      const cvr::PreviewOut f = shaded ? cvr::preview_pixel<true>(tex, Q, x, y) : cvr::preview_pixel<false>(tex, Q, x, y);
      float* o = out_rgba + 4 * ((size_t)y * tile_w + x);
      o[0] = f.r, o[1] = f.g, o[2] = f.b, o[3] = f.w;
    }
  return CVR_OK;
}

int cvr_preview_buffers(cvr_ctx* c, const cvr_preview_desc* desc, float* d_out_rgba) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !d_out_rgba) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = preview_check(c, desc);
  if (r) return r;
  if ((uintptr_t)d_out_rgba & 15u) return set_err(&c->err, CVR_ERR_INVALID, "preview: out_rgba must be 16-byte aligned");
  if ((r = cvr::ensure_device(c))) return r;
  return preview_launch(c, desc, reinterpret_cast<float4*>(d_out_rgba));
}

int cvr_preview(cvr_ctx* c, const cvr_preview_desc* desc, float* host_rgba, size_t host_floats) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !host_rgba) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = preview_check(c, desc);
  if (r) return r;
  const size_t px = (size_t)c->tile_w * c->tile_h;
  if (host_floats < px * 4u)
    return set_err(&c->err, CVR_ERR_INVALID, "host image holds %zu floats, the %ux%u tile needs %zu", host_floats,
                   c->tile_w, c->tile_h, px * 4u);
  if ((r = cvr::ensure_device(c))) return r;
  // pinned or registered memory is stored into by the kernel, other memory through a staging copy
  void* drgba = nullptr;
  if (((uintptr_t)host_rgba & 15u) || hipHostGetDevicePointer(&drgba, host_rgba, 0) != hipSuccess) drgba = nullptr;
  (void)hipGetLastError();  // pageable memory: not an error
  float4* stage = nullptr;
  if (!drgba) HIP_TRY(c, hipMalloc(&stage, px * sizeof(float4)));
  r = preview_launch(c, desc, stage ? stage : static_cast<float4*>(drgba));
  hipError_t e = hipStreamSynchronize(c->stream);
  if (!r && e == hipSuccess && stage) e = hipMemcpy(host_rgba, stage, px * sizeof(float4), hipMemcpyDeviceToHost);
  if (stage) (void)hipFree(stage);
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "preview: %s", hipGetErrorString(e));
  return CVR_OK;
}

}  // extern "C"
