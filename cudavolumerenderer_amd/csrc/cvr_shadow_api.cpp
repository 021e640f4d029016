// cvr_shadow_api.cpp - C ABI of the light volume and the shadowed preview (cvr.h, CVR_HAS_SHADOWS):
// the two host statements on a dense medium's host arrays, the build into memory the context owns
// and the pass on the medium a context holds.  The arithmetic: cvr_shadow.h; the kernels:
// cvr_shadow.hip; the march's and the shading's checks: cvr_features_api.cpp, cvr_preview_api.cpp.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cvr_ctx.h"
#include "cvr_shadow.h"

using cvr::set_err;

namespace {

// cvr_build_light_volume's refusals, in cvr.h's order
int volume_desc_check(std::string* err, const cvr_light_volume_desc* d) {
  if (!d) return set_err(err, CVR_ERR_INVALID, "NULL light volume descriptor");
  if (d->flags != 0u) return set_err(err, CVR_ERR_INVALID, "light volume: flags must be 0");
  for (int a = 0; a < 3; ++a)
    if (d->res[a] == 0 || d->res[a] > 1024u)
      return set_err(err, CVR_ERR_INVALID, "light volume: res %u x %u x %u, each axis 1..1024", d->res[0], d->res[1],
                     d->res[2]);
  if ((uint64_t)d->res[0] * d->res[1] * d->res[2] > (1ull << 27))
    return set_err(err, CVR_ERR_INVALID, "light volume: res %u x %u x %u holds more than 2^27 nodes", d->res[0], d->res[1],
                   d->res[2]);
  const float* l = d->light;
  float L[3];
  const float len = cvr::light_normalise(l, L);
  if (!std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2]) || !(len > 0.0f) || !std::isfinite(len))
    return set_err(err, CVR_ERR_INVALID, "light volume: the light direction must be finite and of a length above zero");
  return cvr::features_desc_check(err, &d->march);
}

// The shadowed preview's own refusals after cvr_preview's (the light is not read: not judged)
int shadowed_desc_check(std::string* err, const cvr_preview_desc* d, float shadow) {
  int r = cvr::preview_shading_check(err, d, false);
  if (r) return r;
  if (d->flags & CVR_PREVIEW_HEADLIGHT)
    return set_err(err, CVR_ERR_INVALID, "shadowed preview: CVR_PREVIEW_HEADLIGHT is set, shadows need the directional light");
  if (!(shadow >= 0.0f && shadow <= 1.0f))
    return set_err(err, CVR_ERR_INVALID, "shadowed preview: shadow %g not in [0, 1]", (double)shadow);
  return CVR_OK;
}

// State, descriptor, tile and volume of a context call
int shadowed_check(cvr_ctx* c, const cvr_preview_desc* d, float shadow) {
  int r = cvr::features_check(c, d ? &d->march : nullptr);
  if (r) return r;
  if ((r = shadowed_desc_check(&c->err, d, shadow))) return r;
  if (!c->lightvol.valid || !c->d_lightvol)
    return set_err(&c->err, CVR_ERR_STATE, "no light volume (cvr_build_light_volume)");
  if (c->lightvol.world_to_aabb != c->world_to_aabb)
    return set_err(&c->err, CVR_ERR_STATE, "the light volume is stale: built under CVR_OPT_WORLD_TO_AABB %d, now %d",
                   c->lightvol.world_to_aabb, c->world_to_aabb);
  return CVR_OK;
}

cvr::ShadowGrid shadow_grid(const float* S, const uint32_t res[3], float shadow) {
  cvr::ShadowGrid G{};
  G.S = S;
  for (int a = 0; a < 3; ++a) G.res[a] = res[a], G.fres[a] = (float)res[a];
  G.shadow = shadow;
  return G;
}

int shadowed_launch(cvr_ctx* c, const cvr_preview_desc* d, float shadow, float4* rgba) {
  cvr::MediumParams m = c->m;
  if (!c->empty_mask) m.emask = nullptr;  // CVR_OPT_EMPTY_MASK 0, as features_launch honours it
  cvr::PreviewParams Q{};
  Q.F = cvr::features_ctx_params(c, &d->march);
  cvr::preview_set_shading(Q, d, c->lightvol.light, c->minfo.max_density_eff);
  HIP_TRY(c, cvr::launch_preview_shadowed(m, Q, shadow_grid(c->d_lightvol, c->lightvol.res, shadow),
                                          !(d->flags & CVR_PREVIEW_UNSHADED), rgba, c->stream));
  return CVR_OK;
}

int host_medium_check(const cvr_medium_desc* medium, int world_to_aabb) {
  if (!medium->density || !medium->albedo) return set_err(nullptr, CVR_ERR_INVALID, "NULL medium array");
  if (medium->res[0] == 0 || medium->res[1] == 0 || medium->res[2] == 0)
    return set_err(nullptr, CVR_ERR_INVALID, "empty grid");
  if (world_to_aabb != 0 && world_to_aabb != 1)
    return set_err(nullptr, CVR_ERR_INVALID, "world_to_aabb must be 0 or 1");
  return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_light_volume_host(const cvr_medium_desc* medium, int world_to_aabb, const cvr_light_volume_desc* desc,
                          float* out) {
  if (!desc) return set_err(nullptr, CVR_ERR_INVALID, "NULL light volume descriptor");
  if (!medium || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = host_medium_check(medium, world_to_aabb);
  if (r) return r;
  if ((r = volume_desc_check(nullptr, desc))) return r;
  cvr::LightVolumeParams V{};
  cvr::feature_geometry(V.F, medium->res, medium->box_min, medium->box_max, medium->scale, world_to_aabb,
                        desc->march.step, desc->march.t_stop, desc->march.max_steps);
  cvr::light_volume_constants(V, desc->res, desc->light);
  const cvr::FeatureHostTexels tex{medium->density, medium->albedo, medium->res[0], medium->res[1]};
  size_t at = 0;
  for (uint32_t k = 0; k < desc->res[2]; ++k)
    for (uint32_t j = 0; j < desc->res[1]; ++j)
      for (uint32_t i = 0; i < desc->res[0]; ++i) out[at++] = cvr::light_node(tex, V, i, j, k);
  return CVR_OK;
}

int cvr_build_light_volume(cvr_ctx* c, const cvr_light_volume_desc* desc) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc) return set_err(&c->err, CVR_ERR_INVALID, "NULL light volume descriptor");
  if (!c->have_medium) return set_err(&c->err, CVR_ERR_STATE, "medium not set (cvr_set_medium)");
  int r = volume_desc_check(&c->err, desc);
  if (r) return r;
  if ((r = cvr::ensure_device(c))) return r;
  const size_t n = (size_t)desc->res[0] * desc->res[1] * desc->res[2];
  c->lightvol.valid = false;
  if (n > c->lightvol_floats) {
    // (a pass still reading the previous volume is on this stream: hipFree waits for the device)
    if (c->d_lightvol) (void)hipFree(c->d_lightvol);
    c->d_lightvol = nullptr;
    c->lightvol_floats = 0;
    HIP_TRY(c, hipMalloc(&c->d_lightvol, n * sizeof(float)));
    c->lightvol_floats = n;
  }
  cvr::MediumParams m = c->m;
  if (!c->empty_mask) m.emask = nullptr;  // CVR_OPT_EMPTY_MASK 0, as features_launch honours it
  cvr::LightVolumeParams V{};
  const uint32_t res[3] = {c->m.rx, c->m.ry, c->m.rz};
  const float bmin[3] = {c->m.bmin.x, c->m.bmin.y, c->m.bmin.z}, bmax[3] = {c->m.bmax.x, c->m.bmax.y, c->m.bmax.z};
  cvr::feature_geometry(V.F, res, bmin, bmax, c->m.scale, c->world_to_aabb, desc->march.step, desc->march.t_stop,
                        desc->march.max_steps);
  cvr::light_volume_constants(V, desc->res, desc->light);
  HIP_TRY(c, cvr::launch_light_volume(m, V, c->d_lightvol, c->stream));
  for (int a = 0; a < 3; ++a) {
    c->lightvol.res[a] = desc->res[a];
    c->lightvol.light[a] = desc->light[a];
    c->lightvol.L[a] = V.L[a];
  }
  c->lightvol.world_to_aabb = c->world_to_aabb;
  c->lightvol.valid = true;
  return CVR_OK;
}

int cvr_light_volume_default_res(const cvr_ctx* c, uint32_t res[3]) {
  if (!c || !res) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->have_medium) return set_err(nullptr, CVR_ERR_STATE, "medium not set (cvr_set_medium)");
  const uint32_t m[3] = {c->m.rx, c->m.ry, c->m.rz};
  for (int a = 0; a < 3; ++a) res[a] = m[a] >= 512u ? 256u : (m[a] + 1u) / 2u;
  return CVR_OK;
}

int cvr_light_volume_info(const cvr_ctx* c, struct cvr_light_volume_info* out) {
  if (!c || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  struct cvr_light_volume_info info {};
  if (c->lightvol.valid) {
    info.valid = 1;
    for (int a = 0; a < 3; ++a) info.res[a] = c->lightvol.res[a], info.light[a] = c->lightvol.L[a];
    info.bytes = (uint64_t)c->lightvol.res[0] * c->lightvol.res[1] * c->lightvol.res[2] * sizeof(float);
  }
  *out = info;
  return CVR_OK;
}

int cvr_copy_light_volume(cvr_ctx* c, float* host, size_t host_floats) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!host) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  if (!c->lightvol.valid) return set_err(&c->err, CVR_ERR_STATE, "no light volume (cvr_build_light_volume)");
  const size_t n = (size_t)c->lightvol.res[0] * c->lightvol.res[1] * c->lightvol.res[2];
  if (host_floats < n)
    return set_err(&c->err, CVR_ERR_INVALID, "host array holds %zu floats, the light volume %zu", host_floats, n);
  int r = cvr::ensure_device(c);
  if (r) return r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(host, c->d_lightvol, n * sizeof(float), hipMemcpyDeviceToHost));
  return CVR_OK;
}

int cvr_clear_light_volume(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  cvr::drop_light_volume(c);
  if (!c->d_lightvol) return CVR_OK;
  int r = cvr::ensure_device(c);
  if (r) return r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  (void)hipFree(c->d_lightvol);
  c->d_lightvol = nullptr;
  c->lightvol_floats = 0;
  return CVR_OK;
}

int cvr_preview_shadowed_host(const cvr_medium_desc* medium, const float inv_view[12], const float raster_to_view[2],
                              const float full_res[2], uint32_t tile_w, uint32_t tile_h, uint32_t off_x,
                              uint32_t off_y, int world_to_aabb, const cvr_preview_desc* desc,
                              const cvr_light_volume_desc* volume_desc, const float* volume, float shadow,
                              float* out_rgba) {
  if (!desc) return set_err(nullptr, CVR_ERR_INVALID, "NULL preview descriptor");
  if (!medium || !inv_view || !raster_to_view || !full_res || !volume || !out_rgba)
    return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = host_medium_check(medium, world_to_aabb);
  if (r) return r;
  if ((r = cvr::features_desc_check(nullptr, &desc->march))) return r;
  if ((r = shadowed_desc_check(nullptr, desc, shadow))) return r;
  if ((r = volume_desc_check(nullptr, volume_desc))) return r;
  if ((r = cvr::features_tile_check(nullptr, tile_w, tile_h))) return r;
  cvr::PreviewParams Q{};
  cvr::feature_geometry(Q.F, medium->res, medium->box_min, medium->box_max, medium->scale, world_to_aabb,
                        desc->march.step, desc->march.t_stop, desc->march.max_steps);
  cvr::features_set_view(Q.F, inv_view, raster_to_view, full_res, tile_w, tile_h, off_x, off_y);
  cvr::preview_set_shading(Q, desc, volume_desc->light, medium->max_density);
  const cvr::ShadowGrid G = shadow_grid(volume, volume_desc->res, shadow);
  const cvr::FeatureHostTexels tex{medium->density, medium->albedo, medium->res[0], medium->res[1]};
  const bool shaded = !(desc->flags & CVR_PREVIEW_UNSHADED);
  for (uint32_t y = 0; y < tile_h; ++y)
    for (uint32_t x = 0; x < tile_w; ++x) {
      const cvr::PreviewOut f =
          shaded ? cvr::preview_shadowed_pixel<true>(tex, Q, G, x, y) : cvr::preview_shadowed_pixel<false>(tex, Q, G, x, y);
      float* o = out_rgba + 4 * ((size_t)y * tile_w + x);
      o[0] = f.r, o[1] = f.g, o[2] = f.b, o[3] = f.w;
    }
  return CVR_OK;
}

int cvr_preview_shadowed_buffers(cvr_ctx* c, const cvr_preview_desc* desc, float shadow, float* d_out_rgba) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !d_out_rgba) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = shadowed_check(c, desc, shadow);
  if (r) return r;
  if ((uintptr_t)d_out_rgba & 15u)
    return set_err(&c->err, CVR_ERR_INVALID, "shadowed preview: out_rgba must be 16-byte aligned");
  if ((r = cvr::ensure_device(c))) return r;
  return shadowed_launch(c, desc, shadow, reinterpret_cast<float4*>(d_out_rgba));
}

int cvr_preview_shadowed(cvr_ctx* c, const cvr_preview_desc* desc, float shadow, float* host_rgba, size_t host_floats) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !host_rgba) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = shadowed_check(c, desc, shadow);
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
  r = shadowed_launch(c, desc, shadow, stage ? stage : static_cast<float4*>(drgba));
  hipError_t e = hipStreamSynchronize(c->stream);
  if (!r && e == hipSuccess && stage) e = hipMemcpy(host_rgba, stage, px * sizeof(float4), hipMemcpyDeviceToHost);
  if (stage) (void)hipFree(stage);
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "shadowed preview: %s", hipGetErrorString(e));
  return CVR_OK;
}

}  // extern "C"
