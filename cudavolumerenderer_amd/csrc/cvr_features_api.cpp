// cvr_features_api.cpp - C ABI of the primary-ray feature pass (cvr.h, CVR_HAS_FEATURES): the host
// statement on a dense medium's host arrays and the device pass on the medium a context holds.
// The pass itself: cvr_features.h; the kernel: cvr_features.hip.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cvr_ctx.h"
#include "cvr_features.h"

using cvr::set_err;

int cvr::features_desc_check(std::string* err, const cvr_features_desc* d) {
  if (!d) return set_err(err, CVR_ERR_INVALID, "NULL features descriptor");
  if (!(d->step >= 0.125f && d->step <= 8.0f))
    return set_err(err, CVR_ERR_INVALID, "features: step %g not in [1/8, 8]", (double)d->step);
  if (!(d->t_stop >= 0.0f && d->t_stop < 1.0f))
    return set_err(err, CVR_ERR_INVALID, "features: t_stop %g not in [0, 1)", (double)d->t_stop);
  if (d->max_steps < 1u || d->max_steps > 65536u)
    return set_err(err, CVR_ERR_INVALID, "features: max_steps %u not in 1..65536", d->max_steps);
  if (d->flags != 0u) return set_err(err, CVR_ERR_INVALID, "features: flags must be 0");
  return CVR_OK;
}

int cvr::features_tile_check(std::string* err, uint32_t w, uint32_t h) {
  if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 24))
    return set_err(err, CVR_ERR_INVALID, "features: a %ux%u tile (1 to 2^24 pixels)", w, h);
  return CVR_OK;
}

void cvr::features_set_view(cvr::FeatureParams& P, const float inv_view[12], const float r2v[2],
                            const float full_res[2], uint32_t tile_w, uint32_t tile_h, uint32_t off_x, uint32_t off_y) {
  for (int i = 0; i < 12; ++i) P.M[i] = inv_view[i];
  P.r2v[0] = r2v[0], P.r2v[1] = r2v[1];
  P.full_res[0] = full_res[0], P.full_res[1] = full_res[1];
  P.off[0] = off_x, P.off[1] = off_y;
  P.tile_w = tile_w, P.tile_h = tile_h;
}

// The pass for the context's medium, camera, tile and offset (checked: ready, desc valid)
cvr::FeatureParams cvr::features_ctx_params(const cvr_ctx* c, const cvr_features_desc* d) {
  cvr::FeatureParams P{};
  const uint32_t res[3] = {c->m.rx, c->m.ry, c->m.rz};
  const float bmin[3] = {c->m.bmin.x, c->m.bmin.y, c->m.bmin.z}, bmax[3] = {c->m.bmax.x, c->m.bmax.y, c->m.bmax.z};
  cvr::feature_geometry(P, res, bmin, bmax, c->m.scale, c->world_to_aabb, d->step, d->t_stop, d->max_steps);
  features_set_view(P, c->inv_view, c->r2v, c->full_res, c->tile_w, c->tile_h, c->off[0], c->off[1]);
  return P;
}

int cvr::features_check(cvr_ctx* c, const cvr_features_desc* d) {
  if (!c->have_medium) return set_err(&c->err, CVR_ERR_STATE, "medium not set (cvr_set_medium)");
  if (!c->have_camera) return set_err(&c->err, CVR_ERR_STATE, "camera not set (cvr_set_camera)");
  if (c->tile_w == 0 || c->tile_h == 0) return set_err(&c->err, CVR_ERR_STATE, "resolution not set");
  int r = features_desc_check(&c->err, d);
  if (r) return r;
  return features_tile_check(&c->err, c->tile_w, c->tile_h);
}

int cvr::features_launch(cvr_ctx* c, const cvr_features_desc* d, float4* rgba, float* depth) {
  cvr::MediumParams m = c->m;
  if (!c->empty_mask) m.emask = nullptr;  // CVR_OPT_EMPTY_MASK 0: every point loads its brick word
  HIP_TRY(c, cvr::launch_features(m, features_ctx_params(c, d), rgba, depth, c->stream));
  return CVR_OK;
}

extern "C" {

int cvr_features_host(const cvr_medium_desc* medium, const float inv_view[12], const float raster_to_view[2],
                      const float full_res[2], uint32_t tile_w, uint32_t tile_h, uint32_t off_x, uint32_t off_y,
                      int world_to_aabb, const cvr_features_desc* desc, float* out_rgba, float* out_depth) {
  if (!medium || !inv_view || !raster_to_view || !full_res || !desc || !out_rgba)
    return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!medium->density || !medium->albedo) return set_err(nullptr, CVR_ERR_INVALID, "NULL medium array");
  if (medium->res[0] == 0 || medium->res[1] == 0 || medium->res[2] == 0)
    return set_err(nullptr, CVR_ERR_INVALID, "empty grid");
  if (world_to_aabb != 0 && world_to_aabb != 1)
    return set_err(nullptr, CVR_ERR_INVALID, "features: world_to_aabb must be 0 or 1");
  int r = cvr::features_desc_check(nullptr, desc);
  if (r) return r;
  if ((r = cvr::features_tile_check(nullptr, tile_w, tile_h))) return r;
  cvr::FeatureParams P{};
  cvr::feature_geometry(P, medium->res, medium->box_min, medium->box_max, medium->scale, world_to_aabb, desc->step,
                        desc->t_stop, desc->max_steps);
  cvr::features_set_view(P, inv_view, raster_to_view, full_res, tile_w, tile_h, off_x, off_y);
  const cvr::FeatureHostTexels tex{medium->density, medium->albedo, medium->res[0], medium->res[1]};
  for (uint32_t y = 0; y < tile_h; ++y)
    for (uint32_t x = 0; x < tile_w; ++x) {
      const cvr::FeatureOut f = cvr::feature_pixel(tex, P, x, y);
      const size_t i = (size_t)y * tile_w + x;
      out_rgba[4 * i] = f.r;
      out_rgba[4 * i + 1] = f.g;
      out_rgba[4 * i + 2] = f.b;
      out_rgba[4 * i + 3] = f.w;
      if (out_depth) out_depth[i] = f.depth;
    }
  return CVR_OK;
}

int cvr_features_buffers(cvr_ctx* c, const cvr_features_desc* desc, float* d_out_rgba, float* d_out_depth) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !d_out_rgba) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = cvr::features_check(c, desc);
  if (r) return r;
  if ((uintptr_t)d_out_rgba & 15u) return set_err(&c->err, CVR_ERR_INVALID, "features: out_rgba must be 16-byte aligned");
  if ((uintptr_t)d_out_depth & 3u) return set_err(&c->err, CVR_ERR_INVALID, "features: out_depth must be 4-byte aligned");
  if ((r = cvr::ensure_device(c))) return r;
  return cvr::features_launch(c, desc, reinterpret_cast<float4*>(d_out_rgba), d_out_depth);
}

int cvr_features(cvr_ctx* c, const cvr_features_desc* desc, float* host_rgba, float* host_depth, size_t host_floats) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (!desc || !host_rgba) return set_err(&c->err, CVR_ERR_INVALID, "NULL argument");
  int r = cvr::features_check(c, desc);
  if (r) return r;
  const size_t px = (size_t)c->tile_w * c->tile_h;
  if (host_floats < px * 4u)
    return set_err(&c->err, CVR_ERR_INVALID, "host image holds %zu floats, the %ux%u tile needs %zu", host_floats,
                   c->tile_w, c->tile_h, px * 4u);
  if ((r = cvr::ensure_device(c))) return r;
  // pinned or registered memory is stored into by the kernel, other memory through a staging copy
  void *drgba = nullptr, *ddepth = nullptr;
  if (((uintptr_t)host_rgba & 15u) || hipHostGetDevicePointer(&drgba, host_rgba, 0) != hipSuccess) drgba = nullptr;
  if (host_depth && (((uintptr_t)host_depth & 3u) || hipHostGetDevicePointer(&ddepth, host_depth, 0) != hipSuccess))
    ddepth = nullptr;
  (void)hipGetLastError();  // pageable memory: not an error
  const bool stage_rgba = !drgba, stage_depth = host_depth && !ddepth;
  float4* stage = nullptr;  // [rgba: px float4][depth: px floats], each part only if staged
  if (stage_rgba || stage_depth)
    HIP_TRY(c, hipMalloc(&stage, (stage_rgba ? px * sizeof(float4) : 0) + (stage_depth ? px * sizeof(float) : 0)));
  float4* o_rgba = stage_rgba ? stage : static_cast<float4*>(drgba);
  float* s_depth = reinterpret_cast<float*>(stage + (stage_rgba ? px : 0));
  float* o_depth = !host_depth ? nullptr : stage_depth ? s_depth : static_cast<float*>(ddepth);
  r = cvr::features_launch(c, desc, o_rgba, o_depth);
  hipError_t e = hipStreamSynchronize(c->stream);
  if (!r && e == hipSuccess && stage_rgba) e = hipMemcpy(host_rgba, stage, px * sizeof(float4), hipMemcpyDeviceToHost);
  if (!r && e == hipSuccess && stage_depth) e = hipMemcpy(host_depth, s_depth, px * sizeof(float), hipMemcpyDeviceToHost);
  if (stage) (void)hipFree(stage);
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "features: %s", hipGetErrorString(e));
  return CVR_OK;
}

}  // extern "C"
