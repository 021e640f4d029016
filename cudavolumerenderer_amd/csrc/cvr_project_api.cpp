// cvr_project_api.cpp - C ABI of the field projections (cvr.h, CVR_HAS_FIELD_PROJECT): the host
// statement on a field in host memory and the device pass on one in device memory.  The context
// supplies the device, the stream, the camera and the tile and is otherwise only read.  The pass
// itself: cvr_project.h; the kernels: cvr_project.hip.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cvr_ctx.h"
#include "cvr_project.h"

using cvr::set_err;

namespace {

size_t scalar_size(uint32_t type) { return type == CVR_SCALAR_U8 ? 1 : type == CVR_SCALAR_F32 ? 4 : 2; }
bool weight_ok(float v) { return std::isfinite(v) && !(v < 0.0f); }

// The refusals of cvr.h in their order, rules 2 to 8 (rule 1, the NULL arguments, is the entry
// point's; 9 and 10 follow the tile)
int project_check(std::string* err, const cvr_field_desc* f, const cvr_project_desc* d) {
  const uint64_t voxels = (uint64_t)f->res[0] * f->res[1];  // < 2^64
  if (f->res[0] == 0 || f->res[1] == 0 || f->res[2] == 0) return set_err(err, CVR_ERR_INVALID, "empty field");
  if (voxels > 0xFFFFFFFFull || voxels * f->res[2] > 0xFFFFFFFFull)
    return set_err(err, CVR_ERR_INVALID, "field of %u x %u x %u voxels: more than 2^32 - 1", f->res[0], f->res[1],
                   f->res[2]);
  if (f->scalar_type > CVR_SCALAR_I16) return set_err(err, CVR_ERR_INVALID, "unknown scalar_type %u", f->scalar_type);
  if (d->mode > CVR_PROJECT_ISO) return set_err(err, CVR_ERR_INVALID, "project: unknown mode %u", d->mode);
  if (d->flags & ~CVR_PROJECT_HEADLIGHT) return set_err(err, CVR_ERR_INVALID, "project: unknown flags 0x%x", d->flags);
  if (f->reserved || d->reserved)
    return set_err(err, CVR_ERR_INVALID, "project: reserved 0x%x (field), 0x%x: both must be 0", f->reserved, d->reserved);
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(d->box_min[a]) || !std::isfinite(d->box_max[a]) || !(d->box_max[a] > d->box_min[a]))
      return set_err(err, CVR_ERR_INVALID, "project: box axis %d is %g .. %g: finite and box_max > box_min", a,
                     (double)d->box_min[a], (double)d->box_max[a]);
  if (!(d->step >= 0.125f && d->step <= 8.0f))
    return set_err(err, CVR_ERR_INVALID, "project: step %g not in [1/8, 8]", (double)d->step);
  if (d->max_steps < 1u || d->max_steps > 65536u)
    return set_err(err, CVR_ERR_INVALID, "project: max_steps %u not in 1..65536", d->max_steps);
  if (d->mode != CVR_PROJECT_ISO) {
    if (!std::isfinite(d->lo) || !std::isfinite(d->hi) || !(d->hi > d->lo))
      return set_err(err, CVR_ERR_INVALID, "project: window lo %g, hi %g: both finite and hi > lo", (double)d->lo,
                     (double)d->hi);
  } else {
    if (!std::isfinite(d->iso)) return set_err(err, CVR_ERR_INVALID, "project: iso %g must be finite", (double)d->iso);
    if (d->refine > 8u) return set_err(err, CVR_ERR_INVALID, "project: refine %u not in 0..8", d->refine);
    if (!weight_ok(d->ambient) || !weight_ok(d->diffuse) || !weight_ok(d->specular))
      return set_err(err, CVR_ERR_INVALID, "project: ambient %g, diffuse %g, specular %g must be finite and >= 0",
                     (double)d->ambient, (double)d->diffuse, (double)d->specular);
    if (d->shininess_log2 > 10u)
      return set_err(err, CVR_ERR_INVALID, "project: shininess_log2 %u not in 0..10", d->shininess_log2);
    if (!(d->flags & CVR_PROJECT_HEADLIGHT)) {
      // the length as preview_constants computes it: components that underflow or overflow it are refused too
      const float* l = d->light;
      const float len = det_sqrtf((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
      if (!std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2]) || !(len > 0.0f) || !std::isfinite(len))
        return set_err(err, CVR_ERR_INVALID, "project: the light direction must be finite and of a length above zero");
    }
  }
  for (int a = 0; a < 3; ++a)
    if (!weight_ok(d->colour[a]) || !weight_ok(d->background[a]))
      return set_err(err, CVR_ERR_INVALID, "project: colour %g, background %g must be finite and >= 0",
                     (double)d->colour[a], (double)d->background[a]);
  return CVR_OK;
}

int tile_check(std::string* err, uint32_t w, uint32_t h) {
  if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 24))
    return set_err(err, CVR_ERR_INVALID, "project: a %ux%u tile (1 to 2^24 pixels)", w, h);
  return CVR_OK;
}

// Rules 9 and 10 but the device's part
int pointer_check(std::string* err, const cvr_field_desc* f, const float* rgba, size_t rgba_align, const float* value,
                  const float* depth) {
  if (!f->scalar) return set_err(err, CVR_ERR_INVALID, "scalar is NULL");
  if (!rgba) return set_err(err, CVR_ERR_INVALID, "project: out_rgba is NULL");
  const size_t size = scalar_size(f->scalar_type);
  if ((uintptr_t)f->scalar & (size - 1)) return set_err(err, CVR_ERR_INVALID, "scalar must be %zu-byte aligned", size);
  if ((uintptr_t)rgba & (rgba_align - 1))
    return set_err(err, CVR_ERR_INVALID, "project: out_rgba must be %zu-byte aligned", rgba_align);
  if (((uintptr_t)value & 3u) || ((uintptr_t)depth & 3u))
    return set_err(err, CVR_ERR_INVALID, "project: out_value and out_depth must be 4-byte aligned");
  return CVR_OK;
}

int device_check(cvr_ctx* c, const void* p, const char* name) {
  if (p && !cvr::device_readable(c, p))
    return set_err(&c->err, CVR_ERR_INVALID, "%s is not device-accessible memory of device %d", name, c->device);
  return CVR_OK;
}

cvr::ProjectParams params_of(const cvr_field_desc* f, const cvr_project_desc* d) {
  cvr::ProjectParams R{};
  const bool iso = d->mode == CVR_PROJECT_ISO;
  const int headlight = !iso || (d->flags & CVR_PROJECT_HEADLIGHT);  // (the projections read no light)
  cvr::project_constants(R, f->res, d->box_min, d->box_max, d->step, d->max_steps, iso ? 0.0f : d->lo,
                         iso ? 1.0f : d->hi, iso ? d->iso : 0.0f, iso ? d->refine : 0u, d->light, headlight,
                         iso ? d->ambient : 0.0f, iso ? d->diffuse : 0.0f, iso ? d->specular : 0.0f,
                         iso ? d->shininess_log2 : 0u, d->colour, d->background);
  return R;
}

template <class T, int Mode>
void host_tile(const cvr_field_desc* f, const cvr::ProjectParams& R, float* rgba, float* value, float* depth) {
  const cvr::FeatureParams& P = R.Q.F;
  const cvr::ProjectTexels<T> tex{static_cast<const T*>(f->scalar), f->res[0], f->res[1]};
  for (uint32_t y = 0; y < P.tile_h; ++y)
    for (uint32_t x = 0; x < P.tile_w; ++x) {
      const cvr::ProjectOut o = cvr::project_pixel<cvr::ProjectTexels<T>, Mode>(tex, R, x, y);
      const size_t i = (size_t)y * P.tile_w + x;
      rgba[4 * i] = o.r, rgba[4 * i + 1] = o.g, rgba[4 * i + 2] = o.b, rgba[4 * i + 3] = o.a;
      if (value) value[i] = o.value;
      if (depth) depth[i] = o.depth;
    }
}

template <class T>
void host_typed(const cvr_field_desc* f, uint32_t mode, const cvr::ProjectParams& R, float* rgba, float* value,
                float* depth) {
  switch (mode) {
    case CVR_PROJECT_MAX: host_tile<T, cvr::kProjectMax>(f, R, rgba, value, depth); break;
    case CVR_PROJECT_MIN: host_tile<T, cvr::kProjectMin>(f, R, rgba, value, depth); break;
    case CVR_PROJECT_MEAN: host_tile<T, cvr::kProjectMean>(f, R, rgba, value, depth); break;
    default: host_tile<T, cvr::kProjectIso>(f, R, rgba, value, depth); break;
  }
}

// Rule 1 and the state of a context call, then rules 2 to 8 and the tile
int ctx_check(cvr_ctx* c, const cvr_field_desc* f, const cvr_project_desc* d) {
  if (!c || !f || !d) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->have_camera) return set_err(&c->err, CVR_ERR_STATE, "camera not set (cvr_set_camera)");
  if (c->tile_w == 0 || c->tile_h == 0) return set_err(&c->err, CVR_ERR_STATE, "resolution not set");
  if (int r = project_check(&c->err, f, d)) return r;
  return tile_check(&c->err, c->tile_w, c->tile_h);
}

int ctx_launch(cvr_ctx* c, const cvr_field_desc* f, const cvr_project_desc* d, float4* rgba, float* value, float* depth) {
  cvr::ProjectParams R = params_of(f, d);
  cvr::features_set_view(R.Q.F, c->inv_view, c->r2v, c->full_res, c->tile_w, c->tile_h, c->off[0], c->off[1]);
  HIP_TRY(c, cvr::launch_project(f->scalar, f->scalar_type, (int)d->mode, R, rgba, value, depth, c->stream));
  return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_field_project_host(const cvr_field_desc* f, const cvr_project_desc* d, const float inv_view[12],
                           const float raster_to_view[2], const float full_res[2], uint32_t tile_w, uint32_t tile_h,
                           uint32_t off_x, uint32_t off_y, float* out_rgba, float* out_value, float* out_depth) {
  if (!f || !d || !inv_view || !raster_to_view || !full_res) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (int r = project_check(nullptr, f, d)) return r;
  if (int r = tile_check(nullptr, tile_w, tile_h)) return r;
  if (int r = pointer_check(nullptr, f, out_rgba, 16, out_value, out_depth)) return r;
  cvr::ProjectParams R = params_of(f, d);
  cvr::features_set_view(R.Q.F, inv_view, raster_to_view, full_res, tile_w, tile_h, off_x, off_y);
  switch (f->scalar_type) {
    case CVR_SCALAR_U8: host_typed<uint8_t>(f, d->mode, R, out_rgba, out_value, out_depth); break;
    case CVR_SCALAR_U16: host_typed<uint16_t>(f, d->mode, R, out_rgba, out_value, out_depth); break;
    case CVR_SCALAR_I16: host_typed<int16_t>(f, d->mode, R, out_rgba, out_value, out_depth); break;
    default: host_typed<float>(f, d->mode, R, out_rgba, out_value, out_depth); break;
  }
  return CVR_OK;
}

int cvr_field_project_buffers(cvr_ctx* c, const cvr_field_desc* f, const cvr_project_desc* d, float* d_out_rgba,
                              float* d_out_value, float* d_out_depth) {
  int r = ctx_check(c, f, d);
  if (r) return r;
  if ((r = pointer_check(&c->err, f, d_out_rgba, 16, d_out_value, d_out_depth))) return r;
  if ((r = cvr::ensure_device(c))) return r;
  if ((r = device_check(c, f->scalar, "scalar")) || (r = device_check(c, d_out_rgba, "d_out_rgba")) ||
      (r = device_check(c, d_out_value, "d_out_value")) || (r = device_check(c, d_out_depth, "d_out_depth")))
    return r;
  return ctx_launch(c, f, d, reinterpret_cast<float4*>(d_out_rgba), d_out_value, d_out_depth);
}

int cvr_field_project(cvr_ctx* c, const cvr_field_desc* f, const cvr_project_desc* d, float* host_rgba,
                      float* host_value, float* host_depth, size_t host_floats) {
  int r = ctx_check(c, f, d);
  if (r) return r;
  const size_t px = (size_t)c->tile_w * c->tile_h;
  if (host_rgba && host_floats < px * 4u)
    return set_err(&c->err, CVR_ERR_INVALID, "host image holds %zu floats, the %ux%u tile needs %zu", host_floats,
                   c->tile_w, c->tile_h, px * 4u);
  if ((r = pointer_check(&c->err, f, host_rgba, 4, host_value, host_depth))) return r;
  if ((r = cvr::ensure_device(c))) return r;
  if ((r = device_check(c, f->scalar, "scalar"))) return r;
  // pinned or registered memory is stored into by the kernel, other memory through a staging copy:
  // [rgba: px float4][value: px floats][depth: px floats], each part only if staged
  float* host[3] = {host_rgba, host_value, host_depth};
  const size_t floats[3] = {px * 4u, px, px};
  void* dev[3] = {nullptr, nullptr, nullptr};
  size_t at[3] = {0, 0, 0}, stage_floats = 0;
  for (int k = 0; k < 3; ++k) {
    if (!host[k]) continue;
    if (((uintptr_t)host[k] & (k == 0 ? 15u : 3u)) || hipHostGetDevicePointer(&dev[k], host[k], 0) != hipSuccess) {
      dev[k] = nullptr;
      at[k] = stage_floats;
      stage_floats += floats[k];
    }
  }
  (void)hipGetLastError();  // pageable memory: not an error
  float* stage = nullptr;
  if (stage_floats) HIP_TRY(c, hipMalloc((void**)&stage, stage_floats * sizeof(float)));
  float* out[3];
  for (int k = 0; k < 3; ++k) out[k] = !host[k] ? nullptr : dev[k] ? static_cast<float*>(dev[k]) : stage + at[k];
  r = ctx_launch(c, f, d, reinterpret_cast<float4*>(out[0]), out[1], out[2]);
  hipError_t e = hipStreamSynchronize(c->stream);
  for (int k = 0; k < 3; ++k)
    if (!r && e == hipSuccess && host[k] && !dev[k])
      e = hipMemcpy(host[k], stage + at[k], floats[k] * sizeof(float), hipMemcpyDeviceToHost);
  if (stage) (void)hipFree(stage);
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "cvr_field_project: %s", hipGetErrorString(e));
  return CVR_OK;
}

}  // extern "C"
