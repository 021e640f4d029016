// cvr_project.h - the field projections (cvr_field_project*, include/cvr.h, CVR_HAS_FIELD_PROJECT):
// maximum, minimum and mean intensity projections of a raw scalar field and its first-hit
// isosurface lit by the field's own gradient, by the feature pass's deterministic march along the
// straight camera ray.  The one definition, compiled for the host statement
// (cvr_field_project_host) and for k_project (cvr_project.hip): the ray, the chord, the steps, the
// clamp and the trilinear are cvr_features.h's, the light's terms cvr_preview.h's, every further
// operation is fp32 in the order cvr.h writes (-ffp-contract=off, correctly rounded / and sqrt),
// so both sides return the same bits.  The texels come through a functor:
//   float value(x, y, z)      one voxel as a float (indices already clamped into the grid)
#pragma once

#include "cvr_preview.h"

namespace cvr {

enum { kProjectMax = 0, kProjectMin = 1, kProjectMean = 2, kProjectIso = 3 };  // cvr.h: CVR_PROJECT_*

// Everything a pixel reads besides the texels; filled once per call on the host
// (project_constants), passed by value to the kernel.  Of Q.F the density coordinate's shift and
// g, scale and t_stop are not read, of Q knee_abs is not.
struct ProjectParams {
  PreviewParams Q;
  float lo, hi;  // the display window of the three projections
  float iso;
  uint32_t refine;
  float colour[3];
};

// The descriptor's numbers (checked) for a field of `res` voxels; the camera and the tile:
// features_set_view.  light: not read with the headlight.
inline void project_constants(ProjectParams& R, const uint32_t res[3], const float bmin[3], const float bmax[3],
                              float step, uint32_t max_steps, float lo, float hi, float iso, uint32_t refine,
                              const float light[3], int headlight, float ambient, float diffuse, float specular,
                              uint32_t shininess_log2, const float colour[3], const float background[3]) {
  feature_geometry(R.Q.F, res, bmin, bmax, 0.0f, 1, step, 0.0f, max_steps);
  preview_constants(R.Q, light, headlight, ambient, diffuse, specular, shininess_log2, 0.0f, background, 0.0f);
  R.lo = lo;
  R.hi = hi;
  R.iso = iso;
  R.refine = refine;
  for (int a = 0; a < 3; ++a) R.colour[a] = colour[a];
}

// S(p): the field at world point p.  Voxel i sits at node i / (res - 1) of the box (feat_albedo's
// coordinate), lower corner floor, weights coordinate - corner, the 8 taps clamped by feat_texel,
// feat_trilerp8 (x, then y, then z).
template <class Tex>
CVR_HD float project_value(const Tex& tex, const FeatureParams& P, F3 p) {
  const float cx = ((p.x - P.bmin[0]) / P.ext[0]) * P.ag[0];
  const float cy = ((p.y - P.bmin[1]) / P.ext[1]) * P.ag[1];
  const float cz = ((p.z - P.bmin[2]) / P.ext[2]) * P.ag[2];
  const int x1 = det_floor_i32(cx), y1 = det_floor_i32(cy), z1 = det_floor_i32(cz);
  const float fx = cx - (float)x1, fy = cy - (float)y1, fz = cz - (float)z1;
  const uint32_t xa = feat_texel(x1, P.res[0]), xb = feat_texel(x1 + 1, P.res[0]);
  const uint32_t ya = feat_texel(y1, P.res[1]), yb = feat_texel(y1 + 1, P.res[1]);
  const uint32_t za = feat_texel(z1, P.res[2]), zb = feat_texel(z1 + 1, P.res[2]);
  float d[8];
  d[0] = tex.value(xa, ya, za), d[1] = tex.value(xb, ya, za);
  d[2] = tex.value(xa, yb, za), d[3] = tex.value(xb, yb, za);
  d[4] = tex.value(xa, ya, zb), d[5] = tex.value(xb, ya, zb);
  d[6] = tex.value(xa, yb, zb), d[7] = tex.value(xb, yb, zb);
  return feat_trilerp8(d, fx, fy, fz);
}

struct ProjectOut {
  float r, g, b, a, value, depth;
};

// The colour of the isosurface at p, ray direction d: the preview's gradient construction on S
// and its light, without a knee.
template <class Tex>
CVR_HD F3 project_shade(const Tex& tex, const ProjectParams& R, F3 p, F3 d) {
  const PreviewParams& Q = R.Q;
  const FeatureParams& P = Q.F;
  const float hx = Q.h[0], hy = Q.h[1], hz = Q.h[2];
  const float gx = (project_value(tex, P, F3{p.x + hx, p.y, p.z}) - project_value(tex, P, F3{p.x - hx, p.y, p.z})) / hx;
  const float gy = (project_value(tex, P, F3{p.x, p.y + hy, p.z}) - project_value(tex, P, F3{p.x, p.y - hy, p.z})) / hy;
  const float gz = (project_value(tex, P, F3{p.x, p.y, p.z + hz}) - project_value(tex, P, F3{p.x, p.y, p.z - hz})) / hz;
  PreviewTerms k;
  if (!preview_light_terms(Q, gx, gy, gz, d, k)) return F3{R.colour[0], R.colour[1], R.colour[2]};
  const float f = Q.ambient + Q.diffuse * k.nl;
  const float s = Q.specular * k.sp;
  return F3{f * R.colour[0] + s, f * R.colour[1] + s, f * R.colour[2] + s};
}

// One pixel of the pass, as cvr.h writes it.
template <class Tex, int Mode>
CVR_HD ProjectOut project_pixel(const Tex& tex, const ProjectParams& R, uint32_t ix, uint32_t iy) {
  const PreviewParams& Q = R.Q;
  const FeatureParams& P = Q.F;
  const ProjectOut none{Q.bg[0], Q.bg[1], Q.bg[2], 0.0f, 0.0f, 0.0f};
  F3 o, d;
  feat_ray(P, ix, iy, o, d);
  float t0, t1;
  if (!feat_chord(P, o, d, t0, t1)) return none;
  // the feature pass's step count: bounded by max_steps whatever the chord is
  const float q = __builtin_ceilf((t1 - t0) / P.delta);
  uint32_t n = P.max_steps;
  if (q < (float)P.max_steps) n = q > 0.0f ? (uint32_t)q : 0u;
  if (Mode == kProjectIso) {
    float tb = 0.0f, ta = 0.0f;
    uint32_t i = 0;
    bool hit = false;
    for (; i < n; ++i) {
      tb = t0 + ((float)i + 0.5f) * P.delta;
      if (!(tb < t1)) break;
      if (project_value(tex, P, F3{o.x + tb * d.x, o.y + tb * d.y, o.z + tb * d.z}) >= R.iso) {
        hit = true;
        break;
      }
      ta = tb;
    }
    if (!hit) return none;
    if (i > 0u)  // (i == 0: the cut face, where the box slices the solid)
      for (uint32_t r = 0; r < R.refine; ++r) {
        const float tm = ta + 0.5f * (tb - ta);
        if (project_value(tex, P, F3{o.x + tm * d.x, o.y + tm * d.y, o.z + tm * d.z}) >= R.iso)
          tb = tm;
        else
          ta = tm;
      }
    const F3 p{o.x + tb * d.x, o.y + tb * d.y, o.z + tb * d.z};
    const float value = project_value(tex, P, p);
    const F3 c = project_shade(tex, R, p, d);
    return ProjectOut{c.x, c.y, c.z, 1.0f, value, tb / P.diag};
  }
  float V = 0.0f, tz = 0.0f;
  uint32_t cnt = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const float t = t0 + ((float)i + 0.5f) * P.delta;
    if (!(t < t1)) break;  // dropped, and so is every later one (t does not decrease)
    const float v = project_value(tex, P, F3{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z});
    if (v != v) continue;
    if (Mode == kProjectMean) {
      V += v;
    } else if (cnt == 0u || (Mode == kProjectMax ? v > V : v < V)) {  // the first extremum wins
      V = v;
      tz = t;
    }
    ++cnt;
  }
  if (cnt == 0u) return none;
  const float value = Mode == kProjectMean ? V / (float)cnt : V;
  const float t = (value - R.lo) / (R.hi - R.lo);
  float u = t > 0.0f ? t : 0.0f;
  u = u < 1.0f ? u : 1.0f;
  return ProjectOut{u * R.colour[0], u * R.colour[1], u * R.colour[2], 1.0f, value, tz / P.diag};
}

// Host and device: a typed field, x fastest.  The index is below the voxel count, which the entry
// points hold below 2^32.
template <class T>
struct ProjectTexels {
  const T* s;
  uint32_t rx, ry;
  CVR_HD float value(uint32_t x, uint32_t y, uint32_t z) const { return (float)s[(z * ry + y) * rx + x]; }
};

// k_project on stream s: the tile of R.Q.F into out_rgba (tile float4), out_value and out_depth
// (tile floats each, may be null); device memory or the device address of pinned host memory.
// scalar: res product elements of scalar_type (cvr.h: CVR_SCALAR_*), aligned to its element.
hipError_t launch_project(const void* scalar, uint32_t scalar_type, int mode, const ProjectParams& R, float4* out_rgba,
                          float* out_value, float* out_depth, hipStream_t s);

}  // namespace cvr
