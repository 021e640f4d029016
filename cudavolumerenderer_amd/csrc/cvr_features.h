// cvr_features.h - the primary-ray feature pass (cvr_features*, include/cvr.h): opacity, mean
// first-collision albedo and mean collision depth of the straight camera ray through a pixel's
// centre, by one deterministic ray march.  The one definition, compiled for the host statement
// (cvr_features_host) and for k_features (cvr_features.hip): fp32 only, every operation in the
// order cvr.h writes (-ffp-contract=off, correctly rounded / and sqrt, the only fused
// multiply-adds the det_fmaf of the trilinear lerps and of the grid coordinate), so both sides
// return the same bits.  The texels come through a functor:
//   float density(x, y, z)            one density voxel (indices already clamped into the grid)
//   F3    albedo(x, y, z)             one albedo voxel's rgb
//   int   cell(x1, y1, z1, float d[8]) the 8 texel-clamped corners of the cell whose lower corner
//                                     (x1, y1, z1) lies in the grid, as d000, d001, d010, d011, d100,
//                                     d101, d110, d111 (d{z}{y}{x}): 1 filled; 0 not available (the
//                                     caller takes the 8 density() taps: the same values); 2 the 8
//                                     corners are known to be +0 without a load (exact skipping)
// so the order of the arithmetic does not depend on where the medium is kept.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvr_detmath.h"

namespace cvr {

struct F3 {
  float x, y, z;
};

// Everything a pixel's march reads besides the texels; filled once per call on the host
// (feature_geometry + the caller's camera, tile and descriptor), passed by value to the kernel.
struct FeatureParams {
  float M[12], r2v[2], full_res[2];  // the camera (cvr_set_camera)
  uint32_t off[2], tile_w, tile_h;
  uint32_t res[3];
  float fres[3];            // (float)res
  float bmin[3], bmax[3];
  float ext[3];             // bmax - bmin
  float shift[3], g[3];     // density coordinate c = (p - shift) * g (MediumParams::shift, gx; quirk Q4)
  float ag[3];              // (float)(res - 1): the albedo coordinate's grid scale
  float scale;
  float delta;              // step * min_a(ext_a / res_a)
  float diag;               // |bmax - bmin|
  float t_stop;
  uint32_t max_steps;
};

// The box, the grid and the march's constants.  w2a: CVR_OPT_WORLD_TO_AABB.
inline void feature_geometry(FeatureParams& P, const uint32_t res[3], const float bmin[3], const float bmax[3],
                             float scale, int w2a, float step, float t_stop, uint32_t max_steps) {
  for (int a = 0; a < 3; ++a) {
    P.res[a] = res[a];
    P.fres[a] = (float)res[a];
    P.bmin[a] = bmin[a];
    P.bmax[a] = bmax[a];
    P.ext[a] = bmax[a] - bmin[a];
    P.ag[a] = (float)(res[a] - 1u);
    P.shift[a] = w2a ? bmin[a] : bmin[a] / P.ext[a];
    P.g[a] = w2a ? P.ag[a] / P.ext[a] : P.ag[a];
  }
  P.scale = scale;
  const float cx = P.ext[0] / P.fres[0], cy = P.ext[1] / P.fres[1], cz = P.ext[2] / P.fres[2];
  P.delta = step * det_fminf(det_fminf(cx, cy), cz);
  P.diag = det_sqrtf((P.ext[0] * P.ext[0] + P.ext[1] * P.ext[1]) + P.ext[2] * P.ext[2]);
  P.t_stop = t_stop;
  P.max_steps = max_steps;
}

// Volume.h:47-69's clamp, lerp and 8-tap trilinear, as cvr_walk.h's texel / lerpf / trilerp8
CVR_HD uint32_t feat_texel(int i, uint32_t res) {
  const uint32_t u = (uint32_t)i;
  return u < res - 1u ? u : res - 1u;
}
CVR_HD float feat_lerp(float a, float b, float f, float fi) { return det_fmaf(b, f, a * fi); }
CVR_HD float feat_trilerp8(const float d[8], float fx, float fy, float fz) {
  const float _fx = 1.0f - fx, _fy = 1.0f - fy, _fz = 1.0f - fz;
  const float a = feat_lerp(feat_lerp(d[0], d[1], fx, _fx), feat_lerp(d[2], d[3], fx, _fx), fy, _fy);
  const float b = feat_lerp(feat_lerp(d[4], d[5], fx, _fx), feat_lerp(d[6], d[7], fx, _fx), fy, _fy);
  return feat_lerp(a, b, fz, _fz);
}

// The walk's interpolated density at world point p (woodcock_coords + woodcock_density /
// density_lookup_gather): c = p - shift, grid coordinate fma(c, g, +0) (the product, a -0 becoming
// +0), lower corner floor, weights coordinate - corner, the 8 taps clamped as the reference's
// point-sampled texture (the uint wrap of quirk Q5 included).
template <class Tex>
CVR_HD float feat_density(const Tex& tex, const FeatureParams& P, F3 p) {
  const float cx = det_fmaf(p.x - P.shift[0], P.g[0], 0.0f);
  const float cy = det_fmaf(p.y - P.shift[1], P.g[1], 0.0f);
  const float cz = det_fmaf(p.z - P.shift[2], P.g[2], 0.0f);
  const int x1 = det_floor_i32(cx), y1 = det_floor_i32(cy), z1 = det_floor_i32(cz);
  const float fx = cx - (float)x1, fy = cy - (float)y1, fz = cz - (float)z1;
  // 0 <= c < res on every axis, as woodcock_coords tests it (c is never -0; NaN fails)
  const bool in = ((int)(det_f2u(cx) < det_f2u(P.fres[0])) & (int)(det_f2u(cy) < det_f2u(P.fres[1])) &
                   (int)(det_f2u(cz) < det_f2u(P.fres[2]))) != 0;
  float d[8];
  const int have = in ? tex.cell((uint32_t)x1, (uint32_t)y1, (uint32_t)z1, d) : 0;
  if (have == 2) return 0.0f;  // trilinear of eight +0
  if (have == 0) {
    const uint32_t xa = feat_texel(x1, P.res[0]), xb = feat_texel(x1 + 1, P.res[0]);
    const uint32_t ya = feat_texel(y1, P.res[1]), yb = feat_texel(y1 + 1, P.res[1]);
    const uint32_t za = feat_texel(z1, P.res[2]), zb = feat_texel(z1 + 1, P.res[2]);
    d[0] = tex.density(xa, ya, za), d[1] = tex.density(xb, ya, za);
    d[2] = tex.density(xa, yb, za), d[3] = tex.density(xb, yb, za);
    d[4] = tex.density(xa, ya, zb), d[5] = tex.density(xb, ya, zb);
    d[6] = tex.density(xa, yb, zb), d[7] = tex.density(xb, yb, zb);
  }
  return feat_trilerp8(d, fx, fy, fz);
}

// The walk's albedo at world point p (scatter_event's coordinate (p - bmin) / (bmax - bmin) and
// albedo_lookup's operations, one z plane at a time).
template <class Tex>
CVR_HD F3 feat_albedo(const Tex& tex, const FeatureParams& P, F3 p) {
  const float cx = ((p.x - P.bmin[0]) / P.ext[0]) * P.ag[0];
  const float cy = ((p.y - P.bmin[1]) / P.ext[1]) * P.ag[1];
  const float cz = ((p.z - P.bmin[2]) / P.ext[2]) * P.ag[2];
  const int x1 = det_floor_i32(cx), y1 = det_floor_i32(cy), z1 = det_floor_i32(cz);
  const float fx = cx - (float)x1, fy = cy - (float)y1, fz = cz - (float)z1;
  const float _fx = 1.0f - fx, _fy = 1.0f - fy, _fz = 1.0f - fz;
  const uint32_t xa = feat_texel(x1, P.res[0]), xb = feat_texel(x1 + 1, P.res[0]);
  const uint32_t ya = feat_texel(y1, P.res[1]), yb = feat_texel(y1 + 1, P.res[1]);
  const uint32_t za = feat_texel(z1, P.res[2]), zb = feat_texel(z1 + 1, P.res[2]);
  F3 a, b;
  {
    const F3 d00 = tex.albedo(xa, ya, za), d01 = tex.albedo(xb, ya, za);
    const F3 d10 = tex.albedo(xa, yb, za), d11 = tex.albedo(xb, yb, za);
    a.x = feat_lerp(feat_lerp(d00.x, d01.x, fx, _fx), feat_lerp(d10.x, d11.x, fx, _fx), fy, _fy);
    a.y = feat_lerp(feat_lerp(d00.y, d01.y, fx, _fx), feat_lerp(d10.y, d11.y, fx, _fx), fy, _fy);
    a.z = feat_lerp(feat_lerp(d00.z, d01.z, fx, _fx), feat_lerp(d10.z, d11.z, fx, _fx), fy, _fy);
  }
  {
    const F3 d00 = tex.albedo(xa, ya, zb), d01 = tex.albedo(xb, ya, zb);
    const F3 d10 = tex.albedo(xa, yb, zb), d11 = tex.albedo(xb, yb, zb);
    b.x = feat_lerp(feat_lerp(d00.x, d01.x, fx, _fx), feat_lerp(d10.x, d11.x, fx, _fx), fy, _fy);
    b.y = feat_lerp(feat_lerp(d00.y, d01.y, fx, _fx), feat_lerp(d10.y, d11.y, fx, _fx), fy, _fy);
    b.z = feat_lerp(feat_lerp(d00.z, d01.z, fx, _fx), feat_lerp(d10.z, d11.z, fx, _fx), fy, _fy);
  }
  return F3{feat_lerp(a.x, b.x, fz, _fz), feat_lerp(a.y, b.y, fz, _fz), feat_lerp(a.z, b.z, fz, _fz)};
}

// camera_ray (cvr_walk.h) of tile pixel (ix, iy) with both jitters 0.5f: the pixel's centre.
CVR_HD void feat_ray(const FeatureParams& P, uint32_t ix, uint32_t iy, F3& o, F3& d) {
  const float px = (float)ix + (float)P.off[0];
  const float py = (float)iy + (float)P.off[1];
  float rx = ((px + 0.5f) * 2.0f) / P.full_res[0] - 1.0f;
  float ry = ((py + 0.5f) * 2.0f) / P.full_res[1] - 1.0f;
  rx = P.r2v[0] * rx;
  ry = P.r2v[1] * ry;
  const float* M = P.M;
  o = F3{0.0f * M[0] + 0.0f * M[1] + 0.0f * M[2] + 1.0f * M[3], 0.0f * M[4] + 0.0f * M[5] + 0.0f * M[6] + 1.0f * M[7],
         0.0f * M[8] + 0.0f * M[9] + 0.0f * M[10] + 1.0f * M[11]};
  const float inv = 1.0f / det_sqrtf(rx * rx + ry * ry + 1.0f * 1.0f);
  const F3 v{rx * inv, ry * inv, 1.0f * inv};
  d = F3{v.x * M[0] + v.y * M[1] + v.z * M[2], v.x * M[4] + v.y * M[5] + v.z * M[6],
         v.x * M[8] + v.y * M[9] + v.z * M[10]};
}

// The chord of the ray in the box: aabb_intersect's slab operations (cvr_walk.h), so +-0
// direction components and NaN order as they do for the walk: per axis tbot = (1 / d)(bmin - o),
// ttop = (1 / d)(bmax - o), lo = det_fminf(ttop, tbot), hi = det_fmaxf(ttop, tbot) (one NaN
// operand gives the other), enter = max(max(lo_x, lo_y), max(lo_x, lo_z)), t1 = min(min(hi_x,
// hi_y), min(hi_x, hi_z)) with the same two functions, t0 = enter > 0 ? enter : 0.  There is a
// chord iff t1 > enter and t1 > t0 (a NaN compares false: none).
CVR_HD bool feat_chord(const FeatureParams& P, F3 o, F3 d, float& t0, float& t1) {
  const float ix = 1.0f / d.x, iy = 1.0f / d.y, iz = 1.0f / d.z;
  const float bx = ix * (P.bmin[0] - o.x), by = iy * (P.bmin[1] - o.y), bz = iz * (P.bmin[2] - o.z);
  const float tx = ix * (P.bmax[0] - o.x), ty = iy * (P.bmax[1] - o.y), tz = iz * (P.bmax[2] - o.z);
  const float lx = det_fminf(tx, bx), ly = det_fminf(ty, by), lz = det_fminf(tz, bz);
  const float hx = det_fmaxf(tx, bx), hy = det_fmaxf(ty, by), hz = det_fmaxf(tz, bz);
  const float enter = det_fmaxf(det_fmaxf(lx, ly), det_fmaxf(lx, lz));
  t1 = det_fminf(det_fminf(hx, hy), det_fminf(hx, hz));
  t0 = enter > 0.0f ? enter : 0.0f;
  return (t1 > enter) && (t1 > t0);
}

struct FeatureOut {
  float r, g, b, w, depth;
};

// One pixel of the pass, as cvr.h writes it.
template <class Tex>
CVR_HD FeatureOut feature_pixel(const Tex& tex, const FeatureParams& P, uint32_t ix, uint32_t iy) {
  FeatureOut out{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  F3 o, d;
  feat_ray(P, ix, iy, o, d);
  float t0, t1;
  if (!feat_chord(P, o, d, t0, t1)) return out;
  // n = min(max_steps, ceil((t1 - t0) / delta)); anything that is not a count below max_steps
  // (NaN, inf) marches max_steps, a non-positive quotient none: the loop is bounded either way
  const float q = __builtin_ceilf((t1 - t0) / P.delta);
  uint32_t n = P.max_steps;
  if (q < (float)P.max_steps) n = q > 0.0f ? (uint32_t)q : 0u;
  float T = 1.0f, Ar = 0.0f, Ag = 0.0f, Ab = 0.0f, Z = 0.0f, W = 0.0f;
  for (uint32_t i = 0; i < n; ++i) {
    const float t = t0 + ((float)i + 0.5f) * P.delta;
    if (!(t < t1)) break;  // dropped, and so is every later one (t does not decrease)
    const F3 p{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};
    const float rho = feat_density(tex, P, p);
    const float s = (P.scale * rho) * P.delta;
    if (!(s > 0.0f)) continue;
    const float a = s / (1.0f + s);
    const float w = T * a;
    const F3 c = feat_albedo(tex, P, p);
    Ar += w * c.x;
    Ag += w * c.y;
    Ab += w * c.z;
    Z += w * t;
    W += w;
    T = T - w;
    if (T < P.t_stop) break;
  }
  if (W == 0.0f) return out;
  out.r = Ar / W;
  out.g = Ag / W;
  out.b = Ab / W;
  out.w = W;
  out.depth = (Z / W) / P.diag;
  return out;
}

// Host side: the dense fp32 arrays of a cvr_medium_desc.
struct FeatureHostTexels {
  const float* dens;
  const float* alb;  // 4 floats per voxel
  uint32_t rx, ry;
  size_t at(uint32_t x, uint32_t y, uint32_t z) const { return ((size_t)z * ry + y) * rx + x; }
  float density(uint32_t x, uint32_t y, uint32_t z) const { return dens[at(x, y, z)]; }
  F3 albedo(uint32_t x, uint32_t y, uint32_t z) const {
    const float* a = alb + 4 * at(x, y, z);
    return F3{a[0], a[1], a[2]};
  }
  int cell(uint32_t, uint32_t, uint32_t, float*) const { return 0; }
};

struct MediumParams;
// k_features on stream s: tile_w x tile_h pixels of P into out_rgba (tile float4) and out_depth
// (tile floats, may be null); both device memory or the device address of pinned host memory.
hipError_t launch_features(const MediumParams& m, const FeatureParams& P, float4* out_rgba, float* out_depth,
                           hipStream_t s);

}  // namespace cvr
