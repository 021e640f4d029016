// cvr_preview.h - the shaded preview pass (cvr_preview*, include/cvr.h, CVR_HAS_PREVIEW): the
// feature pass's deterministic march along the straight camera ray, compositing colour front to
// back, each contributing sample lit by Blinn-Phong shading on the central-difference gradient of
// the stored density, over a background colour.  The one definition, compiled for the host
// statement (cvr_preview_host) and for k_preview (cvr_preview.hip): the ray, the chord, the steps,
// the density, the albedo and the texel functor are cvr_features.h's, every further operation is
// fp32 in the order cvr.h writes (-ffp-contract=off, correctly rounded / and sqrt), so both sides
// return the same bits.
#pragma once

#include "cvr_features.h"

namespace cvr {

// What a pixel reads besides FeatureParams; filled once per call on the host (preview_constants).
struct PreviewParams {
  FeatureParams F;
  float h[3];       // the cell sizes ext_a / res_a (delta is step times their minimum)
  float L[3];       // the light direction, normalised; not read with the headlight
  float ambient, diffuse, specular;
  uint32_t shininess_log2;
  float knee_abs;   // knee (max_density / min_a h_a)
  float bg[3];
  uint32_t headlight;
};

// Q.F is filled (feature_geometry); light: the descriptor's, not read with the headlight.
inline void preview_constants(PreviewParams& Q, const float light[3], int headlight, float ambient, float diffuse,
                              float specular, uint32_t shininess_log2, float knee, const float background[3],
                              float max_density) {
  const FeatureParams& P = Q.F;
  for (int a = 0; a < 3; ++a) {
    Q.h[a] = P.ext[a] / P.fres[a];
    Q.bg[a] = background[a];
    Q.L[a] = 0.0f;
  }
  Q.headlight = headlight ? 1u : 0u;
  if (!headlight) {
    const float l = det_sqrtf((light[0] * light[0] + light[1] * light[1]) + light[2] * light[2]);
    for (int a = 0; a < 3; ++a) Q.L[a] = light[a] / l;
  }
  Q.ambient = ambient;
  Q.diffuse = diffuse;
  Q.specular = specular;
  Q.shininess_log2 = shininess_log2;
  Q.knee_abs = knee * (max_density / det_fminf(det_fminf(Q.h[0], Q.h[1]), Q.h[2]));
}

// The shading terms of a contributing sample at p, ray direction d: the gradient's magnitude m,
// the diffuse cosine nl and the specular factor sp.  False when not m > 0 (a flat neighbourhood,
// or a NaN): the sample is unlit and nl, sp are not set.
struct PreviewTerms {
  float m, nl, sp;
};
// The terms of a gradient (gx, gy, gz), whatever it was taken of: the stored density below, the
// raw field in cvr_project.h
CVR_HD bool preview_light_terms(const PreviewParams& Q, float gx, float gy, float gz, F3 d, PreviewTerms& k) {
  const float m = det_sqrtf((gx * gx + gy * gy) + gz * gz);
  k.m = m;
  if (!(m > 0.0f)) return false;
  const float nx = gx / m, ny = gy / m, nz = gz / m;  // the outward normal is -n
  const float vx = -d.x, vy = -d.y, vz = -d.z;
  const float lx = Q.headlight ? vx : Q.L[0], ly = Q.headlight ? vy : Q.L[1], lz = Q.headlight ? vz : Q.L[2];
  float nl = -((nx * lx + ny * ly) + nz * lz);
  if (!(nl > 0.0f)) nl = 0.0f;
  float sp = 0.0f;
  if (Q.specular > 0.0f) {
    const float Hx = lx + vx, Hy = ly + vy, Hz = lz + vz;
    const float hh = det_sqrtf((Hx * Hx + Hy * Hy) + Hz * Hz);
    if (hh > 0.0f) {
      float nh = -((nx * Hx + ny * Hy) + nz * Hz) / hh;
      if (!(nh > 0.0f)) nh = 0.0f;
      for (uint32_t k = 0; k < Q.shininess_log2; ++k) nh = nh * nh;  // nh^(2^k): detmath has no pow
      sp = nh;
    }
  }
  k.nl = nl;
  k.sp = sp;
  return true;
}
template <class Tex>
CVR_HD bool preview_terms(const Tex& tex, const PreviewParams& Q, F3 p, F3 d, PreviewTerms& k) {
  const FeatureParams& P = Q.F;
  const float hx = Q.h[0], hy = Q.h[1], hz = Q.h[2];
  const float gx = (feat_density(tex, P, F3{p.x + hx, p.y, p.z}) - feat_density(tex, P, F3{p.x - hx, p.y, p.z})) / hx;
  const float gy = (feat_density(tex, P, F3{p.x, p.y + hy, p.z}) - feat_density(tex, P, F3{p.x, p.y - hy, p.z})) / hy;
  const float gz = (feat_density(tex, P, F3{p.x, p.y, p.z + hz}) - feat_density(tex, P, F3{p.x, p.y, p.z - hz})) / hz;
  return preview_light_terms(Q, gx, gy, gz, d, k);
}

// The emitted colour of a contributing sample at p with albedo c, ray direction d.
template <class Tex>
CVR_HD F3 preview_shade(const Tex& tex, const PreviewParams& Q, F3 p, F3 d, F3 c) {
  PreviewTerms k;
  if (!preview_terms(tex, Q, p, d, k)) return c;
  const float f = Q.ambient + Q.diffuse * k.nl;
  const float s = Q.specular * k.sp;
  const float q = k.m / (k.m + Q.knee_abs), q1 = 1.0f - q;
  return F3{q1 * c.x + q * (f * c.x + s), q1 * c.y + q * (f * c.y + s), q1 * c.z + q * (f * c.z + s)};
}

struct PreviewOut {
  float r, g, b, w;
};

// One pixel of the pass, as cvr.h writes it.  shaded = false: CVR_PREVIEW_UNSHADED, no gradient code.
template <bool shaded, class Tex>
CVR_HD PreviewOut preview_pixel(const Tex& tex, const PreviewParams& Q, uint32_t ix, uint32_t iy) {
  const FeatureParams& P = Q.F;
  F3 o, d;
  feat_ray(P, ix, iy, o, d);
  float t0, t1;
  if (!feat_chord(P, o, d, t0, t1)) return PreviewOut{Q.bg[0], Q.bg[1], Q.bg[2], 0.0f};
  // the feature pass's step count: bounded by max_steps whatever the chord is
  const float q = __builtin_ceilf((t1 - t0) / P.delta);
  uint32_t n = P.max_steps;
  if (q < (float)P.max_steps) n = q > 0.0f ? (uint32_t)q : 0u;
  float T = 1.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, W = 0.0f;
  for (uint32_t i = 0; i < n; ++i) {
    const float t = t0 + ((float)i + 0.5f) * P.delta;
    if (!(t < t1)) break;
    const F3 p{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};
    const float rho = feat_density(tex, P, p);
    const float s = (P.scale * rho) * P.delta;
    if (!(s > 0.0f)) continue;
    const float a = s / (1.0f + s);
    const float w = T * a;
    F3 e = feat_albedo(tex, P, p);
    if (shaded) e = preview_shade(tex, Q, p, d, e);
    Cr += w * e.x;
    Cg += w * e.y;
    Cb += w * e.z;
    W += w;
    T = T - w;
    if (T < P.t_stop) break;
  }
  return PreviewOut{Cr + T * Q.bg[0], Cg + T * Q.bg[1], Cb + T * Q.bg[2], W};
}

struct MediumParams;
// k_preview on stream s: tile_w x tile_h pixels of Q into out_rgba (tile float4), device memory or
// the device address of pinned host memory.  shaded 0: the instance without gradient code.
hipError_t launch_preview(const MediumParams& m, const PreviewParams& Q, int shaded, float4* out_rgba, hipStream_t s);

}  // namespace cvr
