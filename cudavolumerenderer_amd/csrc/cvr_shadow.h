// cvr_shadow.h - the light's transmittance for the shaded preview (cvr_light_volume*,
// cvr_preview_shadowed*, include/cvr.h, CVR_HAS_SHADOWS): a light volume, one transmittance per
// node of a grid over the medium's box, each the feature pass's march from the node towards a
// directional light, and the preview pass with every contributing sample's light scaled by the
// volume's trilinear value at the sample.  The one definition, compiled for the host statements
// (cvr_light_volume_host, cvr_preview_shadowed_host) and for the kernels (cvr_shadow.hip): the
// chord, the density and the texel functor are cvr_features.h's, the shading terms
// cvr_preview.h's, every further operation is fp32 in the order cvr.h writes (-ffp-contract=off,
// correctly rounded / and sqrt), so both sides return the same bits.
#pragma once

#include "cvr_preview.h"

namespace cvr {

// What a node's march reads: the feature pass's constants (F's camera and tile are not read), the
// grid and the direction towards the light.
struct LightVolumeParams {
  FeatureParams F;
  uint32_t sres[3];
  float cell[3];  // ext_a / (float)sres_a
  float L[3];     // normalised as preview_constants normalises the preview's light
};

// light_a / sqrt((lx lx + ly ly) + lz lz); the length is returned (the entry points refuse 0, inf, NaN)
inline float light_normalise(const float light[3], float L[3]) {
  const float l = det_sqrtf((light[0] * light[0] + light[1] * light[1]) + light[2] * light[2]);
  for (int a = 0; a < 3; ++a) L[a] = light[a] / l;
  return l;
}

// V.F is filled (feature_geometry)
inline void light_volume_constants(LightVolumeParams& V, const uint32_t sres[3], const float light[3]) {
  for (int a = 0; a < 3; ++a) {
    V.sres[a] = sres[a];
    V.cell[a] = V.F.ext[a] / (float)sres[a];
  }
  (void)light_normalise(light, V.L);
}

// The transmittance S from node (i, j, k) to the box's surface towards the light, as cvr.h writes it.
template <class Tex>
CVR_HD float light_node(const Tex& tex, const LightVolumeParams& V, uint32_t i, uint32_t j, uint32_t k) {
  const FeatureParams& P = V.F;
  const F3 p0{P.bmin[0] + ((float)i + 0.5f) * V.cell[0], P.bmin[1] + ((float)j + 0.5f) * V.cell[1],
              P.bmin[2] + ((float)k + 0.5f) * V.cell[2]};
  const F3 L{V.L[0], V.L[1], V.L[2]};
  float t0, t1;
  if (!feat_chord(P, p0, L, t0, t1)) return 1.0f;
  // the feature pass's step count on t1 (the march starts at the node): bounded by max_steps
  const float q = __builtin_ceilf(t1 / P.delta);
  uint32_t n = P.max_steps;
  if (q < (float)P.max_steps) n = q > 0.0f ? (uint32_t)q : 0u;
  float T = 1.0f;
  for (uint32_t s_i = 0; s_i < n; ++s_i) {
    const float t = ((float)s_i + 0.5f) * P.delta;
    if (!(t < t1)) break;
    const F3 p{p0.x + t * L.x, p0.y + t * L.y, p0.z + t * L.z};
    const float rho = feat_density(tex, P, p);
    const float s = (P.scale * rho) * P.delta;
    if (!(s > 0.0f)) continue;
    T = T - T * (s / (1.0f + s));
    if (T < P.t_stop) break;
  }
  return T;
}

// What a shadowed preview pixel reads besides PreviewParams: the light volume and the strength.
// A separate kernel argument, so PreviewParams and k_preview stay as they are.
struct ShadowGrid {
  const float* S;  // sres_x * sres_y * sres_z floats, x fastest
  uint32_t res[3];
  float fres[3];  // (float)res
  float shadow;
};

CVR_HD uint32_t shadow_tap(int i, uint32_t res) {
  const int hi = (int)res - 1;
  return (uint32_t)(i < 0 ? 0 : i > hi ? hi : i);
}

// The light volume's trilinear value at world point p (nodes at the cell centres, taps clamped).
CVR_HD float shadow_lookup(const ShadowGrid& G, const FeatureParams& P, F3 p) {
  const float ux = ((p.x - P.bmin[0]) / P.ext[0]) * G.fres[0] - 0.5f;
  const float uy = ((p.y - P.bmin[1]) / P.ext[1]) * G.fres[1] - 0.5f;
  const float uz = ((p.z - P.bmin[2]) / P.ext[2]) * G.fres[2] - 0.5f;
  const int x1 = det_floor_i32(ux), y1 = det_floor_i32(uy), z1 = det_floor_i32(uz);
  const float fx = ux - (float)x1, fy = uy - (float)y1, fz = uz - (float)z1;
  const uint32_t xa = shadow_tap(x1, G.res[0]), xb = shadow_tap(x1 + 1, G.res[0]);
  const uint32_t ya = shadow_tap(y1, G.res[1]), yb = shadow_tap(y1 + 1, G.res[1]);
  const size_t za = (size_t)shadow_tap(z1, G.res[2]) * G.res[1], zb = (size_t)shadow_tap(z1 + 1, G.res[2]) * G.res[1];
  const float* a0 = G.S + (za + ya) * G.res[0];
  const float* a1 = G.S + (za + yb) * G.res[0];
  const float* b0 = G.S + (zb + ya) * G.res[0];
  const float* b1 = G.S + (zb + yb) * G.res[0];
  const float d[8] = {a0[xa], a0[xb], a1[xa], a1[xb], b0[xa], b0[xb], b1[xa], b1[xb]};
  return feat_trilerp8(d, fx, fy, fz);
}

// preview_shade with the visibility V of the light: the unlit part is V c, the diffuse and the
// specular terms are scaled by V, the ambient term is not.
template <class Tex>
CVR_HD F3 preview_shade_shadowed(const Tex& tex, const PreviewParams& Q, F3 p, F3 d, F3 c, float V) {
  const F3 vc{V * c.x, V * c.y, V * c.z};
  PreviewTerms k;
  if (!preview_terms(tex, Q, p, d, k)) return vc;
  const float f = Q.ambient + (Q.diffuse * k.nl) * V;
  const float s = (Q.specular * k.sp) * V;
  const float q = k.m / (k.m + Q.knee_abs), q1 = 1.0f - q;
  return F3{q1 * vc.x + q * (f * c.x + s), q1 * vc.y + q * (f * c.y + s), q1 * vc.z + q * (f * c.z + s)};
}

// One pixel of the shadowed pass: preview_pixel with e as cvr.h writes it under CVR_HAS_SHADOWS.
// Q.headlight is 0 and Q.L the light volume's direction.
template <bool shaded, class Tex>
CVR_HD PreviewOut preview_shadowed_pixel(const Tex& tex, const PreviewParams& Q, const ShadowGrid& G, uint32_t ix,
                                         uint32_t iy) {
  const FeatureParams& P = Q.F;
  F3 o, d;
  feat_ray(P, ix, iy, o, d);
  float t0, t1;
  if (!feat_chord(P, o, d, t0, t1)) return PreviewOut{Q.bg[0], Q.bg[1], Q.bg[2], 0.0f};
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
    const F3 c = feat_albedo(tex, P, p);
    const float V = 1.0f - G.shadow * (1.0f - shadow_lookup(G, P, p));
    const F3 e = shaded ? preview_shade_shadowed(tex, Q, p, d, c, V) : F3{V * c.x, V * c.y, V * c.z};
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
// k_light_volume on stream s: the sres_x * sres_y * sres_z nodes of V into out (device memory).
hipError_t launch_light_volume(const MediumParams& m, const LightVolumeParams& V, float* out, hipStream_t s);
// k_preview_shadowed on stream s: launch_preview's arguments and the light volume.
hipError_t launch_preview_shadowed(const MediumParams& m, const PreviewParams& Q, const ShadowGrid& G, int shaded,
                                   float4* out_rgba, hipStream_t s);

}  // namespace cvr
