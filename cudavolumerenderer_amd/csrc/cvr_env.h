// cvr_env.h - the environment map's lookup (include/cvr.h, CVR_HAS_ENVMAP): the one definition,
// compiled for the host (cvr_environment_eval_host) and for the kernels (k_env_eval, k_trace_env,
// k_wpool's kMedEnv instances).  fp32 only, every operation in the written order
// (-ffp-contract=off, the fused operations are the explicit det_fmaf), so both sides return the
// same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvr_detmath.h"

namespace cvr {

// The stored map: w x h texels (fl(scale r), fl(scale g), fl(scale b), 0), row 0 the top, and the
// row-major world-to-environment rotation.  64 bytes: in device memory it is the header the
// kMedEnv instances reach through LaunchParams::rec (which an instance without records never reads).
struct EnvParams {
  const float4* texels;
  uint32_t w, h;
  float R[9];
  uint32_t pad[3];
};
static_assert(sizeof(EnvParams) == 64, "EnvParams is the 64-byte header LaunchParams::rec points at");

// The four taps and two weights of direction (dx, dy, dz): texel (x, y) is at y * w + x.
struct EnvTaps {
  uint32_t xa, xb, ya, yb;
  float fx, fy;
};
__host__ __device__ inline EnvTaps env_taps(const float R[9], uint32_t w, uint32_t h, float dx, float dy, float dz) {
  const float ex = (R[0] * dx + R[1] * dy) + R[2] * dz;
  const float ey = (R[3] * dx + R[4] * dy) + R[5] * dz;
  const float ez = (R[6] * dx + R[7] * dy) + R[8] * dz;
  float u = det_fmaf(det_atan2f(ex, -ez), 0.15915494309189535f, 0.5f);
  float v = det_acosf(det_fminf(det_fmaxf(ey, -1.0f), 1.0f)) * 0.3183098861837907f;
  u = det_fminf(det_fmaxf(u, 0.0f), 1.0f);  // (a NaN becomes 0: det_fmaxf returns its other operand)
  v = det_fminf(det_fmaxf(v, 0.0f), 1.0f);
  const float x = det_fmaf(u, (float)w, -0.5f), y = det_fmaf(v, (float)h, -0.5f);
  const int x0 = det_floor_i32(x), y0 = det_floor_i32(y);
  const int iw = (int)w, ih = (int)h;
  EnvTaps t;
  t.fx = x - (float)x0;
  t.fy = y - (float)y0;
  t.xa = (uint32_t)(x0 < 0 ? iw - 1 : x0);  // u wraps
  t.xb = (uint32_t)(x0 + 1 >= iw ? 0 : x0 + 1);
  t.ya = (uint32_t)(y0 < 0 ? 0 : y0);  // v clamps
  t.yb = (uint32_t)(y0 + 1 >= ih ? ih - 1 : y0 + 1);
  return t;
}
__host__ __device__ inline float env_lerp2(float A, float B, float C, float D, float fx, float fy) {
  const float t = det_fmaf(fx, B - A, A), b = det_fmaf(fx, D - C, C);
  return det_fmaf(fy, b - t, t);
}
// The radiance of direction d: tap(x, y) returns the stored texel, from wherever the caller keeps
// it (the order of the arithmetic does not depend on that).
template <class Tap>
__host__ __device__ __forceinline__ void env_lookup_at(const Tap& tap, const float R[9], uint32_t w, uint32_t h,
                                                       float dx, float dy, float dz, float out[3]) {
  const EnvTaps t = env_taps(R, w, h, dx, dy, dz);
  const float4 A = tap(t.xa, t.ya), B = tap(t.xb, t.ya), C = tap(t.xa, t.yb), D = tap(t.xb, t.yb);
  out[0] = env_lerp2(A.x, B.x, C.x, D.x, t.fx, t.fy);
  out[1] = env_lerp2(A.y, B.y, C.y, D.y, t.fx, t.fy);
  out[2] = env_lerp2(A.z, B.z, C.z, D.z, t.fx, t.fy);
}
// The map in plain memory: the host statement and the kernels' global loads (one 16-byte load a tap;
// a 16384 x 8192 map's byte offsets pass 2^31, so the index is a size_t).
struct EnvImage {
  const float4* texels;
  uint32_t w;
  __host__ __device__ float4 operator()(uint32_t x, uint32_t y) const { return texels[(size_t)y * w + x]; }
};
__host__ __device__ __forceinline__ void env_lookup(const EnvParams& E, float dx, float dy, float dz, float out[3]) {
  env_lookup_at(EnvImage{E.texels, E.w}, E.R, E.w, E.h, dx, dy, dz, out);
}

// What the conversion pass finds, in device memory; the host sets first_bad to ~0 and max_bits to 0.
struct EnvScan {
  unsigned long long first_bad;  // smallest index (texel * channels + channel) of a stored component < 0 or not finite
  uint32_t max_bits;             // bits of the largest stored component (all are >= +0 when first_bad stays ~0)
  uint32_t pad;
};
// Device side (cvr_env.hip).  src: n_texels * channels floats in device memory; dst: n_texels float4.
hipError_t launch_env_convert(const float* src, uint32_t channels, size_t n_texels, float scale, float4* dst,
                              EnvScan* scan, hipStream_t s);
// out[3 i ..] = the lookup of dirs[3 i ..], i < n (device arrays); E in device memory
hipError_t launch_env_eval(const EnvParams* E, const float* dirs, size_t n, float* out, hipStream_t s);

}  // namespace cvr
