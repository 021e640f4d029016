// cvr_shadow.hip - the light volume and the shadowed preview on the device (cvr_build_light_volume,
// cvr_preview_shadowed*, include/cvr.h).  The arithmetic is light_node and preview_shadowed_pixel of
// cvr_shadow.h, the definitions the host statements run on the CPU: these kernels only map nodes
// and pixels onto lanes and texels onto the context's storage (the feature pass's functor,
// cvr_features_device.h), so device and host agree bit for bit.
//
// k_light_volume: one lane per node, a wave per 4x4x4 node block (x the lane's two low bits, then
// y, then z), a 256-thread workgroup four such blocks along x, the workgroups x fastest over a 1-D
// grid of ceil(sx / 16) * ceil(sy / 4) * ceil(sz / 4) (under 2^22 for any grid the entry points
// accept: the launch has no cap and the kernel no loop over blocks).  The rays of a
// wave are parallel and start inside a cube of four nodes a side, so their cells stay neighbours
// all the way; a lane's four x-neighbours store one 16-byte run.  Lanes outside the grid leave at
// once.  CVR_SHADOW_ROWS 1 is the mapping this one was measured against, a wave per 64-node x-row
// (profiles/shadow/README.md); the library is built with 0.
// k_preview_shadowed: k_preview's pixel mapping, the light volume in an argument of its own.
// Nothing is collective: no LDS, no barrier, no atomics, no waits on other waves; the marches are
// bounded by max_steps, the specular's squarings by shininess_log2 <= 10.
#include "cvr_features_device.h"
#include "cvr_shadow.h"

#ifndef CVR_SHADOW_ROWS
#define CVR_SHADOW_ROWS 0
#endif

namespace cvr {
namespace {

// nodes a workgroup covers per axis
#if CVR_SHADOW_ROWS
constexpr uint32_t kGx = 64u, kGy = 4u, kGz = 1u;
#else
constexpr uint32_t kGx = 16u, kGy = 4u, kGz = 4u;
#endif

__global__ __launch_bounds__(256) void k_light_volume(const MediumParams m, const LightVolumeParams V,
                                                      float* __restrict__ out) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t groups_x = (V.sres[0] + kGx - 1u) / kGx, groups_y = (V.sres[1] + kGy - 1u) / kGy;
  const uint32_t gyz = blockIdx.x / groups_x, gx = blockIdx.x - gyz * groups_x;
  const uint32_t gz = gyz / groups_y, gy = gyz - gz * groups_y;
#if CVR_SHADOW_ROWS
  const uint32_t i = gx * kGx + lane, j = gy * kGy + wave, k = gz;
#else
  const uint32_t i = gx * kGx + wave * 4u + (lane & 3u), j = gy * kGy + ((lane >> 2) & 3u), k = gz * kGz + (lane >> 4);
#endif
  if (i >= V.sres[0] || j >= V.sres[1] || k >= V.sres[2]) return;
  out[((size_t)k * V.sres[1] + j) * V.sres[0] + i] = light_node(FeatureDeviceTexels{m}, V, i, j, k);
}

template <bool shaded>
__global__ __launch_bounds__(256) void k_preview_shadowed(const MediumParams m, const PreviewParams Q, const ShadowGrid G,
                                                          float4* __restrict__ out_rgba) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t groups_x = (Q.F.tile_w + 15u) >> 4;
  const uint32_t gy = blockIdx.x / groups_x, gx = blockIdx.x - gy * groups_x;
  const uint32_t ix = gx * 16u + (wave & 1u) * 8u + (lane & 7u), iy = gy * 16u + (wave >> 1) * 8u + (lane >> 3);
  if (ix >= Q.F.tile_w || iy >= Q.F.tile_h) return;
  const PreviewOut f = preview_shadowed_pixel<shaded>(FeatureDeviceTexels{m}, Q, G, ix, iy);
  gstore4(out_rgba + ((size_t)iy * Q.F.tile_w + ix), make_float4(f.r, f.g, f.b, f.w));
}

bool grid_ok(const uint32_t res[3]) {
  for (int a = 0; a < 3; ++a)
    if (res[a] == 0 || res[a] > 1024u) return false;
  return (uint64_t)res[0] * res[1] * res[2] <= (1ull << 27);
}

}  // namespace

hipError_t launch_light_volume(const MediumParams& m, const LightVolumeParams& V, float* out, hipStream_t s) {
  if (!out || !grid_ok(V.sres) || V.F.max_steps == 0 || V.F.max_steps > 65536u) return hipErrorInvalidValue;
  // (at most 2^10 / 16 * 2^8 * 2^8 = 2^22 workgroups: a 1-D grid holds them)
  const uint32_t grid = ((V.sres[0] + kGx - 1u) / kGx) * ((V.sres[1] + kGy - 1u) / kGy) * ((V.sres[2] + kGz - 1u) / kGz);
  hipLaunchKernelGGL(k_light_volume, dim3(grid), dim3(256), 0, s, m, V, out);
  return hipGetLastError();
}

hipError_t launch_preview_shadowed(const MediumParams& m, const PreviewParams& Q, const ShadowGrid& G, int shaded,
                                   float4* out_rgba, hipStream_t s) {
  const FeatureParams& P = Q.F;
  if (!out_rgba || !G.S || !grid_ok(G.res) || P.tile_w == 0 || P.tile_h == 0 ||
      (uint64_t)P.tile_w * P.tile_h > (1ull << 24) || P.max_steps == 0 || P.max_steps > 65536u || Q.shininess_log2 > 10u)
    return hipErrorInvalidValue;
  const uint32_t grid = ((P.tile_w + 15u) >> 4) * ((P.tile_h + 15u) >> 4);
  if (shaded)
    hipLaunchKernelGGL(k_preview_shadowed<true>, dim3(grid), dim3(256), 0, s, m, Q, G, out_rgba);
  else
    hipLaunchKernelGGL(k_preview_shadowed<false>, dim3(grid), dim3(256), 0, s, m, Q, G, out_rgba);
  return hipGetLastError();
}

}  // namespace cvr
