// cvr_preview.hip - the shaded preview pass on the device (cvr_preview*, include/cvr.h).  The
// arithmetic is preview_pixel of cvr_preview.h, the definition cvr_preview_host runs on the CPU:
// this kernel only maps pixels onto lanes and texels onto the context's storage (the feature
// pass's functor, cvr_features_device.h), so device and host agree bit for bit.
//
// k_features' mapping: one lane per pixel, a wave per 8x8 pixel block, a 256-thread workgroup 2x2
// such blocks, the workgroups row-major over a 1-D grid of ceil(w / 16) * ceil(h / 16).  Lanes
// outside the tile leave at once; the march runs under the exec mask to the wave's last live lane,
// and the gradient's six lookups and the shading run on the lanes whose step contributes, the
// others masked off.  Nothing is collective: no LDS, no barrier, no atomics, no waits on other
// waves; the march is bounded by max_steps, the specular's squarings by shininess_log2 <= 10.
// Two instances: the unshaded one carries no gradient code.
#include "cvr_features_device.h"
#include "cvr_preview.h"

namespace cvr {
namespace {

template <bool shaded>
__global__ __launch_bounds__(256) void k_preview(const MediumParams m, const PreviewParams Q,
                                                 float4* __restrict__ out_rgba) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t groups_x = (Q.F.tile_w + 15u) >> 4;
  const uint32_t gy = blockIdx.x / groups_x, gx = blockIdx.x - gy * groups_x;
  const uint32_t ix = gx * 16u + (wave & 1u) * 8u + (lane & 7u), iy = gy * 16u + (wave >> 1) * 8u + (lane >> 3);
  if (ix >= Q.F.tile_w || iy >= Q.F.tile_h) return;
  const PreviewOut f = preview_pixel<shaded>(FeatureDeviceTexels{m}, Q, ix, iy);
  gstore4(out_rgba + ((size_t)iy * Q.F.tile_w + ix), make_float4(f.r, f.g, f.b, f.w));
}

}  // namespace

hipError_t launch_preview(const MediumParams& m, const PreviewParams& Q, int shaded, float4* out_rgba, hipStream_t s) {
  const FeatureParams& P = Q.F;
  if (!out_rgba || P.tile_w == 0 || P.tile_h == 0 || (uint64_t)P.tile_w * P.tile_h > (1ull << 24) ||
      P.max_steps == 0 || P.max_steps > 65536u || Q.shininess_log2 > 10u)
    return hipErrorInvalidValue;
  const uint32_t grid = ((P.tile_w + 15u) >> 4) * ((P.tile_h + 15u) >> 4);
  if (shaded)
    hipLaunchKernelGGL(k_preview<true>, dim3(grid), dim3(256), 0, s, m, Q, out_rgba);
  else
    hipLaunchKernelGGL(k_preview<false>, dim3(grid), dim3(256), 0, s, m, Q, out_rgba);
  return hipGetLastError();
}

}  // namespace cvr
