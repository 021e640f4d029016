// cvr_features.hip - the primary-ray feature pass on the device (cvr_features*, include/cvr.h).
// The arithmetic is feature_pixel of cvr_features.h, the definition cvr_features_host runs on the
// CPU: this kernel only maps pixels onto lanes and texels onto the context's storage, so device
// and host agree bit for bit.
//
// One lane per pixel.  A wave covers an 8x8 pixel block (neighbouring rays march through
// neighbouring cells and share their cache lines), a 256-thread workgroup 2x2 such blocks, the
// workgroups row-major over a 1-D grid of ceil(w / 16) * ceil(h / 16) (at most 2^16 + edges: the
// tile has at most 2^24 pixels).  Lanes outside the tile leave at once; chords differ and the march
// stops early, so the lanes of a wave finish at different steps and the loop runs under the exec
// mask to the wave's last live lane.  Nothing is collective: no LDS, no barrier, no atomics, no
// waits on other waves, every loop bounded by max_steps.
//
// Storage and exact skipping: the texel functor of cvr_features_device.h.
#include "cvr_features_device.h"

namespace cvr {
namespace {

__global__ __launch_bounds__(256) void k_features(const MediumParams m, const FeatureParams P,
                                                  float4* __restrict__ out_rgba, float* __restrict__ out_depth) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t groups_x = (P.tile_w + 15u) >> 4;
  const uint32_t gy = blockIdx.x / groups_x, gx = blockIdx.x - gy * groups_x;
  const uint32_t ix = gx * 16u + (wave & 1u) * 8u + (lane & 7u), iy = gy * 16u + (wave >> 1) * 8u + (lane >> 3);
  if (ix >= P.tile_w || iy >= P.tile_h) return;
  const FeatureOut f = feature_pixel(FeatureDeviceTexels{m}, P, ix, iy);
  const size_t i = (size_t)iy * P.tile_w + ix;
  gstore4(out_rgba + i, make_float4(f.r, f.g, f.b, f.w));
  if (out_depth) out_depth[i] = f.depth;
}

}  // namespace

hipError_t launch_features(const MediumParams& m, const FeatureParams& P, float4* out_rgba, float* out_depth,
                           hipStream_t s) {
  if (!out_rgba || P.tile_w == 0 || P.tile_h == 0 || (uint64_t)P.tile_w * P.tile_h > (1ull << 24) ||
      P.max_steps == 0 || P.max_steps > 65536u)
    return hipErrorInvalidValue;
  const uint32_t grid = ((P.tile_w + 15u) >> 4) * ((P.tile_h + 15u) >> 4);
  hipLaunchKernelGGL(k_features, dim3(grid), dim3(256), 0, s, m, P, out_rgba, out_depth);
  return hipGetLastError();
}

}  // namespace cvr
