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
// Storage: a dense medium's cell is 2 x 16-byte loads (one in the half format), the 8-tap gather
// where there are no cells or the point's lower corner is off the grid; a sparse medium reads
// its brick word and the cell-leaf pool.  Exact skipping, sparse media only: a point whose
// super-brick's bit in the empty-region mask is clear, or whose brick word names cell-leaf slot 0,
// has the density +0 and loads nothing more.  Dense media do not skip: brick-bound code 0 is the
// bound 2^-15 of the majorant, not zero (k_build_bounds' bound_code rounds a brick maximum of 0
// and one of 2^-16 to the same code).
#include "cvr_features.h"
#include "cvr_walk.h"

namespace cvr {
namespace {

struct FeatureDeviceTexels {
  const MediumParams& m;
  __device__ __forceinline__ float density(uint32_t x, uint32_t y, uint32_t z) const { return texel_density(m, x, y, z); }
  // (a uniform dense albedo and a sparse medium's background are constants: nothing is loaded)
  __device__ __forceinline__ F3 albedo(uint32_t x, uint32_t y, uint32_t z) const {
    const float4 a = texel_albedo(m, x, y, z);
    return F3{a.x, a.y, a.z};
  }
  __device__ __forceinline__ int cell(uint32_t x1, uint32_t y1, uint32_t z1, float d[8]) const {
    if (!m.cells) return 0;
    const float4* cp;
    if (m.sbounds) {
      if (m.emask) {
        const uint32_t sb = ((z1 >> m.eshift) << m.eshz) | ((y1 >> m.eshift) << m.eshy) | (x1 >> m.eshift);
        if (!((m.emask[(sb >> 5) & (uint32_t)(kEmaskWords - 1)] >> (sb & 31u)) & 1u)) return 2;
      }
      const uint32_t slot = m.sbounds[__umul24(z1 >> m.bshift, m.bnxy) + __umul24(y1 >> m.bshift, m.bnx) +
                                      (x1 >> m.bshift)] & 0xFFFFFFu;
      if (slot == 0u) return 2;  // the zero cell leaf
      cp = m.cells + ((((size_t)slot) << 9 | leaf_local(x1, y1, z1)) << cell_shift(m));
    } else {
      cp = dense_cell(m, x1, y1, z1);
    }
    // a cell is (d000, d100, d001, d101), (d010, d110, d011, d111): trilerp_cell's order
    if (m.format) {
      const cvr_h8 h = *reinterpret_cast<const cvr_h8*>(cp);
      d[0] = (float)h[0], d[4] = (float)h[1], d[1] = (float)h[2], d[5] = (float)h[3];
      d[2] = (float)h[4], d[6] = (float)h[5], d[3] = (float)h[6], d[7] = (float)h[7];
    } else {
      const float4 lo = gload4(cp), hi = gload4(cp + 1);
      d[0] = lo.x, d[4] = lo.y, d[1] = lo.z, d[5] = lo.w;
      d[2] = hi.x, d[6] = hi.y, d[3] = hi.z, d[7] = hi.w;
    }
    return 1;
  }
};

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
