// cvr_features_device.h - the texel functor of cvr_features.h on the context's storage, shared by
// the kernels that march it (k_features, k_preview).  Device code only.
//
// Storage: a dense medium's cell is 2 x 16-byte loads (one in the half format), the 8-tap gather
// where there are no cells or the point's lower corner is off the grid; a sparse medium reads
// its brick word and the cell-leaf pool.  Exact skipping, sparse media only: a point whose
// super-brick's bit in the empty-region mask is clear, or whose brick word names cell-leaf slot 0,
// has the density +0 and loads nothing more.  Dense media do not skip: brick-bound code 0 is the
// bound 2^-15 of the majorant, not zero (k_build_bounds' bound_code rounds a brick maximum of 0
// and one of 2^-16 to the same code).
#pragma once

#include "cvr_features.h"
#include "cvr_walk.h"

namespace cvr {

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

}  // namespace cvr
