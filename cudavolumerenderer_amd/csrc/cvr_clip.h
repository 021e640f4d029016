// cvr_clip.h - the clip region of the device builds (cvr.h: CVR_HAS_CLIP), once: the per-voxel
// test that cvr_clip_host states and the build kernels apply, and the test of a whole box of
// voxels that lets a kernel leave a provably clipped extent unread.  fp32 +, x and comparisons
// only, every operation in the written order (-ffp-contract=off), so host statement and kernel
// decide the same voxels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvr {

constexpr uint32_t kClipMaxPlanes = 8;  // CVR_CLIP_MAX_PLANES

// The region as the kernels take it, by value with their voxel source (39 words).  hi is the
// descriptor's, clamped to the grid when the clip is taken: c < hi then says c < min(hi, res).
struct ClipRegion {
  uint32_t lo[3], hi[3];
  uint32_t n_planes;
  float planes[kClipMaxPlanes][4];  // A, B, C, D in voxel-index space
};

// t of plane p at voxel (x, y, z): each product rounded, summed in this order
__host__ __device__ __forceinline__ float clip_plane_t(const float p[4], uint32_t x, uint32_t y, uint32_t z) {
  const float ax = p[0] * (float)x, by = p[1] * (float)y, cz = p[2] * (float)z;
  return ((ax + by) + cz) + p[3];
}

// The voxel is kept: inside the crop box and on no plane's negative side (t == 0 is kept, a NaN t is not)
__host__ __device__ __forceinline__ bool clip_keeps(const ClipRegion& r, uint32_t x, uint32_t y, uint32_t z) {
  bool keep = x >= r.lo[0] && x < r.hi[0] && y >= r.lo[1] && y < r.hi[1] && z >= r.lo[2] && z < r.hi[2];
  // (unrolled over the 8 entries with an exit at n_planes: every index into the region is a
  // constant, so a kernel reads its by-value region from its arguments, not from a private copy)
#pragma unroll
  for (uint32_t k = 0; k < kClipMaxPlanes; ++k) {
    if (k >= r.n_planes) break;
    keep = keep && clip_plane_t(r.planes[k], x, y, z) >= 0.0f;
  }
  return keep;
}

// Every voxel of the box [b0, b1] (inclusive corners) is clipped, decided from the box alone: it
// misses the crop box on some axis, or all 8 corners lie on one plane's negative side.  A rounded
// product and a rounded sum are monotonic in each operand, so t is monotonic in each coordinate
// and is largest at a corner; a NaN at a corner (an overflowed product) decides nothing.  False
// says nothing: the voxels are then tested one by one.
__host__ __device__ __forceinline__ bool clip_box_outside(const ClipRegion& r, const uint32_t b0[3], const uint32_t b1[3]) {
  bool out = b1[0] < r.lo[0] || b0[0] >= r.hi[0] || b1[1] < r.lo[1] || b0[1] >= r.hi[1] || b1[2] < r.lo[2] ||
             b0[2] >= r.hi[2];
#pragma unroll
  for (uint32_t k = 0; k < kClipMaxPlanes; ++k) {
    if (k >= r.n_planes) break;
    bool neg = true;
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c)
      neg = neg && clip_plane_t(r.planes[k], (c & 1u) ? b1[0] : b0[0], (c & 2u) ? b1[1] : b0[1],
                                (c & 4u) ? b1[2] : b0[2]) < 0.0f;
    out = out || neg;
  }
  return out;
}

}  // namespace cvr
